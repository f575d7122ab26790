/* sesrq_demosaic.h -- the classical demosaic of a Bayer frame, on the device: the baseline the raw nets (MFLAG 2, 3, 4: dm, nrdm_3,
 * nrdm_6) are measured against, and a view of the frame they were given.  Two methods: bilinear interpolation, and the 5 x 5 linear
 * filters of Malvar, He and Cutler ("High-quality linear interpolation for demosaicing of Bayer-patterned color images", ICASSP 2004).
 *
 * A library of its own (libsesrq_demosaic.so): it links no other library of the project, and their ABIs are unchanged.  It takes the
 * format struct and the CFA / packing enumerators of include/sesrq_sensor.h.
 *
 * Input, one of two.
 *   raw      a packed sensor frame exactly as sesrq_sensor_unpack takes it (sesrq_sensor_format: CFA order, black, white, U16 / RAW10 /
 *            RAW12; rows row_stride_bytes apart).  The sample of a pixel with code v is s = d(v) = min(max(v, black), white) - black,
 *            an integer 0 .. D = white - black, and the normaliser is K = 16 D.
 *   spread   a device (N, 3, H, W) fp32 frame as the sensor, noise and unprocess libraries write it.  The sample of pixel (y, x) is the
 *            fp32 value at (y, x) of the plane of its site channel, as it is (no clamp); K = 16.  The values of the two other planes
 *            at that pixel never reach a result: they may hold anything, NaN included.
 *
 * Neighbours.  Sample (y + j, x + i), |i|, |j| <= 2, is taken at fold(y + j, H), fold(x + i, W): reflection about the frame's first and
 * last sample without repeating it, fold(t, n) = u < n ? u : 2 (n - 1) - u with u = t mod 2 (n - 1), 0 <= u.  The period is even, so a
 * neighbour stays on its CFA parity for any H, W >= 2, odd sizes included.  H < 2 or W < 2 is refused.
 *
 * Filters.  With c the pixel's own sample and N, S, W, E, NW, NE, SW, SE its neighbours at distance 1, NN, SS, WW, EE those at distance
 * 2 in its row and column, everything is fp32, each operation rounded once, no fused multiply-add.  Group sums, left to right:
 *   A1 = ((N + S) + W) + E     Dg = ((NW + NE) + SW) + SE     V2 = NN + SS     H2 = WW + EE     Hn = W + E     Vn = N + S
 * The numerator S (the value times 16) of every channel of a pixel, its terms added left to right, a product formed before it is added
 * or subtracted:
 *                                                            SESRQ_DEMOSAIC_MALVAR                          SESRQ_DEMOSAIC_BILINEAR
 *   the site channel                                         16 c                                           16 c
 *   G at an R or B site                                      (8 c + 4 A1) - 2 (V2 + H2)                     4 A1
 *   R (B) at a G site with R (B) to its left and right       (((10 c + 8 Hn) - 2 Dg) - 2 H2) + V2           8 Hn
 *   R (B) at a G site with R (B) above and below             (((10 c + 8 Vn) - 2 Dg) - 2 V2) + H2           8 Vn
 *   R at a B site, B at an R site                            (12 c + 4 Dg) - 3 (V2 + H2)                    4 Dg
 * The bilinear numerators other than the site channel's have no c term at all (a NaN at c does not reach them).
 *
 * Output.  out_c = fl(clamp(S) / K), clamp(S) = S > 0 ? fminf(S, K) : 0 -- fminf(fmaxf(S, 0), K) with the two cases C leaves open
 * settled: a NaN and a -0.0 both give +0.0 -- and the quotient a true IEEE fp32 division, as x(v) of sesrq_sensor.h is.  For raw input
 * every sample is an integer <= 65535 and |S| <= 24 D < 2^24, so every intermediate is an exact integer whatever the order.
 * The site channel is therefore x(v) of sesrq_sensor.h for raw input (16 d / 16 D is the quotient d / D) and the input sample clamped
 * to [0, 1] for spread input (NaN and -0.0: +0.0).  out is (N, 3, H, W) fp32, planes R, G, B: the layout of the nets' ground truth. */
#ifndef SESRQ_DEMOSAIC_H
#define SESRQ_DEMOSAIC_H

#include <stddef.h>
#include <stdint.h>

#include "sesrq_sensor.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_DEMOSAIC_BILINEAR = 0, SESRQ_DEMOSAIC_MALVAR = 1 };

/* raw: device, N frames of H rows in `fmt` (valid as sesrq_sensor.h says); row y of frame n starts at raw + (n H + y) row_stride_bytes
 * and holds sesrq_sensor_row_bytes(fmt, W) bytes of pixels, then padding.  out: device (N, 3, H, W) fp32.  Any N >= 1, H, W >= 2 that
 * the packing allows (RAW10: W % 4 == 0, RAW12: W % 2 == 0; odd H and W are legal for U16) with H, W <= 2^31 - 129 and at most
 * 2^31 - 1 tiles of 64 x 32 pixels in the batch; offsets are 64-bit, so a batch may cross 4 GiB.  One kernel enqueued on `stream` (a
 * hipStream_t; NULL = the default stream) of the current device; no allocation, no synchronisation, no workspace, no context.  Every
 * argument is checked before any HIP call; 0 on success, non-zero with sesrq_demosaic_last_error() set otherwise.
 *
 * Caller buffers.  raw may start at any address and row_stride_bytes may be any value >= the row's bytes; out at any 4-byte aligned
 * address.  A workgroup stages its 64 x 32 tile and a halo of 2 samples in segments of 8 (U16) or 16 (RAW10, RAW12) pixels:
 *   loads    a segment that lies whole inside its row is read with one 16-byte load (U16: raw and row_stride_bytes multiples of 16) or
 *            with 4-byte loads (RAW10, RAW12: raw and row_stride_bytes multiples of 4); every other sample -- the halo columns, a
 *            row's tail, or all of them when the address or the stride is not such a multiple -- is read byte by byte
 *   stores   16 bytes (4 pixels of a row of a plane) at a time where W % 4 == 0 and out is 16-byte aligned, per pixel otherwise
 * Both choices are made per launch from the arguments alone and give the same bytes.  Nothing outside out's 3 N H W floats is written,
 * raw is not written, and no byte of a row behind its sesrq_sensor_row_bytes(fmt, W) is read (stride padding never affects a result). */
int sesrq_demosaic_raw(const sesrq_sensor_format *fmt, const void *raw, size_t row_stride_bytes, int method, float *out, int N, int H,
                       int W, void *stream);

/* spread: device (N, 3, H, W) fp32, 4-byte aligned, a frame of CFA order `cfa` (SESRQ_CFA_*); out, N, H, W, stream and the return as
 * above (any H, W >= 2).  Segments of 8 pixels are read with 16-byte loads of the two planes that have sites in the row where W % 4 == 0
 * and spread is 16-byte aligned, per sample otherwise; a loaded value that is not its pixel's site sample is discarded unseen.  spread
 * is not written; out must not overlap it. */
int sesrq_demosaic_spread(int cfa, const float *spread, int method, float *out, int N, int H, int W, void *stream);

/* The kernel instantiations the two entries can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_demosaic_instance_count(void);
const char *sesrq_demosaic_instance_name(int i);
long long sesrq_demosaic_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_demosaic_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
