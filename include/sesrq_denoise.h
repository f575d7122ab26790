/* sesrq_denoise.h -- a classical denoiser of a Bayer frame, on the device: non-local means in the Bayer domain, its sample differences
 * scaled by the variance of the shot / read noise model of include/sesrq_noise.h.  The baseline the denoising raw nets (MFLAG 1: nr;
 * MFLAG 3, 4 on noisy frames, followed by include/sesrq_demosaic.h) are measured against, and a cleaner view of a noisy sensor frame.
 *
 * A library of its own (libsesrq_denoise.so): it links no other library of the project, and their ABIs are unchanged.  It takes the
 * format struct and the CFA / packing enumerators of include/sesrq_sensor.h.
 *
 * Everything below is fp32, each operation rounded once, no fused multiply-add; fl() marks a rounding.
 *
 * Input, one of two, exactly as sesrq_demosaic.h takes them.
 *   raw      a packed sensor frame (sesrq_sensor_format; rows row_stride_bytes apart): the sample of a pixel with code v is
 *            s = fl(fl32(d(v)) / fl32(D)), x(v) of sesrq_sensor.h, a true IEEE quotient
 *   spread   a device (N, 3, H, W) fp32 frame of CFA order cfa: s = the value at the pixel in the plane of its site channel; the two
 *            other planes' values at that pixel are never read
 * Staged sample   c = s > 0 ? fminf(s, 1) : 0        a NaN and a -0.0 give +0.0, so everything downstream is finite.
 *
 * Neighbours.  Sample (y + j, x + i) is taken at fold(y + j, H), fold(x + i, W), the reflection of sesrq_demosaic.h: fold(t, n) =
 * u < n ? u : 2 (n - 1) - u with u = t mod 2 (n - 1), 0 <= u.  Its period is even, so a neighbour stays on its CFA parity for any
 * H, W >= 2.  H < 2 or W < 2 is refused.
 *
 * Levels.  (shot, read) of a frame: the two scalars, or pair n of a device array `levels` of N pairs (as sesrq_noise_unpack takes them).
 * Per staged sample    v = fl(fl(c * shot) + read)     g = fl(1 / fmaxf(fl(2 v), 2^-100))      (one division per sample)
 *
 * Candidates of pixel p: the 49 pixels of its own colour q = p + (2 j, 2 i), |i|, |j| <= 3, visited row-major (j outer, i inner, both
 * ascending).  Per candidate, over the 5 x 5 patch |a|, |b| <= 2 (all colours take part: both patches have the same CFA layout):
 *   e(a, b) = fl(fl(d * d) * g(p + (a, b)))     d = c(p + (a, b)) - c(q + (a, b))
 *   r(a)    = (((e(a, -2) + e(a, -1)) + e(a, 0)) + e(a, 1)) + e(a, 2)
 *   Dp      = (((r(-2) + r(-1)) + r(0)) + r(1)) + r(2)
 *   t       = fmaxf(fl(Dp * 0.04f) - 1, 0)          0.04f: fl32(1 / 25), the patch mean; 1: the expectation of d^2 / (2 v) under the model
 *   k       = fmaxf(1 - fl(t * rh), 0)              rh = fl(1.0f / h), formed on the host
 *   w       = fl(k * k)                             the centre candidate (i = j = 0) has w = 1
 * The row sums first, then their sum: the direct 25 terms and a separable evaluation in which neighbouring pixels share e and r give the
 * same bits.  (A sliding column sum that adds a new term and subtracts an old one would not.)  fmaxf returns its other operand for a NaN.
 *
 * Output.  num = sum of fl(w * c(q)), den = sum of w, both from 0.0f in candidate order; out = fl(num / den), a true quotient, in
 * [0, 1].  out is a spread frame (N, 3, H, W) fp32: the denoised sample in the plane of the pixel's site channel, +0.0f in the two
 * others -- the layout quality.score(., ., 1), sesrq_demosaic_spread and the nets' fp32 input take.
 *
 * h is the filter's strength, a knob: weights reach 0 where the mean scaled squared difference exceeds 1 + h.  1.0 is a sound default:
 * on a 96 x 128 synthetic RGGB frame (a smooth sinusoid times 16 x 24 blocks, per-colour gains) at levels (0.01, 5e-4), (0.002, 1e-5),
 * (0, 1e-3) a numpy prototype of this arithmetic went from 23.7 / 31.1 / 29.9 dB (noisy) to 30.2 / 36.4 / 35.4 dB at h = 1; a search
 * radius of 4 instead of 3 bought less than 0.25 dB. */
#ifndef SESRQ_DENOISE_H
#define SESRQ_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#include "sesrq_sensor.h"

#ifdef __cplusplus
extern "C" {
#endif

/* raw: device, N frames of H rows in `fmt` (valid as sesrq_sensor.h says); row y of frame n starts at raw + (n H + y) row_stride_bytes
 * and holds sesrq_sensor_row_bytes(fmt, W) bytes of pixels, then padding.  shot, read: the levels of every frame; levels: NULL, or a
 * device array of N (shot, read) float pairs, 4-byte aligned, that replaces the two scalars frame by frame.  h: the strength.
 * out: device (N, 3, H, W) fp32.  Any N >= 1, H, W >= 2 that the packing allows (RAW10: W % 4 == 0, RAW12: W % 2 == 0; odd H and W are
 * legal for U16) with H, W <= 2^31 - 129 and at most 2^31 - 1 tiles of 64 x 32 pixels in the batch; offsets are 64-bit, so a batch may
 * cross 4 GiB.  One kernel enqueued on `stream` (a hipStream_t; NULL = the default stream) of the current device; no allocation, no
 * synchronisation, no workspace, no context.  Every argument is checked before any HIP call; 0 on success, non-zero with
 * sesrq_denoise_last_error() set otherwise.  Refused: without `levels`, a scalar level that is negative, NaN or infinite; an h that
 * is not finite or not positive.  The values of a device `levels` array cannot be checked on the host: a negative or non-finite pair
 * there gives unspecified values in that frame only.
 *
 * Caller buffers.  raw may start at any address and row_stride_bytes may be any value >= the row's bytes; out at any 4-byte aligned
 * address; out must not overlap the input.  A workgroup stages its 64 x 32 tile and a halo of 8 samples in segments of 8 (U16) or 16
 * (RAW10, RAW12) pixels.  One of two paths is chosen per launch from the arguments alone, and both give the same bytes:
 *   wide         where raw and row_stride_bytes are multiples of 16 (U16) / 4 (RAW10, RAW12), W % 4 == 0 and out is 16-byte aligned: a
 *                segment that lies whole inside its row is read with one 16-byte load (U16) or with 4-byte loads (packed), every other
 *                sample (a row's tail, the halo columns of a packed frame, what the fold brings in) byte by byte; out is written 16 bytes
 *                (4 pixels of a row of a plane) at a time
 *   per sample   otherwise: every sample is read byte by byte and every float of out written on its own
 * Nothing outside out's 3 N H W floats is written, raw and levels are not written, and no byte of a row behind its
 * sesrq_sensor_row_bytes(fmt, W) is read (stride padding never affects a result). */
int sesrq_denoise_raw(const sesrq_sensor_format *fmt, const void *raw, size_t row_stride_bytes, float shot, float read,
                      const float *levels, float h, float *out, int N, int H, int W, void *stream);

/* spread: device (N, 3, H, W) fp32, 4-byte aligned, a frame of CFA order `cfa` (SESRQ_CFA_*); everything else as above (any H, W >= 2).
 * The wide path (W % 4 == 0, spread and out 16-byte aligned) reads segments of 8 pixels with 16-byte loads of the two planes that
 * have sites in the row; a loaded value that is not its pixel's site sample is discarded unseen.  spread is not written. */
int sesrq_denoise_spread(int cfa, const float *spread, float shot, float read, const float *levels, float h, float *out, int N, int H,
                         int W, void *stream);

/* The kernel instantiations the two entries can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_denoise_instance_count(void);
const char *sesrq_denoise_instance_name(int i);
long long sesrq_denoise_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_denoise_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
