/* sesrq_sensor.h -- Bayer raw frames as sensors deliver them into the 3-channel nets (MFLAG 1-4): any of the four CFA orders, a black
 * pedestal and a white level of up to 16 bits, in 16-bit containers or MIPI CSI-2 packed (RAW10, RAW12).
 *
 * A library of its own (libsesrq_sensor.so): it links nothing of libsesrq.so or libsesrq_raw.so, whose ABIs are unchanged.  Its output
 * q0 is the int8 input of sesrq_forward (SESRQ_I8 with i8_in_scale = 0).  At (SESRQ_CFA_RGGB, 0, 4095, SESRQ_PACK_U16) every output
 * byte is the one sesrq_raw_unpack (include/sesrq_raw.h) writes.
 *
 * Per pixel (y, x) of frame n, with code v (the 10-, 12- or 16-bit value the packing holds at that pixel), D = white - black and the
 * global row / column parity (y & 1, x & 1):
 *   site channel  the CFA order's channel at that parity (table below); the two other channels are non-sites
 *   d(v)          = min(max(v, black), white) - black                    0 .. D
 *   x(v)          = clamp(fl32(d) / fl32(D), 0, 1)                        a true IEEE fp32 quotient
 *   q0(v)         = clamp8(rint(fl(fl(x / s0) + z0)))                    exact_div 0 / 1: the true quotient; 2: x * fl(1 / s0)
 *   spread        = x(v) at the site channel, 0.0f at the non-sites
 *   q0 plane      = q0(v) at the site channel, q0 of x = 0.0f at the non-sites
 *
 * Packing (MIPI CSI-2, a row is a whole number of groups):
 *   RAW10   4 pixels in 5 bytes: bytes 0..3 = P0..P3[9:2], byte 4 = P3[1:0] << 6 | P2[1:0] << 4 | P1[1:0] << 2 | P0[1:0]
 *   RAW12   2 pixels in 3 bytes: bytes 0, 1 = P0[11:4], P1[11:4], byte 2 = P1[3:0] << 4 | P0[3:0]
 *   U16     one little-endian uint16 per pixel */
#ifndef SESRQ_SENSOR_H
#define SESRQ_SENSOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* site channel (0 R, 1 G, 2 B) of the parities (0,0) (0,1) (1,0) (1,1):  RGGB {0,1,1,2}  GRBG {1,0,2,1}  GBRG {1,2,0,1}  BGGR {2,1,1,0} */
enum { SESRQ_CFA_RGGB, SESRQ_CFA_GRBG, SESRQ_CFA_GBRG, SESRQ_CFA_BGGR };
enum { SESRQ_PACK_U16, SESRQ_PACK_RAW10, SESRQ_PACK_RAW12 };

/* Valid when cfa and packing are enumerators above, 0 <= black < white <= 65535, and white <= 1023 (RAW10) / 4095 (RAW12). */
typedef struct { int32_t cfa, black, white, packing; } sesrq_sensor_format;

typedef struct sesrq_sensor_ctx_s *sesrq_sensor_ctx;

/* Bytes of a row of W pixels without padding: 2 W (U16), 5 W / 4 (RAW10, W % 4 == 0), 3 W / 2 (RAW12, W % 2 == 0).  0, with
 * sesrq_sensor_last_error() set, for an invalid format, W < 1 or a W that is not a whole number of pack groups. */
size_t sesrq_sensor_row_bytes(const sesrq_sensor_format *fmt, int W);

/* q0 of every d = 0 .. white - black (host only, no device needed); entries must be white - black + 1.  scale_in =
 * f32(input.0.scale) > 0, zero_in = input.0.zero, exact_div as sesrq_options.exact_div.  The table is monotone non-decreasing.
 * 0 on success, non-zero with sesrq_sensor_last_error() set otherwise. */
int sesrq_sensor_table(const sesrq_sensor_format *fmt, float scale_in, int zero_in, int exact_div, int8_t *table, size_t entries);

/* Build the q0 map of one (format, input domain) and upload it to the CURRENT device once (synchronous): the table itself where it has
 * at most 4096 entries, else its steps (below).  *ctx is released with sesrq_sensor_destroy. */
int sesrq_sensor_create(const sesrq_sensor_format *fmt, float scale_in, int zero_in, int exact_div, sesrq_sensor_ctx *ctx);
void sesrq_sensor_destroy(sesrq_sensor_ctx ctx);

/* raw: device, N frames of H rows; row y of frame n starts at raw + (n H + y) row_stride_bytes and holds sesrq_sensor_row_bytes(fmt, W)
 * bytes of pixels, then padding.  q0: device (N, 3, H, W) int8 or NULL; spread: device (N, 3, H, W) fp32 or NULL (not both NULL).
 * Any N, H, W >= 1 that the packing allows (RAW10: W % 4 == 0, RAW12: W % 2 == 0; odd H and W are legal for U16) and any
 * row_stride_bytes >= the row's bytes.  One kernel enqueued on `stream` (a hipStream_t; NULL = the default stream); no allocation, no
 * synchronisation.  The context's device must be current.  Every argument is checked before any HIP call; 0 on success, non-zero with
 * sesrq_sensor_last_error() set otherwise.
 *
 * The q0 map.  Formats of at most 4096 levels (D <= 4095, so every packed format): the table, staged in LDS per workgroup, one lookup
 * per pixel.  Deeper formats: q0 is monotone in d with at most 255 unit steps, so the context keeps the sorted d at which each step is
 * taken (1 KiB in LDS) and q0(d) = q0(0) + #{steps <= d}, an 8-probe search; it returns the table's byte for every d.
 *
 * Caller buffers.  raw may start at any address and row_stride_bytes may be any value >= the row's bytes; q0 may start at any
 * address, spread at any 4-byte aligned one.  The kernel works on segments of S pixels: S = 8 for U16 (16 bytes), S = 16 for RAW10
 * (20 bytes) and RAW12 (24 bytes):
 *   loads    a whole segment is read with one 16-byte load (U16: raw and row_stride_bytes multiples of 16) or with 4-byte loads
 *            (RAW10, RAW12: raw and row_stride_bytes multiples of 4); every other segment -- a row's tail of fewer than S pixels, or
 *            any segment when the address or the stride is not such a multiple -- is read byte by byte
 *   stores   S bytes of q0 and 16 bytes of spread at a time where W % S == 0, q0 is S-byte and spread 16-byte aligned (those given);
 *            per pixel otherwise
 * Both choices are made per launch from the arguments alone and give the same bytes.  Nothing outside [q0, q0 + 3 N H W) and [spread,
 * spread + 3 N H W floats) is written, raw is not written, no byte of a row behind its sesrq_sensor_row_bytes(fmt, W) is read (stride
 * padding never affects a result), and there is no workspace (tests/test_sensor_buffers.py).
 * One launch takes N H ceil(W / S) segments, 256 per workgroup, with at most 8 workgroups per compute unit looping over them. */
int sesrq_sensor_unpack(sesrq_sensor_ctx ctx, const void *raw, size_t row_stride_bytes, int8_t *q0, float *spread, int N, int H, int W,
                        void *stream);

/* The kernel instantiations sesrq_sensor_unpack can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_sensor_instance_count(void);
const char *sesrq_sensor_instance_name(int i);
long long sesrq_sensor_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_sensor_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
