/* sesrq_raw.h -- 12-bit RGGB Bayer raw frames into the 3-channel nets (MFLAG 1-4): the input side of the reference's evaluation loop
 * (self_dataset.py TestDataset: a uint16 raw frame spread into a sparse 3-channel RGGB mosaic, / (2^12 - 1) in fp32, clamp to [0, 1]).
 *
 * A library of its own (libsesrq_raw.so): it does not link libsesrq.so, and libsesrq.so's ABI (include/sesrq.h) is unchanged.  Its
 * output q0 is the int8 input of sesrq_forward (SESRQ_I8 with i8_in_scale = 0).
 *
 * Per pixel (y, x) of frame n, with code v = raw[n][y][x] (uint16) and the global row / column parity (y & 1, x & 1):
 *   site channel  (0, 0) -> R (0), (0, 1) and (1, 0) -> G (1), (1, 1) -> B (2); the two other channels are non-sites
 *   x(v)          = clamp(fl32(min(v, 4095)) / 4095.0f, 0, 1)           a true IEEE fp32 quotient (codes >= 4095 give 1.0)
 *   q0(v)         = clamp8(rint(fl(fl(x / s0) + z0)))                  exact_div 0 / 1: the true quotient; 2: x * fl(1 / s0)
 *   spread        = x(v) at the site channel, 0.0f at the non-sites    the reference's `inp`, bit for bit
 *   q0 plane      = q0(v) at the site channel, q0(0) at the non-sites  the reference's input.0 of that `inp` */
#ifndef SESRQ_RAW_H
#define SESRQ_RAW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SESRQ_RAW_CODES 4096

typedef struct sesrq_raw_ctx_s *sesrq_raw_ctx;

/* q0 of every code 0 .. 4095 (host only, no device needed).  scale_in = f32(input.0.scale) > 0, zero_in = input.0.zero,
 * exact_div as sesrq_options.exact_div.  0 on success, non-zero with sesrq_raw_last_error() set otherwise. */
int sesrq_raw_table(float scale_in, int zero_in, int exact_div, int8_t table[SESRQ_RAW_CODES]);

/* Build the table and upload it to the CURRENT device once (synchronous).  *ctx is released with sesrq_raw_destroy. */
int sesrq_raw_create(float scale_in, int zero_in, int exact_div, sesrq_raw_ctx *ctx);
void sesrq_raw_destroy(sesrq_raw_ctx ctx);

/* raw: device (N, H, W) uint16; q0: device (N, 3, H, W) int8 or NULL; spread: device (N, 3, H, W) fp32 or NULL (not both NULL).
 * Any N, H, W >= 1.  One kernel enqueued on `stream` (a hipStream_t; NULL = the default stream); no allocation, no synchronisation.
 * The context's device must be current.  Arguments are checked before any HIP call; 0 on success, non-zero with
 * sesrq_raw_last_error() set otherwise. */
/* Caller buffers: raw may start at any 2-byte aligned address, q0 at any address, spread at any 4-byte aligned one.  The kernel takes
 * its 16-byte path only where W % 8 == 0 and raw, q0 (8 bytes) and spread happen to be aligned for it, per launch; otherwise the
 * per-pixel path gives the same bytes.  Nothing outside [q0, q0 + 3 N H W) and [spread, spread + 3 N H W floats) is written, raw is not
 * written, nothing outside raw's N H W codes affects the result, and there is no workspace (tests/test_caller_buffers.py). */
int sesrq_raw_unpack(sesrq_raw_ctx ctx, const uint16_t *raw, int8_t *q0, float *spread, int N, int H, int W, void *stream);

/* The kernel instantiations sesrq_raw_unpack can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_raw_instance_count(void);
const char *sesrq_raw_instance_name(int i);
long long sesrq_raw_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_raw_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
