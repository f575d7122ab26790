/* sesrq_noise.h -- shot and read noise on Bayer raw frames, fused into their unpack: the reference's TEST_RAW_ADD_NOISE
 * (self_dataset.py random_noise_levels / add_noise on TestDataset's sparse 3-channel frame, before its clamp).
 *
 * A library of its own (libsesrq_noise.so): it links nothing of libsesrq.so or of the other side libraries.  It takes the raw frames
 * libsesrq_sensor.so takes (include/sesrq_sensor.h: format, packing, row stride) and writes the same two outputs, q0 -- the int8 input
 * of sesrq_forward (SESRQ_I8 with i8_in_scale = 0) -- and the fp32 frame, of the NOISY frame.  The noise is a counter-based stream: a
 * sample is a function of (seed, frame number, y, x, channel) alone, whatever the batch, packing, stride, alignment or launch shape.
 * The reference draws from torch's CPU generator, so its individual samples cannot be reproduced; its arithmetic (below, "combine") and
 * its distribution are what is pinned.
 *
 * Per pixel (y, x) of frame n, with the global frame number f = frame0 + n (64-bit, wrapping):
 *
 *   words     (w0, w1, w2, w3) = Philox4x32-10(counter = (x, y, lo32(f), hi32(f)), key = (lo32(seed), hi32(seed)))
 *             the Random123 generator: multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on word 2), Weyl constants
 *             0x9E3779B9 / 0xBB67AE85 added to the key words before rounds 2 .. 10; per round
 *             (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
 *   uniforms  u_r(w) = ((w >> 9) + 0.5) * 2^-23   in [2^-24, 1 - 2^-24]      u_t(w) = (w >> 8) * 2^-24   in [0, 1)      exact in fp32
 *   deviates  rho_a = sqrtf(-2 logf(u_r(w0)))   rho_b = sqrtf(-2 logf(u_r(w2)))                       (Box-Muller)
 *             z[0] = rho_a cospi(2 u_t(w1))   z[1] = rho_a sinpi(2 u_t(w1))   z[2] = rho_b cospi(2 u_t(w3))     one per channel
 *             The arguments 2 u_t are exact; logf, sqrtf, sincospif and cospif are the accurate device functions, each product one
 *             fp32 multiply.  u_r >= 2^-24 truncates the normal at |z| <= sqrt(48 ln 2) = 5.77 (a tail mass of 8e-9).
 *   clean     x_c = fl32(d) / fl32(white - black) at the site channel with d = min(max(code, black), white) - black, exactly as
 *             sesrq_sensor.h forms it; 0.0f at the two non-sites
 *   combine   v = fl(fl(x_c * shot) + read)   sigma = sqrtf(v)   y = fl(x_c + fl(sigma * z[c]))        each step one IEEE fp32 operation
 *             spread = min(max(y, 0), 1)      non-sites get read noise too: the noise goes onto the whole 3-channel frame
 *             The clamp is fminf(fmaxf(y, 0), 1), so the frame never holds a NaN: where sigma is infinite (levels near FLT_MAX) and
 *             z[c] is exactly 0, y = x_c + inf * 0 is a NaN and spread is 0.
 *   quantise  q0 = clamp8(rint(fl(fl(spread / s0) + z0)))    exact_div 0 / 1: the true fp32 quotient; 2: spread * fl(1 / s0)
 *             the input quantiser of sesrq_forward applied to that fp32 value
 *
 * With shot = read = 0 every output byte is the one sesrq_sensor_unpack writes. */
#ifndef SESRQ_NOISE_H
#define SESRQ_NOISE_H

#include <stddef.h>
#include <stdint.h>

#include "sesrq_sensor.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sesrq_noise_ctx_s *sesrq_noise_ctx;

/* One (format, input domain) on the CURRENT device.  fmt == NULL: the reference's format (SESRQ_CFA_RGGB, 0, 4095, SESRQ_PACK_U16);
 * otherwise valid as sesrq_sensor_format says.  scale_in = f32(input.0.scale) > 0, zero_in = input.0.zero, exact_div as
 * sesrq_options.exact_div.  Nothing is allocated on the device.  0 on success, non-zero with sesrq_noise_last_error() set otherwise. */
int sesrq_noise_create(const sesrq_sensor_format *fmt, float scale_in, int zero_in, int exact_div, sesrq_noise_ctx *ctx);
void sesrq_noise_destroy(sesrq_noise_ctx ctx);

/* raw, row_stride_bytes, q0, spread, N, H, W: as sesrq_sensor_unpack takes them (q0 and spread may each be NULL, not both).
 * shot, read: the levels of every frame; levels: NULL, or a device array of N (shot, read) float pairs, 4-byte aligned, that replaces
 * the two scalars frame by frame.  seed and frame0 select the stream (above).
 *
 * One kernel enqueued on `stream` (a hipStream_t; NULL = the default stream); no allocation, no synchronisation.  The context's device
 * must be current.  Refused before any HIP call: without `levels`, a scalar level that is negative, NaN or infinite; a W that is not a
 * whole number of pack groups (RAW10: W % 4, RAW12: W % 2); a row stride below the row's bytes; a frame of more segments than one
 * launch takes (the limit of sesrq_sensor_unpack).  The values of a device `levels` array cannot be checked on the host: a negative or
 * non-finite pair there gives unspecified values in that frame only.
 *
 * Caller buffers: the contract of sesrq_sensor_unpack.  raw at any address with any row_stride_bytes >= the row's bytes; q0 at any
 * address, spread at any 4-byte aligned one.  Segments of S pixels (8 for U16, 16 for RAW10 / RAW12) are loaded whole where raw and
 * the stride are multiples of 16 (U16) / 4 (packed) and byte by byte otherwise, and stored S bytes of q0 / 16 bytes of spread at a
 * time where W % S == 0, q0 is S-byte and spread 16-byte aligned, per pixel otherwise; both choices give the same bytes.  Nothing
 * outside [q0, q0 + 3 N H W) and [spread, spread + 3 N H W floats) is written, raw and levels are not written, no byte of a row behind
 * its sesrq_sensor_row_bytes(fmt, W) is read, and there is no workspace. */
int sesrq_noise_unpack(sesrq_noise_ctx ctx, const void *raw, size_t row_stride_bytes, int8_t *q0, float *spread, int N, int H, int W,
                       float shot, float read, const float *levels, uint64_t seed, uint64_t frame0, void *stream);

/* The deviates alone: z (device, 4-byte aligned, (N, 3, H, W) fp32) = z[c] of pixel (y, x) of frame frame0 + n, from the device
 * function sesrq_noise_unpack calls -- a reproducible device normal source.  One kernel on `stream`; no allocation, no
 * synchronisation; N, H, W >= 1 with N H W < 2^31. */
int sesrq_noise_deviates(float *z, int N, int H, int W, uint64_t seed, uint64_t frame0, void *stream);

/* The kernel instantiations of this library (a fixed set), and how often each has been launched in this process. */
int sesrq_noise_instance_count(void);
const char *sesrq_noise_instance_name(int i);
long long sesrq_noise_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_noise_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
