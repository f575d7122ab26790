/* sesrq_resize.h -- predictions out at any size: the nets' output (or any 8-bit image) resampled bicubically to Ho x Wo and written
 * as bytes, one kernel.  The arithmetic is Pillow's Image.resize(size, Image.BICUBIC) on 8-bit images (libImaging/Resample.c), over
 * the whole image including the edges; every byte equals Pillow's.
 *
 * A library of its own (libsesrq_resize.so): it does not link libsesrq.so, and libsesrq.so's ABI (include/sesrq.h) is unchanged.
 *
 * 1. Source byte.  SESRQ_RESIZE_U8: an interleaved (N, H, W, C) uint8 image in RGB order, taken as it is.  SESRQ_RESIZE_F32 / _I8: a
 *    prediction (N, C, H, W), fp32 or int8 dequantised as sesrq_forward forms out_f, p = fl((q - zero) * scale); its byte is
 *    u = trunc(fl32(clip(p, 0, 1) * 255.0f)), a NaN gives 0 -- the byte sesrq_image_export writes.
 * 2. Coefficients of one axis n_in -> n_out, on the host in IEEE double, in this order (no fused multiply-add):
 *      scale = n_in / n_out; fs = max(scale, 1); support = 2 fs; ss = 1 / fs
 *      output i: c = (i + 0.5) scale; xmin = max((int)(c - support + 0.5), 0); xmax = min((int)(c + support + 0.5), n_in)
 *      w_x = K((x + xmin - c + 0.5) ss), x = 0 .. xmax - xmin - 1, K the Keys cubic with a = -1/2:
 *            |t| < 1: ((a + 2) |t| - (a + 3)) |t| |t| + 1;  |t| < 2: (((|t| - 5) |t| + 8) |t| - 4) a;  else 0
 *      ww = sum of w_x in index order; k_x = w_x / ww; weight = (int)(k_x 2^22 - 0.5) for k_x < 0, (int)(k_x 2^22 + 0.5) otherwise
 *    (Pillow multiplies by ss where one might divide by fs; the product is what is specified here.)
 * 3. Passes, horizontal first, then vertical.  Per pass acc = 2^21 + sum of weight * byte in int32 and the byte is
 *    clamp(acc >> 22, 0, 255), >> arithmetic.  A uint8 sits between the passes: the horizontal pass is clamped too.  n_in == n_out
 *    gives the identity table (one weight 2^22 at offset i - xmin), so that pass returns its input.
 * 4. Output: interleaved (N, Ho, Wo, C) uint8, C = 1 or 3; output byte c of a pixel comes from source channel c (RGB) or 2 - c (BGR). */
#ifndef SESRQ_RESIZE_H
#define SESRQ_RESIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_RESIZE_U8 = 0, SESRQ_RESIZE_F32 = 1, SESRQ_RESIZE_I8 = 2 };      /* source dtype */
enum { SESRQ_RESIZE_ORDER_RGB = 0, SESRQ_RESIZE_ORDER_BGR = 1 };

#define SESRQ_RESIZE_MAX_TAPS 17          /* 2 ceil(2 * 4) + 1: the taps of a row at the steepest accepted downscale */
#define SESRQ_RESIZE_MAX_RATIO 4          /* n_in / n_out of a downscale; upscales are unbounded */
#define SESRQ_RESIZE_BITS 22

typedef struct sesrq_resize_ctx_s *sesrq_resize_ctx;

/* The table of one axis (host only, no device needed): xmin[i], count[i] = xmax - xmin and weights[i * SESRQ_RESIZE_MAX_TAPS + x],
 * x < count[i] (the rest 0), for i = 0 .. n_out - 1.  Refuses n_in < 1, n_out < 1, n_in > SESRQ_RESIZE_MAX_RATIO * n_out and any row
 * with 255 * sum |weight| + 2^21 >= 2^31 (the int32 accumulator of a pass is then exact for every image; checked, not assumed).
 * 0 on success, non-zero with sesrq_resize_last_error() set otherwise. */
int sesrq_resize_coeffs(int n_in, int n_out, int32_t *xmin, int32_t *count, int32_t *weights);

/* Build the tables of H x W -> Ho x Wo, upload them to the CURRENT device once (synchronous) and pick the launch geometry: the
 * tallest output tile (64, 32 or 16 rows of 192 output bytes) whose worst source window fits the kernel's LDS.  Refuses what
 * sesrq_resize_coeffs refuses of either axis, before any HIP call.  *ctx is released with sesrq_resize_destroy. */
int sesrq_resize_create(int H, int W, int Ho, int Wo, sesrq_resize_ctx *ctx);
void sesrq_resize_destroy(sesrq_resize_ctx ctx);

/* The output tile of a context in pixels: *tile_w for C = 1 (a third of it for C = 3), *tile_h rows.  0 on success. */
int sesrq_resize_tile(sesrq_resize_ctx ctx, int *tile_w, int *tile_h);

/* src: device, (N, H, W, C) uint8 (SESRQ_RESIZE_U8; scale / zero ignored), (N, C, H, W) fp32 (SESRQ_RESIZE_F32; scale / zero ignored)
 * or (N, C, H, W) int8 (SESRQ_RESIZE_I8, output domain scale > 0, zero in [-128, 127]); out: device (N, Ho, Wo, C) uint8 in `order`
 * (C = 3; ignored for C = 1).  H, W, Ho, Wo must be the context's.  One kernel enqueued on `stream` (a hipStream_t; NULL = the
 * default stream); no allocation, no synchronisation; no intermediate plane and no full-size byte image reaches memory.  The
 * context's device must be current.  Arguments are checked before any HIP call; 0 on success, non-zero with
 * sesrq_resize_last_error() set otherwise. */
/* Caller buffers: src may start at any address aligned to its element type (4 bytes for fp32, 1 otherwise), out at any address.  Whole
 * aligned 32-bit words of a byte source are loaded as such, the rest by bytes; 16-byte stores are chosen per run of 16 output bytes,
 * only where the run is whole and happens to be 16-byte aligned.  Nothing outside out's N Ho Wo C bytes is written, src is not
 * written, nothing outside src is read; no workspace.  Frame bases are formed in 64 bits. */
int sesrq_resize_run(sesrq_resize_ctx ctx, const void *src, int src_dtype, float scale, int zero, int C, int order, uint8_t *out, int N,
                     int H, int W, int Ho, int Wo, void *stream);

/* The kernel instantiations run can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_resize_instance_count(void);
const char *sesrq_resize_instance_name(int i);
long long sesrq_resize_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_resize_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
