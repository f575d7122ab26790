/* sesrq_image.h -- 8-bit images into and out of the super-resolution nets (MFLAG 5 / 6): the image side of the reference's
 * evaluation loop (self_dataset_sr.py TestDataset: a uint8 image / 255 in float64, luma for MFLAG 5; sim.py's PNG export:
 * clip to [0, 1], * 255 in fp32, truncate to uint8).
 *
 * A library of its own (libsesrq_image.so): it does not link libsesrq.so, and libsesrq.so's ABI (include/sesrq.h) is unchanged.  The
 * decoded q0 is the int8 input of sesrq_forward (SESRQ_I8 with i8_in_scale = 0).
 *
 * Images are interleaved (N, H, W, 3) uint8, RGB or BGR byte order.  With d(v) = v / 255.0 in IEEE float64 (correctly rounded):
 *   SESRQ_IMAGE_Y   (1 plane):  s = ((65.481 d(R) + 128.553 d(G)) + 24.966 d(B)) + 16.0, y = s / 255.0, clip to [0, 1] -- float64,
 *                               in this order, no fused multiply-add; x = fl32(y)
 *   SESRQ_IMAGE_RGB (3 planes): x_c = clip(fl32(d(v_c)), 0, 1)
 *   q0 = clamp8(rint(fl(fl(x / s0) + z0)))   exact_div 0 / 1: the true fp32 quotient; 2: x * fl(1 / s0) -- sesrq_forward's quantiser
 * Export, prediction p (N, C, H, W) fp32, or int8 dequantised as sesrq_forward forms out_f: p = fl((q - zero) * scale):
 *   u = trunc(fl32(clip(p, 0, 1) * 255.0f)), written interleaved (N, H, W, C), C = 1 or 3 (RGB or BGR byte order). */
#ifndef SESRQ_IMAGE_H
#define SESRQ_IMAGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_IMAGE_Y = 0, SESRQ_IMAGE_RGB = 1 };          /* decode form */
enum { SESRQ_IMAGE_ORDER_RGB = 0, SESRQ_IMAGE_ORDER_BGR = 1 };
enum { SESRQ_IMAGE_F32 = 0, SESRQ_IMAGE_I8 = 1 };          /* export prediction dtype */

#define SESRQ_IMAGE_CODES 256

typedef struct sesrq_image_ctx_s *sesrq_image_ctx;

/* The RGB form of every byte code 0 .. 255 (host only, no device needed): x[v] = clip(fl32(v / 255.0), 0, 1) and its q0.
 * scale_in = f32(input.0.scale) > 0, zero_in = input.0.zero, exact_div as sesrq_options.exact_div.  0 on success, non-zero with
 * sesrq_image_last_error() set otherwise. */
int sesrq_image_table(float scale_in, int zero_in, int exact_div, int8_t q[SESRQ_IMAGE_CODES], float x[SESRQ_IMAGE_CODES]);

/* Build the tables and upload them to the CURRENT device once (synchronous).  *ctx is released with sesrq_image_destroy. */
int sesrq_image_create(float scale_in, int zero_in, int exact_div, sesrq_image_ctx *ctx);
void sesrq_image_destroy(sesrq_image_ctx ctx);

/* img: device (N, H, W, 3) uint8 in `order`; q0: device (N, C, H, W) int8 or NULL; x: device (N, C, H, W) fp32 or NULL (not both
 * NULL); C = 1 for SESRQ_IMAGE_Y, 3 for SESRQ_IMAGE_RGB.  Any N, H, W >= 1.  One kernel enqueued on `stream` (a hipStream_t; NULL =
 * the default stream); no allocation, no synchronisation.  The context's device must be current.  Arguments are checked before any
 * HIP call; 0 on success, non-zero with sesrq_image_last_error() set otherwise. */
/* Caller buffers of decode: img and q0 may start at any address, x at any 4-byte aligned one.  The 16-byte path is chosen per run of 16
 * pixels and per frame, only where source, q0 and x of that run happen to be 16-byte aligned (a batch whose H * W is no multiple of 16
 * mixes both paths in one launch); the per-pixel path gives the same bytes.  Nothing outside the N C H W elements of q0 and x is
 * written, img is not written, nothing outside img's N H W 3 bytes affects the result; no workspace (tests/test_caller_buffers.py). */
int sesrq_image_decode(sesrq_image_ctx ctx, const uint8_t *img, int form, int order, int8_t *q0, float *x, int N, int H, int W,
                       void *stream);

/* pred: device (N, C, H, W) fp32 (pred_dtype SESRQ_IMAGE_F32; scale / zero ignored) or int8 (SESRQ_IMAGE_I8, output domain scale > 0,
 * zero in [-128, 127]); out: device (N, H, W, C) uint8 in `order` (C = 3; ignored for C = 1).  C = 1 or 3, any N, H, W >= 1.  One
 * kernel enqueued on `stream`; no allocation, no synchronisation.  Arguments are checked before any HIP call. */
/* Caller buffers of export: pred may start at any address aligned to its element type (4 bytes for fp32, 1 for int8), out at any
 * address; the 16-byte path is chosen per run as in decode.  Nothing outside out's N H W C bytes is written, pred is not written, nothing
 * outside pred affects the result; no workspace (tests/test_caller_buffers.py). */
int sesrq_image_export(const void *pred, int pred_dtype, float scale, int zero, int C, int order, uint8_t *out, int N, int H, int W,
                       void *stream);

/* The kernel instantiations decode / export can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_image_instance_count(void);
const char *sesrq_image_instance_name(int i);
long long sesrq_image_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_image_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
