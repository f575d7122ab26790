/* sesrq_downscale.h -- the super-resolution nets' input from the HR image: a bicubic x2 / x4 downscale of the 8-bit ground truth, fused
 * with the decode of sesrq_image.h into the net's q0 / fp32 input -- one kernel, and the LR image need never exist in memory.  The
 * reference's dataset (self_dataset_sr.py) reads a pre-made LR file (LRbicx4 / LRbicx2: MATLAB imresize(img, 1 / r, 'bicubic') of the
 * mod-12-cropped HR image) next to the HR one; this header fixes the arithmetic that stands for that step here, and
 * tests/downscale_oracle.py restates it in numpy.
 *
 * A library of its own (libsesrq_downscale.so): it links nothing of libsesrq.so, libsesrq_image.so or libsesrq_colour.so.
 *
 * img is (N, H, W, 3) uint8, interleaved, in `order` (RGB or BGR); r is 2 or 4; H % r == 0 and W % r == 0 (crop first: "modcrop");
 * the LR image is (N, H / r, W / r, 3) uint8 in the same order.
 *
 * 1. The kernel: Keys, a = -1/2, stretched by r (antialiased), half-pixel centres, separable; the VERTICAL pass first, then the
 *    horizontal one.  Output index d along an axis of length n takes the 4 r taps j = r d - 3 r / 2 + k, k = 0 .. 4 r - 1, with the
 *    integer weights w[k] / D -- the exact values of Keys((j - c) / r) / r * D, c = r d + (r - 1) / 2; symmetric; each row sums to D:
 *      r = 2   -3 -9 29 111 111 29 -9 -3                                                  D = 256
 *      r = 4   -7 -45 -75 -49 93 399 745 987 987 745 399 93 -49 -75 -45 -7                D = 4096
 * 2. Edges: an index outside the frame is mirrored with the edge sample repeated: with p = 2 n and i = j mod p (non-negative), sample
 *    i if i < n, else p - 1 - i.  This holds for any n >= r, frames narrower than the kernel included.
 * 3. Each pass is clamp(floor((sum w v + D / 2) / D), 0, 255) and writes a uint8 intermediate (an arithmetic shift, which floors
 *    negative sums as well).  Every sum fits int32: the largest is 255 * 4448 at r = 4.
 * 4. Decode of the LR bytes: exactly sesrq_image.h's -- SESRQ_IMAGE_RGB: x_c = clip(fl32(v / 255.0), 0, 1); SESRQ_IMAGE_Y: the float64
 *    luma line, unfused; q0 = clamp8(rint(fl(fl(x / s0) + z0))), exact_div 0 / 1 / 2 as there.  Both libraries instantiate one device
 *    body (csrc/sesrq_image_decode.h).
 *
 * What this is meant to reproduce, and what pins it.  Two passes with a saturating round to uint8 between them, the pass order for
 * equal scales and the mirrored indices are the published algorithm of MATLAB's imresize on uint8 input, and the INTENT is its
 * imresize(img, 1 / r, 'bicubic').  That is intent, not a pinned fact: no MATLAB output and none of the datasets' LR files have been
 * compared.  The one outside anchor is PIL: Image.resize(BICUBIC) of the transposed image (PIL runs the horizontal pass first) equals
 * this arithmetic on every LR pixel whose taps lie inside the frame (tests/test_downscale_oracle.py); at the border PIL truncates and
 * renormalises its kernel, so there only the numpy restatement pins the bytes. */
#ifndef SESRQ_DOWNSCALE_H
#define SESRQ_DOWNSCALE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_DOWNSCALE_Y = 0, SESRQ_DOWNSCALE_RGB = 1 };          /* decode form: SESRQ_IMAGE_Y / SESRQ_IMAGE_RGB */
enum { SESRQ_DOWNSCALE_ORDER_RGB = 0, SESRQ_DOWNSCALE_ORDER_BGR = 1 };

/* The kernel's tile: a workgroup owns TILE_HR_W x TILE_HR_H HR pixels at either r, that is TILE_W x TILE_H LR pixels at r = 4 and twice
 * that each way (64 x 16) at r = 2, and stages them with the 3 r / 2 HR pixels its taps reach on every side.  Exported so that tests
 * can place frames on the seams. */
#define SESRQ_DOWNSCALE_TILE_HR_W 128
#define SESRQ_DOWNSCALE_TILE_HR_H 32
#define SESRQ_DOWNSCALE_TILE_W 32
#define SESRQ_DOWNSCALE_TILE_H 8

typedef struct sesrq_downscale_ctx_s *sesrq_downscale_ctx;

/* The weights of step 1 (host only, no device needed): w[k], k = 0 .. 4 r - 1, and their sum D.  r = 2 or 4.  0 on success, non-zero
 * with sesrq_downscale_last_error() set otherwise. */
int sesrq_downscale_weights(int r, int16_t *w /* [4 r] */, int *D);

/* The decode tables of one input domain, as sesrq_image_create builds them, uploaded to the CURRENT device once (synchronous).
 * scale_in = f32(input.0.scale) > 0, zero_in = input.0.zero, exact_div as sesrq_options.exact_div.  Released with _destroy. */
int sesrq_downscale_create(float scale_in, int zero_in, int exact_div, sesrq_downscale_ctx *ctx);
void sesrq_downscale_destroy(sesrq_downscale_ctx ctx);

/* Steps 1 - 4 in ONE kernel enqueued on `stream` (a hipStream_t; NULL = the default stream) of the current device; no allocation, no
 * synchronisation, no workspace: neither the uint8 intermediate nor (unless asked for) the LR image reaches memory.
 * img: device (N, H, W, 3) uint8 in `order`, H and W the HR size; any non-empty subset of
 *   lr: device (N, H / r, W / r, 3) uint8 in `order`, or NULL;
 *   q0: device (N, C, H / r, W / r) int8, or NULL;      x: device (N, C, H / r, W / r) fp32, or NULL;
 * C = 1 for SESRQ_DOWNSCALE_Y, 3 for SESRQ_DOWNSCALE_RGB (planes R, G, B whatever the order).  `form` is read only when q0 or x is asked
 * for; ctx may be NULL when only lr is.  The context's device must be current.  Arguments are checked before any HIP call; 0 on
 * success, non-zero with sesrq_downscale_last_error() set otherwise; a size that is no multiple of r is refused with a message that
 * names modcrop.
 * Limits: N, H / r, W / r >= 1; H, W at most 2^31 - 1; N ceil(H / TILE_HR_H) ceil(W / TILE_HR_W) (the grid, one workgroup a tile) at most
 * 2^31 - 1.  Pixel and byte offsets are 64-bit, so no limit comes from a buffer's byte count.
 * Caller buffers: img, lr and q0 may start at any address, x at any 4-byte aligned one.  The kernel reads img in 4-byte words at
 * whatever address a tile's window starts (the hardware's unaligned access; never a word that is not wholly inside img) and single
 * bytes at a frame's borders, and stores per element, the lanes of a wave to consecutive elements; it has no 16-byte path, so no
 * alignment selects other code and there is one set of bytes.  Nothing outside lr's N (H / r) (W / r) 3 bytes and the N C (H / r) (W / r)
 * elements of q0 and x is written, img is not written, nothing outside img's N H W 3 bytes affects the result. */
int sesrq_downscale_run(sesrq_downscale_ctx ctx, const uint8_t *img, int order, int r, int form, uint8_t *lr, int8_t *q0, float *x, int N,
                        int H, int W, void *stream);

/* The kernel instantiations run can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_downscale_instance_count(void);
const char *sesrq_downscale_instance_name(int i);
long long sesrq_downscale_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_downscale_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
