/* sesrq_develop.h -- display images out of the raw nets (MFLAG 2, 3, 4: dm, nrdm_3, nrdm_6).  What these nets return is linear
 * camera RGB in [0, 1]: the reference's data comes from an unprocessing pipeline that inverts the white-balance gains and the colour
 * matrix before the net sees a frame, and its metadata2tensor (self_dataset.py) carries the metadata half of the way back (xyz2cam ->
 * row-normalised rgb2cam -> cam2rgb, red_gain, blue_gain) without ever applying it.  This is the tail of that pipeline's `process`:
 * gains, clip, 3 x 3 colour-correction matrix (CCM), tone curve, bytes -- one kernel.
 *
 * A library of its own (libsesrq_develop.so): it links no other library of the project, and their ABIs are unchanged.
 *
 * The arithmetic.  pred is (N, 3, H, W), planes R, G, B: fp32, or int8 dequantised as sesrq_forward forms out_f,
 * p = fl((q - zero) * scale).  Every step is fp32, each operation rounded once, no fused multiply-add, in this order:
 *   1. l_c = fminf(fmaxf(p_c, 0), 1)                                   a NaN gives 0, as in sesrq_image_export
 *   2. w_c = fminf(fl(l_c * g_c), 1)                                   g = (g_R, g_G, g_B): white balance, with any exposure gain folded in
 *   3. o_r = fl(fl(fl(m00 * w_R) + fl(m01 * w_G)) + fl(m02 * w_B)),    likewise o_g (m10 m11 m12) and o_b (m20 m21 m22): m row-major;
 *      o_c = fminf(fmaxf(o_c, 0), 1)
 *   4. byte_c = #{k in 1 .. 255 : o_c >= T[k]}                         T: 255 fp32 thresholds, non-decreasing -- the tone curve
 *   5. the bytes are written interleaved (N, H, W, 3) in `order` (RGB or BGR)
 * The byte of step 4 is a count of comparisons, so it is exact by construction; the kernel narrows the count with a table keyed on
 * the bits of o_c and finishes it with compares against T, and stores nothing but that count.
 *
 * T is passed as float[255] with T[k] at index k - 1.  Equal neighbours, entries <= 0 and entries > 1 are legal (they skip codes:
 * posterised or limited-range output).  The built-in tables (sesrq_develop_curve) hold the fp32 nearest to the exact preimage of
 * (k - 1/2) / 255 under the curve f, so byte = rint(255 f(o)) with exact boundaries:
 *   SESRQ_DEVELOP_GAMMA22   f(o) = max(o, 1e-8)^(1 / 2.2), the unprocessing paper's curve:  T[k] = ((k - 1/2) / 255)^(11/5)
 *   SESRQ_DEVELOP_SRGB      the piecewise sRGB OETF; with v = (k - 1/2) / 255:  T[k] = ((v + 0.055) / 1.055)^(12/5) for v > 0.04045
 *                           (k >= 11), v / 12.92 below
 *   SESRQ_DEVELOP_TRUNC255  T[k] = the smallest fp32 t with (unsigned)fl(t * 255.0f) >= k: with unit gains and the identity matrix
 *                           the output is sesrq_image_export's byte for every input */
#ifndef SESRQ_DEVELOP_H
#define SESRQ_DEVELOP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_DEVELOP_GAMMA22 = 0, SESRQ_DEVELOP_SRGB = 1, SESRQ_DEVELOP_TRUNC255 = 2 };      /* built-in tone curves */
enum { SESRQ_DEVELOP_ORDER_RGB = 0, SESRQ_DEVELOP_ORDER_BGR = 1 };
enum { SESRQ_DEVELOP_F32 = 0, SESRQ_DEVELOP_I8 = 1 };                                        /* prediction dtype */

#define SESRQ_DEVELOP_LEVELS 255

typedef struct sesrq_develop_ctx_s *sesrq_develop_ctx;

/* A built-in threshold table (host only, no device needed): T[k - 1] for k = 1 .. 255, strictly increasing.  0 on success, non-zero
 * with sesrq_develop_last_error() set otherwise. */
int sesrq_develop_curve(int kind, float T[SESRQ_DEVELOP_LEVELS]);

/* A profile on the CURRENT device: gains (g_R, g_G, g_B), the row-major matrix and the thresholds are checked -- a non-finite or
 * negative gain, a non-finite matrix entry and a non-finite or decreasing table are refused, before any HIP call -- and one small
 * device table (the thresholds and the index that narrows their search) is uploaded once (synchronous).  *ctx is released with
 * sesrq_develop_destroy.  With SESRQ_DEVELOP_SEARCH=full in the environment the index is left empty and every count takes all eight
 * steps of the binary search: the same bytes, for measurements (tools/develop_probe.py). */
int sesrq_develop_create(const float gains[3], const float ccm[9], const float T[SESRQ_DEVELOP_LEVELS], sesrq_develop_ctx *ctx);
void sesrq_develop_destroy(sesrq_develop_ctx ctx);

/* pred: device (N, 3, H, W) fp32 (pred_dtype SESRQ_DEVELOP_F32; scale / zero ignored) or int8 (SESRQ_DEVELOP_I8, output domain
 * scale > 0 and finite, zero in [-128, 127]); out: device (N, H, W, 3) uint8 in `order`.  Any N, H, W >= 1 with H * W < 2^31 and
 * N * ceil(H * W / 16) < 2^31 - 2^21 (the 16-pixel runs and one round of the grid fit an int; offsets are 64-bit, so the batch may
 * cross 4 GiB).  One kernel enqueued on `stream` (a hipStream_t; NULL = the default stream); no allocation, no synchronisation, no
 * workspace.  The context's device must be current.  Arguments are checked before any HIP call; 0 on success, non-zero with
 * sesrq_develop_last_error() set otherwise. */
/* Caller buffers: pred may start at any address aligned to its element type (4 bytes for fp32, 1 for int8), out at any address.  The
 * 16-byte path is chosen per run of 16 pixels, only where the three plane segments and the 48 output bytes of that run happen to be
 * 16-byte aligned (never where H * W is no multiple of 16: the planes of a frame then differ in alignment); the per-pixel path gives
 * the same bytes.  Nothing outside out's N H W 3 bytes is written, pred is not written, nothing outside pred affects the result
 * (tests/test_develop.py). */
int sesrq_develop_export(sesrq_develop_ctx ctx, const void *pred, int pred_dtype, float scale, int zero, int order, uint8_t *out, int N,
                         int H, int W, void *stream);

/* The kernel instantiations export can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_develop_instance_count(void);
const char *sesrq_develop_instance_name(int i);
long long sesrq_develop_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_develop_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
