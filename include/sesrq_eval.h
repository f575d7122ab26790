/* sesrq_eval.h -- on-device quality metrics (PSNR, SSIM) of the integer path's output frames: the reference's evaluation loop
 * (test.py: clip the prediction to [0, 1], then PSNR and SSIM against the ground truth, in the form its network uses).
 *
 * A library of its own (libsesrq_eval.so): it does not link libsesrq.so, and libsesrq.so's ABI (include/sesrq.h) is unchanged.
 *
 * Frames are NCHW, pred and gt of one shape (N, C, H, W).  Per frame, on the device:
 *   SESRQ_EVAL_RGB  (C = 3; MFLAG 3, 4): mse over C*H*W of (gt - clip(pred))^2, psnr = 10 log10(1 / mse) (+inf when mse == 0),
 *                    ssim = mean over channels of the single-channel SSIM (data_range 1)
 *   SESRQ_EVAL_Y255 (C = 1; MFLAG 5):    mse over H*W of (255 gt - 255 clip(pred))^2, psnr = 10 log10(255^2 / (mse + 1e-8)),
 *                    ssim = single-channel SSIM (data_range 1)
 *   SESRQ_EVAL_X2   (C = 3; MFLAG 6):    Y(img) = clip(65.481 R + 128.553 G + 24.966 B + 16, 0, 255); mse over H*W of
 *                    (Y(gt) - Y(clip(pred)))^2, psnr = 10 log10(255^2 / (mse + 1e-8)); ssim as SESRQ_EVAL_RGB.
 *                    pred is the anchored fp32 output (sesrq_options.anchor_add = 1).
 * SSIM is skimage's default: 7x7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance (49/48), mean of the SSIM map over the
 * windows that lie wholly inside the frame (the frame cropped by 3 pixels on each side); H and W must be at least 7.
 * gt is never clipped.
 *
 * NaN inside a frame: the clip is np.clip's, which passes a NaN on.  A NaN anywhere in an fp32 pred or in gt (for
 * sesrq_eval_anchored, also in lr: the prediction is pred + up2(lr)) makes that frame's mse, psnr and ssim NaN, as the reference
 * prints them; the other frames of the batch keep their bits.  An int8 pred has no NaN.  +-Inf in a frame is unspecified.
 * (tests/test_quality_seams.py) */
#ifndef SESRQ_EVAL_H
#define SESRQ_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_EVAL_RGB = 0, SESRQ_EVAL_Y255 = 1, SESRQ_EVAL_X2 = 2 };
enum { SESRQ_EVAL_F32 = 0, SESRQ_EVAL_I8 = 1 };

typedef struct sesrq_eval_desc {
    int32_t form;          /* SESRQ_EVAL_* */
    int32_t pred_dtype;    /* SESRQ_EVAL_F32: fp32 frame; SESRQ_EVAL_I8: int8 frame, dequantised in-kernel as (q - pred_zero) * pred_scale
                            * in fp32 -- the bits of sesrq_forward's out_f.  Not with SESRQ_EVAL_X2 (the anchor exists in out_f only). */
    float   pred_scale;    /* int8 pred: the net's scale_out, f32(input.L.scale) */
    int32_t pred_zero;     /* int8 pred: zero[L] */
} sesrq_eval_desc;

/* Device workspace sesrq_eval needs for N frames of (C, H, W): one slab of per-tile partial sums.  Host only; 0 for an invalid shape. */
size_t sesrq_eval_workspace_bytes(int N, int C, int H, int W);

/* Score N frames.  pred: device (N, C, H, W) fp32 or int8 (desc->pred_dtype); gt: device fp32 of the same shape;
 * out: device double[N][3] = {mse, psnr, ssim} per frame.  No allocation, no synchronisation: two kernels enqueued on `stream`
 * (a hipStream_t; NULL = the default stream).  Bitwise reproducible: a frame's result has the same bits alone or inside a batch,
 * on any stream.  Arguments are checked before any HIP call; 0 on success, non-zero with sesrq_eval_last_error() set otherwise. */
/* Caller buffers (sesrq_eval and sesrq_eval_anchored): gt, an fp32 pred and lr may start at any 4-byte aligned address, an int8 pred
 * at any address; the 16-byte loads are used only where W % 4 == 0 and gt and pred happen to be aligned for them (16 bytes; 4 for an
 * int8 pred), per launch -- the results are the same either way.  out and the workspace hold doubles: 8-byte aligned (16 is always
 * enough), the workspace of sesrq_eval_workspace_bytes() bytes, no more.  Nothing outside [out, out + 3 N doubles) and the workspace is
 * written, pred / gt / lr are not written, nothing outside them affects the scores (a NaN beside a frame does not reach them), and the
 * workspace's prior contents do not matter (tests/test_caller_buffers.py). */
int sesrq_eval(const sesrq_eval_desc *desc, const void *pred, const float *gt, int N, int C, int H, int W,
               double *out, void *workspace, size_t workspace_bytes, void *stream);

/* The kernel instantiations sesrq_eval can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_eval_kernel_count(void);
const char *sesrq_eval_kernel_name(int i);
long long sesrq_eval_kernel_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_eval_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
