/* sesrq_mosaic.h -- the reference's MFLAG 1 (nr, denoise) metric on the device: PSNR and SSIM of the Bayer mosaics of the prediction
 * and of the ground truth (test.py: clip the prediction to [0, 1], three2one() both frames, compare_psnr(gt, pred, data_range=1.0)
 * and the single-channel compare_ssim of the two mosaics).
 *
 * A library of its own (libsesrq_mosaic.so): it links neither libsesrq.so nor libsesrq_eval.so.
 *
 * Frames are NCHW with C = 3, pred and gt of one shape (N, 3, H, W).  Per frame, on the device:
 *   m(t)[r, c] = t[(r & 1) + (c & 1), r, c]      R where row and column are even, G where exactly one is odd, B where both are odd
 *   x = m(clip01(pred))                          np.clip: a NaN passes through
 *   y = m(gt)                                    gt is never clipped
 *   mse  = sum((y - x)^2) / (H W)                in fp64
 *   psnr = 10 log10(1 / mse)                     +inf when mse == 0
 *   ssim = single-channel SSIM of (x, y) as include/sesrq_eval.h defines it: 7x7 uniform window, K1 = 0.01, K2 = 0.03, sample
 *          covariance (49/48), mean of the SSIM map over the frame cropped by 3 pixels on each side
 * H and W may be odd; both must be at least 7.
 *
 * One pass, no mosaic frame in memory: a row reads only the two channel planes it selects from (even rows 0 and 1, odd rows 1 and 2).
 * The arithmetic is that of libsesrq_eval.so's SESRQ_EVAL_Y255 form on the gathered mono frames (fp64 moments, fp32 final quotient):
 * ssim has the same bits, and mse_y255 == 65025.0 * mse bit for bit.
 *
 * NaN: only selected samples count.  A NaN at a selected (pixel, channel) of pred or gt makes that frame's mse, psnr and ssim NaN and
 * leaves the other frames' bits alone; a NaN at an unselected position has no effect -- unselected samples enter no arithmetic.
 * An int8 pred has no NaN.  +-Inf in a frame is unspecified. */
#ifndef SESRQ_MOSAIC_H
#define SESRQ_MOSAIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_MOSAIC_F32 = 0, SESRQ_MOSAIC_I8 = 1 };

typedef struct sesrq_mosaic_desc {
    int32_t pred_dtype;    /* SESRQ_MOSAIC_F32: fp32 frame; SESRQ_MOSAIC_I8: int8 frame, dequantised in-kernel as (q - pred_zero) * pred_scale
                            * in fp32 -- the bits of sesrq_forward's out_f, as sesrq_eval does it */
    float   pred_scale;    /* int8 pred: the net's scale_out, f32(input.L.scale) */
    int32_t pred_zero;     /* int8 pred: zero[L] */
} sesrq_mosaic_desc;

/* Device workspace sesrq_mosaic_score needs for N frames of (3, H, W): two doubles per tile.  Host only; 0 for an invalid shape. */
size_t sesrq_mosaic_workspace_bytes(int N, int H, int W);

/* Score N frames.  pred: device (N, 3, H, W) fp32 or int8 (desc->pred_dtype); gt: device fp32 of the same shape;
 * out: device double[N][3] = {mse, psnr, ssim} per frame.  No allocation, no synchronisation: two kernels enqueued on `stream`
 * (a hipStream_t; NULL = the default stream).  Bitwise reproducible: a frame's result has the same bits alone or inside a batch,
 * on any stream.  Arguments are checked before any HIP call; 0 on success, non-zero with sesrq_mosaic_last_error() set otherwise.
 *
 * Caller buffers: gt and an fp32 pred may start at any 4-byte aligned address, an int8 pred at any address; the 16-byte loads are
 * used only where W % 4 == 0 and gt and pred happen to be aligned for them (16 bytes; 4 for an int8 pred), per launch -- the results
 * are the same either way.  out and the workspace hold doubles: 8-byte aligned, the workspace of sesrq_mosaic_workspace_bytes()
 * bytes, no more.  Nothing outside [out, out + 3 N doubles) and the workspace is written, pred / gt are not written, nothing outside
 * them affects the scores, and the workspace's prior contents do not matter (tests/test_mosaic_quality.py). */
int sesrq_mosaic_score(const sesrq_mosaic_desc *desc, const void *pred, const float *gt, int N, int H, int W,
                       double *out, void *workspace, size_t workspace_bytes, void *stream);

/* The kernel instantiations sesrq_mosaic_score can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_mosaic_kernel_count(void);
const char *sesrq_mosaic_kernel_name(int i);
long long sesrq_mosaic_kernel_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_mosaic_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
