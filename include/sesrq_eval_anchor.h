/* sesrq_eval_anchor.h -- the anchored x2 score of libsesrq_eval.so: the MFLAG 6 metrics of pred + up2(lr) without forming that frame.
 * A companion of sesrq_eval.h (whose entry points and sesrq_eval_desc it uses unchanged); the same library exports it. */
#ifndef SESRQ_EVAL_ANCHOR_H
#define SESRQ_EVAL_ANCHOR_H

#include "sesrq_eval.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sesrq_eval of the anchored x2 prediction without forming it: pred is the fp32 output of a net without the fused anchor (the
 * calibration pass's mode-0 output), lr the net's fp32 input (N, C, H/2, W/2); each pixel is scored as fl32(pred + up2(lr)), up2 the
 * nearest upsampling (the reference's test.py:148-155), with the bits of sesrq_eval on a frame the anchor was added to beforehand.
 * desc->form must be SESRQ_EVAL_X2 and desc->pred_dtype SESRQ_EVAL_F32; H and W even.  Same kernels, workspace and stream
 * behaviour as sesrq_eval. */
int sesrq_eval_anchored(const sesrq_eval_desc *desc, const float *pred, const float *lr, const float *gt, int N, int C, int H, int W,
                        double *out, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
