/* sesrq_video_hr.h -- the super-resolution nets' video input from the HR clip alone: a bicubic x2 / x4 downscale of an 8-bit YUV 4:2:0
 * surface (NV12 / I420), fused with the decode of its LR luma into the net's q0 / fp32 input -- one kernel, all three planes, and no
 * intermediate plane reaches memory.  Video SR test sets ship HR sequences; this header makes the LR side with the arithmetic the image
 * route already fixed, so image and video scores of one net are comparable.  It adds no numerics of its own: every step is a
 * sibling's, and tests/video_hr_oracle.py restates it by slicing planes into tests/downscale_oracle.py.
 *
 * A library of its own (libsesrq_video_hr.so): it links nothing of the other libraries.  Surfaces are sesrq_video.h's
 * sesrq_video_surface; formats are SESRQ_VIDEO_NV12 / SESRQ_VIDEO_I420.
 *
 * Planes.  Each plane of the HR surface is an image of its own, CENTRE sited, as sesrq_video.h says: Y, Cb and Cr.  Each is downscaled
 * by r (2 or 4) with steps 1 - 3 of sesrq_downscale.h, word for word: the stretched Keys a = -1/2 integer weights (r = 2: D = 256;
 * r = 4: D = 4096), mirrored indices with the edge sample repeated, the VERTICAL pass first, a clamped uint8 between the passes, each
 * pass clamp(floor((sum w v + D / 2) / D), 0, 255).  Every sum fits int32: the largest is 255 * 4448 at r = 4, in every plane.
 *
 * Sizes.  The HR luma is 2 r h x 2 r w for integers h, w >= 1, so that the LR luma (2 h x 2 w) and both chroma planes (r h x r w ->
 * h x w) divide exactly; any other size is refused with a message that names modcrop.  Odd LR sizes stay the province of ready-made LR
 * clips (sesrq_video.h takes them); left-sited chroma is out of scope, as there.
 *
 * Decode.  The LR luma byte v goes through step 1 of sesrq_video.h: x = clip(fl32(v / 255.0), 0, 1) and its q0, the 256-code table of
 * one input domain, kept by a context (csrc/sesrq_image_decode.h builds it for every byte library). */
#ifndef SESRQ_VIDEO_HR_H
#define SESRQ_VIDEO_HR_H

#include <stdint.h>

#include "sesrq_video.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The kernel's tile: a workgroup owns TILE_HR_W x TILE_HR_H HR luma pixels at either r and the TILE_HR_W / 2 x TILE_HR_H / 2 chroma
 * samples a plane under them, that is TILE_HR_W / r x TILE_HR_H / r LR luma pixels; it stages each with the 3 r / 2 samples its taps
 * reach on every side.  Exported so that tests can place frames on the seams. */
#define SESRQ_VIDEO_HR_TILE_HR_W 128
#define SESRQ_VIDEO_HR_TILE_HR_H 32

typedef struct sesrq_video_hr_ctx_s *sesrq_video_hr_ctx;

/* The weights of sesrq_downscale.h's step 1 (host only, no device needed): w[k], k = 0 .. 4 r - 1, and their sum D; equal to
 * sesrq_downscale_weights.  r = 2 or 4.  0 on success, non-zero with sesrq_video_hr_last_error() set otherwise. */
int sesrq_video_hr_weights(int r, int16_t *w /* [4 r] */, int *D);

/* The decode table of one input domain, as sesrq_video_create builds it, uploaded to the CURRENT device once (synchronous).
 * scale_in = f32(input.0.scale) > 0, zero_in = input.0.zero, exact_div as sesrq_options.exact_div.  Released with _destroy. */
int sesrq_video_hr_create(float scale_in, int zero_in, int exact_div, sesrq_video_hr_ctx *ctx);
void sesrq_video_hr_destroy(sesrq_video_hr_ctx ctx);

/* ONE kernel enqueued on `stream` (a hipStream_t; NULL = the default stream) of the current device; no allocation, no
 * synchronisation, no workspace: neither a uint8 intermediate nor (unless asked for) an LR plane reaches memory.
 * hr: the HR surface, N frames of r H x r W luma; H, W: the LR luma size, both even; r: 2 or 4.  Any non-empty subset of
 *   lr: the LR surface of H x W luma, or NULL; its format is independent of hr's.  lr->y may be NULL: then only the chroma plane(s)
 *       are written (what the luma route needs for its export) and lr's luma strides are not looked at;
 *   q0: device (N, 1, H, W) int8, or NULL;      x: device (N, 1, H, W) fp32, or NULL.
 * ctx may be NULL when neither q0 nor x is asked for; otherwise its device must be current.  Only the planes of hr that an output
 * needs are read: Y for q0, x and lr->y, the chroma for lr.  Arguments are checked before any HIP call; 0 on success, non-zero with
 * sesrq_video_hr_last_error() set otherwise; an odd H or W (an HR luma that is no multiple of 2 r) is refused with a message that
 * names modcrop.
 * Limits: N >= 1; H, W >= 2; r H and r W at most 2^31 - 1; N ceil(r H / TILE_HR_H) ceil(r W / TILE_HR_W) (the grid, one workgroup a
 * tile) at most 2^31 - 1; pitches and frame strides >= 0, a pitch at least its row's bytes; with N > 1 an output frame stride at least
 * the plane's extent (rows - 1) pitch + row bytes.  All offsets are 64-bit: a batch may hold more than 2^32 bytes.
 * Caller buffers: every plane and q0 may start at any address and pitches may be odd, x at any 4-byte aligned address.  The kernel
 * reads hr in 4-byte words at whatever address a tile's window starts (the hardware's unaligned access; never a word that is not
 * wholly inside a row's bytes) and single bytes at a frame's borders.  A lane owns 16 consecutive output bytes of one row -- of lr's Y,
 * of q0, of a chroma plane (NV12: eight Cb,Cr pairs), or four elements of x; it takes a 16-byte store only where that run is whole and
 * its address happens to be 16-byte aligned, otherwise per-element ones (NV12 chroma: 2-byte elements): the same bytes.  Nothing
 * outside the rows of lr's planes and the N H W elements of q0 and x is written, hr is not written, nothing outside the rows of hr's
 * planes affects the result. */
int sesrq_video_hr_run(sesrq_video_hr_ctx ctx, const sesrq_video_surface *hr, int r, const sesrq_video_surface *lr, int8_t *q0, float *x,
                       int N, int H, int W, void *stream);

/* The kernel instantiations run can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_video_hr_instance_count(void);
const char *sesrq_video_hr_instance_name(int i);
long long sesrq_video_hr_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_video_hr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
