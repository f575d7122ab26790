/* sesrq_video.h -- YUV 4:2:0 video frames (NV12 / I420) into and out of the luma super-resolution nets (MFLAG 5: Y in, Y out, BT.601
 * studio range).  A decoder's surface goes in as it is: its Y plane is the net's input, its chroma planes are upscaled bicubically on
 * the high-resolution side and leave with the net's luma as a 4:2:0 surface again -- no RGB on the way.  The reference has no video
 * path, so there is no output of its own to match: this header fixes the arithmetic, every step of it taken from a sibling header,
 * and tests/video_oracle.py restates it in numpy.
 *
 * A library of its own (libsesrq_video.so): it links nothing of libsesrq.so, libsesrq_image.so or libsesrq_colour.so.
 *
 * A surface is H x W bytes of luma and ceil(H / 2) x ceil(W / 2) samples of each chroma; odd H and W are legal.  Bytes are taken as
 * they are: studio range is what the net was trained on, a full-range stream is the caller's to convert.  Chroma is CENTRE sited:
 * each chroma plane is an image of its own, half-pixel centres.  Left-sited (MPEG-2) chroma would need a second weight table whose
 * entries are not integers over 1024; it is out of scope.
 *
 * 1. Decode, Y byte v (the SESRQ_IMAGE_RGB per-code form of sesrq_image.h, word for word):
 *      x  = clip(fl32(v / 255.0), 0, 1), v / 255.0 in IEEE float64 (correctly rounded)
 *      q0 = clamp8(rint(fl(fl(x / s0) + z0)))   exact_div 0 / 1: the true fp32 quotient; 2: x * fl(1 / s0) -- sesrq_forward's quantiser
 *    256 codes: a table per input domain, kept by a context.
 *
 * 2. Output luma, p the net's output (N, 1, rH, rW), fp32, or int8 dequantised as sesrq_forward forms out_f, p = fl((q - zero) * scale):
 *      u = trunc(fl32(clip(p, 0, 1) * 255.0f)); a NaN gives 0 -- sesrq_image_export at C = 1, byte for byte.
 *
 * 3. Output chroma, per plane, LR sample byte c: C = 64 c (Q6), then step 2 of sesrq_colour.h verbatim: the Keys a = -1/2 kernel,
 *    half-pixel centres, indices clamped to the plane (edge replicate), the HORIZONTAL pass first, then the vertical one, each
 *    floor((sum w C + 512) / 1024) in exact integers with that header's weights for r = 2 and 4:
 *      r = 4  phi 0  taps j-2 .. j+1   -45, 399, 745, -75          r = 2  phi 0  taps j-2 .. j+1   -24, 232, 888, -72
 *             phi 1  taps j-2 .. j+1    -7,  93, 987, -49                 phi 1  taps j-1 .. j+2   -72, 888, 232, -24
 *             phi 2  taps j-1 .. j+2   -49, 987,  93,  -7
 *             phi 3  taps j-1 .. j+2   -75, 745, 399, -45
 *    The output byte is min(max((C^ + 32) >> 6, 0), 255), C^ the upscaled Q6 sample.  The HR chroma plane is (rH / 2) x (rW / 2): for
 *    odd H or W the top-left part of the upscaled r ceil(H / 2) x r ceil(W / 2) plane.
 *    Bounds, for C in 0 .. 16320: the horizontal pass lies in -1912 .. 18233, the vertical one in -4273 .. 20594 (r = 4; each end is
 *    reached by a plane of 0 and 255 laid out after the weights' signs; r = 2: -1530 .. 17850 and -3347 .. 19667): every intermediate
 *    fits int16, every sum int32. */
#ifndef SESRQ_VIDEO_H
#define SESRQ_VIDEO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_VIDEO_NV12 = 0, SESRQ_VIDEO_I420 = 1 };
enum { SESRQ_VIDEO_F32 = 0, SESRQ_VIDEO_I8 = 1 };          /* dtype of the luma y */

#define SESRQ_VIDEO_CODES 256

/* One 4:2:0 frame, or a batch of them: a contiguous .yuv file frame and a decoder's pitched surface alike.  All planes are 8-bit
 * device memory; pitches and frame strides are in bytes.  A pitch is at least the row's bytes (checked); the bytes between a row's end
 * and the pitch are never read for a result and never written.  Planes may start at any address and pitches may be odd. */
typedef struct sesrq_video_surface {
    int format;                 /* SESRQ_VIDEO_NV12 or SESRQ_VIDEO_I420 */
    void *y, *c0, *c1;          /* NV12: c0 = interleaved Cb,Cr rows of 2*ceil(W/2) bytes, c1 ignored; I420: c0 = Cb, c1 = Cr, rows of ceil(W/2) bytes */
    int64_t pitch_y, pitch_c;   /* bytes between rows; >= the row's bytes (checked) */
    int64_t frame_y, frame_c;   /* bytes between the same plane of consecutive frames of the batch */
} sesrq_video_surface;

/* The export kernel's tile: a workgroup owns TILE_OUT_W x TILE_OUT_H output luma bytes at either r and the chroma under them
 * (TILE_OUT_W / 2 x TILE_OUT_H / 2 samples a plane), that is TILE_OUT_W / r x TILE_OUT_H / r LR luma pixels.  Exported so that tests
 * can place frames on the seams. */
#define SESRQ_VIDEO_TILE_OUT_W 128
#define SESRQ_VIDEO_TILE_OUT_H 32

typedef struct sesrq_video_ctx_s *sesrq_video_ctx;

/* Step 1 for every byte code 0 .. 255 (host only, no device needed): x[v] and its q0 -- what sesrq_image_table returns.
 * scale_in = f32(input.0.scale) > 0, zero_in = input.0.zero, exact_div as sesrq_options.exact_div.  0 on success, non-zero with
 * sesrq_video_last_error() set otherwise. */
int sesrq_video_table(float scale_in, int zero_in, int exact_div, int8_t q[SESRQ_VIDEO_CODES], float x[SESRQ_VIDEO_CODES]);

/* Build the table and upload it to the CURRENT device once (synchronous).  *ctx is released with sesrq_video_destroy. */
int sesrq_video_create(float scale_in, int zero_in, int exact_div, sesrq_video_ctx *ctx);
void sesrq_video_destroy(sesrq_video_ctx ctx);

/* Every device entry: one kernel enqueued on `stream` (a hipStream_t; NULL = the default stream) of the current device; no allocation,
 * no synchronisation, no workspace.  Arguments are checked before any HIP call; 0 on success, non-zero with
 * sesrq_video_last_error() set otherwise.  All offsets are 64-bit: a batch may hold more than 2^32 bytes. */

/* Step 1: the Y plane of src (N frames of H x W, through pitch_y and frame_y) -> q0 device (N, 1, H, W) int8 or NULL, x device
 * (N, 1, H, W) fp32 or NULL (not both NULL).  src's chroma pointers and chroma strides are not looked at.  Any N, H, W >= 1 with
 * N H ceil(W / 16) below 2^31 less one grid round.  The context's device must be current.
 * Caller buffers: the Y plane and q0 may start at any address, x at any 4-byte aligned one.  A lane owns 16 consecutive pixels of a
 * row; it takes 16-byte loads and stores only where that run is whole and its source, q0 and x addresses happen to be 16-byte
 * aligned, otherwise per-element ones: the same bytes.  Nothing outside q0 and x is written, src is not written, nothing outside
 * the W bytes of each row affects the result. */
int sesrq_video_decode(sesrq_video_ctx ctx, const sesrq_video_surface *src, int8_t *q0, float *x, int N, int H, int W, void *stream);

/* Steps 2 and 3 in one kernel; no upscaled chroma plane and no int16 plane is written to memory.  y: device (N, 1, rH, rW) fp32
 * (y_dtype SESRQ_VIDEO_F32; scale / zero ignored) or int8 (SESRQ_VIDEO_I8: the net's output domain, scale > 0 and finite, zero in
 * [-128, 127]); lr: the LR surface whose chroma planes are read (lr->y may be NULL, its luma strides are not looked at); out: the HR
 * surface of rH x rW luma, written whole: the Y plane and the chroma plane(s).  lr->format and out->format are independent.  H, W are
 * the LR luma size, r is 2 or 4.
 * Limits: N, H, W >= 1; r H and r W at most 2^31 - 1; N ceil(r H / TILE_OUT_H) ceil(r W / TILE_OUT_W) (the grid, one workgroup a
 * tile) at most 2^31 - 1; pitches and frame strides >= 0, a pitch at least its row's bytes; with N > 1 an output frame stride at least
 * the plane's extent (rows - 1) pitch + row bytes.
 * Caller buffers: every plane and an int8 y may start at any address, an fp32 y at any 4-byte aligned one.  A lane owns 16 consecutive
 * output bytes of one row, of Y and of chroma (NV12: eight Cb,Cr pairs); it takes 16-byte loads and stores only where that run is
 * whole and its addresses happen to be 16-byte aligned, otherwise per-element ones: the same bytes.  Nothing outside the rows of out's
 * planes is written, y and lr are not written, nothing outside y and the rows of lr's chroma affects the result. */
int sesrq_video_export(const void *y, int y_dtype, float scale, int zero, const sesrq_video_surface *lr, int r,
                       const sesrq_video_surface *out, int N, int H, int W, void *stream);

/* The kernel instantiations decode / export can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_video_instance_count(void);
const char *sesrq_video_instance_name(int i);
long long sesrq_video_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_video_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
