/* sesrq_video_rgb.h -- YUV 4:2:0 video frames (NV12 / I420) into and out of the RGB super-resolution nets (MFLAG 6: SESR-x2, 3 channels
 * in, 3 out; BT.601 studio range, chroma CENTRE sited).  A decoder's surface goes in at 1.5 B/px: one kernel upscales its chroma to
 * 4:4:4, converts YCbCr to RGB bytes and looks each byte up in the net's input table; one kernel takes the net's prediction to RGB
 * bytes, converts them to YCbCr and writes a 4:2:0 surface.  No RGB image and no full-resolution chroma plane is held in memory on
 * the way.  The reference has no video path, so there is no output of its own to match: this header fixes the arithmetic, every
 * step taken from a sibling header where one exists, and tests/video_rgb_oracle.py restates it in numpy.
 *
 * A library of its own (libsesrq_video_rgb.so): it links no other library of the project.  Surfaces are sesrq_video.h's
 * sesrq_video_surface: H x W bytes of luma, ceil(H / 2) x ceil(W / 2) samples of each chroma; odd H and W are legal.
 *
 * DECODE: a surface of N frames of H x W luma -> the RGB net's input (N, 3, H, W), planes R, G, B.  Any H, W >= 1.
 *
 * D1. Chroma to 4:4:4.  Each chroma plane goes through step 3 of sesrq_video.h at r = 2, verbatim: C = 64 c (Q6), the Keys a = -1/2
 *     weights (phi 0: taps j-2 .. j+1  -24, 232, 888, -72; phi 1: taps j-1 .. j+2  -72, 888, 232, -24), half-pixel centres, indices
 *     clamped to the plane (edge replicate), the HORIZONTAL pass first, each pass floor((sum w C + 512) / 1024) in exact integers.
 *     The result is NOT rounded to a byte: Cb^, Cr^ are the Q6 samples, the plane video_export<.,r2,.> forms before its
 *     (C + 32) >> 6.  The top-left H x W of the upscaled 2 ceil(H / 2) x 2 ceil(W / 2) plane is used.  Bounds, as stated there for
 *     r = 2: the horizontal pass lies in -1530 .. 17850, the vertical one in -3347 .. 19667: every intermediate fits int16.
 * D2. Colour: step 4 of sesrq_colour.h word for word, with Y = (float) y_byte (exact) and Cb^, Cr^ of D1 -- fp32, each operation
 *     rounded, no fused multiply-add:
 *       a   = fl(1.16438356f * fl(Y - 16.0f))
 *       cbf = (float)(Cb^ - 8192) * 0.015625f,  crf = (float)(Cr^ - 8192) * 0.015625f          (both exact)
 *       R   = fl(a + fl(1.59602679f * crf))
 *       G   = fl(fl(a - fl(0.39176229f * cbf)) - fl(0.81296765f * crf))
 *       B   = fl(a + fl(2.01723214f * cbf))
 *     each of R, G, B a byte by clamp(rintf(.), 0, 255), ties to even.
 * D3. Net input, per byte v: the SESRQ_IMAGE_RGB per-code form of sesrq_image.h: x = clip(fl32(v / 255.0), 0, 1) and q0 from the
 *     256-code table sesrq_image_table returns, kept by a context.  Going through the byte is deliberate: the net was trained on
 *     8-bit RGB, and the decoded input equals the image decode of the RGB image D2 describes.
 *
 * EXPORT: the net's prediction p (N, 3, H, W), planes R, G, B, fp32 or int8 dequantised as sesrq_forward forms out_f,
 * p = fl((q - zero) * scale) -> a surface of H x W.  Any H, W >= 1 (an r = 1 RGB net need not give even sizes).
 *
 * E1. Bytes, per channel: u = trunc(fl32(clip(p, 0, 1) * 255.0f)); a NaN gives 0 -- sesrq_image_export's byte, so the surface is
 *     the conversion of the PNG that export would write.
 * E2. Luma, exact integers: Y = floor((65481 R + 128553 G + 24966 B + 4207500) / 255000); it lies in 16 .. 235.
 * E3. Chroma, one sample per 2 x 2 block of pixels (2i .. 2i+1, 2j .. 2j+1), pixel indices clamped to the frame; the sum is taken
 *     before the one rounding.  With S the sum over the four pixels of  -37797 R - 74203 G + 112000 B  (Cb)  or
 *     112000 R - 93786 G - 18214 B  (Cr):  byte = floor((2 S + 262140000) / 2040000).  The numerator is positive and below 2^31; the
 *     byte lies in 16 .. 240.
 *     These are the constants of the reference's luma line and of step 1 of sesrq_colour.h, x 1000; no float64 is needed.
 *
 * Facts, over all 2^24 byte triples (tests/test_video_rgb_oracle.py re-derives them): the integer luma differs from rint of
 * sesrq_image.h's float64 line at 120 triples, all among the 194 exact ties (the integer form rounds half up, rint to even); the
 * one-pixel Cb form floor((2 S + 65535000) / 510000) never differs from rint of the float64 cb (there are 0 ties); the one-pixel Cr
 * form differs at 6 of 12 ties.  E2 / E3 of one pixel followed by D2 returns every triple within 2 per channel: 99.65 % within 1,
 * 15.9 % exact. */
#ifndef SESRQ_VIDEO_RGB_H
#define SESRQ_VIDEO_RGB_H

#include <stdint.h>

#include "sesrq_video.h" /* sesrq_video_surface, SESRQ_VIDEO_NV12 / _I420, SESRQ_VIDEO_F32 / _I8 */

#ifdef __cplusplus
extern "C" {
#endif

#define SESRQ_VIDEO_RGB_CODES 256

/* The decode kernel's tile: a workgroup owns TILE_W x TILE_H luma pixels and stages the TILE_W / 2 x TILE_H / 2 chroma samples a plane
 * under them with a halo of 2.  The export kernel has no tile: a lane owns a block of EXPORT_BLOCK_W x 2 pixels, a workgroup
 * EXPORT_LANES consecutive blocks counted along the rows of block pairs of the batch.  Exported so that tests can sit on the seams. */
#define SESRQ_VIDEO_RGB_TILE_W 128
#define SESRQ_VIDEO_RGB_TILE_H 32
#define SESRQ_VIDEO_RGB_EXPORT_BLOCK_W 16
#define SESRQ_VIDEO_RGB_EXPORT_LANES 256

typedef struct sesrq_video_rgb_ctx_s *sesrq_video_rgb_ctx;

/* D3 for every byte code 0 .. 255 (host only, no device needed): x[v] and its q0 -- what sesrq_image_table returns.
 * scale_in = f32(input.0.scale) > 0, zero_in = input.0.zero, exact_div as sesrq_options.exact_div.  0 on success, non-zero with
 * sesrq_video_rgb_last_error() set otherwise. */
int sesrq_video_rgb_table(float scale_in, int zero_in, int exact_div, int8_t q[SESRQ_VIDEO_RGB_CODES], float x[SESRQ_VIDEO_RGB_CODES]);

/* Build the table and upload it to the CURRENT device once (synchronous).  *ctx is released with sesrq_video_rgb_destroy. */
int sesrq_video_rgb_create(float scale_in, int zero_in, int exact_div, sesrq_video_rgb_ctx *ctx);
void sesrq_video_rgb_destroy(sesrq_video_rgb_ctx ctx);

/* Every device entry: one kernel enqueued on `stream` (a hipStream_t; NULL = the default stream) of the current device; no allocation,
 * no synchronisation, no workspace.  Arguments are checked before any HIP call; 0 on success, non-zero with
 * sesrq_video_rgb_last_error() set otherwise.  All offsets are 64-bit: a batch may hold more than 2^32 bytes. */

/* D1 - D3 in one kernel: src (N frames of H x W: the Y plane and the chroma plane(s), through their pitches and frame strides) -> q0
 * device (N, 3, H, W) int8 or NULL, x device (N, 3, H, W) fp32 or NULL (not both NULL).  Any N, H, W >= 1 with
 * N ceil(H / TILE_H) ceil(W / TILE_W) (the grid, one workgroup a tile) at most 2^31 - 1; pitches at least their row's bytes, frame
 * strides >= 0.  The context's device must be current.
 * Caller buffers: the planes of src and q0 may start at any address, x at any 4-byte aligned one; pitches may be odd.  A lane owns 16
 * consecutive pixels of a row; it takes 16-byte loads and stores only where that run is whole and its Y, q0 and x addresses (of all
 * three planes) happen to be 16-byte aligned, otherwise per-element ones: the same bytes.  Chroma is read sample by sample.
 * Nothing outside q0 and x is written, src is not written, nothing outside the rows of src's planes affects the result. */
int sesrq_video_rgb_decode(sesrq_video_rgb_ctx ctx, const sesrq_video_surface *src, int8_t *q0, float *x, int N, int H, int W,
                           void *stream);

/* E1 - E3 in one kernel.  pred: device (N, 3, H, W) fp32 (dtype SESRQ_VIDEO_F32; scale / zero ignored) or int8 (SESRQ_VIDEO_I8: the
 * net's output domain, scale > 0 and finite, zero in [-128, 127]); out: the surface of H x W luma, written whole: the Y plane and the
 * chroma plane(s) of ceil(H / 2) x ceil(W / 2) samples.
 * Limits: N, H, W >= 1; N ceil(H / 2) ceil(W / 16) (the blocks, one a lane) below 2^31 less one workgroup; pitches and frame
 * strides >= 0, a pitch at least its row's bytes; with N > 1 a frame stride at least the plane's extent (rows - 1) pitch + row bytes.
 * Caller buffers: every plane and an int8 pred may start at any address, an fp32 pred at any 4-byte aligned one; pitches may be odd.
 * A lane owns 2 rows x 16 columns: it reads two runs of 16 values of each of the three planes and writes two runs of 16 Y bytes and
 * 8 chroma samples a plane (NV12: sixteen interleaved bytes, I420: eight bytes a plane).  It takes 16-byte loads and 16-byte (Y,
 * NV12) / 8-byte (I420 chroma) stores only where the block is whole (16 columns) and the addresses concerned happen to be that
 * aligned, otherwise per-element ones: the same bytes.  Nothing outside the rows of out's planes is written, pred is not written,
 * nothing outside pred affects the result. */
int sesrq_video_rgb_export(const void *pred, int dtype, float scale, int zero, const sesrq_video_surface *out, int N, int H, int W,
                           void *stream);

/* The kernel instantiations decode / export can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_video_rgb_instance_count(void);
const char *sesrq_video_rgb_instance_name(int i);
long long sesrq_video_rgb_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_video_rgb_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
