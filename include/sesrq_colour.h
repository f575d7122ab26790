/* sesrq_colour.h -- colour out of the luma super-resolution nets: the net super-resolves Y, Cb and Cr of the low-resolution image are
 * upscaled bicubically, YCbCr goes back to RGB -- one fused kernel on the high-resolution side.  The reference stops at the Y score
 * (self_dataset_sr.py: Y in, Y out), so there is no output of its own to match: this header fixes the arithmetic, and
 * tests/colour_oracle.py restates it in numpy.
 *
 * A library of its own (libsesrq_colour.so): it links nothing of libsesrq.so or libsesrq_image.so.
 *
 * img is a low-resolution image (N, H, W, 3) uint8, interleaved, in `order` (RGB or BGR); r is 2 or 4; the output is
 * (N, rH, rW, 3) uint8 in the same order.  With d(v) = v / 255.0 in IEEE float64 (correctly rounded), as in sesrq_image.h:
 *
 * 1. LR chroma, Q6 fixed point (float64, each product rounded once, sums left to right, no fused multiply-add):
 *      cb = ((-37.797 d(R) + -74.203 d(G)) + 112.0 d(B)) + 128.0
 *      cr = ((112.0 d(R) + -93.786 d(G)) + -18.214 d(B)) + 128.0
 *      Cb = (int) rint(64 cb), Cr = (int) rint(64 cr), ties to even; both lie in 1024 .. 15360.
 *    The BT.601 studio constants of the reference's luma line (MATLAB rgb2ycbcr).
 *
 * 2. Bicubic upscale: the Keys kernel with a = -1/2 (MATLAB imresize, PIL BICUBIC), half-pixel centres, indices clamped to the frame
 *    (edge replicate), separable, the HORIZONTAL pass first, then the vertical one, both in exact integers.  Output coordinate
 *    X = r j + phi takes four LR taps with integer weights / 1024:
 *      r = 4  phi 0  taps j-2 .. j+1   -45, 399, 745, -75          r = 2  phi 0  taps j-2 .. j+1   -24, 232, 888, -72
 *             phi 1  taps j-2 .. j+1    -7,  93, 987, -49                 phi 1  taps j-1 .. j+2   -72, 888, 232, -24
 *             phi 2  taps j-1 .. j+2   -49, 987,  93,  -7
 *             phi 3  taps j-1 .. j+2   -75, 745, 399, -45
 *    Each pass is floor((sum w c + 512) / 1024): an arithmetic shift, which floors negative sums as well.  The weights are the Keys
 *    polynomial at t = k / 8 (r = 4) and k / 4 (r = 2) times 1024, exactly; every row sums to 1024.  Intermediates stay within about
 *    +-19 000 (int16); every sum fits int32.
 *
 * 3. Luma: p is the net's output (N, 1, rH, rW), fp32, or int8 dequantised as sesrq_forward forms out_f: p = fl((q - zero) * scale).
 *      Y = fl(fminf(fmaxf(p, 0), 1) * 255.0f)  -- the image export's value before truncation; a NaN gives 0, as there.
 *
 * 4. Colour, fp32, each operation rounded, in this order (Cb^, Cr^ the upscaled Q6 chroma):
 *      a   = fl(1.16438356f * fl(Y - 16.0f))
 *      cbf = (float)(Cb^ - 8192) * 0.015625f,  crf = (float)(Cr^ - 8192) * 0.015625f          (both exact)
 *      R   = fl(a + fl(1.59602679f * crf))
 *      G   = fl(fl(a - fl(0.39176229f * cbf)) - fl(0.81296765f * crf))
 *      B   = fl(a + fl(2.01723214f * cbf))
 *    each byte clamp(rintf(.), 0, 255), ties to even. */
#ifndef SESRQ_COLOUR_H
#define SESRQ_COLOUR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_COLOUR_ORDER_RGB = 0, SESRQ_COLOUR_ORDER_BGR = 1 };
enum { SESRQ_COLOUR_F32 = 0, SESRQ_COLOUR_I8 = 1 };          /* dtype of the luma y */

/* The export kernel's tile: a workgroup owns TILE_OUT_W x TILE_OUT_H output pixels at either r, that is TILE_W x TILE_H LR pixels at
 * r = 4 and twice that each way (64 x 16) at r = 2, and stages them with a halo of 2 LR pixels on every side.  Exported so that tests
 * can place frames on the seams. */
#define SESRQ_COLOUR_TILE_OUT_W 128
#define SESRQ_COLOUR_TILE_OUT_H 32
#define SESRQ_COLOUR_TILE_W 32
#define SESRQ_COLOUR_TILE_H 8

/* The weight table of step 2 (host only, no device needed): w[4 phi + k] is the weight of tap k of phase phi, first[phi] the offset of
 * tap 0 from j (-2 or -1).  r = 2 or 4.  0 on success, non-zero with sesrq_colour_last_error() set otherwise. */
int sesrq_colour_weights(int r, int16_t *w /* [4 r] */, int8_t *first /* [r] */);

/* Every device entry: one kernel enqueued on `stream` (a hipStream_t; NULL = the default stream) of the current device; no allocation,
 * no synchronisation, no workspace.  Arguments are checked before any HIP call; 0 on success, non-zero with
 * sesrq_colour_last_error() set otherwise.  All offsets are 64-bit: a batch may hold more than 2^32 bytes. */

/* Step 1 alone: img device (N, H, W, 3) uint8 in `order` -> cbcr device (N, 2, H, W) int16, plane 0 = Cb, plane 1 = Cr (Q6).  Any
 * N, H, W >= 1.  img may start at any address, cbcr at any 2-byte aligned one.  The kernel calls the device function the export calls. */
int sesrq_colour_chroma(const uint8_t *img, int order, int16_t *cbcr, int N, int H, int W, void *stream);

/* Steps 1 - 4 in one kernel; no chroma plane is written to memory.  y: device (N, 1, rH, rW) fp32 (y_dtype SESRQ_COLOUR_F32; scale /
 * zero ignored) or int8 (SESRQ_COLOUR_I8: the net's output domain, scale > 0 and finite, zero in [-128, 127]); img: device
 * (N, H, W, 3) uint8 in `order`; out: device (N, rH, rW, 3) uint8 in `order`.  H, W are the LR size, r is 2 or 4.
 * Limits: N, H, W >= 1; r H and r W at most 2^31 - 1; N ceil(r H / TILE_OUT_H) ceil(r W / TILE_OUT_W) (the grid, one workgroup a tile) at
 * most 2^31 - 1.  Pixel and byte offsets are 64-bit, so no limit comes from the output's byte count.
 * Caller buffers: img, out and an int8 y may start at any address, an fp32 y at any 4-byte aligned one.  A lane owns 16 consecutive
 * output pixels of one row; it takes 16-byte loads and stores only where that run is whole and its y and out addresses happen to be
 * 16-byte aligned (r W 3 is a multiple of 16 only when r W % 16 == 0), otherwise per-element ones: the same bytes.  Nothing outside
 * out's N rH rW 3 bytes is written, y and img are not written, nothing outside y and img affects the result. */
int sesrq_colour_export(const void *y, int y_dtype, float scale, int zero, const uint8_t *img, int order, int r, uint8_t *out, int N,
                        int H, int W, void *stream);

/* The kernel instantiations chroma / export can launch (a fixed set), and how often each has been launched in this process. */
int sesrq_colour_instance_count(void);
const char *sesrq_colour_instance_name(int i);
long long sesrq_colour_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_colour_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
