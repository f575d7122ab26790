/* sesrq_unprocess.h -- raw-net inputs and their ground truth from an sRGB image.  The raw nets (MFLAG 1-4: nr, dm, nrdm_3, nrdm_6) are
 * trained and scored on frames an unprocessing pipeline made out of ordinary images: inverse tone curve, gamma expansion, rgb2cam,
 * inverse white-balance gains, mosaic.  The reference reads the results of an external project from disk; this is that first step
 * on the device, one kernel: 8-bit sRGB image -> linear camera RGB -> the Bayer frame a sensor would have written, the net's input and
 * the ground truth.  It is the counterpart of sesrq_develop.h, which takes the nets' output back to display bytes.
 *
 * A library of its own (libsesrq_unprocess.so): it links no other library of the project, and their ABIs are unchanged.
 *
 * The arithmetic.  img is (N, H, W, 3) uint8, interleaved in `order` (RGB or BGR).  Every step is fp32, each operation rounded once
 * (fl), no fused multiply-add, in this order, per pixel and channel c in R, G, B:
 *   1. l_c = L[byte_c]                                                 L: float[256], inverse tone curve and gamma expansion in one
 *   2. c_i = fl(fl(fl(m_i0 * l_R) + fl(m_i1 * l_G)) + fl(m_i2 * l_B))  m: rgb2cam, row-major
 *   3. inverse gains d = (d_R, d_G, d_B).  highlight = 0: s_c = d_c.  highlight = 1 (the unprocessing paper's safe_invert_gains):
 *        g   = fl(fl(fl(c_R + c_G) + c_B) / 3.0f)
 *        t   = fl(fmaxf(fl(g - 0.9f), 0) / 0.1f)
 *        k   = fl(t * t)
 *        s_c = fmaxf(fl(k + fl(fl(1 - k) * d_c)), d_c)
 *   4. r_c = fminf(fmaxf(fl(c_c * s_c), 0), 1)                         a NaN gives 0
 *   5. k_c = (int)rintf(fl(r_c * (float)D))                            D = white - black in [1, 65535]; ties to even
 * The divisions are true IEEE quotients.
 *
 * Outputs (device; each pointer may be NULL, not all of them).  s = the site channel of (y & 1, x & 1) under `cfa`, the CFA orders
 * numbered as SESRQ_CFA_* of sesrq_sensor.h: RGGB 0 {0,1,1,2}, GRBG 1 {1,0,2,1}, GBRG 2 {1,2,0,1}, BGGR 3 {2,1,1,0}.
 *   raw     (N, H, W) uint16      black + k_s: the frame a sensor would have written, in 16-bit containers (MIPI packing stays the
 *                                 sensor module's job)
 *   gt      (N, 3, H, W) fp32     fl((float)k_c / (float)D): at D = 4095 the bits raw.load_gt returns for a 16-bit PNG that holds k_c
 *   q0      (N, 3, H, W) int8     table[k_s] at the site channel, table[0] at the non-sites: what sesrq_sensor_unpack / sesrq_raw_unpack
 *                                 give from `raw`; table[d] = clamp8(rint(fl(fl(x / s0) + z0))), x = fl((float)d / (float)D)
 *                                 (exact_div 2: x * fl(1 / s0))
 *   spread  (N, 3, H, W) fp32     fl((float)k_s / (float)D) at the site channel, 0.0f at the non-sites: the fp32 input frame */
#ifndef SESRQ_UNPROCESS_H
#define SESRQ_UNPROCESS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SESRQ_UNPROCESS_PAPER = 0, SESRQ_UNPROCESS_GAMMA22 = 1, SESRQ_UNPROCESS_SRGB = 2, SESRQ_UNPROCESS_LINEAR = 3 };   /* built-in L */
enum { SESRQ_UNPROCESS_ORDER_RGB = 0, SESRQ_UNPROCESS_ORDER_BGR = 1 };

#define SESRQ_UNPROCESS_CODES 256

typedef struct sesrq_unprocess_ctx_s *sesrq_unprocess_ctx;

/* A built-in table (host only, no device needed), b = 0 .. 255; each entry is the fp32 nearest to the exact value:
 *   PAPER    max(u, 1e-8)^2.2 with u = 1/2 - sin(asin(1 - 2 b / 255) / 3): the unprocessing paper's inverse smoothstep and gamma expansion
 *   GAMMA22  (b / 255)^(11/5)
 *   SRGB     the piecewise sRGB EOTF: v / 12.92 for v = b / 255 <= 0.04045, ((v + 0.055) / 1.055)^(12/5) above
 *   LINEAR   fl(b / 255.0f)
 * 0 on success, non-zero with sesrq_unprocess_last_error() set otherwise. */
int sesrq_unprocess_curve(int kind, float L[SESRQ_UNPROCESS_CODES]);

/* A profile on the CURRENT device.  Refused before any HIP call: a non-finite entry of L or m, a non-finite or negative d, highlight
 * other than 0 / 1, cfa outside 0 .. 3, levels outside 0 <= black < white <= 65535, and an input domain sesrq_sensor_create would
 * refuse (scale_in = f32(input.0.scale) > 0 and finite, zero_in = input.0.zero, exact_div 0 .. 2).  L and the q0 table of the
 * white - black + 1 levels are uploaded once (synchronous).  *ctx is released with sesrq_unprocess_destroy. */
int sesrq_unprocess_create(const float L[SESRQ_UNPROCESS_CODES], const float m[9], const float d[3], int highlight, int cfa, int black,
                           int white, float scale_in, int zero_in, int exact_div, sesrq_unprocess_ctx *ctx);
void sesrq_unprocess_destroy(sesrq_unprocess_ctx ctx);

/* img: device (N, H, W, 3) uint8 in `order`; raw, gt, q0, spread: device outputs as above, each may be NULL.  Any N, H, W >= 1 with
 * N * H * ceil(W / 16) < 2^31 - 2^21 (the 16-pixel row segments and one round of the grid fit an int; offsets are 64-bit).  One
 * kernel enqueued on `stream` (a hipStream_t; NULL = the default stream); no allocation, no synchronisation, no workspace.  The
 * context's device must be current.  Arguments are checked before any HIP call; 0 on success, non-zero with
 * sesrq_unprocess_last_error() set otherwise. */
/* Caller buffers: every buffer may start at any address aligned to its element type (img, q0: any; raw: 2 bytes; gt, spread: 4).
 * A lane owns 16 pixels of one row.  It reads them as three 16-byte words where the segment is whole and its 48 bytes are 16-byte
 * aligned, byte by byte otherwise; it writes raw as two 16-byte words, q0 as one a plane, gt and spread as four a plane, each where
 * that output's addresses of that segment are 16-byte aligned and the segment is whole, element by element otherwise.  Each choice
 * is made per segment and per buffer and gives the same bytes.  Nothing outside the outputs is written, img is not written and
 * nothing outside img affects a result (tests/test_unprocess.py). */
int sesrq_unprocess_run(sesrq_unprocess_ctx ctx, const uint8_t *img, int order, uint16_t *raw, float *gt, int8_t *q0, float *spread,
                        int N, int H, int W, void *stream);

/* The kernel instantiations run can launch (a fixed set: one per set of outputs, and for the sets with q0 one per home of the q0
 * table -- LDS up to 4096 levels, global memory above), and how often each has been launched in this process. */
int sesrq_unprocess_instance_count(void);
const char *sesrq_unprocess_instance_name(int i);
long long sesrq_unprocess_instance_launches(int i);

/* Message of the last failed call on this thread ("" if none). */
const char *sesrq_unprocess_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
