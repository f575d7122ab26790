// libsesrq_video_rgb.so: YUV 4:2:0 video frames (NV12 / I420) into and out of the RGB super-resolution nets
// (include/sesrq_video_rgb.h, which fixes the arithmetic).  A library of its own: it links no other library of the project and
// registers nothing in their instance tables; the per-code table of the decode is the image library's (sesrq_image_decode.h), the
// weight table and the row padding of the chroma upscale the colour library's (sesrq_chroma_upscale.h); the kernels are this file's.
//
// Decode: a workgroup of 256 lanes owns 128 x 32 luma pixels and the 64 x 16 chroma samples a plane under them.  A lane owns 16
// consecutive pixels of one row and requests its 16 Y bytes first, then its share of the two chroma tiles plus a halo of 2, coordinates
// clamped to the chroma plane of THIS frame of the batch; NV12 and I420 differ only in the byte step and the base of Cr.  While those
// fly the per-code table goes to LDS.  The staged samples become Q6 int16 in LDS; the horizontal pass takes every staged row to 128
// output columns, int16 in LDS; then every lane runs the vertical pass for its 16 pixels, four at a time -- four 8-byte LDS reads a
// plane -- the fp32 matrix, the byte (one v_cvt_pk_u8_f32: clamp(rint(.), 0, 255)) and the table lookup, and stores its run of each
// of the three planes.  No chroma plane at full resolution and no RGB byte reaches memory.
//
// Export: a stream.  A lane owns 2 rows x 16 columns: it reads two runs of each of the three planes (int8: one 16-byte load a run,
// fp32: four), forms the bytes (an int8 code looks its byte up in an LDS table of 256, the only LDS of the kernel), the 32 luma
// bytes and, from the sums over its eight 2 x 2 blocks, eight samples of each chroma plane in exact 32-bit integers, and writes two
// 16-byte runs of Y and one 16-byte run of interleaved Cb,Cr (NV12) or 8 bytes a plane (I420).  Rows and columns beyond the frame
// (odd sizes) repeat the last one: the header's clamped indices.
// Runs that are partial or whose addresses are not aligned take per-element loads and stores around the same arithmetic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_video_rgb.h"
#include "sesrq_side.h"
#include "sesrq_image_decode.h"
#include "sesrq_chroma_upscale.h"

namespace sesrq_vrgb {

constexpr int TW = SESRQ_VIDEO_RGB_TILE_W, TH = SESRQ_VIDEO_RGB_TILE_H;      // a decode workgroup's tile, luma pixels
constexpr int CW = TW / 2, CH = TH / 2;                     // ... and in chroma samples a plane
using sesrq_chroma::HALO;
using sesrq_chroma::SEG;                                    // pixels per lane and run
using sesrq_chroma::first_tap;
using sesrq_chroma::half_of;
using sesrq_chroma::weight;
using sesrq_chroma::weight_of;
constexpr int SW = CW + 2 * HALO, SH = CH + 2 * HALO;       // the staged chroma tile
constexpr int RUNS = TW / SEG;                              // runs of a tile's row: 8
constexpr int THREADS = RUNS * TH;                          // a lane a run: 256
constexpr int HWORDS = sesrq_chroma::hwords(TW);            // words per row of the horizontal pass
constexpr int STAGE = (2 * SW * SH + THREADS - 1) / THREADS;
constexpr int HPASS = (2 * SH * CW + THREADS - 1) / THREADS;
constexpr int CODES = SESRQ_VIDEO_RGB_CODES;
constexpr int EXP_THREADS = SESRQ_VIDEO_RGB_EXPORT_LANES;
enum { OUT_Q = 1, OUT_F = 2 };
static_assert(SEG == SESRQ_VIDEO_RGB_EXPORT_BLOCK_W, "a lane's run is the export block's width");
static_assert(EXP_THREADS == CODES, "one int8 code a lane");

using sesrq_imgdec::Tables;
using sesrq_imgdec::RGB_WORDS;
static_assert(CODES == sesrq_imgdec::CODES, "one table for both libraries");

struct DecodeArgs {
    const uint8_t *y, *cb, *cr;     // chroma sample (row, col) of plane p at p[row * pitch_c + col * step], step 2 (NV12) or 1
    const Tables *tab;
    int8_t *q0;
    float *x;
    int64_t pitch_y, frame_y, pitch_c, frame_c;
    int H, W, tiles_x, tiles_y;
};

struct ExportArgs {
    const void *pred;
    uint8_t *oy, *o0, *o1;
    int64_t pitch_y, frame_y, pitch_c, frame_c;
    int64_t items;                  // N pairs segs blocks
    int H, W, pairs, segs;          // row pairs and 16-column blocks of a frame
    float scale;
    int zero;
};

__device__ inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int FMT, int OUT>
__global__ __launch_bounds__(THREADS) void vrgb_decode(DecodeArgs a) {
    constexpr int STEP = FMT == SESRQ_VIDEO_NV12 ? 2 : 1;
    __shared__ uint4 s_tab[RGB_WORDS];
    __shared__ int16_t s_c[2][SH][SW];                                // staged chroma, Q6
    __shared__ __align__(8) unsigned s_h[2][SH][HWORDS];              // the horizontal pass, two int16 a word
    const int tid = threadIdx.x;

    unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)a.tiles_x);
    t /= (unsigned)a.tiles_x;
    const int ty = (int)(t % (unsigned)a.tiles_y);
    const int64_t n = t / (unsigned)a.tiles_y;
    const int lW = (a.W + 1) / 2, lH = (a.H + 1) / 2;                 // the chroma planes

    // a lane's run: 16 pixels of one row; its Y bytes are requested first
    const int row = tid / RUNS, run = tid % RUNS;
    const int64_t Y = (int64_t)ty * TH + row, X0 = (int64_t)tx * TW + (int64_t)run * SEG;
    const bool live = Y < a.H && X0 < a.W;
    const int npx = live ? (int)min((int64_t)SEG, a.W - X0) : 0;
    const uint8_t *src = a.y + (live ? n * a.frame_y + Y * a.pitch_y + X0 : 0);
    const int64_t plane = (int64_t)a.H * a.W;
    const int64_t o = live ? n * 3 * plane + Y * a.W + X0 : 0;      // the run in plane R; G and B lie `plane` and 2 `plane` behind
    const bool vec = npx == SEG && aligned16(src) && (!(OUT & OUT_Q) || (aligned16(a.q0 + o) && (plane & 15) == 0)) &&
                     (!(OUT & OUT_F) || (aligned16(a.x + o) && (plane & 3) == 0));
    unsigned yw[4] = {0, 0, 0, 0};
    if (vec) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        yw[0] = v.x; yw[1] = v.y; yw[2] = v.z; yw[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < SEG; ++k)
            if (k < npx) yw[k >> 2] |= (unsigned)src[k] << (8 * (k & 3));
    }

    // stage: both chroma tiles and their halo, clamped to this frame's planes; every load is requested before the first is used
    const int cx0 = tx * CW, cy0 = ty * CH;
    unsigned cs[STAGE];
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
        const int p = tid + i * THREADS;
        cs[i] = 0;
        if (p < 2 * SH * SW) {
            const int pl = p / (SH * SW), rem = p - pl * (SH * SW);
            const int hy = rem / SW, hx = rem - hy * SW;
            const int gy = min(max(cy0 - HALO + hy, 0), lH - 1), gx = min(max(cx0 - HALO + hx, 0), lW - 1);
            cs[i] = (pl ? a.cr : a.cb)[n * a.frame_c + (int64_t)gy * a.pitch_c + (int64_t)gx * STEP];
        }
    }
    sesrq_imgdec::stage_tables<SESRQ_IMAGE_RGB, THREADS>(s_tab, a.tab);
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
        const int p = tid + i * THREADS;
        if (p < 2 * SH * SW) (&s_c[0][0][0])[p] = (int16_t)(cs[i] << 6);
    }
    __syncthreads();

    // horizontal pass: chroma column j of a staged row gives output columns 2 j and 2 j + 1
#pragma unroll
    for (int i = 0; i < HPASS; ++i) {
        const int u = tid + i * THREADS;
        if (u < 2 * SH * CW) {
            const int pl = u / (SH * CW), rem = u - pl * (SH * CW);
            const int hy = rem / CW, j = rem - hy * CW;
            int c[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) c[k] = s_c[pl][hy][j + k];          // chroma columns j - 2 .. j + 2
            int h[2];
#pragma unroll
            for (int phi = 0; phi < 2; ++phi) {
                const int f = first_tap(2, phi) + HALO;
                int s = 512;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += weight(2, phi, k) * c[f + k];
                h[phi] = s >> 10;
            }
            s_h[pl][hy][j] = ((unsigned)h[0] & 0xffffu) | ((unsigned)h[1] << 16);
        }
    }
    __syncthreads();
    if (!live) return;

    const float *tx_ = sesrq_imgdec::table_x(s_tab);
    const int8_t *tq = sesrq_imgdec::table_q(s_tab);

    // the vertical pass over four rows of the horizontal pass, four pixels at a time, both planes
    const int li = row >> 1, phi = row & 1;
    const int r0 = li + HALO + first_tap(2, phi);
    int wy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wy[k] = weight_of<2>(phi, k);
    unsigned qq[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int g = 0; g < SEG / 4; ++g) {
        int up[2][4];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int s[4] = {512, 512, 512, 512};
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) {
                const uint2 v = *reinterpret_cast<const uint2 *>(&s_h[p][r0 + tp][(run * SEG + 4 * g) / 2]);
                s[0] += __mul24(wy[tp], half_of(v.x, 0));                // |w| <= 1024, |h| < 2^15: a 24-bit multiply is exact
                s[1] += __mul24(wy[tp], half_of(v.x, 1));
                s[2] += __mul24(wy[tp], half_of(v.y, 0));
                s[3] += __mul24(wy[tp], half_of(v.y, 1));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) up[p][k] = s[k] >> 10;
        }
        unsigned b[3] = {0, 0, 0};                                       // the four bytes of R, G, B
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            // D2: fp32, every operation rounded.  The header's c * 0.015625f is exact and a power of two, so it is folded into the
            // coefficients: fl(k * (c / 64)) == fl((k / 64) * c) bit for bit
            const float yy = (float)((yw[g] >> (8 * kk)) & 0xffu);
            const float aa = __fmul_rn(1.16438356f, __fsub_rn(yy, 16.0f));
            const float cb = (float)(up[0][kk] - 8192), cr = (float)(up[1][kk] - 8192);
            const float fr = __fadd_rn(aa, __fmul_rn(1.59602679f * 0.015625f, cr));
            const float fg = __fsub_rn(__fsub_rn(aa, __fmul_rn(0.39176229f * 0.015625f, cb)), __fmul_rn(0.81296765f * 0.015625f, cr));
            const float fb = __fadd_rn(aa, __fmul_rn(2.01723214f * 0.015625f, cb));
            // one v_cvt_pk_u8_f32 a byte: clamp(rint(.), 0, 255), ties to even
            b[0] = __builtin_amdgcn_cvt_pk_u8_f32(fr, kk, b[0]);
            b[1] = __builtin_amdgcn_cvt_pk_u8_f32(fg, kk, b[1]);
            b[2] = __builtin_amdgcn_cvt_pk_u8_f32(fb, kk, b[2]);
        }
        // D3: the table, per byte
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (OUT & OUT_Q) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) qq[c][g] |= (unsigned)(uint8_t)tq[(b[c] >> (8 * kk)) & 0xffu] << (8 * kk);
            }
            if (OUT & OUT_F) {
                float *d = a.x + o + c * plane + 4 * g;
                const float f0 = tx_[b[c] & 0xffu], f1 = tx_[(b[c] >> 8) & 0xffu], f2 = tx_[(b[c] >> 16) & 0xffu], f3 = tx_[b[c] >> 24];
                if (vec) {
                    *reinterpret_cast<float4 *>(d) = make_float4(f0, f1, f2, f3);
                } else {
                    if (4 * g < npx) d[0] = f0;
                    if (4 * g + 1 < npx) d[1] = f1;
                    if (4 * g + 2 < npx) d[2] = f2;
                    if (4 * g + 3 < npx) d[3] = f3;
                }
            }
        }
    }
    if (OUT & OUT_Q) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int8_t *d = a.q0 + o + c * plane;
            if (vec) {
                *reinterpret_cast<uint4 *>(d) = make_uint4(qq[c][0], qq[c][1], qq[c][2], qq[c][3]);
            } else {
#pragma unroll
                for (int k = 0; k < SEG; ++k)
                    if (k < npx) d[k] = (int8_t)(qq[c][k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

// E1 of the header: u = trunc(fl32(clip(p, 0, 1) * 255)); a NaN gives 0
__device__ inline unsigned to_byte(float p) { return (unsigned)__fmul_rn(fminf(fmaxf(p, 0.f), 1.f), 255.f); }

// four waves a workgroup; no occupancy is asked for: the block's 24 words of bytes and the loads in flight of the per-element path
// want more than the 128 VGPRs of 4 waves a SIMD, and a cap would spill them
template <int DT, int FMT>
__global__ __launch_bounds__(EXP_THREADS) void vrgb_export(ExportArgs a) {
    __shared__ uint8_t s_u[DT == SESRQ_VIDEO_I8 ? CODES : 4];         // the byte of int8 code q at [q + 128]
    const int tid = threadIdx.x;
    if (DT == SESRQ_VIDEO_I8) {
        s_u[tid] = (uint8_t)to_byte(__fmul_rn((float)(tid - 128 - a.zero), a.scale));
        __syncthreads();
    }
    const int64_t it = (int64_t)blockIdx.x * EXP_THREADS + tid;
    if (it >= a.items) return;
    const int64_t rp = it / a.segs;                                   // row pairs count over the batch: n pairs + pair
    const int seg = (int)(it - rp * a.segs);
    const int64_t n = rp / a.pairs;
    const int pair = (int)(rp - n * a.pairs);
    const int64_t Y0 = 2 * (int64_t)pair, X0 = (int64_t)seg * SEG;
    const int npx = (int)min((int64_t)SEG, a.W - X0);
    const bool two = Y0 + 1 < a.H;                                    // the last row pair of an odd H repeats its one row
    const int64_t plane = (int64_t)a.H * a.W;
    const int64_t px = n * 3 * plane + Y0 * a.W + X0;                 // the block in plane R
    const int64_t down = two ? a.W : 0;

    // E1: the bytes of the block, four pixels a word; [channel][row][word].  Columns beyond the frame repeat the last one.
    unsigned u[3][2][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int64_t at = px + c * plane + (r ? down : 0);
            unsigned(&w)[4] = u[c][r];
            if (DT == SESRQ_VIDEO_F32) {
                const float *p = static_cast<const float *>(a.pred) + at;
                if (npx == SEG && aligned16(p)) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 v = reinterpret_cast<const float4 *>(p)[g];
                        w[g] = to_byte(v.x) | to_byte(v.y) << 8 | to_byte(v.z) << 16 | to_byte(v.w) << 24;
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        w[g] = 0;
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) w[g] |= to_byte(p[min(4 * g + kk, npx - 1)]) << (8 * kk);
                    }
                }
            } else {
                const int8_t *p = static_cast<const int8_t *>(a.pred) + at;
                unsigned q[4];
                if (npx == SEG && aligned16(p)) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(p);
                    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        q[g] = 0;
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) q[g] |= (unsigned)(uint8_t)p[min(4 * g + kk, npx - 1)] << (8 * kk);
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    w[g] = 0;
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)       // code + 128 = the byte with its top bit flipped
                        w[g] |= (unsigned)s_u[((q[g] >> (8 * kk)) & 0xffu) ^ 0x80u] << (8 * kk);
                }
            }
        }
    }

    // E2 and E3 in exact integers; every numerator is positive and below 2^31
    unsigned yo[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    unsigned cbo[2] = {0, 0}, cro[2] = {0, 0};                        // eight samples a plane
#pragma unroll
    for (int j = 0; j < SEG / 2; ++j) {
        int sb = 0, sr = 0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const int k = 2 * j + d;
                const int R = (int)((u[0][r][k >> 2] >> (8 * (k & 3))) & 0xffu), G = (int)((u[1][r][k >> 2] >> (8 * (k & 3))) & 0xffu),
                          B = (int)((u[2][r][k >> 2] >> (8 * (k & 3))) & 0xffu);
                const unsigned yy = (unsigned)(65481 * R + 128553 * G + 24966 * B + 4207500) / 255000u;
                yo[r][k >> 2] |= yy << (8 * (k & 3));
                sb += -37797 * R - 74203 * G + 112000 * B;
                sr += 112000 * R - 93786 * G - 18214 * B;
            }
        }
        cbo[j >> 2] |= ((unsigned)(2 * sb + 262140000) / 2040000u) << (8 * (j & 3));
        cro[j >> 2] |= ((unsigned)(2 * sr + 262140000) / 2040000u) << (8 * (j & 3));
    }

    // the Y runs
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r == 1 && !two) break;
        uint8_t *d = a.oy + n * a.frame_y + (Y0 + r) * a.pitch_y + X0;
        if (npx == SEG && aligned16(d)) {
            *reinterpret_cast<uint4 *>(d) = make_uint4(yo[r][0], yo[r][1], yo[r][2], yo[r][3]);
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k)
                if (k < npx) d[k] = (uint8_t)(yo[r][k >> 2] >> (8 * (k & 3)));
        }
    }
    // the chroma samples: eight a plane where the block is whole, ceil(npx / 2) otherwise
    const int ns = (npx + 1) / 2;
    const int64_t C0 = X0 / 2;
    if (FMT == SESRQ_VIDEO_NV12) {
        uint8_t *d = a.o0 + n * a.frame_c + (int64_t)pair * a.pitch_c + 2 * C0;
        unsigned w[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const unsigned b0 = cbo[g >> 1] >> (16 * (g & 1)), b1 = cro[g >> 1] >> (16 * (g & 1));
            w[g] = (b0 & 0xffu) | (b1 & 0xffu) << 8 | (b0 & 0xff00u) << 8 | (b1 & 0xff00u) << 16;
        }
        if (npx == SEG && aligned16(d)) {
            *reinterpret_cast<uint4 *>(d) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k)
                if (k < 2 * ns) d[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    } else {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            uint8_t *d = (p ? a.o1 : a.o0) + n * a.frame_c + (int64_t)pair * a.pitch_c + C0;
            const unsigned(&w)[2] = p ? cro : cbo;
            if (npx == SEG && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
                *reinterpret_cast<uint2 *>(d) = make_uint2(w[0], w[1]);
            } else {
#pragma unroll
                for (int k = 0; k < SEG / 2; ++k)
                    if (k < ns) d[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

}  // namespace sesrq_vrgb

using namespace sesrq_vrgb;

struct sesrq_video_rgb_ctx_s {
    DeviceTable t;     // Tables
    InQuant q;
};

enum { K_NQ = 0, K_NF, K_NQF, K_IQ, K_IF, K_IQF, K_EFN, K_EFI, K_EQN, K_EQI, K_COUNT };
static const char *const kNames[K_COUNT] = {"vrgb_decode<nv12,q0>", "vrgb_decode<nv12,x>",   "vrgb_decode<nv12,q0,x>", "vrgb_decode<i420,q0>",
                                            "vrgb_decode<i420,x>",  "vrgb_decode<i420,q0,x>", "vrgb_export<f32,nv12>",  "vrgb_export<f32,i420>",
                                            "vrgb_export<i8,nv12>", "vrgb_export<i8,i420>"};
static Counters<K_COUNT> g_count{kNames};

using sesrq_imgdec::build;

extern "C" int sesrq_video_rgb_table(float scale_in, int zero_in, int exact_div, int8_t q[SESRQ_VIDEO_RGB_CODES],
                                     float x[SESRQ_VIDEO_RGB_CODES]) {
    g_err[0] = 0;
    if (!q || !x) return fail("sesrq_video_rgb_table: q or x is NULL");
    if (check_domain("sesrq_video_rgb_table", scale_in, zero_in, exact_div)) return 1;
    static thread_local Tables t;
    build(in_quant(scale_in, zero_in, exact_div), t);
    for (int v = 0; v < CODES; ++v) {
        q[v] = t.q[v];
        x[v] = t.x[v];
    }
    return 0;
}

extern "C" int sesrq_video_rgb_create(float scale_in, int zero_in, int exact_div, sesrq_video_rgb_ctx *out) {
    g_err[0] = 0;
    const char *who = "sesrq_video_rgb_create";
    if (!out) return fail("%s: ctx is NULL", who);
    *out = nullptr;
    if (check_domain(who, scale_in, zero_in, exact_div)) return 1;
    auto *c = new sesrq_video_rgb_ctx_s();
    c->q = in_quant(scale_in, zero_in, exact_div);
    Tables *host = new Tables();
    build(c->q, *host);
    const int rc = ctx_publish(who, c, host, sizeof(Tables), out);
    delete host;
    return rc;
}

extern "C" void sesrq_video_rgb_destroy(sesrq_video_rgb_ctx c) { ctx_destroy(c); }

static int check_format(const char *who, const char *what, int format) {
    if (format != SESRQ_VIDEO_NV12 && format != SESRQ_VIDEO_I420) return fail("%s: %s format %d (0 = NV12, 1 = I420)", who, what, format);
    return 0;
}

// the bytes of a chroma row of a surface whose chroma planes are cw samples wide
static long long chroma_row_bytes(int format, long long cw) { return format == SESRQ_VIDEO_NV12 ? 2 * cw : cw; }

extern "C" int sesrq_video_rgb_decode(sesrq_video_rgb_ctx c, const sesrq_video_surface *src, int8_t *q0, float *x, int N, int H, int W,
                                      void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_video_rgb_decode";
    if (!c) return fail("%s: ctx is NULL", who);
    if (!src) return fail("%s: src is NULL", who);
    if (check_format(who, "src", src->format)) return 1;
    if (!src->y) return fail("%s: the Y plane of src is NULL", who);
    if (!src->c0 || (src->format == SESRQ_VIDEO_I420 && !src->c1)) return fail("%s: a chroma plane of src is NULL", who);
    if (!q0 && !x) return fail("%s: neither q0 nor x requested", who);
    if (reinterpret_cast<uintptr_t>(x) & 3) return fail("%s: x is not 4-byte aligned", who);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    const long long crow = chroma_row_bytes(src->format, ((long long)W + 1) / 2);
    if (src->pitch_y < W) return fail("%s: pitch_y %lld is below the row's %d bytes", who, (long long)src->pitch_y, W);
    if (src->pitch_c < crow) return fail("%s: pitch_c %lld is below the row's %lld bytes", who, (long long)src->pitch_c, crow);
    if (src->frame_y < 0) return fail("%s: frame_y %lld is negative", who, (long long)src->frame_y);
    if (src->frame_c < 0) return fail("%s: frame_c %lld is negative", who, (long long)src->frame_c);
    const long long tx = ((long long)W + TW - 1) / TW, ty = ((long long)H + TH - 1) / TH;
    if ((long long)N * tx * ty > 0x7fffffffLL) return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);
    if (table_on_current(who, c->t)) return 1;

    DecodeArgs a;
    const bool nv = src->format == SESRQ_VIDEO_NV12;
    a.y = static_cast<const uint8_t *>(src->y);
    a.cb = static_cast<const uint8_t *>(src->c0);
    a.cr = nv ? a.cb + 1 : static_cast<const uint8_t *>(src->c1);
    a.tab = static_cast<const Tables *>(c->t.ptr);
    a.q0 = q0;
    a.x = x;
    a.pitch_y = src->pitch_y;
    a.frame_y = src->frame_y;
    a.pitch_c = src->pitch_c;
    a.frame_c = src->frame_c;
    a.H = H;
    a.W = W;
    a.tiles_x = (int)tx;
    a.tiles_y = (int)ty;
    const unsigned grid = (unsigned)((long long)N * tx * ty);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int outs = (q0 ? OUT_Q : 0) | (x ? OUT_F : 0);
    int k;
#define SESRQ_VRGB_DECODE(F, O, K)                              \
    if (src->format == F && outs == (O)) {                      \
        k = K;                                                  \
        vrgb_decode<F, (O)><<<grid, THREADS, 0, st>>>(a);       \
    }
    SESRQ_VRGB_DECODE(SESRQ_VIDEO_NV12, OUT_Q, K_NQ)
    else SESRQ_VRGB_DECODE(SESRQ_VIDEO_NV12, OUT_F, K_NF)
    else SESRQ_VRGB_DECODE(SESRQ_VIDEO_NV12, OUT_Q | OUT_F, K_NQF)
    else SESRQ_VRGB_DECODE(SESRQ_VIDEO_I420, OUT_Q, K_IQ)
    else SESRQ_VRGB_DECODE(SESRQ_VIDEO_I420, OUT_F, K_IF)
    else SESRQ_VRGB_DECODE(SESRQ_VIDEO_I420, OUT_Q | OUT_F, K_IQF)
    else return fail("%s: unreachable instantiation", who);
#undef SESRQ_VRGB_DECODE
    return launched(who, g_count, k);
}

extern "C" int sesrq_video_rgb_export(const void *pred, int dtype, float scale, int zero, const sesrq_video_surface *out, int N, int H,
                                      int W, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_video_rgb_export";
    if (!pred) return fail("%s: pred is NULL", who);
    if (dtype != SESRQ_VIDEO_F32 && dtype != SESRQ_VIDEO_I8) return fail("%s: dtype %d (0 = fp32, 1 = int8)", who, dtype);
    if (dtype == SESRQ_VIDEO_I8 && (!(scale > 0.f) || !std::isfinite(scale)))
        return fail("%s: an int8 pred needs a positive, finite output scale", who);
    if (dtype == SESRQ_VIDEO_I8 && (zero < -128 || zero > 127)) return fail("%s: zero %d outside the int8 range", who, zero);
    if (dtype == SESRQ_VIDEO_F32 && (reinterpret_cast<uintptr_t>(pred) & 3)) return fail("%s: an fp32 pred is not 4-byte aligned", who);
    if (!out) return fail("%s: out is NULL", who);
    if (check_format(who, "out", out->format)) return 1;
    if (!out->y) return fail("%s: the Y plane of out is NULL", who);
    if (!out->c0 || (out->format == SESRQ_VIDEO_I420 && !out->c1)) return fail("%s: a chroma plane of out is NULL", who);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    const long long pairs = ((long long)H + 1) / 2, segs = ((long long)W + SEG - 1) / SEG;
    const long long crow = chroma_row_bytes(out->format, ((long long)W + 1) / 2);
    if (out->pitch_y < W) return fail("%s: pitch_y %lld of out is below the row's %d bytes", who, (long long)out->pitch_y, W);
    if (out->pitch_c < crow) return fail("%s: pitch_c %lld of out is below the row's %lld bytes", who, (long long)out->pitch_c, crow);
    if (out->frame_y < 0 || out->frame_c < 0)
        return fail("%s: a frame stride of out (%lld, %lld) is negative", who, (long long)out->frame_y, (long long)out->frame_c);
    if (N > 1 && (out->frame_y < (H - 1) * out->pitch_y + W || out->frame_c < (pairs - 1) * out->pitch_c + crow))
        return fail("%s: a frame stride of out (%lld, %lld) is below its plane's extent", who, (long long)out->frame_y,
                    (long long)out->frame_c);
    // N pairs segs cannot overflow 64 bits: each factor is below 2^31 and segs below 2^27
    if ((long long)N * pairs > 0x7fffffffLL || (long long)N * pairs * segs > 0x7fffffffLL - EXP_THREADS)
        return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);

    ExportArgs a;
    a.pred = pred;
    a.oy = static_cast<uint8_t *>(out->y);
    a.o0 = static_cast<uint8_t *>(out->c0);
    a.o1 = static_cast<uint8_t *>(out->c1);
    a.pitch_y = out->pitch_y;
    a.frame_y = out->frame_y;
    a.pitch_c = out->pitch_c;
    a.frame_c = out->frame_c;
    a.items = (long long)N * pairs * segs;
    a.H = H;
    a.W = W;
    a.pairs = (int)pairs;
    a.segs = (int)segs;
    a.scale = scale;
    a.zero = zero;
    const unsigned grid = (unsigned)((a.items + EXP_THREADS - 1) / EXP_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int k;
#define SESRQ_VRGB_EXPORT(D, F, K)                                  \
    if (dtype == D && out->format == F) {                           \
        k = K;                                                      \
        vrgb_export<D, F><<<grid, EXP_THREADS, 0, st>>>(a);         \
    }
    SESRQ_VRGB_EXPORT(SESRQ_VIDEO_F32, SESRQ_VIDEO_NV12, K_EFN)
    else SESRQ_VRGB_EXPORT(SESRQ_VIDEO_F32, SESRQ_VIDEO_I420, K_EFI)
    else SESRQ_VRGB_EXPORT(SESRQ_VIDEO_I8, SESRQ_VIDEO_NV12, K_EQN)
    else SESRQ_VRGB_EXPORT(SESRQ_VIDEO_I8, SESRQ_VIDEO_I420, K_EQI)
    else return fail("%s: unreachable instantiation", who);
#undef SESRQ_VRGB_EXPORT
    return launched(who, g_count, k);
}

extern "C" int sesrq_video_rgb_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_video_rgb_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_video_rgb_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_video_rgb_last_error(void) { return g_err; }
