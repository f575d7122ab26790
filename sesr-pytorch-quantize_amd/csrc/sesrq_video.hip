// libsesrq_video.so: YUV 4:2:0 video frames (NV12 / I420) into and out of the luma super-resolution nets (include/sesrq_video.h, which
// fixes the arithmetic).  A library of its own: it links nothing of libsesrq.so, libsesrq_image.so or libsesrq_colour.so and registers
// nothing in their instance tables; the per-code table of the decode is the image library's (sesrq_image_decode.h), built once, and
// the weight table and the row padding of the export the colour library's too (sesrq_chroma_upscale.h); the
// staging through pitch and step, the luma load and the two passes (twins of the colour export's: see that header), the luma and
// chroma bytes and the NV12 / I420 stores are this file's.
//
// Decode: a stream over the Y plane, 1 B/px read through the surface's pitch; 1 B/px of q0 and 4 B/px of fp32 written.  A lane owns a
// run of 16 pixels of one row and looks each byte up in the 256-code table, staged in LDS after the lane's first run was requested.
//
// Export: a workgroup of 256 lanes owns 128 x 32 output luma bytes and the 64 x 16 chroma samples a plane under them: 16 x 4 LR chroma
// samples at r = 4, 32 x 8 at r = 2.  A lane owns 16 consecutive luma bytes of one row and requests its luma first (one 16-byte load of
// int8 Y, four of fp32), then its share of the two LR chroma tiles plus a halo of 2, coordinates clamped to the chroma plane of THIS
// frame of the batch; NV12 and I420 sources differ only in the byte step and the base of Cr.  While those fly the byte of every int8
// code goes to an LDS table.  The staged samples become Q6 int16 in LDS; the horizontal pass takes every staged row to 64 output
// columns, int16 in LDS, while the luma bytes are formed and stored; then the first two waves run the vertical pass, a lane 16 chroma
// bytes of one row -- 16 samples of a plane (I420) or eight Cb,Cr pairs (NV12) -- four LDS rows a sample, and store one 16-byte word.
// Runs that are partial (a plane's right edge) or whose addresses are not 16-byte aligned take per-element loads and stores around
// the same arithmetic.  No upscaled plane and no int16 plane reaches memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_video.h"
#include "sesrq_side.h"
#include "sesrq_image_decode.h"
#include "sesrq_chroma_upscale.h"

namespace sesrq_vidk {

constexpr int OUT_W = SESRQ_VIDEO_TILE_OUT_W, OUT_H = SESRQ_VIDEO_TILE_OUT_H;        // a workgroup's output luma tile, at r = 2 and 4
constexpr int CW = OUT_W / 2, CH = OUT_H / 2;               // ... and its output chroma tile, samples a plane
using sesrq_chroma::HALO;
using sesrq_chroma::SEG;                                    // output bytes per lane and run
using sesrq_chroma::first_tap;
using sesrq_chroma::half_of;
using sesrq_chroma::weight;
using sesrq_chroma::weight_of;
constexpr int CODES = SESRQ_VIDEO_CODES;
constexpr int DEC_THREADS = 128;
constexpr int BLOCKS_PER_CU = 16;                           // 128-thread blocks: a full CU (32 waves)
enum { OUT_Q = 1, OUT_F = 2 };

using sesrq_imgdec::Tables;
using sesrq_imgdec::RGB_WORDS;
static_assert(CODES == sesrq_imgdec::CODES, "one table for both libraries");

struct DecodeArgs {
    const uint8_t *y;
    const Tables *tab;
    int8_t *q0;
    float *x;
    int64_t pitch, frame;
    int H, W, segs, items;
};

struct ExportArgs {
    const void *y;
    const uint8_t *cb, *cr;         // LR chroma: sample (row, col) of plane p at p[row * lr_pitch + col * lr_step]
    uint8_t *oy, *o0, *o1;          // HR planes
    int64_t lr_pitch, lr_frame, pitch_y, frame_y, pitch_c, frame_c;
    int lr_step, H, W, tiles_x, tiles_y;
    float scale;
    int zero;
};

template <int OUT>
__global__ __launch_bounds__(DEC_THREADS) void video_decode(DecodeArgs a) {
    __shared__ uint4 s_tab[RGB_WORDS];
    const int stride = gridDim.x * DEC_THREADS;
    int i = blockIdx.x * DEC_THREADS + threadIdx.x;

    // the run of item i: source, first output index, pixel count, and whether it takes the 16-byte path
    auto run = [&](int it, const uint8_t *&src, size_t &o, int &npx, bool &vec) {
        const int row = it / a.segs, x0 = (it - row * a.segs) * SEG;        // row counts over the batch: n H + y
        const int n = row / a.H, yy = row - n * a.H;
        src = a.y + (int64_t)n * a.frame + (int64_t)yy * a.pitch + x0;
        o = (size_t)row * (size_t)a.W + (size_t)x0;
        npx = min(SEG, a.W - x0);
        vec = npx == SEG && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
              (!(OUT & OUT_Q) || (reinterpret_cast<uintptr_t>(a.q0 + o) & 15) == 0) &&
              (!(OUT & OUT_F) || (reinterpret_cast<uintptr_t>(a.x + o) & 15) == 0);
    };
    const uint8_t *src = nullptr;
    size_t o = 0;
    int npx = 0;
    bool vec = false;
    unsigned w[4] = {0, 0, 0, 0};
    auto load = [&]() {
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    };
    if (i < a.items) {                                    // requested before the table is staged
        run(i, src, o, npx, vec);
        if (vec) load();
    }
    sesrq_imgdec::stage_tables<SESRQ_IMAGE_RGB, DEC_THREADS>(s_tab, a.tab);
    __syncthreads();
    const float *tx = sesrq_imgdec::table_x(s_tab);
    const int8_t *tq = sesrq_imgdec::table_q(s_tab);

    for (; i < a.items; i += stride) {
        if (vec) {
            if (OUT & OUT_Q) {
                unsigned qq[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < SEG; ++k) qq[k >> 2] |= (unsigned)(uint8_t)tq[(w[k >> 2] >> (8 * (k & 3))) & 0xffu] << (8 * (k & 3));
                *reinterpret_cast<uint4 *>(a.q0 + o) = make_uint4(qq[0], qq[1], qq[2], qq[3]);
            }
            if (OUT & OUT_F) {
                float4 *d = reinterpret_cast<float4 *>(a.x + o);
#pragma unroll
                for (int k = 0; k < SEG / 4; ++k)
                    d[k] = make_float4(tx[w[k] & 0xffu], tx[(w[k] >> 8) & 0xffu], tx[(w[k] >> 16) & 0xffu], tx[w[k] >> 24]);
            }
        } else {
            for (int k = 0; k < npx; ++k) {
                const unsigned v = src[k];
                if (OUT & OUT_Q) a.q0[o + k] = tq[v];
                if (OUT & OUT_F) a.x[o + k] = tx[v];
            }
        }
        const int nx = i + stride;
        if (nx < a.items) {
            run(nx, src, o, npx, vec);
            if (vec) load();
        }
    }
}

// step 2 of the header: u = trunc(fl32(clip(p, 0, 1) * 255)); a NaN gives 0
__device__ inline unsigned to_byte(float p) { return (unsigned)__fmul_rn(fminf(fmaxf(p, 0.f), 1.f), 255.f); }

// step 3's last line: the byte of an upscaled Q6 sample
__device__ inline unsigned chroma_byte(int c) { return (unsigned)min(max((c + 32) >> 6, 0), 255); }

template <int R>
struct Shape {
    static constexpr int TW = CW / R, TH = CH / R;                 // the tile in LR chroma samples: 16 x 4 (r = 4), 32 x 8 (r = 2)
    static constexpr int SW = TW + 2 * HALO, SH = TH + 2 * HALO;   // the staged tile
    static constexpr int RUNS = OUT_W / SEG;                       // luma runs of a row: 8
    static constexpr int THREADS = RUNS * OUT_H;                   // a lane a luma run: 256
    static constexpr int CRUNS = 2 * CW * CH / SEG;                // chroma runs of a tile, both planes: 128
    static constexpr int HWORDS = sesrq_chroma::hwords(CW);        // words per row of the horizontal pass
    static constexpr int STAGE = (2 * SW * SH + THREADS - 1) / THREADS;
    static constexpr int HPASS = (2 * SH * TW + THREADS - 1) / THREADS;
};
static_assert(Shape<4>::THREADS == CODES && Shape<2>::THREADS == CODES, "one int8 code a lane");
static_assert(Shape<4>::CRUNS == 128 && Shape<4>::CRUNS % 64 == 0, "whole waves run the vertical pass");

// 8 waves a SIMD: four waves a workgroup, eight workgroups a CU
template <int YD, int R, int OF>
__global__ __launch_bounds__(Shape<R>::THREADS, 8) void video_export(ExportArgs a) {
    using S = Shape<R>;
    constexpr int THREADS = S::THREADS, RUNS = S::RUNS, TW = S::TW, TH = S::TH, SW = S::SW, SH = S::SH;
    __shared__ uint8_t s_u[YD == SESRQ_VIDEO_I8 ? CODES : 4];         // the byte of int8 code q at [q + 128]
    __shared__ int16_t s_c[2][SH][SW];                                // staged LR chroma, Q6
    __shared__ __align__(8) unsigned s_h[2][SH][S::HWORDS];           // the horizontal pass, two int16 a word
    const int tid = threadIdx.x;

    unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)a.tiles_x);
    t /= (unsigned)a.tiles_x;
    const int ty = (int)(t % (unsigned)a.tiles_y);
    const int64_t n = t / (unsigned)a.tiles_y;
    const int64_t rW = (int64_t)a.W * R, rH = (int64_t)a.H * R;       // the HR luma plane
    const int64_t cW = rW / 2, cH = rH / 2;                           // the HR chroma planes
    const int lW = (a.W + 1) / 2, lH = (a.H + 1) / 2;                 // the LR chroma planes

    // a lane's luma run: 16 output bytes of one row, requested first: the load flies while the chroma tile is staged
    const int row = tid / RUNS, run = tid % RUNS;
    const int64_t Y = (int64_t)ty * OUT_H + row, X0 = (int64_t)tx * OUT_W + (int64_t)run * SEG;
    const bool live = Y < rH && X0 < rW;
    const int npx = live ? (int)min((int64_t)SEG, rW - X0) : 0;
    const int64_t px = live ? (n * rH + Y) * rW + X0 : 0;
    uint8_t *dst = a.oy + (live ? n * a.frame_y + Y * a.pitch_y + X0 : 0);
    const float *yf = static_cast<const float *>(a.y) + px;
    const int8_t *yq = static_cast<const int8_t *>(a.y) + px;
    const bool vec = npx == SEG && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(YD == SESRQ_VIDEO_F32 ? (const void *)yf : (const void *)yq) & 15) == 0;
    float lum[YD == SESRQ_VIDEO_F32 ? SEG : 1];
    unsigned yw[4] = {0, 0, 0, 0};
    if (YD == SESRQ_VIDEO_F32) {
        if (vec) {
#pragma unroll
            for (int k = 0; k < SEG / 4; ++k) {
                const float4 v = reinterpret_cast<const float4 *>(yf)[k];
                lum[4 * k] = v.x; lum[4 * k + 1] = v.y; lum[4 * k + 2] = v.z; lum[4 * k + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k) lum[k] = k < npx ? yf[k] : 0.f;
        }
    } else {
        if (vec) {
            const uint4 v = *reinterpret_cast<const uint4 *>(yq);
            yw[0] = v.x; yw[1] = v.y; yw[2] = v.z; yw[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k)
                if (k < npx) yw[k >> 2] |= (unsigned)(uint8_t)yq[k] << (8 * (k & 3));
        }
    }

    // stage: both chroma tiles and their halo, clamped to this frame's planes; every load is requested before the first is used
    const int cx0 = tx * TW, cy0 = ty * TH;
    unsigned cs[S::STAGE];
#pragma unroll
    for (int i = 0; i < S::STAGE; ++i) {
        const int p = tid + i * THREADS;
        cs[i] = 0;
        if (p < 2 * SH * SW) {
            const int pl = p / (SH * SW), rem = p - pl * (SH * SW);
            const int hy = rem / SW, hx = rem - hy * SW;
            const int gy = min(max(cy0 - HALO + hy, 0), lH - 1), gx = min(max(cx0 - HALO + hx, 0), lW - 1);
            cs[i] = (pl ? a.cr : a.cb)[n * a.lr_frame + (int64_t)gy * a.lr_pitch + (int64_t)gx * a.lr_step];
        }
    }
    if (YD == SESRQ_VIDEO_I8)                                        // an int8 luma has 256 codes: the byte of each, one code a lane
        s_u[tid] = (uint8_t)to_byte(__fmul_rn((float)(tid - 128 - a.zero), a.scale));
#pragma unroll
    for (int i = 0; i < S::STAGE; ++i) {
        const int p = tid + i * THREADS;
        if (p < 2 * SH * SW) (&s_c[0][0][0])[p] = (int16_t)(cs[i] << 6);
    }
    __syncthreads();

    // horizontal pass: LR column j of a staged row gives output columns r j .. r j + r - 1
#pragma unroll
    for (int i = 0; i < S::HPASS; ++i) {
        const int u = tid + i * THREADS;
        if (u < 2 * SH * TW) {
            const int pl = u / (SH * TW), rem = u - pl * (SH * TW);
            const int hy = rem / TW, j = rem - hy * TW;
            int c[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) c[k] = s_c[pl][hy][j + k];          // LR columns j - 2 .. j + 2
            int o[R];
#pragma unroll
            for (int phi = 0; phi < R; ++phi) {
                const int f = first_tap(R, phi) + HALO;
                int s = 512;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += weight(R, phi, k) * c[f + k];
                o[phi] = s >> 10;
            }
            unsigned *hd = &s_h[pl][hy][R * j / 2];
#pragma unroll
            for (int k = 0; k < R / 2; ++k) hd[k] = ((unsigned)o[2 * k] & 0xffffu) | ((unsigned)o[2 * k + 1] << 16);
        }
    }

    // the luma bytes: an int8 code looks its byte up (code + 128 = the byte with its top bit flipped)
    if (live) {
        unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < SEG; ++k) {
            const unsigned u = YD == SESRQ_VIDEO_F32 ? to_byte(lum[k]) : (unsigned)s_u[((yw[k >> 2] >> (8 * (k & 3))) & 0xffu) ^ 0x80u];
            o[k >> 2] |= u << (8 * (k & 3));
        }
        if (vec) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k)
                if (k < npx) dst[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
        }
    }
    __syncthreads();
    if (tid >= S::CRUNS) return;                                     // whole waves

    // a lane's chroma run: 16 output bytes of one chroma row.  I420: 16 samples of one plane (a wave a plane); NV12: 8 Cb,Cr pairs
    constexpr bool NV = OF == SESRQ_VIDEO_NV12;
    constexpr int CR_ROW = NV ? 2 * CW / SEG : CW / SEG;             // runs of a tile's row: 8 (both planes) or 4 (one plane)
    const int pl = NV ? 0 : tid / (CR_ROW * CH);
    const int crow = (tid / CR_ROW) % CH, crun = tid % CR_ROW;
    constexpr int SPR = NV ? SEG / 2 : SEG;                          // samples a plane of a run
    const int x0 = crun * SPR;                                       // first sample, in the tile
    const int64_t CY = (int64_t)ty * CH + crow, CX0 = (int64_t)tx * CW + x0;
    if (CY >= cH || CX0 >= cW) return;
    const int ns = (int)min((int64_t)SPR, cW - CX0);
    uint8_t *cd = (NV || pl == 0 ? a.o0 : a.o1) + n * a.frame_c + CY * a.pitch_c + (NV ? 2 * CX0 : CX0);
    const bool cvec = ns == SPR && (reinterpret_cast<uintptr_t>(cd) & 15) == 0;

    // the vertical pass over four rows of the horizontal pass, four samples at a time
    const int li = crow / R, phi = crow % R;
    const int r0 = li + HALO + first_tap(R, phi);
    int wy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wy[k] = weight_of<R>(phi, k);
    auto four = [&](int p, int xs, unsigned (&b)[4]) {               // samples xs .. xs + 3 of plane p as bytes
        int up[4] = {512, 512, 512, 512};
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
            const uint2 v = *reinterpret_cast<const uint2 *>(&s_h[p][r0 + tp][xs / 2]);
            up[0] += __mul24(wy[tp], half_of(v.x, 0));               // |w| <= 1024, |h| < 2^15: a 24-bit multiply is exact
            up[1] += __mul24(wy[tp], half_of(v.x, 1));
            up[2] += __mul24(wy[tp], half_of(v.y, 0));
            up[3] += __mul24(wy[tp], half_of(v.y, 1));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = chroma_byte(up[k] >> 10);
    };
    unsigned o[4];
    if (NV) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            unsigned b0[4], b1[4];
            four(0, x0 + 4 * g, b0);
            four(1, x0 + 4 * g, b1);
            o[2 * g] = b0[0] | b1[0] << 8 | b0[1] << 16 | b1[1] << 24;
            o[2 * g + 1] = b0[2] | b1[2] << 8 | b0[3] << 16 | b1[3] << 24;
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            unsigned b[4];
            four(pl, x0 + 4 * g, b);
            o[g] = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
        }
    }
    if (cvec) {
        *reinterpret_cast<uint4 *>(cd) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        const int nb = NV ? 2 * ns : ns;
#pragma unroll
        for (int k = 0; k < SEG; ++k)
            if (k < nb) cd[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
}

}  // namespace sesrq_vidk

using namespace sesrq_vidk;

struct sesrq_video_ctx_s {
    DeviceTable t;     // Tables
    InQuant q;
};

static_assert(SESRQ_VIDEO_F32 == LUMA_F32 && SESRQ_VIDEO_I8 == LUMA_I8, "check_luma_export's y_dtype");

enum { K_DQ = 0, K_DF, K_DQF, K_Q2N, K_Q2I, K_Q4N, K_Q4I, K_F2N, K_F2I, K_F4N, K_F4I, K_COUNT };
static const char *const kNames[K_COUNT] = {"video_decode<q0>",           "video_decode<x>",           "video_decode<q0,x>",
                                            "video_export<i8,r2,nv12>",   "video_export<i8,r2,i420>",  "video_export<i8,r4,nv12>",
                                            "video_export<i8,r4,i420>",   "video_export<f32,r2,nv12>", "video_export<f32,r2,i420>",
                                            "video_export<f32,r4,nv12>",  "video_export<f32,r4,i420>"};
static Counters<K_COUNT> g_count{kNames};

using sesrq_imgdec::build;

extern "C" int sesrq_video_table(float scale_in, int zero_in, int exact_div, int8_t q[SESRQ_VIDEO_CODES], float x[SESRQ_VIDEO_CODES]) {
    g_err[0] = 0;
    if (!q || !x) return fail("sesrq_video_table: q or x is NULL");
    if (check_domain("sesrq_video_table", scale_in, zero_in, exact_div)) return 1;
    static thread_local Tables t;
    build(in_quant(scale_in, zero_in, exact_div), t);
    for (int v = 0; v < CODES; ++v) {
        q[v] = t.q[v];
        x[v] = t.x[v];
    }
    return 0;
}

extern "C" int sesrq_video_create(float scale_in, int zero_in, int exact_div, sesrq_video_ctx *out) {
    g_err[0] = 0;
    if (!out) return fail("sesrq_video_create: ctx is NULL");
    *out = nullptr;
    if (check_domain("sesrq_video_create", scale_in, zero_in, exact_div)) return 1;
    auto *c = new sesrq_video_ctx_s();
    c->q = in_quant(scale_in, zero_in, exact_div);
    Tables *host = new Tables();
    build(c->q, *host);
    const hipError_t e = table_create(c->t, host, sizeof(Tables));
    delete host;
    if (e != hipSuccess) {
        delete c;
        return fail("sesrq_video_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

extern "C" void sesrq_video_destroy(sesrq_video_ctx c) { ctx_destroy(c); }

static int check_format(const char *who, const char *what, int format) {
    if (format != SESRQ_VIDEO_NV12 && format != SESRQ_VIDEO_I420) return fail("%s: %s format %d (0 = NV12, 1 = I420)", who, what, format);
    return 0;
}

// the bytes of a chroma row of a surface whose chroma planes are cw samples wide
static long long chroma_row_bytes(int format, long long cw) { return format == SESRQ_VIDEO_NV12 ? 2 * cw : cw; }

extern "C" int sesrq_video_decode(sesrq_video_ctx c, const sesrq_video_surface *src, int8_t *q0, float *x, int N, int H, int W,
                                  void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_video_decode";
    if (!c) return fail("%s: ctx is NULL", who);
    if (!src) return fail("%s: src is NULL", who);
    if (!src->y) return fail("%s: the Y plane of src is NULL", who);
    if (!q0 && !x) return fail("%s: neither q0 nor x requested", who);
    if (reinterpret_cast<uintptr_t>(x) & 3) return fail("%s: x is not 4-byte aligned", who);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    if (src->pitch_y < W) return fail("%s: pitch_y %lld is below the row's %d bytes", who, (long long)src->pitch_y, W);
    if (src->frame_y < 0) return fail("%s: frame_y %lld is negative", who, (long long)src->frame_y);
    // the generous grid round (1024 CUs) keeps the size check before any HIP call
    if ((long long)N * H > 0x7fffffffLL) return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);
    int segs, items;
    if (segment_items(who, N, H, W, SEG, (long long)DEC_THREADS * 1024 * BLOCKS_PER_CU, &segs, &items)) return 1;
    if (table_on_current(who, c->t)) return 1;

    DecodeArgs a;
    a.y = static_cast<const uint8_t *>(src->y);
    a.tab = static_cast<const Tables *>(c->t.ptr);
    a.q0 = q0;
    a.x = x;
    a.pitch = src->pitch_y;
    a.frame = src->frame_y;
    a.H = H;
    a.W = W;
    a.segs = segs;
    a.items = items;
    const int grid = grid_cap(items, DEC_THREADS, c->t.num_cu > 1024 ? 1024 : c->t.num_cu, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int k;
    if (q0 && x) {
        k = K_DQF;
        video_decode<OUT_Q | OUT_F><<<grid, DEC_THREADS, 0, st>>>(a);
    } else if (q0) {
        k = K_DQ;
        video_decode<OUT_Q><<<grid, DEC_THREADS, 0, st>>>(a);
    } else {
        k = K_DF;
        video_decode<OUT_F><<<grid, DEC_THREADS, 0, st>>>(a);
    }
    return launched(who, g_count, k);
}

extern "C" int sesrq_video_export(const void *y, int y_dtype, float scale, int zero, const sesrq_video_surface *lr, int r,
                                  const sesrq_video_surface *out, int N, int H, int W, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_video_export";
    ExportArgs a;
    if (check_luma_export(who, y, y_dtype, scale, zero, r, N, H, W, OUT_W, OUT_H, &a.tiles_x, &a.tiles_y)) return 1;
    if (!lr) return fail("%s: lr is NULL", who);
    if (!out) return fail("%s: out is NULL", who);
    if (check_format(who, "lr", lr->format) || check_format(who, "out", out->format)) return 1;
    if (!lr->c0 || (lr->format == SESRQ_VIDEO_I420 && !lr->c1)) return fail("%s: a chroma plane of lr is NULL", who);
    if (!out->y) return fail("%s: the Y plane of out is NULL", who);
    if (!out->c0 || (out->format == SESRQ_VIDEO_I420 && !out->c1)) return fail("%s: a chroma plane of out is NULL", who);
    const long long rW = (long long)r * W, rH = (long long)r * H;
    const long long lrow = chroma_row_bytes(lr->format, ((long long)W + 1) / 2), orow = chroma_row_bytes(out->format, rW / 2);
    if (lr->pitch_c < lrow) return fail("%s: pitch_c %lld of lr is below the row's %lld bytes", who, (long long)lr->pitch_c, lrow);
    if (out->pitch_y < rW) return fail("%s: pitch_y %lld of out is below the row's %lld bytes", who, (long long)out->pitch_y, rW);
    if (out->pitch_c < orow) return fail("%s: pitch_c %lld of out is below the row's %lld bytes", who, (long long)out->pitch_c, orow);
    if (lr->frame_c < 0) return fail("%s: frame_c %lld of lr is negative", who, (long long)lr->frame_c);
    if (N > 1 && (out->frame_y < (rH - 1) * out->pitch_y + rW || out->frame_c < (rH / 2 - 1) * out->pitch_c + orow))
        return fail("%s: a frame stride of out (%lld, %lld) is below its plane's extent", who, (long long)out->frame_y,
                    (long long)out->frame_c);

    a.y = y;
    const bool lnv = lr->format == SESRQ_VIDEO_NV12;
    a.cb = static_cast<const uint8_t *>(lr->c0);
    a.cr = lnv ? a.cb + 1 : static_cast<const uint8_t *>(lr->c1);
    a.lr_step = lnv ? 2 : 1;
    a.lr_pitch = lr->pitch_c;
    a.lr_frame = lr->frame_c;
    a.oy = static_cast<uint8_t *>(out->y);
    a.o0 = static_cast<uint8_t *>(out->c0);
    a.o1 = static_cast<uint8_t *>(out->c1);
    a.pitch_y = out->pitch_y;
    a.frame_y = out->frame_y;
    a.pitch_c = out->pitch_c;
    a.frame_c = out->frame_c;
    a.H = H;
    a.W = W;
    a.scale = scale;
    a.zero = zero;
    const unsigned grid = (unsigned)N * a.tiles_x * a.tiles_y;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int of = out->format;
    int k;
#define SESRQ_VIDEO_EXPORT(D, R, F, K)                                                 \
    if (y_dtype == D && r == R && of == F) {                                           \
        k = K;                                                                         \
        video_export<D, R, F><<<grid, Shape<R>::THREADS, 0, st>>>(a);                  \
    }
    SESRQ_VIDEO_EXPORT(SESRQ_VIDEO_I8, 2, SESRQ_VIDEO_NV12, K_Q2N)
    else SESRQ_VIDEO_EXPORT(SESRQ_VIDEO_I8, 2, SESRQ_VIDEO_I420, K_Q2I)
    else SESRQ_VIDEO_EXPORT(SESRQ_VIDEO_I8, 4, SESRQ_VIDEO_NV12, K_Q4N)
    else SESRQ_VIDEO_EXPORT(SESRQ_VIDEO_I8, 4, SESRQ_VIDEO_I420, K_Q4I)
    else SESRQ_VIDEO_EXPORT(SESRQ_VIDEO_F32, 2, SESRQ_VIDEO_NV12, K_F2N)
    else SESRQ_VIDEO_EXPORT(SESRQ_VIDEO_F32, 2, SESRQ_VIDEO_I420, K_F2I)
    else SESRQ_VIDEO_EXPORT(SESRQ_VIDEO_F32, 4, SESRQ_VIDEO_NV12, K_F4N)
    else SESRQ_VIDEO_EXPORT(SESRQ_VIDEO_F32, 4, SESRQ_VIDEO_I420, K_F4I)
    else return fail("%s: unreachable instantiation", who);
#undef SESRQ_VIDEO_EXPORT
    return launched(who, g_count, k);
}

extern "C" int sesrq_video_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_video_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_video_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_video_last_error(void) { return g_err; }
