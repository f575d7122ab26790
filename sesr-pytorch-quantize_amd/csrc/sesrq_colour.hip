// libsesrq_colour.so: colour out of the luma super-resolution nets (include/sesrq_colour.h, which fixes the arithmetic).  A library of
// its own: it links nothing of libsesrq.so or libsesrq_image.so and registers nothing in their instance tables.  The weight
// table and the row padding are sesrq_chroma_upscale.h's, which the video library uses too; the Q6 chroma of
// RGB bytes, the wave-uniform phases, the luma load and the two passes (twins of the video export's: see that header), the colour
// matrix and the 48-byte store are this file's.
//
// The net super-resolves Y; Cb and Cr of the LR image are upscaled bicubically (Keys a = -1/2, exact integers) and YCbCr goes back to
// RGB bytes, in ONE kernel on the HR side: per output pixel 1 (int8) or 4 (fp32) bytes of Y and 3 / r^2 bytes of the LR image are
// read, 3 bytes written, and no chroma plane ever reaches memory.
//
// Export: a workgroup of 256 lanes owns 128 x 32 output pixels: 32 x 8 LR pixels at r = 4, 64 x 16 at r = 2.  A lane owns 16
// consecutive output pixels of one output row, as image_export does, and requests its luma first (one 16-byte load of int8 Y, four
// of fp32), then its share of the LR tile plus a halo of 2, coordinates clamped to the frame of THIS image of the batch.  While those
// fly, d(v) = v / 255.0 of every byte code goes to LDS (one float64 division a lane; the six products of the chroma matrix are formed
// per staged pixel from it).  The staged pixels become (Cb, Cr) Q6, int16 in LDS; the horizontal pass takes every staged row to 128
// output columns, int16 in LDS; then the lane runs the vertical pass over four LDS rows and the colour matrix, four pixels at a time,
// and stores three 16-byte words.  A wave takes the rows of one vertical phase, so its four weights are scalars.  Runs that are
// partial (the frame's right edge) or whose Y / out addresses are not 16-byte aligned take per-element loads and stores around the
// same arithmetic.  An int8 luma has 256 codes, so a(q) of steps 3 and 4 is an LDS table made in the prologue.  64 VGPRs or fewer:
// eight waves a SIMD, so the 2040 tiles of a 540p -> 4K frame are resident at once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_colour.h"
#include "sesrq_side.h"
#include "sesrq_chroma_upscale.h"

namespace sesrq_colk {

using sesrq_chroma::HALO;
using sesrq_chroma::SEG;                                    // output pixels per lane
using sesrq_chroma::first_tap;
using sesrq_chroma::half_of;
using sesrq_chroma::weight;
using sesrq_chroma::weight_of;

constexpr int OUT_W = SESRQ_COLOUR_TILE_OUT_W, OUT_H = SESRQ_COLOUR_TILE_OUT_H;      // a workgroup's output tile, at r = 2 and 4
constexpr int CODES = 256;
constexpr int CHROMA_THREADS = 256;
constexpr int CHROMA_BLOCKS = 2048;

struct ExportArgs {
    const void *y;
    const uint8_t *img;
    uint8_t *out;
    int H, W, tiles_x, tiles_y, bgr;
    float scale;
    int zero;
};

struct ChromaArgs {
    const uint8_t *img;
    int16_t *cbcr;
    size_t HW;
    int N, bgr;
};

// d(v) of every byte code into LDS
template <int THREADS>
__device__ inline void stage_codes(double *s_d) {
    for (int v = threadIdx.x; v < CODES; v += THREADS) s_d[v] = __ddiv_rn((double)v, 255.0);   // a true quotient
}

// step 1 of the header: the Q6 chroma of one pixel from its three bytes in memory order
__device__ inline void chroma_q6(const double *d, unsigned b0, unsigned b1, unsigned b2, int bgr, int &Cb, int &Cr) {
    const double dr = d[bgr ? b2 : b0], dg = d[b1], db = d[bgr ? b0 : b2];
    double cb = __dadd_rn(__dmul_rn(-37.797, dr), __dmul_rn(-74.203, dg));
    cb = __dadd_rn(cb, __dmul_rn(112.0, db));
    cb = __dadd_rn(cb, 128.0);
    double cr = __dadd_rn(__dmul_rn(112.0, dr), __dmul_rn(-93.786, dg));
    cr = __dadd_rn(cr, __dmul_rn(-18.214, db));
    cr = __dadd_rn(cr, 128.0);
    Cb = __double2int_rn(__dmul_rn(64.0, cb));
    Cr = __double2int_rn(__dmul_rn(64.0, cr));
}

__global__ __launch_bounds__(CHROMA_THREADS) void colour_chroma(ChromaArgs a) {
    __shared__ double s_d[CODES];
    stage_codes<CHROMA_THREADS>(s_d);
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * CHROMA_THREADS;
    for (int n = 0; n < a.N; ++n) {
        const uint8_t *src = a.img + (size_t)n * a.HW * 3;
        int16_t *dst = a.cbcr + (size_t)n * 2 * a.HW;
        for (size_t p = (size_t)blockIdx.x * CHROMA_THREADS + threadIdx.x; p < a.HW; p += stride) {
            int Cb, Cr;
            chroma_q6(s_d, src[3 * p], src[3 * p + 1], src[3 * p + 2], a.bgr, Cb, Cr);
            dst[p] = (int16_t)Cb;
            dst[a.HW + p] = (int16_t)Cr;
        }
    }
}

// steps 3 and 4 up to a: a = 1.16438356 (clip(p, 0, 1) * 255 - 16), every operation rounded; a NaN p gives a(0)
__device__ inline float luma_term(float p) {
    const float yy = __fmul_rn(fminf(fmaxf(p, 0.f), 1.f), 255.f);
    return __fmul_rn(1.16438356f, __fsub_rn(yy, 16.0f));
}

template <int R>
struct Shape {
    static constexpr int TW = OUT_W / R, TH = OUT_H / R;           // the tile in LR pixels: 32 x 8 (r = 4), 64 x 16 (r = 2)
    static constexpr int SW = TW + 2 * HALO, SH = TH + 2 * HALO;   // the staged tile
    static constexpr int RUNS = OUT_W / SEG;
    static constexpr int THREADS = RUNS * OUT_H;                   // a lane a run: 256
    static constexpr int HWORDS = sesrq_chroma::hwords(OUT_W);     // words per row of the horizontal pass
    static constexpr int STAGE = (SW * SH + THREADS - 1) / THREADS;
};
static_assert(Shape<4>::TW == SESRQ_COLOUR_TILE_W && Shape<4>::TH == SESRQ_COLOUR_TILE_H, "the header's r = 4 tile");
static_assert(Shape<2>::TW == 2 * SESRQ_COLOUR_TILE_W && Shape<2>::TH == 2 * SESRQ_COLOUR_TILE_H, "the header's r = 2 tile");

// 8 waves a SIMD: with four waves a workgroup, a 540p -> 4K frame's 2040 tiles are resident at once on 256 CUs
template <int YD, int R>
__global__ __launch_bounds__(Shape<R>::THREADS, 8) void colour_export(ExportArgs a) {
    using S = Shape<R>;
    constexpr int THREADS = S::THREADS, RUNS = S::RUNS, TW = S::TW, TH = S::TH, SW = S::SW, SH = S::SH;
    __shared__ double s_d[CODES];
    __shared__ float s_a[YD == SESRQ_COLOUR_I8 ? CODES : 1];          // a of int8 code q at [q + 128]
    __shared__ int16_t s_c[2][SH][SW];
    __shared__ __align__(8) unsigned s_h[2][SH][S::HWORDS];           // two int16 a word
    const int tid = threadIdx.x;

    unsigned t = blockIdx.x;
    const int tx0 = (int)(t % (unsigned)a.tiles_x) * TW;
    t /= (unsigned)a.tiles_x;
    const int ty0 = (int)(t % (unsigned)a.tiles_y) * TH;
    const size_t n = t / (unsigned)a.tiles_y;
    const size_t W = (size_t)a.W, H = (size_t)a.H, rW = W * R, rH = H * R;

    // a lane's run: 16 output pixels of one output row.  A wave takes the rows of ONE vertical phase (r = 4: wave w the rows 4 i + w;
    // r = 2: rows 2 i + (w & 1) of the tile's upper or lower half), so the four vertical weights are wave-uniform.  The run's luma
    // is requested first: the load flies while the tile is staged
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int phi = wave % R, li = (wave / R) * (64 / RUNS) + lane / RUNS, run = lane % RUNS;
    const int row = li * R + phi;
    const size_t Y = (size_t)ty0 * R + row, X0 = (size_t)tx0 * R + (size_t)run * SEG;
    const bool live = Y < rH && X0 < rW;
    const int npx = live ? (int)min((size_t)SEG, rW - X0) : 0;
    const size_t px = live ? (n * rH + Y) * rW + X0 : 0;
    uint8_t *dst = a.out + px * 3;
    const float *yf = static_cast<const float *>(a.y) + px;
    const int8_t *yq = static_cast<const int8_t *>(a.y) + px;
    const bool vec = npx == SEG && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(YD == SESRQ_COLOUR_F32 ? (const void *)yf : (const void *)yq) & 15) == 0;
    float lum[YD == SESRQ_COLOUR_F32 ? SEG : 1];
    unsigned yw[4] = {0, 0, 0, 0};
    if (YD == SESRQ_COLOUR_F32) {
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

    // stage: the tile and its halo, clamped to this frame, as Q6 chroma; every load is requested before the first is used
    const uint8_t *frame = a.img + n * H * W * 3;
    unsigned rgb[S::STAGE];
#pragma unroll
    for (int i = 0; i < S::STAGE; ++i) {
        const int p = tid + i * THREADS;
        rgb[i] = 0;
        if (p < SH * SW) {
            const int hy = p / SW, hx = p - hy * SW;
            const int gy = min(max(ty0 - HALO + hy, 0), a.H - 1), gx = min(max(tx0 - HALO + hx, 0), a.W - 1);
            const uint8_t *src = frame + ((size_t)gy * W + (size_t)gx) * 3;
            rgb[i] = (unsigned)src[0] | (unsigned)src[1] << 8 | (unsigned)src[2] << 16;
        }
    }
    stage_codes<THREADS>(s_d);
    if (YD == SESRQ_COLOUR_I8) {                                     // an int8 luma has 256 codes: a(q) of steps 3 and 4, one code a lane
        static_assert(THREADS == CODES, "one int8 code a lane");
        s_a[tid] = luma_term(__fmul_rn((float)(tid - 128 - a.zero), a.scale));
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < S::STAGE; ++i) {
        const int p = tid + i * THREADS;
        if (p < SH * SW) {
            const int hy = p / SW, hx = p - hy * SW;
            int Cb, Cr;
            chroma_q6(s_d, rgb[i] & 0xffu, (rgb[i] >> 8) & 0xffu, rgb[i] >> 16, a.bgr, Cb, Cr);
            s_c[0][hy][hx] = (int16_t)Cb;
            s_c[1][hy][hx] = (int16_t)Cr;
        }
    }
    __syncthreads();

    // horizontal pass: LR column j of a staged row gives output columns r j .. r j + r - 1
    for (int u = tid; u < 2 * SH * TW; u += THREADS) {
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
    __syncthreads();
    if (!live) return;

    // the vertical pass over four rows of the horizontal pass and the colour matrix, four pixels at a time
    const int r0 = li + HALO + first_tap(R, phi);
    int wy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wy[k] = weight_of<R>(phi, k);
    unsigned o[3 * SEG / 4];
#pragma unroll
    for (int j = 0; j < 3 * SEG / 4; ++j) o[j] = 0;
#pragma unroll
    for (int g = 0; g < SEG / 4; ++g) {
        int up[2][4];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
            for (int k = 0; k < 4; ++k) up[pl][k] = 512;
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) {
                const uint2 v = *reinterpret_cast<const uint2 *>(&s_h[pl][r0 + tp][run * SEG / 2 + 2 * g]);
                up[pl][0] += __mul24(wy[tp], half_of(v.x, 0));          // |w| <= 1024, |h| < 2^15: a 24-bit multiply is exact
                up[pl][1] += __mul24(wy[tp], half_of(v.x, 1));
                up[pl][2] += __mul24(wy[tp], half_of(v.y, 0));
                up[pl][3] += __mul24(wy[tp], half_of(v.y, 1));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) up[pl][k] >>= 10;
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = 4 * g + kk;
            // luma: a of the header's steps 3 and 4; an int8 code looks it up (code + 128 = the byte with its top bit flipped)
            const float aa = YD == SESRQ_COLOUR_F32 ? luma_term(lum[k]) : s_a[((yw[g] >> (8 * kk)) & 0xffu) ^ 0x80u];
            // colour: fp32, every operation rounded.  The header's c * 0.015625f is exact and a power of two, so it is folded into the
            // coefficients: fl(k * (c / 64)) == fl((k / 64) * c) bit for bit (k / 64 is exact, nothing here under- or overflows)
            const float cb = (float)(up[0][kk] - 8192), cr = (float)(up[1][kk] - 8192);
            const float fr = __fadd_rn(aa, __fmul_rn(1.59602679f * 0.015625f, cr));
            const float fg = __fsub_rn(__fsub_rn(aa, __fmul_rn(0.39176229f * 0.015625f, cb)), __fmul_rn(0.81296765f * 0.015625f, cr));
            const float fb = __fadd_rn(aa, __fmul_rn(2.01723214f * 0.015625f, cb));
            // one v_cvt_pk_u8_f32 a byte: clamp(rint(.), 0, 255), ties to even, inserted into its byte of the word
            const float b[3] = {a.bgr ? fb : fr, fg, a.bgr ? fr : fb};
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(3 * k + c) >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(b[c], (3 * k + c) & 3, o[(3 * k + c) >> 2]);
        }
    }
    if (vec) {
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
#pragma unroll
        for (int k = 0; k < 3; ++k) d4[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    } else {
        const int nb = 3 * npx;
#pragma unroll
        for (int j = 0; j < 3 * SEG; ++j)
            if (j < nb) dst[j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
    }
}

}  // namespace sesrq_colk

using namespace sesrq_colk;

static_assert(SESRQ_COLOUR_F32 == LUMA_F32 && SESRQ_COLOUR_I8 == LUMA_I8, "check_luma_export's y_dtype");

enum { K_Q2 = 0, K_Q4, K_F2, K_F4, K_CHROMA, K_COUNT };
static const char *const kNames[K_COUNT] = {"colour_export<i8,r2>", "colour_export<i8,r4>", "colour_export<f32,r2>",
                                            "colour_export<f32,r4>", "colour_chroma"};
static Counters<K_COUNT> g_count{kNames};

extern "C" int sesrq_colour_weights(int r, int16_t *w, int8_t *first) {
    g_err[0] = 0;
    if (r != 2 && r != 4) return fail("sesrq_colour_weights: r = %d (2 or 4)", r);
    if (!w || !first) return fail("sesrq_colour_weights: w or first is NULL");
    for (int phi = 0; phi < r; ++phi) {
        first[phi] = (int8_t)first_tap(r, phi);
        for (int k = 0; k < 4; ++k) w[4 * phi + k] = (int16_t)weight(r, phi, k);
    }
    return 0;
}

static int check_order(const char *who, int order) {
    if (order != SESRQ_COLOUR_ORDER_RGB && order != SESRQ_COLOUR_ORDER_BGR) return fail("%s: order %d (0 = RGB, 1 = BGR)", who, order);
    return 0;
}

extern "C" int sesrq_colour_chroma(const uint8_t *img, int order, int16_t *cbcr, int N, int H, int W, void *stream) {
    g_err[0] = 0;
    if (!img) return fail("sesrq_colour_chroma: img is NULL");
    if (!cbcr) return fail("sesrq_colour_chroma: cbcr is NULL");
    if (reinterpret_cast<uintptr_t>(cbcr) & 1) return fail("sesrq_colour_chroma: cbcr is not 2-byte aligned");
    if (check_order("sesrq_colour_chroma", order)) return 1;
    if (N < 1 || H < 1 || W < 1) return fail("sesrq_colour_chroma: empty frame (N = %d, H = %d, W = %d)", N, H, W);

    ChromaArgs a;
    a.img = img;
    a.cbcr = cbcr;
    a.HW = (size_t)H * (size_t)W;
    a.N = N;
    a.bgr = order == SESRQ_COLOUR_ORDER_BGR;
    const size_t want = (a.HW + CHROMA_THREADS - 1) / CHROMA_THREADS;
    const int grid = (int)(want < (size_t)CHROMA_BLOCKS ? want : (size_t)CHROMA_BLOCKS);
    colour_chroma<<<grid, CHROMA_THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    return launched("sesrq_colour_chroma", g_count, K_CHROMA);
}

extern "C" int sesrq_colour_export(const void *y, int y_dtype, float scale, int zero, const uint8_t *img, int order, int r,
                                   uint8_t *out, int N, int H, int W, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_colour_export";
    ExportArgs a;
    if (check_luma_export(who, y, y_dtype, scale, zero, r, N, H, W, OUT_W, OUT_H, &a.tiles_x, &a.tiles_y)) return 1;
    if (!img) return fail("%s: img is NULL", who);
    if (!out) return fail("%s: out is NULL", who);
    if (check_order(who, order)) return 1;

    a.y = y;
    a.img = img;
    a.out = out;
    a.H = H;
    a.W = W;
    a.bgr = order == SESRQ_COLOUR_ORDER_BGR;
    a.scale = scale;
    a.zero = zero;
    const unsigned grid = (unsigned)N * a.tiles_x * a.tiles_y;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int k;
#define SESRQ_COLOUR_EXPORT(D, R, K)                                                   \
    if (y_dtype == D && r == R) {                                                      \
        k = K;                                                                         \
        colour_export<D, R><<<grid, Shape<R>::THREADS, 0, st>>>(a);                    \
    }
    SESRQ_COLOUR_EXPORT(SESRQ_COLOUR_I8, 2, K_Q2)
    else SESRQ_COLOUR_EXPORT(SESRQ_COLOUR_I8, 4, K_Q4)
    else SESRQ_COLOUR_EXPORT(SESRQ_COLOUR_F32, 2, K_F2)
    else SESRQ_COLOUR_EXPORT(SESRQ_COLOUR_F32, 4, K_F4)
    else return fail("%s: unreachable instantiation", who);
#undef SESRQ_COLOUR_EXPORT
    return launched(who, g_count, k);
}

extern "C" int sesrq_colour_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_colour_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_colour_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_colour_last_error(void) { return g_err; }
