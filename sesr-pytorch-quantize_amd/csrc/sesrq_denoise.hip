// libsesrq_denoise.so: non-local means of a Bayer frame with the shot / read noise model's variance (include/sesrq_denoise.h, which
// fixes the arithmetic): the classical denoise baseline of the raw nets.  A library of its own: it links nothing of the other
// libraries and registers nothing in their instance tables.  The packed formats are decoded with the helpers of sesrq_bayer_unpack.h
// (device code, compiled into this library's own kernels).
//
// Kernel.  One 256-lane workgroup owns a tile of 64 x 32 output pixels.  Some 2600 fp32 operations a pixel against 14 - 20 B of traffic:
// the design is about VALU issue and LDS reads, not HBM.
//   stage    the tile and its halo of 8 (6 of the search, 2 of the patch: 80 x 48 samples) go to LDS as two fp32 planes, c (the clamped
//            sample) and g = 1 / max(2 v, 2^-100) (the one division per sample).  A plane holds ROW PAIRS: element (row, col) is float
//            (row >> 1) * 2 PITCH + 2 col + (row & 1), so one 16-byte word is the 2 x 2 cell of two rows and two columns.  Tile origins,
//            the halo, a lane's block and every candidate shift are even, so every window any lane ever reads starts on such a word.
//            One work item is a row pair of a segment (8 pixels of U16 / spread: 24 x 10 items, one round of the workgroup; 16 of a
//            packed row, the halo's 8 columns sample by sample): two loads of the kind the demosaic kernel makes, then 16-byte LDS
//            writes.  Coordinates are folded while staging, so the loops below carry no edge tests.
//   compute  lane (lx, ly) = (tid >> 4, tid & 15) owns the 4 x 2 block at (4 lx, 2 ly) of the tile.  Its 8 x 6 footprint (block + patch
//            radius 2) of c and of g is read once into 2 x 48 VGPRs as 24 + 24 vertical pairs and stays there for all 49 candidates.
//            Per candidate only the shifted footprint c(q + .) comes from LDS: 12 ds_read_b128, all aligned, nothing read twice and
//            nothing unused.  Then, on vertical pairs throughout (the compiler issues v_pk_add_f32 / v_pk_mul_f32 on them):
//            e over the footprint once (24 pairs, not 8 x 25 values), the row sums r once per footprint row (12 pairs x 4 adds), the
//            block's 8 Dp from them, the weights and the two accumulators as 4 pairs.  6 e a pixel and candidate instead of 25.
//            LDS banks: the 16 lanes of one lx read 16 bytes each, PITCH * 8 = 656 bytes apart = 4 banks (mod 32; 36 mod 64): each group
//            of lanes the LDS serves together covers the banks evenly.  That is why ly, not lx, is the fast lane index.
//   store    out = num / den in the site plane, +0.0 in the two others: per block row and plane one 16-byte store (wide path), else
//            per pixel.  The site planes are arithmetic on (cfa, y & 1, x & 1) at the store; the CFA order is no template parameter.
// Instantiations: input (u16, raw10, raw12, spread) x levels (scalars, device array) x path (wide, per sample).
// No MFMA: every sum here is fp32 in a fixed order and every product is elementwise; there is no matrix product to hand over.
// The inner candidate loop is unrolled (its 7 LDS offsets are immediates): 7 - 14 % faster than the rolled loop at 8 more VGPRs
// (profiles/denoise_probe.txt).  Two side builds of tools/denoise_probe.py, never shipped: -DSESRQ_DENOISE_DIRECT evaluates each
// pixel's 25 terms on their own, -DSESRQ_DENOISE_UNROLL_I=1 keeps the inner loop rolled.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_bayer_unpack.h"
#include "sesrq_denoise.h"
#include "sesrq_side.h"

#ifndef SESRQ_DENOISE_UNROLL_I
#define SESRQ_DENOISE_UNROLL_I 7
#endif
#define SESRQ_PRAGMA(x) _Pragma(#x)
#define SESRQ_UNROLL(n) SESRQ_PRAGMA(unroll n)

namespace sesrq_denoisek {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int TW = 64, TH = 32;                    // tile of output pixels
constexpr int SEARCH = 3, PATCH = 2;               // candidates q = p + 2 (j, i), |i|, |j| <= SEARCH; patch radius
constexpr int HALO = 2 * SEARCH + PATCH;           // 8
constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO, LP = LH / 2;      // 80 x 48 staged samples; 24 row pairs
constexpr int PITCH = 82;                          // row pairs are PITCH float2 apart: >= LW, even, and PITCH * 2 = 4 mod 8 banks
constexpr int PW = 4, PH = 2;                      // a lane's block
constexpr int FW = PW + 2 * PATCH, FP = (PH + 2 * PATCH) / 2;           // its footprint: 8 columns, 3 row pairs
enum { IN_U16, IN_RAW10, IN_RAW12, IN_SPREAD, IN_COUNT };
static_assert(IN_U16 == sesrq_bayer::PACK_U16 && IN_RAW10 == sesrq_bayer::PACK_RAW10 && IN_RAW12 == sesrq_bayer::PACK_RAW12, "raw inputs are the body's packings");
static_assert(SESRQ_PACK_U16 == IN_U16 && SESRQ_PACK_RAW10 == IN_RAW10 && SESRQ_PACK_RAW12 == IN_RAW12, "... and the header's");
static_assert((TW / PW) * (TH / PH) == THREADS && PH == 2 && PW % 2 == 0 && HALO % 2 == 0 && PITCH >= LW && PITCH % 2 == 0, "tile geometry");

struct Args {
    const uint8_t *src;      // raw rows, or the spread frame's floats
    float *out;
    const float *levels;     // N (shot, read) pairs, or unused
    size_t stride;           // raw: bytes between rows
    int H, W, tiles_x, tiles_y;
    unsigned black, white;   // raw levels
    float D;                 // fl32(white - black)
    float shot, read, rh;    // scalar levels; fl(1 / h)
    int sites;               // 2 bits per parity (py * 2 + px): its site channel
};

template <int IN>
constexpr int seg_px() { return IN == IN_SPREAD ? 8 : sesrq_bayer::seg_px<IN>(); }

// reflection without repeating the edge sample, period 2 (n - 1); n >= 2, any t
__device__ inline int fold(int t, int n) {
    if ((unsigned)t < (unsigned)n) return t;
    const int p = 2 * (n - 1);
    t %= p;
    if (t < 0) t += p;
    return t < n ? t : p - t;
}

__device__ inline int site_plane(const Args &a, int y, int x) { return (a.sites >> (2 * ((y & 1) * 2 + (x & 1)))) & 3; }

// the sample s of pixel (y, x) of frame n, both inside the frame
template <int IN>
__device__ inline float sample(const Args &a, int n, int y, int x) {
    if constexpr (IN == IN_SPREAD) {
        return reinterpret_cast<const float *>(a.src)[(((size_t)n * 3 + site_plane(a, y, x)) * a.H + y) * a.W + x];
    } else {
        const unsigned v = sesrq_bayer::load_px<IN>(a.src + ((size_t)n * a.H + y) * a.stride, x);
        return __fdiv_rn((float)(min(max(v, a.black), a.white) - a.black), a.D);
    }
}

// a whole segment of row y (inside the frame) at column xs, a multiple of the segment, from addresses the wide loads can take
template <int IN>
__device__ inline void segment(const Args &a, int n, int y, int xs, float (&d)[seg_px<IN>()]) {
    constexpr int SEG = seg_px<IN>();
    if constexpr (IN == IN_SPREAD) {
        const float *f = reinterpret_cast<const float *>(a.src);
        const float4 *e = reinterpret_cast<const float4 *>(f + (((size_t)n * 3 + site_plane(a, y, 0)) * a.H + y) * a.W + xs);
        const float4 *o = reinterpret_cast<const float4 *>(f + (((size_t)n * 3 + site_plane(a, y, 1)) * a.H + y) * a.W + xs);
#pragma unroll
        for (int j = 0; j < SEG / 4; ++j) {
            const float4 ev = e[j], ov = o[j];
            d[4 * j] = ev.x; d[4 * j + 1] = ov.y; d[4 * j + 2] = ev.z; d[4 * j + 3] = ov.w;
        }
    } else {
        unsigned v[SEG];
        sesrq_bayer::load_wide<IN>(a.src + ((size_t)n * a.H + y) * a.stride + (size_t)(xs / SEG) * sesrq_bayer::seg_bytes<IN>(), v);
#pragma unroll
        for (int k = 0; k < SEG; ++k) d[k] = __fdiv_rn((float)(min(max(v[k], a.black), a.white) - a.black), a.D);
    }
}

__device__ inline f2 max0(f2 v) { return f2{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f)}; }

// element (row, col) of a footprint held as vertical pairs
__device__ inline float at(const f2 (&w)[FP][FW], int row, int col) { return (row & 1) ? w[row >> 1][col].y : w[row >> 1][col].x; }

// 3 row pairs x 8 columns from the plane, first pair `word` (a 16-byte word index: row pair * PITCH / 2 + column / 2)
__device__ inline void footprint(const f4 *plane, int word, f2 (&w)[FP][FW]) {
#pragma unroll
    for (int p = 0; p < FP; ++p)
#pragma unroll
        for (int b = 0; b < FW / 2; ++b) {
            const f4 v = plane[word + p * (PITCH / 2) + b];
            w[p][2 * b] = f2{v.x, v.y};
            w[p][2 * b + 1] = f2{v.z, v.w};
        }
}

template <int IN, bool LEVELS, bool WIDE>
__global__ __launch_bounds__(THREADS) void denoise(Args a) {
    constexpr int SEG = seg_px<IN>();
    constexpr int UNITS = SEG == 8 ? LW / 8 : TW / 16 + 2;          // per row pair: segments, and for packed rows the two halo runs of 8
    __shared__ f4 s_c[LP * PITCH / 2], s_g[LP * PITCH / 2];
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const unsigned b = blockIdx.x;
    const int tx = b % (unsigned)a.tiles_x, t = b / (unsigned)a.tiles_x, ty = t % a.tiles_y, n = t / a.tiles_y;
    const int x0 = tx * TW, y0 = ty * TH;
    const float shot = LEVELS ? a.levels[2 * (size_t)n] : a.shot, read = LEVELS ? a.levels[2 * (size_t)n + 1] : a.read;

    for (int i = tid; i < LP * UNITS; i += THREADS) {
        const int pr = i / UNITS, u = i - pr * UNITS;
        // LDS column, length and whether the unit is a segment of the packing
        const int lc = SEG == 8 ? 8 * u : u == 0 ? 0 : u == UNITS - 1 ? LW - 8 : 8 + 16 * (u - 1);
        const int len = SEG == 8 || (u != 0 && u != UNITS - 1) ? SEG : 8;
        const int xs = x0 - HALO + lc;
        const bool wide = WIDE && len == SEG && xs >= 0 && xs + SEG <= W;
        float c[2][SEG], g[2][SEG];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int yf = fold(y0 - HALO + 2 * pr + h, H);
            float d[SEG];
            if (wide) {
                segment<IN>(a, n, yf, xs, d);
            } else {
#pragma unroll
                for (int k = 0; k < SEG; ++k) d[k] = k < len ? sample<IN>(a, n, yf, fold(xs + k, W)) : 0.f;
            }
#pragma unroll
            for (int k = 0; k < SEG; ++k) {
                const float s = d[k];
                c[h][k] = s > 0.f ? fminf(s, 1.f) : 0.f;
                const float v = c[h][k] * shot + read;
                g[h][k] = __fdiv_rn(1.f, fmaxf(v + v, 0x1p-100f));
            }
        }
        const int word = pr * (PITCH / 2) + lc / 2;
#pragma unroll
        for (int k = 0; k < SEG / 2; ++k)
            if (2 * k < len) {
                s_c[word + k] = f4{c[0][2 * k], c[1][2 * k], c[0][2 * k + 1], c[1][2 * k + 1]};
                s_g[word + k] = f4{g[0][2 * k], g[1][2 * k], g[0][2 * k + 1], g[1][2 * k + 1]};
            }
    }
    __syncthreads();

    const int ly = tid & (TH / PH - 1), lx = tid / (TH / PH);
    const int x = x0 + PW * lx, y = y0 + PH * ly;          // the block's first pixel: even, even
    if (x >= W || y >= H) return;
    // the footprint's first 16-byte word: LDS row HALO - PATCH + 2 ly, column HALO - PATCH + 4 lx
    const int home = ((HALO - PATCH) / 2 + ly) * (PITCH / 2) + (HALO - PATCH) / 2 + (PW / 2) * lx;
    f2 C[FP][FW], G[FP][FW];
    footprint(s_c, home, C);
    footprint(s_g, home, G);
    const f2 rh = f2{a.rh, a.rh};
    f2 num[PW], den[PW];
#pragma unroll
    for (int k = 0; k < PW; ++k) num[k] = den[k] = f2{0.f, 0.f};

#pragma unroll 1
    for (int j = -SEARCH; j <= SEARCH; ++j) {
        SESRQ_UNROLL(SESRQ_DENOISE_UNROLL_I)
        for (int i = -SEARCH; i <= SEARCH; ++i) {
            f2 Q[FP][FW];
            footprint(s_c, home + j * (PITCH / 2) + i, Q);
            f2 Dp[PW];                                     // (Dp of block row 0, of block row 1) per block column
#ifndef SESRQ_DENOISE_DIRECT
            f2 R[FP][PW];                                  // R[p][k]: the row sums of footprint rows 2 p, 2 p + 1 for block column k
#pragma unroll
            for (int p = 0; p < FP; ++p) {
                f2 E[FW];
#pragma unroll
                for (int c = 0; c < FW; ++c) {
                    const f2 d = C[p][c] - Q[p][c];
                    E[c] = (d * d) * G[p][c];
                }
#pragma unroll
                for (int k = 0; k < PW; ++k) R[p][k] = (((E[k] + E[k + 1]) + E[k + 2]) + E[k + 3]) + E[k + 4];
            }
#pragma unroll
            for (int k = 0; k < PW; ++k) {
                const float r0 = R[0][k].x, r1 = R[0][k].y, r2 = R[1][k].x, r3 = R[1][k].y, r4 = R[2][k].x, r5 = R[2][k].y;
                Dp[k] = f2{(((r0 + r1) + r2) + r3) + r4, (((r1 + r2) + r3) + r4) + r5};
            }
#else
            // every pixel's 25 terms on their own; the empty asm keeps the compiler from sharing them between pixels
#pragma unroll
            for (int k = 0; k < PW; ++k) {
                float dp[PH];
#pragma unroll
                for (int oy = 0; oy < PH; ++oy) {
                    float r[5];
#pragma unroll
                    for (int r_ = 0; r_ < 5; ++r_) {
                        float e[5];
#pragma unroll
                        for (int c_ = 0; c_ < 5; ++c_) {
                            float cc = at(C, oy + r_, k + c_);
                            asm volatile("" : "+v"(cc));
                            const float d = cc - at(Q, oy + r_, k + c_);
                            e[c_] = (d * d) * at(G, oy + r_, k + c_);
                        }
                        r[r_] = (((e[0] + e[1]) + e[2]) + e[3]) + e[4];
                    }
                    dp[oy] = (((r[0] + r[1]) + r[2]) + r[3]) + r[4];
                }
                Dp[k] = f2{dp[0], dp[1]};
            }
#endif
            const bool centre = (i | j) == 0;
#pragma unroll
            for (int k = 0; k < PW; ++k) {
                const f2 t = max0(Dp[k] * 0.04f - 1.f);
                const f2 kk = max0(1.f - t * rh);
                const f2 w = centre ? f2{1.f, 1.f} : kk * kk;
                num[k] += w * Q[PATCH / 2][PATCH + k];     // c(q) of the block's two rows: footprint rows 2, 3
                den[k] += w;
            }
        }
    }

    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int oy = 0; oy < PH; ++oy) {
        if (y + oy >= H) break;
        float v[PW];
#pragma unroll
        for (int k = 0; k < PW; ++k) v[k] = oy ? __fdiv_rn(num[k].y, den[k].y) : __fdiv_rn(num[k].x, den[k].x);
        const int ce = (a.sites >> (4 * oy)) & 3, co = (a.sites >> (4 * oy + 2)) & 3;      // site planes of the even / odd columns
        float *o = a.out + ((size_t)n * 3 * H + (y + oy)) * W + x;            // plane c of the frame starts c * plane further
        if constexpr (WIDE) {                              // W % 4 == 0: the run of 4 is inside the row
            static_assert(PW == 4, "a block row is one 16-byte store per plane");
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<float4 *>(o + c * plane) = make_float4(c == ce ? v[0] : 0.f, c == co ? v[1] : 0.f, c == ce ? v[2] : 0.f,
                                                                          c == co ? v[3] : 0.f);
        } else {
#pragma unroll
            for (int k = 0; k < PW; ++k)
                if (x + k < W) {
                    const int cs = (k & 1) ? co : ce;
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c * plane + k] = c == cs ? v[k] : 0.f;
                }
        }
    }
}

}  // namespace sesrq_denoisek

using namespace sesrq_denoisek;

// one instantiation per (input, levels, path)
enum { K_COUNT = IN_COUNT * 2 * 2 };
static const char *const kNames[K_COUNT] = {
    "denoise<u16,scalar,wide>",   "denoise<u16,scalar,sample>",   "denoise<u16,array,wide>",   "denoise<u16,array,sample>",
    "denoise<raw10,scalar,wide>", "denoise<raw10,scalar,sample>", "denoise<raw10,array,wide>", "denoise<raw10,array,sample>",
    "denoise<raw12,scalar,wide>", "denoise<raw12,scalar,sample>", "denoise<raw12,array,wide>", "denoise<raw12,array,sample>",
    "denoise<spread,scalar,wide>", "denoise<spread,scalar,sample>", "denoise<spread,array,wide>", "denoise<spread,array,sample>"};
static Counters<K_COUNT> g_count{kNames};

static int check_format(const char *who, const sesrq_sensor_format *f) {
    if (!f) return fail("%s: format is NULL", who);
    if (f->cfa < SESRQ_CFA_RGGB || f->cfa > SESRQ_CFA_BGGR) return fail("%s: cfa %d is not a Bayer order (0 .. 3)", who, f->cfa);
    if (f->packing < SESRQ_PACK_U16 || f->packing > SESRQ_PACK_RAW12) return fail("%s: packing %d (0 u16, 1 raw10, 2 raw12)", who, f->packing);
    if (f->black < 0 || f->black >= f->white || f->white > 65535)
        return fail("%s: levels need 0 <= black < white <= 65535, got black %d, white %d", who, f->black, f->white);
    const int top = f->packing == SESRQ_PACK_RAW10 ? 1023 : f->packing == SESRQ_PACK_RAW12 ? 4095 : 65535;
    if (f->white > top) return fail("%s: white %d is above the packing's range (%d)", who, f->white, top);
    return 0;
}

// What both entries refuse of the levels, the strength, the output and the frame; then the tiles of the batch, which must fit a grid.
static int check_frame(const char *who, float shot, float read, const float *levels, float h, float *out, int N, int H, int W, Args *a,
                       long long *tiles) {
    if (levels && reinterpret_cast<uintptr_t>(levels) % 4) return fail("%s: levels is not 4-byte aligned", who);
    if (!levels && !(std::isfinite(shot) && shot >= 0.f && std::isfinite(read) && read >= 0.f))
        return fail("%s: shot %g and read %g must be finite and not negative", who, (double)shot, (double)read);
    if (!(std::isfinite(h) && h > 0.f)) return fail("%s: the strength h = %g must be finite and positive", who, (double)h);
    if (!out) return fail("%s: out is NULL", who);
    if (reinterpret_cast<uintptr_t>(out) % 4) return fail("%s: out is not 4-byte aligned", who);
    if (N < 1) return fail("%s: empty batch (N = %d)", who, N);
    if (H < 2 || W < 2) return fail("%s: the reflection needs H, W >= 2, got H = %d, W = %d", who, H, W);
    if (H > 0x7fffffff - 128 || W > 0x7fffffff - 128) return fail("%s: frame of %d x %d is too large", who, H, W);
    const long long tx = ((long long)W + TW - 1) / TW, ty = ((long long)H + TH - 1) / TH;
    if (tx * ty > 0x7fffffffLL / N) return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);
    const volatile float rh = 1.0f / h;                    // fl(1 / h), formed once
    a->out = out;
    a->levels = levels;
    a->shot = shot;
    a->read = read;
    a->rh = rh;
    a->H = H;
    a->W = W;
    a->tiles_x = (int)tx;
    a->tiles_y = (int)ty;
    *tiles = (long long)N * tx * ty;
    return 0;
}

template <int IN>
static void launch_in(bool levels, bool wide, unsigned grid, hipStream_t st, const Args &a) {
    if (levels)
        wide ? denoise<IN, true, true><<<grid, THREADS, 0, st>>>(a) : denoise<IN, true, false><<<grid, THREADS, 0, st>>>(a);
    else
        wide ? denoise<IN, false, true><<<grid, THREADS, 0, st>>>(a) : denoise<IN, false, false><<<grid, THREADS, 0, st>>>(a);
}

// `wide`: the input allows the wide loads; the stores need W % 4 == 0 and a 16-byte aligned out.  One path for both; then one kernel.
static int launch(const char *who, int in, int cfa, bool wide, long long tiles, void *stream, Args &a) {
    wide = wide && a.W % 4 == 0 && reinterpret_cast<uintptr_t>(a.out) % 16 == 0;
    a.sites = sesrq_bayer::SITES[cfa];
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)tiles;
    const bool levels = a.levels != nullptr;
    switch (in) {
        case IN_U16: launch_in<IN_U16>(levels, wide, grid, st, a); break;
        case IN_RAW10: launch_in<IN_RAW10>(levels, wide, grid, st, a); break;
        case IN_RAW12: launch_in<IN_RAW12>(levels, wide, grid, st, a); break;
        default: launch_in<IN_SPREAD>(levels, wide, grid, st, a); break;
    }
    return launched(who, g_count, (in * 2 + levels) * 2 + !wide);
}

extern "C" int sesrq_denoise_raw(const sesrq_sensor_format *fmt, const void *raw, size_t row_stride_bytes, float shot, float read,
                                 const float *levels, float h, float *out, int N, int H, int W, void *stream) {
    static const char who[] = "sesrq_denoise_raw";
    g_err[0] = 0;
    if (check_format(who, fmt)) return 1;
    if (!raw) return fail("%s: raw is NULL", who);
    Args a = {};
    long long tiles;
    if (check_frame(who, shot, read, levels, h, out, N, H, W, &a, &tiles)) return 1;
    const int pack = fmt->packing, group = pack == SESRQ_PACK_RAW10 ? 4 : pack == SESRQ_PACK_RAW12 ? 2 : 1;
    if (W % group) return fail("%s: W = %d is not a multiple of the %d pixels of a pack group", who, W, group);
    const size_t need = pack == SESRQ_PACK_RAW10 ? (size_t)W / 4 * 5 : pack == SESRQ_PACK_RAW12 ? (size_t)W / 2 * 3 : (size_t)W * 2;
    if (row_stride_bytes < need)
        return fail("%s: row_stride_bytes %zu is less than the %zu bytes of a row of %d pixels", who, row_stride_bytes, need, W);
    const uintptr_t in_align = pack == SESRQ_PACK_U16 ? 16 : 4;
    a.src = static_cast<const uint8_t *>(raw);
    a.stride = row_stride_bytes;
    a.black = (unsigned)fmt->black;
    a.white = (unsigned)fmt->white;
    a.D = (float)(fmt->white - fmt->black);
    return launch(who, pack, fmt->cfa, reinterpret_cast<uintptr_t>(raw) % in_align == 0 && row_stride_bytes % in_align == 0, tiles, stream, a);
}

extern "C" int sesrq_denoise_spread(int cfa, const float *spread, float shot, float read, const float *levels, float h, float *out, int N,
                                    int H, int W, void *stream) {
    static const char who[] = "sesrq_denoise_spread";
    g_err[0] = 0;
    if (cfa < SESRQ_CFA_RGGB || cfa > SESRQ_CFA_BGGR) return fail("%s: cfa %d is not a Bayer order (0 .. 3)", who, cfa);
    if (!spread) return fail("%s: spread is NULL", who);
    if (reinterpret_cast<uintptr_t>(spread) % 4) return fail("%s: spread is not 4-byte aligned", who);
    Args a = {};
    long long tiles;
    if (check_frame(who, shot, read, levels, h, out, N, H, W, &a, &tiles)) return 1;
    a.src = reinterpret_cast<const uint8_t *>(spread);
    return launch(who, IN_SPREAD, cfa, reinterpret_cast<uintptr_t>(spread) % 16 == 0, tiles, stream, a);
}

extern "C" int sesrq_denoise_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_denoise_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_denoise_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_denoise_last_error(void) { return g_err; }
