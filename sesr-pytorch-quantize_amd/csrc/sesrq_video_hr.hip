// libsesrq_video_hr.so: the super-resolution nets' video input from the HR clip alone (include/sesrq_video_hr.h, which fixes the
// arithmetic by reference to sesrq_downscale.h and sesrq_video.h).  A library of its own: it links nothing of the other libraries and
// registers nothing in their instance tables; the surface checks are the video libraries' (sesrq_video_surface.h), the per-code table
// of the luma decode the image library's (sesrq_image_decode.h).
//
// ONE kernel reads an HR 4:2:0 surface once (1.5 B/px) and writes the LR chroma planes, the LR luma and / or its decode into q0 and
// the fp32 frame.  A workgroup of 256 lanes owns 128 x 32 HR luma pixels and the 64 x 16 chroma samples a plane under them: 32 x 8 LR
// luma and 16 x 4 LR chroma samples at r = 4, 64 x 16 and 32 x 8 at r = 2.
//   stage       the luma window, (32 + 3 r) rows of (128 + 3 r) bytes, and the chroma window, (16 + 3 r) rows of (64 + 3 r) samples a
//               plane, go to LDS a row at a time as 4-byte words through the pitches: the part of a row inside the plane is one run
//               of memory, read in words at whatever address it starts; the columns beyond a plane's left or right edge and the odd
//               bytes at the ends of the run are read one by one through the mirrored index; rows are mirrored as a whole.  NV12
//               chroma is one interleaved plane of Cb,Cr pairs and is staged as it lies; I420 planes are staged side by side.
//   vertical    a staged row is so many independent byte columns -- interleaving does not matter to it: a lane takes one word (4
//               columns) of one LR row, 4 r taps down the window, and writes the clamped uint8 intermediate to LDS.  Luma and chroma
//               items share one loop.
//   horizontal  luma: a lane takes 4 HR-aligned bytes' worth of LR pixels of one intermediate row as whole words (one LR pixel at
//               r = 4: 4 words; two neighbours at r = 2: 3 words), lanes one word apart.  Chroma: a lane takes one sample position
//               and filters both components, from the pair bytes of an NV12 window or from the two planes of an I420 one.  The bytes
//               go to an LDS output tile laid out as the OUTPUT format wants them: luma rows, NV12 pair rows or two I420 planes.
//   store       a lane owns 16 consecutive output bytes of one row (lr's Y, q0 through the table, a chroma row) or four fp32
//               elements, consecutive lanes consecutive runs; a 16-byte store where the run is whole and aligned, per-element
//               stores otherwise (NV12 chroma: 2-byte elements).
// LDS at r = 4: 6160 B luma window + 4256 B chroma window + 1728 B intermediates + 384 B output tile + 1280 B tables = 13.8 KB; at
// r = 2 14.5 KB: eight workgroups a CU (eight waves a SIMD) need 20 KB or less each.  Weights are literals of the unrolled tap loops;
// the factor, the two formats and the luma outputs are template parameters, an absent lr->y a uniform branch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_video_hr.h"
#include "sesrq_side.h"
#include "sesrq_image_decode.h"
#include "sesrq_video_surface.h"

namespace sesrq_vhrk {

using sesrq_imgdec::RGB_WORDS;
using sesrq_imgdec::Tables;

constexpr int HR_W = SESRQ_VIDEO_HR_TILE_HR_W, HR_H = SESRQ_VIDEO_HR_TILE_HR_H;      // a workgroup's tile in HR luma pixels
constexpr int HC_W = HR_W / 2, HC_H = HR_H / 2;                                     // ... and in HR chroma samples a plane
constexpr int THREADS = 256;
constexpr int SEG = 16;                                         // output bytes per lane and run
constexpr int FMT_NONE = -1;                                    // no LR surface
enum { OUT_Q = 1, OUT_F = 2 };
static_assert(SESRQ_VIDEO_CODES == sesrq_imgdec::CODES, "one table for the byte libraries");

// Keys a = -1/2 stretched by r, times D: tap k of 4 r (sesrq_downscale.h step 1)
__host__ __device__ constexpr int weight(int r, int k) {
    constexpr int W2[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
    constexpr int W4[16] = {-7, -45, -75, -49, 93, 399, 745, 987, 987, 745, 399, 93, -49, -75, -45, -7};
    return r == 4 ? W4[k] : W2[k];
}

template <int R, int IF>
struct Shape {
    static constexpr int TAPS = 4 * R, REACH = 3 * R / 2;        // tap 0 of LR index d is HR index r d - REACH
    static constexpr int SHIFT = R == 4 ? 12 : 8, D = 1 << SHIFT;
    // luma
    static constexpr int YW = HR_W / R, YH = HR_H / R;           // the tile in LR luma pixels
    static constexpr int Y_WP = HR_W + 3 * R, Y_WR = HR_H + 3 * R;      // the staged window: columns, rows
    static constexpr int Y_KW = (Y_WP + 3) / 4;                  // words of a window row: 35 (r = 4), 34 (r = 2)
    static constexpr int PX = 4 / R;                             // LR pixels an item of the horizontal pass takes: it starts at word m
    static constexpr int IW = YW / PX, Y_ITEMS = IW * YH;        // items a row (32), items a tile
    static constexpr int HWORDS = (R * (PX - 1) + TAPS + 3) / 4; // words an item reads: 4, 3
    static_assert(IW - 1 + HWORDS <= Y_KW, "the last item stays inside its row");
    // chroma
    static constexpr bool NV = IF == SESRQ_VIDEO_NV12;
    static constexpr int CW = HC_W / R, CH = HC_H / R;           // the tile in LR chroma samples a plane
    static constexpr int C_WP = HC_W + 3 * R, C_WR = HC_H + 3 * R;
    static constexpr int C_KWP = ((NV ? 2 : 1) * C_WP + 3) / 4;  // words of a staged row of one plane in memory: 38 / 19 (r = 4), 35 / 18
    static constexpr int C_KW = NV ? C_KWP : 2 * C_KWP;          // words of a window row: Cb and Cr of I420 side by side
    static constexpr int V_Y = YH * Y_KW, V_C = CH * C_KW;       // items of the vertical pass
};

struct Args {
    const uint8_t *iy, *ic0, *ic1;      // HR planes
    uint8_t *oy, *oc0, *oc1;            // LR planes; oy may be NULL
    const Tables *tab;
    int8_t *q0;
    float *x;
    int64_t ipy, ipc, ify, ifc, opy, opc, ofy, ofc;
    int H, W, tiles_x, tiles_y;         // H, W: the LR luma size
};

// step 2 of sesrq_downscale.h: index j of an axis of length n, mirrored with the edge sample repeated
__device__ inline long long mirror(long long j, long long n) {
    const long long p = 2 * n;
    long long i = j % p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// four bytes at any address
__device__ inline unsigned load_u32(const uint8_t *p) {
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

template <int WORDS>
__device__ inline int byte_of(const unsigned (&w)[WORDS], int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 0xffu); }

// step 3: clamp(floor((s + D / 2) / D), 0, 255) of a sum that already holds D / 2: clamped first, shifted second, as the downscale
// library forms it (the shift-then-clamp form selects a packed instruction that gave other bytes there)
template <int SHIFT>
__device__ inline unsigned round_clamp(int s) { return (unsigned)min(max(s, 0), (256 << SHIFT) - 1) >> SHIFT; }

// Stage `rows` window rows of one plane in memory (BPS bytes a sample: 2 for the NV12 pair plane) as KW words a row, `stride` words
// apart in LDS.  The plane is PH x PW samples; window row 0 is plane row ys, window column 0 plane column xs; WP columns, of which
// those below PW + reach feed a sample of the frame.
template <int BPS, int WP, int KW>
__device__ inline void stage(unsigned *dst, int stride, int rows, const uint8_t *plane, int64_t pitch, long long PH, long long PW,
                             long long xs, long long ys, int reach) {
    const int c_lo = xs < 0 ? (int)-xs : 0;
    const int c_hi = (int)min((long long)WP, PW - xs);
    const int c_need = (int)min((long long)WP, PW - xs + reach);
    for (int it = threadIdx.x; it < rows * KW; it += THREADS) {
        const int row = it / KW, k = it - row * KW, b0 = 4 * k;
        long long gy = ys + row;
        if (gy < 0 || gy >= PH) gy = mirror(gy, PH);
        const uint8_t *line = plane + gy * pitch;
        unsigned w = 0;
        if (b0 >= BPS * c_lo && b0 + 4 <= BPS * c_hi) {
            w = load_u32(line + (xs * BPS + b0));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = b0 + j;
                if (b < BPS * c_need) {
                    const int c = b / BPS, ch = b - BPS * c;
                    long long gx = xs + c;
                    if (c < c_lo || c >= c_hi) gx = mirror(gx, PW);
                    w |= (unsigned)line[gx * BPS + ch] << (8 * j);
                }
            }
        }
        dst[row * stride + k] = w;
    }
}

// one item of the vertical pass: four byte columns, taps KW words apart
template <int R, int KW, int SHIFT>
__device__ inline unsigned vertical(const unsigned *win) {
    int acc[4] = {1 << (SHIFT - 1), 1 << (SHIFT - 1), 1 << (SHIFT - 1), 1 << (SHIFT - 1)};
#pragma unroll
    for (int tp = 0; tp < 4 * R; ++tp) {
        const unsigned wd = win[tp * KW];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += weight(R, tp) * (int)((wd >> (8 * c)) & 0xffu);
    }
    return round_clamp<SHIFT>(acc[0]) | round_clamp<SHIFT>(acc[1]) << 8 | round_clamp<SHIFT>(acc[2]) << 16 | round_clamp<SHIFT>(acc[3]) << 24;
}

__device__ inline unsigned word_of(const uint4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// a run of nb <= 16 bytes: one 16-byte store where it is whole and aligned, else elements of ELEM bytes
template <int ELEM>
__device__ inline void store_run(uint8_t *dst, const uint4 &v, int nb) {
    if (nb == SEG && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<uint4 *>(dst) = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < SEG; k += ELEM) {
        if (k < nb) {
            const unsigned e = word_of(v, k >> 2) >> (8 * (k & 3));
            if (ELEM == 2) {
                const uint16_t h = (uint16_t)e;
                __builtin_memcpy(dst + k, &h, 2);
            } else {
                dst[k] = (uint8_t)e;
            }
        }
    }
}

// 8 waves a SIMD: four waves a workgroup, eight workgroups a CU
template <int R, int IF, int OF, int LUMA>
__global__ __launch_bounds__(THREADS, 8) void video_hr(Args a) {
    using S = Shape<R, IF>;
    constexpr bool CHROMA = OF != FMT_NONE;
    constexpr int YW = S::YW, YH = S::YH, CW = S::CW, CH = S::CH;
    __shared__ uint4 s_tab[LUMA ? RGB_WORDS : 1];
    __shared__ unsigned s_wy[S::Y_WR * S::Y_KW];
    __shared__ unsigned s_wc[CHROMA ? S::C_WR * S::C_KW : 1];
    __shared__ unsigned s_vy[S::V_Y];
    __shared__ unsigned s_vc[CHROMA ? S::V_C : 1];
    __shared__ __align__(16) uint8_t s_oy[YH * YW];
    __shared__ __align__(16) uint8_t s_oc[CHROMA ? 2 * CH * CW : 16];
    const int tid = threadIdx.x;
    if (LUMA) sesrq_imgdec::stage_tables<SESRQ_IMAGE_RGB, THREADS>(s_tab, a.tab);

    unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)a.tiles_x);
    t /= (unsigned)a.tiles_x;
    const int ty = (int)(t % (unsigned)a.tiles_y);
    const int64_t n = t / (unsigned)a.tiles_y;
    const long long Wl = a.W, Hl = a.H, Wc = Wl / 2, Hc = Hl / 2;      // the LR planes
    const bool luma = LUMA || (CHROMA && a.oy);                        // uniform: is the Y plane needed at all

    // stage
    if (luma)
        stage<1, S::Y_WP, S::Y_KW>(s_wy, S::Y_KW, S::Y_WR, a.iy + n * a.ify, a.ipy, Hl * R, Wl * R, (long long)tx * HR_W - S::REACH,
                                   (long long)ty * HR_H - S::REACH, S::REACH);
    if (CHROMA) {
        const long long xs = (long long)tx * HC_W - S::REACH, ys = (long long)ty * HC_H - S::REACH;
        if (S::NV) {
            stage<2, S::C_WP, S::C_KWP>(s_wc, S::C_KW, S::C_WR, a.ic0 + n * a.ifc, a.ipc, Hc * R, Wc * R, xs, ys, S::REACH);
        } else {
            stage<1, S::C_WP, S::C_KWP>(s_wc, S::C_KW, S::C_WR, a.ic0 + n * a.ifc, a.ipc, Hc * R, Wc * R, xs, ys, S::REACH);
            stage<1, S::C_WP, S::C_KWP>(s_wc + S::C_KWP, S::C_KW, S::C_WR, a.ic1 + n * a.ifc, a.ipc, Hc * R, Wc * R, xs, ys, S::REACH);
        }
    }
    __syncthreads();

    // vertical pass: LR row l of the tile, word k of the row (4 byte columns); taps are window rows r l .. r l + 4 r - 1
    for (int it = luma ? tid : tid + S::V_Y; it < S::V_Y + (CHROMA ? S::V_C : 0); it += THREADS) {
        if (it < S::V_Y) {
            const int l = it / S::Y_KW, k = it - l * S::Y_KW;
            s_vy[it] = vertical<R, S::Y_KW, S::SHIFT>(s_wy + R * l * S::Y_KW + k);
        } else if (CHROMA) {
            const int i = it - S::V_Y, l = i / S::C_KW, k = i - l * S::C_KW;
            s_vc[i] = vertical<R, S::C_KW, S::SHIFT>(s_wc + R * l * S::C_KW + k);
        }
    }
    __syncthreads();

    // horizontal pass, luma: item m of a row is LR pixels PX m .. PX m + PX - 1, whose taps start at byte 4 m of the row
    if (luma) {
        for (int it = tid; it < S::Y_ITEMS; it += THREADS) {
            const int l = it / S::IW, m = it - l * S::IW;
            unsigned w[S::HWORDS];
#pragma unroll
            for (int j = 0; j < S::HWORDS; ++j) w[j] = s_vy[l * S::Y_KW + m + j];
#pragma unroll
            for (int p = 0; p < S::PX; ++p) {
                int acc = S::D / 2;
#pragma unroll
                for (int tp = 0; tp < S::TAPS; ++tp) acc += weight(R, tp) * byte_of(w, R * p + tp);
                s_oy[l * YW + m * S::PX + p] = (uint8_t)round_clamp<S::SHIFT>(acc);
            }
        }
    }
    // ... chroma: one sample position a lane, both components
    if (CHROMA) {
        for (int it = tid; it < CW * CH; it += THREADS) {
            const int l = it / CW, c = it - l * CW;
            const uint8_t *row = reinterpret_cast<const uint8_t *>(s_vc + l * S::C_KW);
#pragma unroll
            for (int comp = 0; comp < 2; ++comp) {
                const uint8_t *p = S::NV ? row + 2 * R * c + comp : row + 4 * S::C_KWP * comp + R * c;
                int acc = S::D / 2;
#pragma unroll
                for (int tp = 0; tp < S::TAPS; ++tp) acc += weight(R, tp) * (int)p[(S::NV ? 2 : 1) * tp];
                const uint8_t v = (uint8_t)round_clamp<S::SHIFT>(acc);
                if (OF == SESRQ_VIDEO_NV12)
                    s_oc[(l * CW + c) * 2 + comp] = v;
                else
                    s_oc[(comp * CH + l) * CW + c] = v;
            }
        }
    }
    __syncthreads();

    // store, luma bytes: lr's Y plane as they are, q0 through the table
    const long long lx0 = (long long)tx * YW, ly0 = (long long)ty * YH;
    const float *tabx = sesrq_imgdec::table_x(s_tab);
    const int8_t *tabq = sesrq_imgdec::table_q(s_tab);
    if (luma && (CHROMA || (LUMA & OUT_Q))) {
        constexpr int RUNS = YW / SEG;
        for (int u = tid; u < RUNS * YH; u += THREADS) {
            const int l = u / RUNS, run = u - l * RUNS;
            const long long gy = ly0 + l, gx = lx0 + run * SEG;
            if (gy >= Hl || gx >= Wl) continue;
            const int npx = (int)min((long long)SEG, Wl - gx);
            const uint4 v = *reinterpret_cast<const uint4 *>(s_oy + l * YW + run * SEG);
            if (CHROMA && a.oy) store_run<1>(a.oy + n * a.ofy + gy * a.opy + gx, v, npx);
            if (LUMA & OUT_Q) {
                unsigned q[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < SEG; ++k)
                    q[k >> 2] |= (unsigned)(uint8_t)tabq[(word_of(v, k >> 2) >> (8 * (k & 3))) & 0xffu] << (8 * (k & 3));
                store_run<1>(reinterpret_cast<uint8_t *>(a.q0) + ((n * Hl + gy) * Wl + gx), make_uint4(q[0], q[1], q[2], q[3]), npx);
            }
        }
    }
    // ... the fp32 frame: four elements a lane
    if (LUMA & OUT_F) {
        constexpr int RUNS = YW / 4;
        for (int u = tid; u < RUNS * YH; u += THREADS) {
            const int l = u / RUNS, run = u - l * RUNS;
            const long long gy = ly0 + l, gx = lx0 + run * 4;
            if (gy >= Hl || gx >= Wl) continue;
            const int npx = (int)min(4LL, Wl - gx);
            const unsigned v = *reinterpret_cast<const unsigned *>(s_oy + l * YW + run * 4);
            const float4 f = make_float4(tabx[v & 0xffu], tabx[(v >> 8) & 0xffu], tabx[(v >> 16) & 0xffu], tabx[v >> 24]);
            float *d = a.x + ((n * Hl + gy) * Wl + gx);
            if (npx == 4 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
                *reinterpret_cast<float4 *>(d) = f;
            } else {
                d[0] = f.x;
                if (npx > 1) d[1] = f.y;
                if (npx > 2) d[2] = f.z;
                if (npx > 3) d[3] = f.w;
            }
        }
    }
    // ... chroma: NV12 rows of pairs (eight a run), or the rows of two I420 planes (16 samples a run)
    if (CHROMA) {
        const long long cx0 = (long long)tx * CW, cy0 = (long long)ty * CH;
        constexpr bool ONV = OF == SESRQ_VIDEO_NV12;
        constexpr int SPR = ONV ? SEG / 2 : SEG;                       // samples a plane of a run
        constexpr int RUNS = (CW + SPR - 1) / SPR, PLANES = ONV ? 1 : 2;
        for (int u = tid; u < PLANES * CH * RUNS; u += THREADS) {
            const int pl = u / (CH * RUNS), rem = u - pl * (CH * RUNS);
            const int l = rem / RUNS, run = rem - l * RUNS;
            const long long gy = cy0 + l, gx = cx0 + run * SPR;
            if (gy >= Hc || gx >= Wc) continue;
            const int ns = (int)min((long long)SPR, Wc - gx);
            const uint4 v = *reinterpret_cast<const uint4 *>(s_oc + (ONV ? l * 2 * CW : (pl * CH + l) * CW) + run * SEG);
            uint8_t *d = (pl ? a.oc1 : a.oc0) + n * a.ofc + gy * a.opc + (ONV ? 2 * gx : gx);
            if (ONV)
                store_run<2>(d, v, 2 * ns);
            else
                store_run<1>(d, v, ns);
        }
    }
}

}  // namespace sesrq_vhrk

using namespace sesrq_vhrk;

struct sesrq_video_hr_ctx_s : sesrq_imgdec::CodeCtx {};

// every instantiation: X(r, input format, its name, LR format, its name, luma outputs, their name)
#define VHR_LUMA(X, R, I, IN, O, ON) X(R, I, IN, O, ON, OUT_Q, "q0") X(R, I, IN, O, ON, OUT_F, "x") X(R, I, IN, O, ON, OUT_Q | OUT_F, "q0,x")
#define VHR_OUT(X, R, I, IN)                                                                                \
    VHR_LUMA(X, R, I, IN, FMT_NONE, "none")                                                                 \
    X(R, I, IN, SESRQ_VIDEO_NV12, "nv12", 0, "none") VHR_LUMA(X, R, I, IN, SESRQ_VIDEO_NV12, "nv12")        \
    X(R, I, IN, SESRQ_VIDEO_I420, "i420", 0, "none") VHR_LUMA(X, R, I, IN, SESRQ_VIDEO_I420, "i420")
#define VHR_ALL(X) VHR_OUT(X, 2, SESRQ_VIDEO_NV12, "nv12") VHR_OUT(X, 2, SESRQ_VIDEO_I420, "i420") \
                   VHR_OUT(X, 4, SESRQ_VIDEO_NV12, "nv12") VHR_OUT(X, 4, SESRQ_VIDEO_I420, "i420")

#define VHR_NAME(R, I, IN, O, ON, L, LN) "video_hr<r" #R "," IN "->" ON "," LN ">",
static const char *const kNames[] = {VHR_ALL(VHR_NAME)};
#undef VHR_NAME
constexpr int K_COUNT = sizeof kNames / sizeof kNames[0];
static_assert(K_COUNT == 44, "2 factors x 2 input formats x (3 LR formats x 4 luma sets - the empty one)");
static Counters<K_COUNT> g_count{kNames};

extern "C" int sesrq_video_hr_weights(int r, int16_t *w, int *D) {
    g_err[0] = 0;
    if (r != 2 && r != 4) return fail("sesrq_video_hr_weights: r = %d (2 or 4)", r);
    if (!w || !D) return fail("sesrq_video_hr_weights: w or D is NULL");
    for (int k = 0; k < 4 * r; ++k) w[k] = (int16_t)weight(r, k);
    *D = r == 4 ? Shape<4, 0>::D : Shape<2, 0>::D;
    return 0;
}

extern "C" int sesrq_video_hr_create(float scale_in, int zero_in, int exact_div, sesrq_video_hr_ctx *out) {
    return sesrq_imgdec::code_create("sesrq_video_hr_create", scale_in, zero_in, exact_div, out);
}

extern "C" void sesrq_video_hr_destroy(sesrq_video_hr_ctx c) { ctx_destroy(c); }

extern "C" int sesrq_video_hr_run(sesrq_video_hr_ctx c, const sesrq_video_surface *hr, int r, const sesrq_video_surface *lr, int8_t *q0,
                                  float *x, int N, int H, int W, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_video_hr_run";
    const bool dec = q0 || x;
    if (!hr) return fail("%s: hr is NULL", who);
    if (!lr && !dec) return fail("%s: none of lr, q0 and x requested", who);
    if (dec && !c) return fail("%s: ctx is NULL (q0 and x need the decode table)", who);
    if (r != 2 && r != 4) return fail("%s: r = %d (2 or 4)", who, r);
    if (x && (reinterpret_cast<uintptr_t>(x) & 3)) return fail("%s: x is not 4-byte aligned", who);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    const long long rW = (long long)r * W, rH = (long long)r * H;
    if (H % 2 || W % 2)
        return fail("%s: an HR frame of %lld x %lld luma is no multiple of 2 r = %d each way; crop it first (modcrop)", who, rH, rW, 2 * r);
    const long long tx = (rW + HR_W - 1) / HR_W, ty = (rH + HR_H - 1) / HR_H, tiles = (long long)N * tx * ty;
    if (rH > 0x7fffffffLL || rW > 0x7fffffffLL || tiles > 0x7fffffffLL)
        return fail("%s: frame of %d x %d x %d at r = %d is too large", who, N, H, W, r);
    if (check_format(who, "hr", hr->format) || (lr && check_format(who, "lr", lr->format))) return 1;
    const bool luma = dec || (lr && lr->y);
    const int in_planes = (luma ? PLANE_Y : 0) | (lr ? PLANE_C : 0), out_planes = lr ? (lr->y ? PLANE_Y : 0) | PLANE_C : 0;
    if (check_planes(who, "hr", hr, in_planes) || (lr && check_planes(who, "lr", lr, out_planes))) return 1;
    if (check_pitches(who, " of hr", hr, in_planes, rW) || (lr && check_pitches(who, " of lr", lr, out_planes, W))) return 1;
    if (check_frames_in(who, " of hr", hr, in_planes)) return 1;
    if (lr) {
        sesrq_video_surface o = *lr;
        if (!o.y) {                       // the luma strides of an absent plane are not looked at
            o.pitch_y = W;
            o.frame_y = (int64_t)H * W;
        }
        if (check_frames_out(who, "lr", &o, N, H, W, true)) return 1;
    }
    if (dec && table_on_current(who, c->t)) return 1;

    Args a;
    a.iy = static_cast<const uint8_t *>(hr->y);
    a.ic0 = static_cast<const uint8_t *>(hr->c0);
    a.ic1 = static_cast<const uint8_t *>(hr->c1);
    a.ipy = hr->pitch_y;
    a.ipc = hr->pitch_c;
    a.ify = hr->frame_y;
    a.ifc = hr->frame_c;
    a.oy = lr ? static_cast<uint8_t *>(lr->y) : nullptr;
    a.oc0 = lr ? static_cast<uint8_t *>(lr->c0) : nullptr;
    a.oc1 = lr ? static_cast<uint8_t *>(lr->c1) : nullptr;
    a.opy = lr ? lr->pitch_y : 0;
    a.opc = lr ? lr->pitch_c : 0;
    a.ofy = lr ? lr->frame_y : 0;
    a.ofc = lr ? lr->frame_c : 0;
    a.tab = dec ? static_cast<const Tables *>(c->t.ptr) : nullptr;
    a.q0 = q0;
    a.x = x;
    a.H = H;
    a.W = W;
    a.tiles_x = (int)tx;
    a.tiles_y = (int)ty;
    const unsigned grid = (unsigned)tiles;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int fi = hr->format, fo = lr ? lr->format : FMT_NONE, lm = (q0 ? OUT_Q : 0) | (x ? OUT_F : 0);
    int k = -1, idx = 0;
#define VHR_RUN(R, I, IN, O, ON, L, LN)                              \
    if (r == R && fi == I && fo == O && lm == (L)) {                 \
        k = idx;                                                     \
        video_hr<R, I, O, (L)><<<grid, THREADS, 0, st>>>(a);         \
    }                                                                \
    ++idx;
    VHR_ALL(VHR_RUN)
#undef VHR_RUN
    if (k < 0) return fail("%s: unreachable instantiation", who);
    return launched(who, g_count, k);
}

extern "C" int sesrq_video_hr_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_video_hr_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_video_hr_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_video_hr_last_error(void) { return g_err; }
