// libsesrq_demosaic.so: bilinear and Malvar-He-Cutler demosaic of a Bayer frame (include/sesrq_demosaic.h, which fixes the arithmetic):
// the classical baseline of the raw nets.  A library of its own: it links nothing of the other libraries and registers nothing in
// their instance tables.  The packed formats are decoded with the helpers of sesrq_bayer_unpack.h (device code, compiled into this
// library's own kernels).
//
// Kernel.  One 256-lane workgroup owns a tile of 64 x 32 output pixels.
//   stage    the tile and its halo of 2 (68 x 36 samples) go to LDS as fp32 samples: a raw code is decoded and levelled, d(v), the site
//            plane of a spread frame is gathered.  The work is cut into row units -- the 64 tile columns in segments of 8 (U16, spread)
//            or 16 (RAW10, RAW12) pixels, each one lane's 16-byte load (U16), 4-byte loads (packed) or four 16-byte loads of the row's
//            two site planes (spread) where the address, stride and W allow, else sample by sample; and one unit for the row's four
//            halo columns, always sample by sample.  Coordinates are folded only where they leave the frame (edge tiles); samples that
//            no output pixel of the frame needs (further than 2 behind its last row or column) are not loaded.
//   compute  lane (lx, ly) = (tid & 15, tid >> 4) owns the 4 x 2 patch at (4 lx, 2 ly) of the tile: two Bayer quads.  Tile origins are
//            even, so patch pixel (ox, oy) has the CFA parity (ox & 1, oy & 1) in every lane: all lanes run the same four phase
//            formulas, no divergence.  Its 8 x 6 window is 12 ds_read_b128 (window column 0 is LDS column 4 lx, 16-byte aligned; the
//            row pitch of 72 floats keeps every row aligned; an empty asm keeps each read whole, see below).  The 16 lanes of a tile row read 16 consecutive 16-byte words, so any
//            group of lanes the LDS serves together reads one contiguous run: no bank conflict at any pitch that is a multiple of 4.
//            All window indices are compile-time constants after unrolling: 48 VGPRs of samples, no scratch.
//   store    per patch row and plane one 16-byte store where W % 4 == 0 and out is 16-byte aligned, else per pixel.
// The green diagonal of the CFA (RGGB / BGGR: G at the odd parities; GRBG / GBRG: at the even ones) and the method are template
// parameters; R and B differ only in which output (and spread input) plane the chroma of tile row 0 / row 1 goes to, two arguments.
// No MFMA: three channels from 13-tap filters that differ by CFA phase are no matrix product of a shape the matrix units take, and
// at 14 - 20 B/px of traffic for some 60 flops the kernel is a stream anyway.  Offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sesrq_bayer_unpack.h"
#include "sesrq_demosaic.h"
#include "sesrq_side.h"

namespace sesrq_demosaick {

constexpr int THREADS = 256;
constexpr int TW = 64, TH = 32, HALO = 2;          // tile of output pixels; filter reach
constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;
constexpr int PITCH = 72;                          // floats between LDS rows: >= LW, a multiple of 4
constexpr int PW = 4, PH = 2;                      // a lane's patch
enum { IN_U16, IN_RAW10, IN_RAW12, IN_SPREAD, IN_COUNT };
static_assert(IN_U16 == sesrq_bayer::PACK_U16 && IN_RAW10 == sesrq_bayer::PACK_RAW10 && IN_RAW12 == sesrq_bayer::PACK_RAW12, "raw inputs are the body's packings");
static_assert(SESRQ_PACK_U16 == IN_U16 && SESRQ_PACK_RAW10 == IN_RAW10 && SESRQ_PACK_RAW12 == IN_RAW12, "... and the header's");
static_assert((TW / PW) * (TH / PH) == THREADS && PITCH >= LW && PITCH % 4 == 0 && TW % 2 == 0 && TH % 2 == 0, "tile geometry");

struct Args {
    const uint8_t *src;      // raw rows, or the spread frame's floats
    float *out;
    size_t stride;           // raw: bytes between rows
    int H, W, tiles_x, tiles_y;
    unsigned black, white;   // raw levels
    float K;                 // 16 D, or 16
    int cP, cQ;              // plane (0 R, 2 B) of the chroma that has its sites in even / in odd rows
    int in_vec, out_vec;
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

// plane of the site of (y, x): chroma where the column parity is GD ^ row parity, else green
template <bool GD>
__device__ inline int site_plane(const Args &a, int y, int x) {
    return ((x & 1) == ((int)GD ^ (y & 1))) ? ((y & 1) ? a.cQ : a.cP) : 1;
}

// the sample of pixel (y, x) of frame n, both inside the frame
template <int IN, bool GD>
__device__ inline float sample(const Args &a, int n, int y, int x) {
    if constexpr (IN == IN_SPREAD) {
        return reinterpret_cast<const float *>(a.src)[(((size_t)n * 3 + site_plane<GD>(a, y, x)) * a.H + y) * a.W + x];
    } else {
        const unsigned v = sesrq_bayer::load_px<IN>(a.src + ((size_t)n * a.H + y) * a.stride, x);
        return (float)(min(max(v, a.black), a.white) - a.black);
    }
}

// a whole segment of row y (inside the frame) at column xs, a multiple of the segment, from addresses the wide loads can take
template <int IN, bool GD>
__device__ inline void segment(const Args &a, int n, int y, int xs, float (&d)[seg_px<IN>()]) {
    constexpr int SEG = seg_px<IN>();
    if constexpr (IN == IN_SPREAD) {
        const int ce = site_plane<GD>(a, y, 0), co = site_plane<GD>(a, y, 1);
        const float *f = reinterpret_cast<const float *>(a.src);
        const float4 *e = reinterpret_cast<const float4 *>(f + (((size_t)n * 3 + ce) * a.H + y) * a.W + xs);
        const float4 *o = reinterpret_cast<const float4 *>(f + (((size_t)n * 3 + co) * a.H + y) * a.W + xs);
#pragma unroll
        for (int j = 0; j < SEG / 4; ++j) {
            const float4 ev = e[j], ov = o[j];
            d[4 * j] = ev.x; d[4 * j + 1] = ov.y; d[4 * j + 2] = ev.z; d[4 * j + 3] = ov.w;
        }
    } else {
        unsigned v[SEG];
        sesrq_bayer::load_wide<IN>(a.src + ((size_t)n * a.H + y) * a.stride + (size_t)(xs / SEG) * sesrq_bayer::seg_bytes<IN>(), v);
#pragma unroll
        for (int k = 0; k < SEG; ++k) d[k] = (float)(min(max(v[k], a.black), a.white) - a.black);
    }
}

// the numerators of one pixel from its window position (r, c): everything fp32, one rounding per operation (-ffp-contract=off)
template <int METHOD>
struct Taps {
    float site, green, horiz, vert, diag;
    __device__ inline Taps(const float (&w)[PH + 2 * HALO][PW + 2 * HALO], int r, int c) {
        const float x = w[r][c];
        const float A1 = ((w[r - 1][c] + w[r + 1][c]) + w[r][c - 1]) + w[r][c + 1];
        const float Dg = ((w[r - 1][c - 1] + w[r - 1][c + 1]) + w[r + 1][c - 1]) + w[r + 1][c + 1];
        const float V2 = w[r - 2][c] + w[r + 2][c], H2 = w[r][c - 2] + w[r][c + 2];
        const float Hn = w[r][c - 1] + w[r][c + 1], Vn = w[r - 1][c] + w[r + 1][c];
        site = 16.f * x;
        if constexpr (METHOD == SESRQ_DEMOSAIC_MALVAR) {
            green = (8.f * x + 4.f * A1) - 2.f * (V2 + H2);
            horiz = (((10.f * x + 8.f * Hn) - 2.f * Dg) - 2.f * H2) + V2;
            vert = (((10.f * x + 8.f * Vn) - 2.f * Dg) - 2.f * V2) + H2;
            diag = (12.f * x + 4.f * Dg) - 3.f * (V2 + H2);
        } else {
            green = 4.f * A1;
            horiz = 8.f * Hn;
            vert = 8.f * Vn;
            diag = 4.f * Dg;
        }
    }
};

__device__ inline float finish(float S, float K) { return __fdiv_rn(S > 0.f ? fminf(S, K) : 0.f, K); }

template <int IN, bool GD, int METHOD>
__global__ __launch_bounds__(THREADS) void demosaic(Args a) {
    constexpr int SEG = seg_px<IN>(), SEGS = TW / SEG, UNITS = SEGS + 1;
    __shared__ float4 s_tile4[LH * PITCH / 4];
    float *tile = reinterpret_cast<float *>(s_tile4);
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const unsigned b = blockIdx.x;
    const int tx = b % (unsigned)a.tiles_x, t = b / (unsigned)a.tiles_x, ty = t % a.tiles_y, n = t / a.tiles_y;
    const int x0 = tx * TW, y0 = ty * TH;

    // a sample the frame's output needs (at most 2 behind the last row / column), folded at the frame's edge; 0 where none does
    auto at = [&](int yf, int gx) { return gx > W + 1 ? 0.f : sample<IN, GD>(a, n, yf, fold(gx, W)); };
    for (int i = tid; i < LH * UNITS; i += THREADS) {
        const int r = i / UNITS, u = i - r * UNITS, gy = y0 - HALO + r;
        const bool live = gy <= H + 1;
        const int yf = live ? fold(gy, H) : 0;
        float *row = tile + r * PITCH;
        if (u == SEGS) {                                   // the four halo columns
            row[0] = live ? at(yf, x0 - 2) : 0.f;
            row[1] = live ? at(yf, x0 - 1) : 0.f;
            row[HALO + TW] = live ? at(yf, x0 + TW) : 0.f;
            row[HALO + TW + 1] = live ? at(yf, x0 + TW + 1) : 0.f;
            continue;
        }
        const int xs = x0 + u * SEG;
        float d[SEG];
        if (live && a.in_vec && xs + SEG <= W) {
            segment<IN, GD>(a, n, yf, xs, d);
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k) d[k] = live ? at(yf, xs + k) : 0.f;
        }
        float2 *dst = reinterpret_cast<float2 *>(row + HALO + u * SEG);       // LDS column 2 + a multiple of 8: 8-byte aligned
#pragma unroll
        for (int k = 0; k < SEG / 2; ++k) dst[k] = make_float2(d[2 * k], d[2 * k + 1]);
    }
    __syncthreads();

    const int lx = tid & (TW / PW - 1), ly = tid / (TW / PW);
    const int x = x0 + PW * lx, y = y0 + PH * ly;          // the patch's first pixel: even, even
    if (x >= W || y >= H) return;
    float w[PH + 2 * HALO][PW + 2 * HALO];
#pragma unroll
    for (int r = 0; r < PH + 2 * HALO; ++r) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const f32x4 *p = reinterpret_cast<const f32x4 *>(s_tile4) + (PH * ly + r) * (PITCH / 4) + lx;      // LDS column PW lx
        static_assert(PW == 4, "a patch starts on a 16-byte word of its LDS row");
        const f32x4 lo = p[0], hi = p[1];
        asm volatile("" ::"v"(lo), "v"(hi));               // whole words: else the reads are split around the window's unused corners
        w[r][0] = lo.x; w[r][1] = lo.y; w[r][2] = lo.z; w[r][3] = lo.w;
        w[r][4] = hi.x; w[r][5] = hi.y; w[r][6] = hi.z; w[r][7] = hi.w;
    }
    const size_t plane = (size_t)H * W;
    const float K = a.K;
#pragma unroll
    for (int oy = 0; oy < PH; ++oy) {
        if (y + oy >= H) break;
        // the row's chroma X has its sites at column parity GD ^ oy; Y is the other chroma
        float vX[PW], vG[PW], vY[PW];
#pragma unroll
        for (int ox = 0; ox < PW; ++ox) {
            const Taps<METHOD> tp(w, oy + HALO, ox + HALO);
            const bool chroma = (ox & 1) == ((int)GD ^ oy);
            vX[ox] = finish(chroma ? tp.site : tp.horiz, K);
            vG[ox] = finish(chroma ? tp.green : tp.site, K);
            vY[ox] = finish(chroma ? tp.diag : tp.vert, K);
        }
        const int cX = oy ? a.cQ : a.cP, cY = oy ? a.cP : a.cQ;
        float *o = a.out + ((size_t)n * 3 * H + (y + oy)) * W + x;            // plane c of the frame starts c * plane further
        if (a.out_vec) {                                   // W % 4 == 0: the run of 4 is inside the row
            *reinterpret_cast<float4 *>(o + cX * plane) = make_float4(vX[0], vX[1], vX[2], vX[3]);
            *reinterpret_cast<float4 *>(o + plane) = make_float4(vG[0], vG[1], vG[2], vG[3]);
            *reinterpret_cast<float4 *>(o + cY * plane) = make_float4(vY[0], vY[1], vY[2], vY[3]);
        } else {
#pragma unroll
            for (int ox = 0; ox < PW; ++ox)
                if (x + ox < W) {
                    o[cX * plane + ox] = vX[ox];
                    o[plane + ox] = vG[ox];
                    o[cY * plane + ox] = vY[ox];
                }
        }
    }
}

}  // namespace sesrq_demosaick

using namespace sesrq_demosaick;

// one instantiation per (method, input, green diagonal)
enum { K_COUNT = 2 * IN_COUNT * 2 };
static const char *const kNames[K_COUNT] = {
    "demosaic<bilinear,u16,rggb|bggr>",   "demosaic<bilinear,u16,grbg|gbrg>",   "demosaic<bilinear,raw10,rggb|bggr>",  "demosaic<bilinear,raw10,grbg|gbrg>",
    "demosaic<bilinear,raw12,rggb|bggr>", "demosaic<bilinear,raw12,grbg|gbrg>", "demosaic<bilinear,spread,rggb|bggr>", "demosaic<bilinear,spread,grbg|gbrg>",
    "demosaic<malvar,u16,rggb|bggr>",     "demosaic<malvar,u16,grbg|gbrg>",     "demosaic<malvar,raw10,rggb|bggr>",    "demosaic<malvar,raw10,grbg|gbrg>",
    "demosaic<malvar,raw12,rggb|bggr>",   "demosaic<malvar,raw12,grbg|gbrg>",   "demosaic<malvar,spread,rggb|bggr>",   "demosaic<malvar,spread,grbg|gbrg>"};
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

// What both entries refuse of the method, the output and the frame; then the tiles of the batch, which must fit a grid.
static int check_frame(const char *who, int method, float *out, int N, int H, int W, Args *a, long long *tiles) {
    if (method != SESRQ_DEMOSAIC_BILINEAR && method != SESRQ_DEMOSAIC_MALVAR) return fail("%s: method %d (0 bilinear, 1 malvar)", who, method);
    if (!out) return fail("%s: out is NULL", who);
    if (reinterpret_cast<uintptr_t>(out) % 4) return fail("%s: out is not 4-byte aligned", who);
    if (N < 1) return fail("%s: empty batch (N = %d)", who, N);
    if (H < 2 || W < 2) return fail("%s: the reflection needs H, W >= 2, got H = %d, W = %d", who, H, W);
    if (H > 0x7fffffff - 128 || W > 0x7fffffff - 128) return fail("%s: frame of %d x %d is too large", who, H, W);
    const long long tx = ((long long)W + TW - 1) / TW, ty = ((long long)H + TH - 1) / TH;
    if (tx * ty > 0x7fffffffLL / N) return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);
    a->out = out;
    a->H = H;
    a->W = W;
    a->tiles_x = (int)tx;
    a->tiles_y = (int)ty;
    a->out_vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    *tiles = (long long)N * tx * ty;
    return 0;
}

template <int IN, bool GD>
static void launch_method(int method, unsigned grid, hipStream_t st, const Args &a) {
    if (method == SESRQ_DEMOSAIC_MALVAR)
        demosaic<IN, GD, SESRQ_DEMOSAIC_MALVAR><<<grid, THREADS, 0, st>>>(a);
    else
        demosaic<IN, GD, SESRQ_DEMOSAIC_BILINEAR><<<grid, THREADS, 0, st>>>(a);
}

// cfa fixes the green diagonal and which chroma the even rows hold; then one kernel
static int launch(const char *who, int in, int cfa, int method, long long tiles, void *stream, Args &a) {
    const bool gd = cfa == SESRQ_CFA_GRBG || cfa == SESRQ_CFA_GBRG;
    const bool red_first = cfa == SESRQ_CFA_RGGB || cfa == SESRQ_CFA_GRBG;      // R has its sites in the even rows
    a.cP = red_first ? 0 : 2;
    a.cQ = red_first ? 2 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)tiles;
    switch (in * 2 + gd) {
        case IN_U16 * 2: launch_method<IN_U16, false>(method, grid, st, a); break;
        case IN_U16 * 2 + 1: launch_method<IN_U16, true>(method, grid, st, a); break;
        case IN_RAW10 * 2: launch_method<IN_RAW10, false>(method, grid, st, a); break;
        case IN_RAW10 * 2 + 1: launch_method<IN_RAW10, true>(method, grid, st, a); break;
        case IN_RAW12 * 2: launch_method<IN_RAW12, false>(method, grid, st, a); break;
        case IN_RAW12 * 2 + 1: launch_method<IN_RAW12, true>(method, grid, st, a); break;
        case IN_SPREAD * 2: launch_method<IN_SPREAD, false>(method, grid, st, a); break;
        default: launch_method<IN_SPREAD, true>(method, grid, st, a); break;
    }
    return launched(who, g_count, (method * IN_COUNT + in) * 2 + gd);
}

extern "C" int sesrq_demosaic_raw(const sesrq_sensor_format *fmt, const void *raw, size_t row_stride_bytes, int method, float *out, int N,
                                  int H, int W, void *stream) {
    static const char who[] = "sesrq_demosaic_raw";
    g_err[0] = 0;
    if (check_format(who, fmt)) return 1;
    if (!raw) return fail("%s: raw is NULL", who);
    Args a = {};
    long long tiles;
    if (check_frame(who, method, out, N, H, W, &a, &tiles)) return 1;
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
    a.K = 16.f * (float)(fmt->white - fmt->black);
    a.in_vec = reinterpret_cast<uintptr_t>(raw) % in_align == 0 && row_stride_bytes % in_align == 0;
    return launch(who, pack, fmt->cfa, method, tiles, stream, a);
}

extern "C" int sesrq_demosaic_spread(int cfa, const float *spread, int method, float *out, int N, int H, int W, void *stream) {
    static const char who[] = "sesrq_demosaic_spread";
    g_err[0] = 0;
    if (cfa < SESRQ_CFA_RGGB || cfa > SESRQ_CFA_BGGR) return fail("%s: cfa %d is not a Bayer order (0 .. 3)", who, cfa);
    if (!spread) return fail("%s: spread is NULL", who);
    if (reinterpret_cast<uintptr_t>(spread) % 4) return fail("%s: spread is not 4-byte aligned", who);
    Args a = {};
    long long tiles;
    if (check_frame(who, method, out, N, H, W, &a, &tiles)) return 1;
    a.src = reinterpret_cast<const uint8_t *>(spread);
    a.K = 16.f;
    a.in_vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(spread) % 16 == 0;
    return launch(who, IN_SPREAD, cfa, method, tiles, stream, a);
}

extern "C" int sesrq_demosaic_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_demosaic_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_demosaic_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_demosaic_last_error(void) { return g_err; }
