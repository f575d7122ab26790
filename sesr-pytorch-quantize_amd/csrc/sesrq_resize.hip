// libsesrq_resize.so: predictions out at any size (include/sesrq_resize.h).  A library of its own: it links nothing of libsesrq.so and
// registers nothing in its instance table.
//
// The arithmetic is Pillow's 8-bit bicubic resize (libImaging/Resample.c): per axis a table of xmin, tap count and 22-bit integer
// weights built on the host in double, a horizontal pass into bytes, a vertical pass into bytes.  The phase of the taps differs from
// output pixel to output pixel, their number grows with the downscale ratio (5 for every upscale, 17 at / 4) and the window is cut
// and renormalised at the frame edge, so nothing of the fixed-ratio resamplers applies; the tables carry all of it.
//
// One 256-lane workgroup owns a tile of 192 output bytes (64 RGB pixels, 192 grey ones) by th output rows, th = 64, 32 or 16 chosen
// at create.  Its source window is [xmin(first column), xmax(last column)) x [ymin(first row), ymax(last row)): a few rows for many
// output rows when upscaling, 4 th + 13 rows of 4 tw + 13 pixels at / 4.  The tile's two tables are copied to LDS once (weight rows
// at a pitch of 17 words: odd, so the lanes of a wave, one output column or row each, hit different banks).  Then the window's source
// rows are streamed, SR = 8 at a time:
//   load        a run is a row of an interleaved image or a row of one plane of a prediction; whole aligned 32-bit words of a byte
//               source are loaded as such, the ragged ends by bytes, fp32 by elements, every word or element a lane's item of its
//               own (a wave walking one run at a time waited for memory once a run); each element becomes its byte (taken as
//               it is, or dequantised and clipped as every export does) on the way into the LDS strip, kept at the source's own
//               address phase so that the word stores stay aligned;
//   horizontal  a lane takes (source row, output pixel): its C accumulators share each weight read; the clamped bytes go to the
//               filtered window in LDS, 192 bytes a row, interleaved as the output is.
// Only the horizontally filtered window (window rows x 192 bytes, at most 80 rows) stays in LDS; the vertical pass reads it from
// there.  Its filter is the same for every byte of a row, so it no longer knows about channels: a lane takes (output row, run of 16
// bytes), reads one 16-byte word per tap, keeps 16 accumulators and stores one 16-byte word where the run is whole and aligned, bytes
// elsewhere.  The products are 22-bit weight x 8-bit byte and must be exact in 32 bits; no MFMA format carries a 22-bit integer
// operand (the int8 ones would need the weight in three limbs and three times the issue), so this is vector ALU work.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "sesrq_resize.h"
#include "sesrq_side.h"
#include "sesrq_pred_byte.h"

namespace sesrq_rsz {

constexpr int THREADS = 256;
constexpr int K = SESRQ_RESIZE_MAX_TAPS;      // pitch of a weight row, in the tables and in LDS
constexpr int BITS = SESRQ_RESIZE_BITS;
constexpr int TB = 192;                       // output bytes of a tile row: 64 pixels of 3, 192 of 1
constexpr int RUNS = TB / 16;                 // 16-byte runs of a tile row
constexpr int TH_MAX = 64;                    // output rows of a tile: 64, 32 or 16
constexpr int HROWS = 80;                     // rows of the filtered window LDS holds
constexpr int SR = 8;                         // source rows streamed at a time
constexpr int tile_w(int C) { return TB / C; }
constexpr int max_cols(int C) { return SESRQ_RESIZE_MAX_RATIO * tile_w(C) + 13; }      // window pixels of a tile at / 4
constexpr int plane_pitch(int C) { return (max_cols(C) + 3 + 3) & ~3; }                // + 3: the address phase of a byte run

struct Args {
    const void *src;
    uint8_t *out;
    const int *tab;                           // hmin[Wo] hcnt[Wo] hw[Wo][K] vmin[Ho] vcnt[Ho] vw[Ho][K]
    int H, W, Ho, Wo, th, tiles_x, tiles_y, bgr;
    float scale;
    int zero;
};

__device__ inline unsigned clamp_byte(int acc) { return (unsigned)min(max(acc >> BITS, 0), 255); }

// the byte of source code `raw` (the low 8 bits of a word)
template <int SRC>
__device__ inline unsigned code_byte(unsigned raw, const Args &a) {
    if (SRC == SESRQ_RESIZE_U8) return raw & 0xffu;
    return sesrq_pred::to_byte(sesrq_pred::dequant((int)(int8_t)(raw & 0xffu), a.zero, a.scale));
}

template <int SRC, int C>
__global__ __launch_bounds__(THREADS) void resize_bicubic(Args a) {
    constexpr int TW = tile_w(C), PW = plane_pitch(C), SP = C * PW;
    constexpr int RC = SRC == SESRQ_RESIZE_U8 ? 1 : C;           // runs of a source row
    static_assert(TW + TH_MAX <= THREADS, "one lane per table row");
    static_assert(max_cols(C) * C + 3 <= SP, "an interleaved row with its phase fits the strip");
    __shared__ __attribute__((aligned(16))) uint8_t s_h[HROWS * TB];
    __shared__ __attribute__((aligned(16))) uint8_t s_src[SR * SP];
    __shared__ int s_hw[TW * K], s_vw[TH_MAX * K], s_hx[TW], s_vy[TH_MAX], s_ph[SR * C];

    const int tid = threadIdx.x;
    const int b = blockIdx.x, bx = b % a.tiles_x, by = (b / a.tiles_x) % a.tiles_y, n = b / (a.tiles_x * a.tiles_y);
    const int x0 = bx * TW, y0 = by * a.th, tw = min(TW, a.Wo - x0), th = min(a.th, a.Ho - y0);
    const int *hmin = a.tab, *hcnt = hmin + a.Wo, *hw = hcnt + a.Wo;
    const int *vmin = hw + (size_t)a.Wo * K, *vcnt = vmin + a.Ho, *vw = vcnt + a.Ho;
    const int wx0 = hmin[x0], wcols = hmin[x0 + tw - 1] + hcnt[x0 + tw - 1] - wx0;
    const int wy0 = vmin[y0], wrows = vmin[y0 + th - 1] + vcnt[y0 + th - 1] - wy0;

    // the tile's tables: offset into the window and tap count packed, weights at pitch K; columns and rows past the frame get no taps
    if (tid < TW) {
        int cnt = 0, off = 0;
        if (tid < tw) {
            const int g = x0 + tid;
            cnt = hcnt[g];
            off = hmin[g] - wx0;
            for (int k = 0; k < cnt; ++k) s_hw[tid * K + k] = hw[(size_t)g * K + k];
        }
        s_hx[tid] = off | (cnt << 16);
    } else if (tid - TW < TH_MAX) {
        const int y = tid - TW;
        int cnt = 0, off = 0;
        if (y < th) {
            const int g = y0 + y;
            cnt = vcnt[g];
            off = vmin[g] - wy0;
            for (int k = 0; k < cnt; ++k) s_vw[y * K + k] = vw[(size_t)g * K + k];
        }
        s_vy[y] = off | (cnt << 16);
    }

    const uint8_t *sb = static_cast<const uint8_t *>(a.src);
    const float *sf = static_cast<const float *>(a.src);
    for (int r0 = 0; r0 < wrows; r0 += SR) {
        const int nr = min(SR, wrows - r0);
        // ---- load: source rows r0 .. r0 + nr of the window, as bytes
        const int L = SRC == SESRQ_RESIZE_U8 ? wcols * C : wcols;
        // every (run, slot) is an item of its own, so that a lane's loads are all in flight together: a slot is an element of an fp32
        // run, an aligned 32-bit word of a byte run (L + 6 >> 2 of them cover every address phase)
        const int slots = SRC == SESRQ_RESIZE_F32 ? L : (L + 6) >> 2;
        for (int it = tid; it < nr * RC * slots; it += THREADS) {
            const int run = it / slots, w = it - run * slots;
            const int r = RC == 1 ? run : run / C, c = RC == 1 ? 0 : run - r * C;
            const int sy = wy0 + r0 + r;
            const size_t base = SRC == SESRQ_RESIZE_U8 ? (((size_t)n * a.H + sy) * a.W + wx0) * C
                                                       : (((size_t)n * C + c) * a.H + sy) * a.W + wx0;
            uint8_t *d = s_src + r * SP + c * PW;
            if (SRC == SESRQ_RESIZE_F32) {
                d[w] = (uint8_t)sesrq_pred::to_byte(sf[base + w]);
                if (w == 0) s_ph[run] = 0;
            } else {
                const uint8_t *p = sb + base;
                const int ph = (int)(reinterpret_cast<uintptr_t>(p) & 3), lo = 4 * w;
                const uint8_t *q = p - ph;                        // 4-byte aligned; only bytes ph .. ph + L of it are read
                if (lo >= ph && lo + 4 <= ph + L) {
                    const unsigned v = *reinterpret_cast<const unsigned *>(q + lo);
                    *reinterpret_cast<unsigned *>(d + lo) = code_byte<SRC>(v, a) | (code_byte<SRC>(v >> 8, a) << 8) |
                                                            (code_byte<SRC>(v >> 16, a) << 16) | (code_byte<SRC>(v >> 24, a) << 24);
                } else {
                    for (int j = lo; j < lo + 4; ++j)
                        if (j >= ph && j < ph + L) d[j] = (uint8_t)code_byte<SRC>(q[j], a);
                }
                if (w == 0) s_ph[run] = ph;
            }
        }
        __syncthreads();
        // ---- horizontal: (source row, output pixel) -> C clamped bytes of the filtered window
        for (int it = tid; it < nr * TW; it += THREADS) {
            const int r = it / TW, x = it - r * TW, hx = s_hx[x], off = hx & 0xffff, cnt = hx >> 16;
            const uint8_t *sp[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int sc = C == 3 && a.bgr ? 2 - c : c;
                sp[c] = SRC == SESRQ_RESIZE_U8 ? s_src + r * SP + s_ph[r] + off * C + sc : s_src + r * SP + sc * PW + s_ph[r * C + sc] + off;
            }
            constexpr int STEP = SRC == SESRQ_RESIZE_U8 ? C : 1;
            int acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 1 << (BITS - 1);
            for (int k = 0; k < cnt; ++k) {
                const int w = s_hw[x * K + k];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += w * (int)sp[c][k * STEP];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) s_h[(r0 + r) * TB + x * C + c] = (uint8_t)clamp_byte(acc[c]);
        }
        __syncthreads();
    }

    // ---- vertical: (output row, run of 16 bytes) -> 16 bytes of the output
    const int row_bytes = tw * C;
    for (int it = tid; it < th * RUNS; it += THREADS) {
        const int y = it / RUNS, g = it - y * RUNS, nb = min(16, row_bytes - 16 * g);
        if (nb <= 0) continue;
        const int vy = s_vy[y], off = vy & 0xffff, cnt = vy >> 16;
        int acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 1 << (BITS - 1);
        for (int k = 0; k < cnt; ++k) {
            const int w = s_vw[y * K + k];
            const uint4 v = *reinterpret_cast<const uint4 *>(s_h + (off + k) * TB + 16 * g);
            const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += w * (int)((u[j >> 2] >> (8 * (j & 3))) & 0xffu);
        }
        unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j >> 2] |= clamp_byte(acc[j]) << (8 * (j & 3));
        uint8_t *dst = a.out + (((size_t)n * a.Ho + (y0 + y)) * a.Wo + x0) * C + 16 * g;
        if (nb == 16 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < nb) dst[j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
static double keys(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// The table of one axis (include/sesrq_resize.h, 2.), weights at pitch K; what it refuses is what every entry refuses of an axis.
static int axis_table(const char *who, const char *axis, int n_in, int n_out, int *xmin, int *count, int *weights) {
    if (n_in < 1 || n_out < 1) return fail("%s: %s %d -> %d: sizes must be at least 1", who, axis, n_in, n_out);
    if (n_in > (1 << 24) || n_out > (1 << 24)) return fail("%s: %s %d -> %d: sizes above 2^24 are not exact in Pillow's fp32 box", who, axis, n_in, n_out);
    if ((long long)n_in > (long long)SESRQ_RESIZE_MAX_RATIO * n_out)
        return fail("%s: %s %d -> %d is a downscale ratio above %d", who, axis, n_in, n_out, SESRQ_RESIZE_MAX_RATIO);
    const double scale = (double)n_in / n_out;
    const double fs = scale < 1.0 ? 1.0 : scale, support = 2.0 * fs, ss = 1.0 / fs;
    for (int i = 0; i < n_out; ++i) {
        const double c = (i + 0.5) * scale;
        int lo = (int)(c - support + 0.5), hi = (int)(c + support + 0.5);
        if (lo < 0) lo = 0;
        if (hi > n_in) hi = n_in;
        const int cnt = hi - lo;
        if (cnt < 1 || cnt > K) return fail("%s: %s %d -> %d: row %d has %d taps (1 .. %d)", who, axis, n_in, n_out, i, cnt, K);
        double w[K], ww = 0.0;
        for (int x = 0; x < cnt; ++x) {
            w[x] = keys((x + lo - c + 0.5) * ss);
            ww += w[x];
        }
        long long mag = 0;
        for (int x = 0; x < K; ++x) {
            int q = 0;
            if (x < cnt) {
                const double k = ww != 0.0 ? w[x] / ww : w[x];
                q = k < 0 ? (int)(-0.5 + k * (1 << BITS)) : (int)(0.5 + k * (1 << BITS));
            }
            weights[(size_t)i * K + x] = q;
            mag += q < 0 ? -(long long)q : q;
        }
        if (255 * mag + (1LL << (BITS - 1)) >= (1LL << 31))
            return fail("%s: %s %d -> %d: row %d can overflow the int32 accumulator (sum |weight| = %lld)", who, axis, n_in, n_out, i, mag);
        xmin[i] = lo;
        count[i] = cnt;
    }
    return 0;
}

// the widest source window of tiles of `t` outputs
static int worst_window(const int *xmin, const int *count, int n_out, int t) {
    int worst = 0;
    for (int o = 0; o < n_out; o += t) {
        const int l = (o + t < n_out ? o + t : n_out) - 1, span = xmin[l] + count[l] - xmin[o];
        if (span > worst) worst = span;
    }
    return worst;
}

}  // namespace sesrq_rsz

using namespace sesrq_rsz;

struct sesrq_resize_ctx_s {
    DeviceTable t;
    int H, W, Ho, Wo, th;
};
static_assert(SESRQ_RESIZE_F32 - 1 == PRED_F32 && SESRQ_RESIZE_I8 - 1 == PRED_I8, "check_pred's dtype");

enum { K_U1 = 0, K_U3, K_F1, K_F3, K_Q1, K_Q3, K_COUNT };
static const char *const kNames[K_COUNT] = {"resize<u8,C1>", "resize<u8,C3>", "resize<f32,C1>", "resize<f32,C3>", "resize<i8,C1>", "resize<i8,C3>"};
static Counters<K_COUNT> g_count{kNames};

extern "C" int sesrq_resize_coeffs(int n_in, int n_out, int32_t *xmin, int32_t *count, int32_t *weights) {
    g_err[0] = 0;
    if (!xmin || !count || !weights) return fail("sesrq_resize_coeffs: an output is NULL");
    return axis_table("sesrq_resize_coeffs", "axis", n_in, n_out, xmin, count, weights);
}

extern "C" int sesrq_resize_create(int H, int W, int Ho, int Wo, sesrq_resize_ctx *out) {
    g_err[0] = 0;
    const char *who = "sesrq_resize_create";
    if (!out) return fail("%s: ctx is NULL", who);
    if (H < 1 || W < 1 || Ho < 1 || Wo < 1) return fail("%s: sizes must be at least 1 (%d x %d -> %d x %d)", who, H, W, Ho, Wo);
    std::vector<int> tab((size_t)(Wo + Ho) * (K + 2));
    int *hmin = tab.data(), *hcnt = hmin + Wo, *hw = hcnt + Wo, *vmin = hw + (size_t)Wo * K, *vcnt = vmin + Ho, *vw = vcnt + Ho;
    if (axis_table(who, "width", W, Wo, hmin, hcnt, hw) || axis_table(who, "height", H, Ho, vmin, vcnt, vw)) return 1;
    // the tile: 192 output bytes wide whatever C is; the tallest whose worst window fits the filtered-window rows LDS holds
    for (int C = 1; C <= 3; C += 2)
        if (worst_window(hmin, hcnt, Wo, TB / C) > (C == 1 ? max_cols(1) : max_cols(3)))
            return fail("%s: a tile's source window is wider than LDS holds (unreachable below ratio %d)", who, SESRQ_RESIZE_MAX_RATIO);
    int th = TH_MAX;
    while (th >= 16 && worst_window(vmin, vcnt, Ho, th) > HROWS) th /= 2;
    if (th < 16) return fail("%s: a tile's source window is taller than LDS holds (unreachable below ratio %d)", who, SESRQ_RESIZE_MAX_RATIO);
    auto *c = new sesrq_resize_ctx_s{};
    c->H = H; c->W = W; c->Ho = Ho; c->Wo = Wo; c->th = th;
    return ctx_publish(who, c, tab.data(), tab.size() * sizeof(int), out);
}

extern "C" void sesrq_resize_destroy(sesrq_resize_ctx c) { ctx_destroy(c); }

extern "C" int sesrq_resize_tile(sesrq_resize_ctx c, int *tile_w, int *tile_h) {
    g_err[0] = 0;
    if (!c || !tile_w || !tile_h) return fail("sesrq_resize_tile: an argument is NULL");
    *tile_w = TB;
    *tile_h = c->th;
    return 0;
}

extern "C" int sesrq_resize_run(sesrq_resize_ctx c, const void *src, int src_dtype, float scale, int zero, int C, int order, uint8_t *out,
                                int N, int H, int W, int Ho, int Wo, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_resize_run";
    if (!c) return fail("%s: ctx is NULL", who);
    if (!src) return fail("%s: src is NULL", who);
    if (!out) return fail("%s: out is NULL", who);
    if (src_dtype != SESRQ_RESIZE_U8 && src_dtype != SESRQ_RESIZE_F32 && src_dtype != SESRQ_RESIZE_I8)
        return fail("%s: src_dtype %d (0 = uint8, 1 = fp32, 2 = int8)", who, src_dtype);
    if (src_dtype != SESRQ_RESIZE_U8 && check_pred(who, "src", src, src_dtype - 1, scale, zero, true)) return 1;
    if (C != 1 && C != 3) return fail("%s: %d channels (1 or 3)", who, C);
    if (order != SESRQ_RESIZE_ORDER_RGB && order != SESRQ_RESIZE_ORDER_BGR) return fail("%s: order %d (0 = RGB, 1 = BGR)", who, order);
    if (N < 1) return fail("%s: empty batch (N = %d)", who, N);
    if (H != c->H || W != c->W || Ho != c->Ho || Wo != c->Wo)
        return fail("%s: the context resizes %d x %d -> %d x %d, not %d x %d -> %d x %d", who, c->H, c->W, c->Ho, c->Wo, H, W, Ho, Wo);
    const int tw = tile_w(C), tx = (Wo + tw - 1) / tw, ty = (Ho + c->th - 1) / c->th;
    if ((long long)N * tx * ty > 0x7fffffffLL) return fail("%s: %d frames of %d x %d are too many tiles for a grid", who, N, Ho, Wo);
    if (table_on_current(who, c->t)) return 1;

    Args a;
    a.src = src;
    a.out = out;
    a.tab = static_cast<const int *>(c->t.ptr);
    a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
    a.th = c->th;
    a.tiles_x = tx;
    a.tiles_y = ty;
    a.bgr = order == SESRQ_RESIZE_ORDER_BGR;
    a.scale = scale;
    a.zero = zero;
    const int grid = N * tx * ty, k = 2 * src_dtype + (C == 3);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SESRQ_RESIZE_LAUNCH(S, CC)                                                       \
    if (src_dtype == S && C == CC) resize_bicubic<S, CC><<<grid, THREADS, 0, st>>>(a);
    SESRQ_RESIZE_LAUNCH(SESRQ_RESIZE_U8, 1)
    else SESRQ_RESIZE_LAUNCH(SESRQ_RESIZE_U8, 3)
    else SESRQ_RESIZE_LAUNCH(SESRQ_RESIZE_F32, 1)
    else SESRQ_RESIZE_LAUNCH(SESRQ_RESIZE_F32, 3)
    else SESRQ_RESIZE_LAUNCH(SESRQ_RESIZE_I8, 1)
    else SESRQ_RESIZE_LAUNCH(SESRQ_RESIZE_I8, 3)
#undef SESRQ_RESIZE_LAUNCH
    return launched(who, g_count, k);
}

extern "C" int sesrq_resize_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_resize_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_resize_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_resize_last_error(void) { return g_err; }
