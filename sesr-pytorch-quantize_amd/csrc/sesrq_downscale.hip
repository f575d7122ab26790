// libsesrq_downscale.so: the super-resolution nets' input from the HR image (include/sesrq_downscale.h, which fixes the arithmetic).  A
// library of its own: it links nothing of the other libraries and registers nothing in their instance tables; the decode of the LR
// bytes is the device body libsesrq_image.so runs (sesrq_image_decode.h).
//
// The reference's dataset reads a pre-made bicubic LR file next to the HR ground truth.  Here the HR image, which is on the device to
// be scored anyway, is the only upload: ONE kernel reads its 3 B/px once and writes q0 and / or the fp32 input (and, when asked, the
// LR image): 3 / r^2 ... 15 / r^2 bytes per HR pixel.  Neither the uint8 intermediate between the two passes nor the LR image needs to
// exist in memory.
//
// A workgroup of 256 lanes owns 128 x 32 HR pixels: 32 x 8 LR pixels at r = 4, 64 x 16 at r = 2.
//   stage       its HR window, (32 + 3 r) rows of (128 + 3 r) pixels, goes to LDS as bytes, a row at a time as 4-byte words: the part
//               of a row that lies inside the frame is one contiguous run of memory, read in words at whatever address it starts;
//               the few columns beyond a frame's left or right edge, and the odd bytes at the ends of the run, are read one by one
//               through the mirrored index.  Rows are mirrored as a whole.  The decode tables are requested before.
//   vertical    treats a staged row as 3 (128 + 3 r) independent byte columns -- interleaving does not matter to it: a lane takes one
//               word (4 columns) of one LR row, 4 r taps down the window, and writes the clamped uint8 intermediate back to LDS.
//   horizontal  a lane takes 12 bytes x 4 LR pixels' worth of one intermediate row as whole words (one LR pixel at r = 4: 16 taps x 3
//               channels = 12 words; two neighbours at r = 2: 10 pixels = 8 words), so taps at a 3-byte stride are register
//               bytes; lanes are 3 words apart, which is free of bank conflicts.
//   decode      the pixel's three bytes through sesrq_image_decode.h, stores per element: consecutive lanes, consecutive elements.
// Weights are literals of the unrolled tap loops.  The outputs asked for are a kernel argument (uniform branches), the factor and the
// form template parameters.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_downscale.h"
#include "sesrq_side.h"
#include "sesrq_image_decode.h"

static_assert(SESRQ_DOWNSCALE_Y == SESRQ_IMAGE_Y && SESRQ_DOWNSCALE_RGB == SESRQ_IMAGE_RGB, "the forms are sesrq_image.h's");

namespace sesrq_dsk {

using sesrq_imgdec::Quant;
using sesrq_imgdec::Tables;

constexpr int HR_W = SESRQ_DOWNSCALE_TILE_HR_W, HR_H = SESRQ_DOWNSCALE_TILE_HR_H;      // a workgroup's tile in HR pixels, at r = 2 and 4
constexpr int THREADS = 256;
constexpr int FORM_NONE = -1;                                   // the LR image alone: no decode, no tables

// Keys a = -1/2 stretched by r, times D: tap k of 4 r
__host__ __device__ constexpr int weight(int r, int k) {
    constexpr int W2[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
    constexpr int W4[16] = {-7, -45, -75, -49, 93, 399, 745, 987, 987, 745, 399, 93, -49, -75, -45, -7};
    return r == 4 ? W4[k] : W2[k];
}

template <int R>
struct Shape {
    static constexpr int TW = HR_W / R, TH = HR_H / R;           // the tile in LR pixels
    static constexpr int TAPS = 4 * R, REACH = 3 * R / 2;        // tap 0 of LR index d is HR index r d - REACH
    static constexpr int SHIFT = R == 4 ? 12 : 8, D = 1 << SHIFT;
    static constexpr int WP = HR_W + 3 * R, WR = HR_H + 3 * R;   // the staged window in HR pixels: r TW + 3 r columns, r TH + 3 r rows
    static constexpr int WB = 3 * WP;                            // bytes of a window row: 420 (r = 4), 402 (r = 2)
    static constexpr int KW = (WB + 3) / 4;                      // words of a window row: 105, 101
    static constexpr int PX = 4 / R;                             // LR pixels an item of the horizontal pass takes: it starts at byte 12 m
    static constexpr int IW = TW / PX, ITEMS = IW * TH;          // items a row (32), items a tile
    static constexpr int HWORDS = (3 * (R * (PX - 1) + TAPS) + 3) / 4;   // words an item reads: 12, 8
    static_assert(3 * (IW - 1) + HWORDS <= KW, "the last item stays inside its row");
};
static_assert(Shape<4>::TW == SESRQ_DOWNSCALE_TILE_W && Shape<4>::TH == SESRQ_DOWNSCALE_TILE_H, "the header's r = 4 tile");
static_assert(Shape<2>::TW == 2 * SESRQ_DOWNSCALE_TILE_W && Shape<2>::TH == 2 * SESRQ_DOWNSCALE_TILE_H, "the header's r = 2 tile");
static_assert(weight(2, 0) + weight(2, 1) + weight(2, 2) + weight(2, 3) == Shape<2>::D / 2, "r = 2 weights sum to D");

struct Args {
    const uint8_t *img;
    const Tables *tab;
    uint8_t *lr;
    int8_t *q0;
    float *x;
    int H, W, tiles_x, tiles_y, bgr;      // H, W: the HR size
    Quant q;
};

// step 2 of the header: index j of an axis of length n, mirrored with the edge sample repeated
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

// step 3: clamp(floor((s + D / 2) / D), 0, 255) of a sum that already holds D / 2.  Clamped first, shifted second: the same value
// (a negative sum gives 0, one of 256 D or more gives 255), in three plain instructions.  The shift-then-clamp form is selected as
// gfx950's packed v_ashr_pk_u8_i32, and a build with it gave bytes one or two above the definition on the device.
template <int SHIFT>
__device__ inline unsigned round_clamp(int s) { return (unsigned)min(max(s, 0), (256 << SHIFT) - 1) >> SHIFT; }

template <int R, int FORM>
__global__ __launch_bounds__(THREADS) void downscale(Args a) {
    using S = Shape<R>;
    constexpr int KW = S::KW, TAPS = S::TAPS;
    __shared__ uint4 s_tab[FORM == FORM_NONE ? 1 : sesrq_imgdec::table_words<FORM == FORM_NONE ? SESRQ_IMAGE_RGB : FORM>()];
    __shared__ unsigned s_win[S::WR * KW];
    __shared__ unsigned s_v[S::TH * KW];
    const int tid = threadIdx.x;
    if (FORM != FORM_NONE) sesrq_imgdec::stage_tables<FORM == FORM_NONE ? SESRQ_IMAGE_RGB : FORM, THREADS>(s_tab, a.tab);

    unsigned t = blockIdx.x;
    const int tx = (int)(t % (unsigned)a.tiles_x);
    t /= (unsigned)a.tiles_x;
    const int ty = (int)(t % (unsigned)a.tiles_y);
    const size_t n = t / (unsigned)a.tiles_y;
    const long long W = a.W, H = a.H;

    // stage.  Window column c is HR column xs + c; [c_lo, c_hi) lie inside the frame, columns from c_need on feed no LR pixel of it
    const long long xs = (long long)tx * HR_W - S::REACH, ys = (long long)ty * HR_H - S::REACH;
    const int c_lo = xs < 0 ? (int)-xs : 0;
    const int c_hi = (int)min((long long)S::WP, W - xs);
    const int c_need = (int)min((long long)S::WP, W - xs + S::REACH);
    const uint8_t *frame = a.img + n * (size_t)H * (size_t)W * 3;
    for (int it = tid; it < S::WR * KW; it += THREADS) {
        const int row = it / KW, b0 = 4 * (it - row * KW);
        long long gy = ys + row;
        if (gy < 0 || gy >= H) gy = mirror(gy, H);
        const uint8_t *line = frame + (size_t)gy * (size_t)W * 3;
        unsigned w = 0;
        if (b0 >= 3 * c_lo && b0 + 4 <= 3 * c_hi) {
            w = load_u32(line + (xs * 3 + b0));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = b0 + j;
                if (b < 3 * c_need) {
                    const int c = b / 3, ch = b - 3 * c;
                    long long gx = xs + c;
                    if (c < c_lo || c >= c_hi) gx = mirror(gx, W);
                    w |= (unsigned)line[gx * 3 + ch] << (8 * j);
                }
            }
        }
        s_win[it] = w;
    }
    __syncthreads();

    // vertical pass: LR row ly of the tile, word k of the row (4 byte columns); taps are window rows r ly .. r ly + 4 r - 1
    for (int it = tid; it < S::TH * KW; it += THREADS) {
        const int ly = it / KW, k = it - ly * KW;
        int acc[4] = {S::D / 2, S::D / 2, S::D / 2, S::D / 2};
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) {
            const unsigned wd = s_win[(R * ly + tp) * KW + k];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] += weight(R, tp) * (int)((wd >> (8 * c)) & 0xffu);
        }
        s_v[it] = round_clamp<S::SHIFT>(acc[0]) | round_clamp<S::SHIFT>(acc[1]) << 8 | round_clamp<S::SHIFT>(acc[2]) << 16 |
                  round_clamp<S::SHIFT>(acc[3]) << 24;
    }
    __syncthreads();

    // horizontal pass and decode
    const size_t Wl = (size_t)(W / R), Hl = (size_t)(H / R), HWl = Hl * Wl;
    const uint4 *tab = s_tab;
    for (int it = tid; it < S::ITEMS; it += THREADS) {
        const int ly = it / S::IW, m = it - ly * S::IW;
        unsigned w[S::HWORDS];
#pragma unroll
        for (int j = 0; j < S::HWORDS; ++j) w[j] = s_v[ly * KW + 3 * m + j];
        const size_t gy = (size_t)ty * S::TH + ly;
#pragma unroll
        for (int p = 0; p < S::PX; ++p) {
            const size_t gx = (size_t)tx * S::TW + m * S::PX + p;
            if (gx >= Wl || gy >= Hl) continue;
            unsigned v[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                int acc = S::D / 2;
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp) acc += weight(R, tp) * byte_of(w, (R * p + tp) * 3 + ch);
                v[ch] = round_clamp<S::SHIFT>(acc);
            }
            const size_t pix = gy * Wl + gx;
            if (a.lr) {
                uint8_t *d = a.lr + (n * HWl + pix) * 3;
                d[0] = (uint8_t)v[0];
                d[1] = (uint8_t)v[1];
                d[2] = (uint8_t)v[2];
            }
            if (FORM == SESRQ_IMAGE_Y) {
                const float f = sesrq_imgdec::luma(sesrq_imgdec::table_y(tab), a.bgr ? v[2] : v[0], v[1], a.bgr ? v[0] : v[2]);
                const size_t o = n * HWl + pix;
                if (a.q0) a.q0[o] = sesrq_imgdec::quant(f, a.q);
                if (a.x) a.x[o] = f;
            }
            if (FORM == SESRQ_IMAGE_RGB) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const size_t oc = (n * 3 + (size_t)(a.bgr ? 2 - c : c)) * HWl + pix;     // byte c of a pixel goes to this plane
                    if (a.q0) a.q0[oc] = sesrq_imgdec::table_q(tab)[v[c]];
                    if (a.x) a.x[oc] = sesrq_imgdec::table_x(tab)[v[c]];
                }
            }
        }
    }
}

}  // namespace sesrq_dsk

using namespace sesrq_dsk;

struct sesrq_downscale_ctx_s {
    DeviceTable t;     // Tables
    InQuant q;
};

enum { K_2L = 0, K_2Y, K_2R, K_4L, K_4Y, K_4R, K_COUNT };
static const char *const kNames[K_COUNT] = {"downscale<r2,lr>", "downscale<r2,Y>", "downscale<r2,RGB>",
                                            "downscale<r4,lr>", "downscale<r4,Y>", "downscale<r4,RGB>"};
static Counters<K_COUNT> g_count{kNames};

extern "C" int sesrq_downscale_weights(int r, int16_t *w, int *D) {
    g_err[0] = 0;
    if (r != 2 && r != 4) return fail("sesrq_downscale_weights: r = %d (2 or 4)", r);
    if (!w || !D) return fail("sesrq_downscale_weights: w or D is NULL");
    for (int k = 0; k < 4 * r; ++k) w[k] = (int16_t)weight(r, k);
    *D = r == 4 ? Shape<4>::D : Shape<2>::D;
    return 0;
}

extern "C" int sesrq_downscale_create(float scale_in, int zero_in, int exact_div, sesrq_downscale_ctx *out) {
    g_err[0] = 0;
    if (!out) return fail("sesrq_downscale_create: ctx is NULL");
    *out = nullptr;
    if (check_domain("sesrq_downscale_create", scale_in, zero_in, exact_div)) return 1;
    auto *c = new sesrq_downscale_ctx_s();
    c->q = in_quant(scale_in, zero_in, exact_div);
    Tables *host = new Tables();
    sesrq_imgdec::build(c->q, *host);
    const int rc = ctx_publish("sesrq_downscale_create", c, host, sizeof(Tables), out);
    delete host;
    return rc;
}

extern "C" void sesrq_downscale_destroy(sesrq_downscale_ctx c) { ctx_destroy(c); }

extern "C" int sesrq_downscale_run(sesrq_downscale_ctx c, const uint8_t *img, int order, int r, int form, uint8_t *lr, int8_t *q0, float *x,
                                   int N, int H, int W, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_downscale_run";
    const bool dec = q0 || x;
    if (!img) return fail("%s: img is NULL", who);
    if (!lr && !dec) return fail("%s: none of lr, q0 and x requested", who);
    if (dec && !c) return fail("%s: ctx is NULL (q0 and x need the decode tables)", who);
    if (order != SESRQ_DOWNSCALE_ORDER_RGB && order != SESRQ_DOWNSCALE_ORDER_BGR) return fail("%s: order %d (0 = RGB, 1 = BGR)", who, order);
    if (r != 2 && r != 4) return fail("%s: r = %d (2 or 4)", who, r);
    if (dec && form != SESRQ_DOWNSCALE_Y && form != SESRQ_DOWNSCALE_RGB) return fail("%s: form %d (0 = Y, 1 = RGB)", who, form);
    if (x && (reinterpret_cast<uintptr_t>(x) & 3)) return fail("%s: x is not 4-byte aligned", who);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    if (H % r || W % r)
        return fail("%s: an HR image of %d x %d is no multiple of r = %d each way; crop it first (modcrop)", who, H, W, r);
    const long long tx = ((long long)W + HR_W - 1) / HR_W, ty = ((long long)H + HR_H - 1) / HR_H, tiles = (long long)N * tx * ty;
    if (tiles > 0x7fffffffLL) return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);
    if (dec && table_on_current(who, c->t)) return 1;

    Args a;
    a.img = img;
    a.tab = dec ? static_cast<const Tables *>(c->t.ptr) : nullptr;
    a.lr = lr;
    a.q0 = q0;
    a.x = x;
    a.H = H;
    a.W = W;
    a.tiles_x = (int)tx;
    a.tiles_y = (int)ty;
    a.bgr = order == SESRQ_DOWNSCALE_ORDER_BGR;
    a.q = dec ? sesrq_imgdec::quant_of(c->q) : Quant{1.f, 1.f, 0.f, 0};
    const unsigned grid = (unsigned)tiles;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int f = dec ? form : FORM_NONE;
    int k;
#define SESRQ_DOWNSCALE_RUN(R, F, K)                            \
    if (r == R && f == F) {                                     \
        k = K;                                                  \
        downscale<R, F><<<grid, THREADS, 0, st>>>(a);           \
    }
    SESRQ_DOWNSCALE_RUN(2, FORM_NONE, K_2L)
    else SESRQ_DOWNSCALE_RUN(2, SESRQ_IMAGE_Y, K_2Y)
    else SESRQ_DOWNSCALE_RUN(2, SESRQ_IMAGE_RGB, K_2R)
    else SESRQ_DOWNSCALE_RUN(4, FORM_NONE, K_4L)
    else SESRQ_DOWNSCALE_RUN(4, SESRQ_IMAGE_Y, K_4Y)
    else SESRQ_DOWNSCALE_RUN(4, SESRQ_IMAGE_RGB, K_4R)
    else return fail("%s: unreachable instantiation", who);
#undef SESRQ_DOWNSCALE_RUN
    return launched(who, g_count, k);
}

extern "C" int sesrq_downscale_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_downscale_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_downscale_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_downscale_last_error(void) { return g_err; }
