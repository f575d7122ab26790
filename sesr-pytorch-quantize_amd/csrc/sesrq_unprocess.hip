// libsesrq_unprocess.so: raw-net inputs and their ground truth from an sRGB image (include/sesrq_unprocess.h).  A library of its own:
// it links nothing of the project's other libraries and registers nothing in their instance tables.
//
// The raw nets are trained and scored on unprocessed images: inverse tone curve, gamma expansion, rgb2cam, inverse gains, mosaic.
// This is that chain as one kernel, with the arithmetic the header fixes, and every tensor the raw route needs behind it from one
// read of the image: the sensor's frame, the ground truth, the net's q0 and its fp32 input frame.
//
// One lane owns 16 pixels of one row (a row segment), so the Bayer parity of its pixels is a per-item constant: (y & 1, k & 1) for
// pixel k of the segment, the segment starting at an even column.  The 48 image bytes come as three 16-byte loads.  The lane then
// walks its four quads of pixels; per pixel three lookups of L in LDS, nine multiplies and six adds, the highlight mask (two true
// quotients; skipped as a whole when the profile has none), three multiplies, clamps and rints.  What a quad produces leaves at
// once where it is wide enough -- gt and spread: one 16-byte store per plane and quad, four a plane -- and is collected in registers
// where it is not: eight dwords of raw (two 16-byte stores), four dwords of q0 per plane (one 16-byte store each).  So a lane never
// holds more than one quad of fp32 results.  Outputs nobody asked for cost nothing: OUT is a template flag set.
//
// The wide load and each wide store are chosen per segment and per buffer, where the segment is whole and that buffer's addresses
// of it are 16-byte aligned; the narrow forms (byte loads into the same twelve dwords, element stores out of the same registers)
// share all the arithmetic, so they give the same bytes.
//
// L (1 KiB) is staged in LDS once per block.  A pixel's three lookups are three instructions, so they cannot conflict with each
// other; lanes of one instruction hit the bank of their own byte (data dependent: equal bytes broadcast, different bytes of one
// bank serialise -- not measured).  The q0 table is staged behind L when it has at most 4096 entries (QLDS), and read through
// global memory when it is larger: at 65536 levels it would take the LDS of five of the eight blocks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "sesrq_unprocess.h"
#include "sesrq_side.h"

namespace sesrq_unpk {

constexpr int THREADS = 256;
constexpr int SEG = 16;                       // pixels per lane and row segment
constexpr int BLOCKS_PER_CU = 8;              // 256-thread blocks: a full CU (32 waves)
constexpr int CODES = SESRQ_UNPROCESS_CODES;
constexpr int L_BYTES = CODES * 4;
constexpr int Q_LDS = 4096;                   // entries of a q0 table that is staged in LDS
enum { OUT_RAW = 1, OUT_GT = 2, OUT_Q = 4, OUT_SPREAD = 8 };

// 2 bits per parity (py * 2 + px) of each CFA order: its site channel (SESRQ_CFA_* of include/sesrq_sensor.h)
constexpr int SITES[4] = {0 | 1 << 2 | 1 << 4 | 2 << 6, 1 | 0 << 2 | 2 << 4 | 1 << 6, 1 | 2 << 2 | 0 << 4 | 1 << 6,
                          2 | 1 << 2 | 1 << 4 | 0 << 6};

struct Args {
    const uint8_t *img;
    uint16_t *raw;
    float *gt;
    int8_t *q0;
    float *spread;
    const uint8_t *tab;    // device: L, then the q0 table (at least Q_LDS entries, a multiple of 16)
    int H, W, segs, items;
    int bgr, highlight, sites, black, t0;
    float range;           // fl32(white - black), exact
    float m[9], d[3];
};

__device__ inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// steps 1 .. 5 of one pixel from its bytes in R, G, B order
__device__ inline void unprocess_px(const Args &a, const float *L, unsigned bR, unsigned bG, unsigned bB, int (&k)[3]) {
    const float l[3] = {L[bR], L[bG], L[bB]};
    float c[3], s[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        c[i] = __fadd_rn(__fadd_rn(__fmul_rn(a.m[3 * i], l[0]), __fmul_rn(a.m[3 * i + 1], l[1])), __fmul_rn(a.m[3 * i + 2], l[2]));
    if (a.highlight) {
        const float g = __fdiv_rn(__fadd_rn(__fadd_rn(c[0], c[1]), c[2]), 3.0f);
        const float t = __fdiv_rn(fmaxf(__fsub_rn(g, 0.9f), 0.f), 0.1f);
        const float kk = __fmul_rn(t, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] = fmaxf(__fadd_rn(kk, __fmul_rn(__fsub_rn(1.f, kk), a.d[i])), a.d[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] = a.d[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float r = fminf(fmaxf(__fmul_rn(c[i], s[i]), 0.f), 1.f);
        k[i] = (int)rintf(__fmul_rn(r, a.range));
    }
}

// Eight waves a SIMD (at most 64 VGPRs) without scratch for every set of outputs but the full one, which takes 66 / 68: seven waves there.
template <int OUT, bool QLDS>
__global__ __launch_bounds__(THREADS, OUT == 15 ? 7 : 8) void unprocess(Args a) {
    constexpr bool STAGE_Q = (OUT & OUT_Q) && QLDS;
    constexpr int WORDS = (L_BYTES + (STAGE_Q ? Q_LDS : 0)) / 16;
    __shared__ uint4 s_tab[WORDS];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.tab);
        for (int i = threadIdx.x; i < WORDS; i += THREADS) s_tab[i] = src[i];
    }
    __syncthreads();
    const float *L = reinterpret_cast<const float *>(s_tab);
    auto q_of = [&](int k) -> unsigned {
        if constexpr (STAGE_Q) return reinterpret_cast<const uint8_t *>(s_tab)[L_BYTES + k];
        else return a.tab[L_BYTES + k];
    };
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W;
    const unsigned t0 = (unsigned)(uint8_t)a.t0, z4 = t0 * 0x01010101u;
    const float range = a.range;

    for (int i = blockIdx.x * THREADS + threadIdx.x; i < a.items; i += gridDim.x * THREADS) {
        const int row = i / a.segs, seg = i - row * a.segs;
        const int n = row / H, y = row - n * H, x0 = seg * SEG;
        const int npx = min(SEG, W - x0);
        const bool whole = npx == SEG;
        // site channel of the even / the odd columns of this row
        const int ph = a.sites >> (4 * (y & 1));
        const int ce = ph & 3, co = (ph >> 2) & 3;
        const size_t pix = (size_t)row * W + x0;                 // of (N, H, W)
        const size_t base = ((size_t)n * 3 * H + y) * W + x0;    // plane (n, c, y) starts at base + c * plane
        const uint8_t *src = a.img + pix * 3;

        // the 48 bytes as twelve dwords: three 16-byte loads where the address allows, byte by byte otherwise.  The third word is
        // fetched when the first two quads are done (quad 2 is the first to read it): four registers fewer while they run.
        unsigned w[12];
        const bool in_w = whole && aligned16(src);
        auto fetch = [&](int first, int last) {          // the 16-byte words first .. last - 1
            if (in_w) {
#pragma unroll
                for (int j = first; j < last; ++j) {
                    const uint4 v = reinterpret_cast<const uint4 *>(src)[j];
                    w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 4 * first; j < 4 * last; ++j) w[j] = 0;
#pragma unroll
                for (int b = 16 * first; b < 16 * last; ++b)
                    if (b < 3 * npx) w[b >> 2] |= (unsigned)src[b] << (8 * (b & 3));
            }
        };
        fetch(0, 2);
        auto byte = [&](int b) { return (w[b >> 2] >> (8 * (b & 3))) & 0xffu; };

        bool gt_w = false, sp_w = false, q_w = false, raw_w = false;
        if (OUT & OUT_GT) gt_w = whole && aligned16(a.gt + base) && aligned16(a.gt + base + plane) && aligned16(a.gt + base + 2 * plane);
        if (OUT & OUT_SPREAD)
            sp_w = whole && aligned16(a.spread + base) && aligned16(a.spread + base + plane) && aligned16(a.spread + base + 2 * plane);
        if (OUT & OUT_Q) q_w = whole && aligned16(a.q0 + base) && aligned16(a.q0 + base + plane) && aligned16(a.q0 + base + 2 * plane);
        if (OUT & OUT_RAW) raw_w = whole && aligned16(a.raw + pix);

        unsigned rw[SEG / 4], qs[SEG / 4];
#pragma unroll
        for (int j = 0; j < SEG / 4; ++j) {
            if (j == 2) fetch(2, 3);
            int k[4][3], ks[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int b = 3 * (4 * j + p);
                unprocess_px(a, L, a.bgr ? byte(b + 2) : byte(b), byte(b + 1), a.bgr ? byte(b) : byte(b + 2), k[p]);
                const int cs = (p & 1) ? co : ce;
                ks[p] = cs == 0 ? k[p][0] : cs == 1 ? k[p][1] : k[p][2];
            }
            if (OUT & OUT_RAW) {
                rw[2 * (j & 1)] = (unsigned)(a.black + ks[0]) | (unsigned)(a.black + ks[1]) << 16;
                rw[2 * (j & 1) + 1] = (unsigned)(a.black + ks[2]) | (unsigned)(a.black + ks[3]) << 16;
                if (j & 1) {             // a half of the segment is complete
                    uint16_t *dst = a.raw + pix + 4 * (j - 1);
                    if (raw_w) {
                        *reinterpret_cast<uint4 *>(dst) = make_uint4(rw[0], rw[1], rw[2], rw[3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < SEG / 2; ++k)
                            if (4 * (j - 1) + k < npx) dst[k] = (uint16_t)(rw[k >> 1] >> (16 * (k & 1)));
                    }
                }
            }
            if (OUT & OUT_Q) {
                qs[j] = q_of(ks[0]) | q_of(ks[1]) << 8 | q_of(ks[2]) << 16 | q_of(ks[3]) << 24;       // every pixel's site byte
            }
            // the fp32 outputs, a plane at a time: plane c of spread holds plane c of gt at its sites
            auto store4 = [&](float *dst, bool wide, const float (&v)[4]) {
                if (wide) {
                    *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        if (4 * j + p < npx) dst[p] = v[p];
                }
            };
            if (OUT & OUT_GT) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float f[4] = {__fdiv_rn((float)k[0][c], range), __fdiv_rn((float)k[1][c], range), __fdiv_rn((float)k[2][c], range),
                                        __fdiv_rn((float)k[3][c], range)};
                    store4(a.gt + base + c * plane + 4 * j, gt_w, f);
                    if (OUT & OUT_SPREAD) {
                        const float v[4] = {c == ce ? f[0] : 0.f, c == co ? f[1] : 0.f, c == ce ? f[2] : 0.f, c == co ? f[3] : 0.f};
                        store4(a.spread + base + c * plane + 4 * j, sp_w, v);
                    }
                    __builtin_amdgcn_sched_barrier(0);       // one plane's quotients at a time
                }
            } else if (OUT & OUT_SPREAD) {
                const float f[4] = {__fdiv_rn((float)ks[0], range), __fdiv_rn((float)ks[1], range), __fdiv_rn((float)ks[2], range),
                                    __fdiv_rn((float)ks[3], range)};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v[4] = {c == ce ? f[0] : 0.f, c == co ? f[1] : 0.f, c == ce ? f[2] : 0.f, c == co ? f[3] : 0.f};
                    store4(a.spread + base + c * plane + 4 * j, sp_w, v);
                }
            }
            __builtin_amdgcn_sched_barrier(0);       // one quad's results at a time: no more live registers than that
        }
        if (OUT & OUT_Q) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int8_t *dst = a.q0 + base + c * plane;
                unsigned v[SEG / 4];
#pragma unroll
                for (int j = 0; j < SEG / 4; ++j)      // the even columns' site bytes in their plane, the odd columns' in theirs, q0(0) elsewhere
                    v[j] = c == ce ? (z4 & 0xff00ff00u) | (qs[j] & 0x00ff00ffu) : c == co ? (z4 & 0x00ff00ffu) | (qs[j] & 0xff00ff00u) : z4;
                if (q_w) {
                    *reinterpret_cast<uint4 *>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < SEG; ++k)
                        if (k < npx) dst[k] = (int8_t)(v[k >> 2] >> (8 * (k & 3)));
                }
            }
        }
    }
}

}  // namespace sesrq_unpk

using namespace sesrq_unpk;

struct sesrq_unprocess_ctx_s {
    DeviceTable t;     // L, then the q0 table
    float m[9], d[3];
    int highlight, sites, black, D, t0;
};

// The fixed instantiation list: every non-empty set of outputs, and for the sets with q0 both homes of its table.
#define SETS_NOQ(X) X(1, "raw") X(2, "gt") X(3, "raw+gt") X(8, "spread") X(9, "raw+spread") X(10, "gt+spread") X(11, "raw+gt+spread")
#define SETS_Q(X)                                                                                                                  \
    X(4, "q0") X(5, "raw+q0") X(6, "gt+q0") X(7, "raw+gt+q0") X(12, "q0+spread") X(13, "raw+q0+spread") X(14, "gt+q0+spread")       \
    X(15, "raw+gt+q0+spread")
#define X(mask, name) K_##mask,
#define XQ(mask, name) K_##mask##_LDS, K_##mask##_GLOBAL,
enum { SETS_NOQ(X) SETS_Q(XQ) K_COUNT };
#undef X
#undef XQ
#define X(mask, name) "unprocess<" name ">",
#define XQ(mask, name) "unprocess<" name ", lds>", "unprocess<" name ", global>",
static const char *const kNames[K_COUNT] = {SETS_NOQ(X) SETS_Q(XQ)};
#undef X
#undef XQ
static Counters<K_COUNT> g_count{kNames};

extern "C" int sesrq_unprocess_curve(int kind, float L[SESRQ_UNPROCESS_CODES]) {
    g_err[0] = 0;
    if (!L) return fail("sesrq_unprocess_curve: L is NULL");
    if (kind < SESRQ_UNPROCESS_PAPER || kind > SESRQ_UNPROCESS_LINEAR)
        return fail("sesrq_unprocess_curve: kind %d (0 = paper, 1 = gamma 2.2, 2 = sRGB, 3 = linear)", kind);
    for (int b = 0; b < CODES; ++b) {
        if (kind == SESRQ_UNPROCESS_LINEAR) {
            const volatile float q = (float)b / 255.0f;
            L[b] = q;
            continue;
        }
        // the exact value in 64 significant bits, rounded once to fp32 (tests/test_unprocess_oracle.py checks every entry against a
        // 60-digit evaluation)
        const long double v = (long double)b / 255.0L;
        long double x;
        if (kind == SESRQ_UNPROCESS_PAPER) {
            const long double u = 0.5L - sinl(asinl(1.0L - 2.0L * v) / 3.0L);
            x = powl(u > 1e-8L ? u : 1e-8L, 11.0L / 5.0L);
        } else if (kind == SESRQ_UNPROCESS_GAMMA22) {
            x = powl(v, 11.0L / 5.0L);
        } else {
            x = v > 0.04045L ? powl((v + 0.055L) / 1.055L, 12.0L / 5.0L) : v / 12.92L;
        }
        L[b] = (float)x;
    }
    return 0;
}

extern "C" int sesrq_unprocess_create(const float L[SESRQ_UNPROCESS_CODES], const float m[9], const float d[3], int highlight, int cfa,
                                      int black, int white, float scale_in, int zero_in, int exact_div, sesrq_unprocess_ctx *out) {
    g_err[0] = 0;
    const char *who = "sesrq_unprocess_create";
    if (!out) return fail("%s: ctx is NULL", who);
    *out = nullptr;
    if (!L || !m || !d) return fail("%s: L, m or d is NULL", who);
    for (int b = 0; b < CODES; ++b)
        if (!std::isfinite(L[b])) return fail("%s: table entry %d is not finite", who, b);
    for (int j = 0; j < 9; ++j)
        if (!std::isfinite(m[j])) return fail("%s: matrix entry %d is not finite", who, j);
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(d[c]) || d[c] < 0.f) return fail("%s: inverse gain %d must be finite and not negative", who, c);
    if (highlight != 0 && highlight != 1) return fail("%s: highlight %d (0 or 1)", who, highlight);
    if (cfa < 0 || cfa > 3) return fail("%s: cfa %d (0 = RGGB, 1 = GRBG, 2 = GBRG, 3 = BGGR)", who, cfa);
    if (black < 0 || black >= white || white > 65535) return fail("%s: levels need 0 <= black < white <= 65535, got %d and %d", who, black, white);
    if (check_domain(who, scale_in, zero_in, exact_div)) return 1;

    const int D = white - black, entries = D + 1 > Q_LDS ? (D + 1 + 15) / 16 * 16 : Q_LDS;
    const size_t bytes = (size_t)L_BYTES + entries;
    uint8_t *host = static_cast<uint8_t *>(calloc(bytes, 1));
    if (!host) return fail("%s: out of host memory", who);
    memcpy(host, L, L_BYTES);
    level_table(D, in_quant(scale_in, zero_in, exact_div), reinterpret_cast<int8_t *>(host + L_BYTES));
    auto *c = new sesrq_unprocess_ctx_s();
    memcpy(c->m, m, sizeof c->m);
    memcpy(c->d, d, sizeof c->d);
    c->highlight = highlight;
    c->sites = SITES[cfa];
    c->black = black;
    c->D = D;
    c->t0 = (int8_t)host[L_BYTES];
    const int rc = ctx_publish(who, c, host, bytes, out);
    free(host);
    return rc;
}

extern "C" void sesrq_unprocess_destroy(sesrq_unprocess_ctx c) { ctx_destroy(c); }

extern "C" int sesrq_unprocess_run(sesrq_unprocess_ctx c, const uint8_t *img, int order, uint16_t *raw, float *gt, int8_t *q0,
                                   float *spread, int N, int H, int W, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_unprocess_run";
    if (!c) return fail("%s: ctx is NULL", who);
    if (!img) return fail("%s: img is NULL", who);
    if (!raw && !gt && !q0 && !spread) return fail("%s: none of raw, gt, q0 and spread requested", who);
    if (order != SESRQ_UNPROCESS_ORDER_RGB && order != SESRQ_UNPROCESS_ORDER_BGR) return fail("%s: order %d (0 = RGB, 1 = BGR)", who, order);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    if (reinterpret_cast<uintptr_t>(raw) & 1) return fail("%s: raw is not 2-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(gt) & 3) || (reinterpret_cast<uintptr_t>(spread) & 3)) return fail("%s: gt or spread is not 4-byte aligned", who);
    // the 16-pixel segments must fit an int together with one round of the grid; a generous bound on the grid (1024 CUs) keeps the
    // check independent of the device
    int segs, items;
    if (segment_items(who, N, H, W, SEG, (long long)THREADS * 1024 * BLOCKS_PER_CU, &segs, &items)) return 1;
    if (table_on_current(who, c->t)) return 1;

    Args a;
    a.img = img;
    a.raw = raw;
    a.gt = gt;
    a.q0 = q0;
    a.spread = spread;
    a.tab = static_cast<const uint8_t *>(c->t.ptr);
    a.H = H;
    a.W = W;
    a.segs = segs;
    a.items = items;
    a.bgr = order == SESRQ_UNPROCESS_ORDER_BGR;
    a.highlight = c->highlight;
    a.sites = c->sites;
    a.black = c->black;
    a.t0 = c->t0;
    a.range = (float)c->D;
    memcpy(a.m, c->m, sizeof a.m);
    memcpy(a.d, c->d, sizeof a.d);
    const int grid = grid_cap(items, THREADS, c->t.num_cu < 1024 ? c->t.num_cu : 1024, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int mask = (raw ? OUT_RAW : 0) | (gt ? OUT_GT : 0) | (q0 ? OUT_Q : 0) | (spread ? OUT_SPREAD : 0);
    const bool lds = c->D + 1 <= Q_LDS;
    int k = -1;
    switch (mask) {
#define X(m, name)                                 \
    case m:                                        \
        unprocess<m, true><<<grid, THREADS, 0, st>>>(a); \
        k = K_##m;                                 \
        break;
#define XQ(m, name)                                               \
    case m:                                                       \
        if (lds) unprocess<m, true><<<grid, THREADS, 0, st>>>(a); \
        else unprocess<m, false><<<grid, THREADS, 0, st>>>(a);    \
        k = lds ? K_##m##_LDS : K_##m##_GLOBAL;                   \
        break;
        SETS_NOQ(X)
        SETS_Q(XQ)
#undef X
#undef XQ
    }
    return launched(who, g_count, k);
}

extern "C" int sesrq_unprocess_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_unprocess_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_unprocess_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_unprocess_last_error(void) { return g_err; }
