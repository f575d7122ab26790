// libsesrq_develop.so: display images out of the raw nets (include/sesrq_develop.h).  A library of its own: it links nothing of the
// project's other libraries and registers nothing in their instance tables.
//
// The nets of MFLAG 2, 3 and 4 return linear camera RGB; the reference's metadata2tensor (self_dataset.py) prepares cam2rgb and the
// white-balance gains and never applies them.  This is the `process` tail of the unprocessing pipeline its data comes from -- gains,
// clip, colour matrix, tone curve, bytes -- as one kernel, with the arithmetic the header fixes.
//
// The skeleton is image_export<PRED, 3> of sesrq_image.hip: a lane owns a run of 16 pixels of the flattened H * W, reads them from the
// three planes (fp32: four 16-byte words a plane; int8: one) and writes the 48 interleaved bytes as three 16-byte words; a grid-stride
// loop over the runs; runs that are partial or not 16-byte aligned take the per-pixel path of the same kernel.  New per pixel: three
// multiplies and clips, nine multiplies and six adds, and three threshold counts.
//
// The count #{k : o >= T[k]} is what is stored.  It is found by a branch-free binary search over the thresholds in LDS that a second
// LDS table shortens: o in [0, 1] is non-negative, so its bits order as its value does, and the top bits (sign masked, exponent and
// SUB mantissa bits, from 2^-OCTAVES up; everything below is one bucket) select a bucket whose entry is the number of thresholds at
// or below the bucket's smallest value.  The host knows the largest number of thresholds that lie inside any one bucket and passes
// the number of search steps that covers it (`depth`: 2^depth - 1 >= that number): 1 for the gamma and sRGB tables, 2 for TRUNC255,
// up to 8 for a table with all its thresholds in one bucket.  With an empty index and depth 8 it is the plain 8-step search.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "sesrq_develop.h"
#include "sesrq_side.h"

namespace sesrq_devk {

constexpr int THREADS = 256;
constexpr int SEG = 16;                       // pixels per lane and run
constexpr int BLOCKS_PER_CU = 8;              // 256-thread blocks: a full CU (32 waves)
constexpr int LEVELS = SESRQ_DEVELOP_LEVELS;
constexpr int T_PAD = 512;                    // T[1 .. 255], then +inf: pos + step <= 255 + 255
constexpr int SUB = 7;                        // mantissa bits of the bucket key: 128 buckets an octave
constexpr int OCTAVES = 20;                   // [2^-20, 1]; below: bucket 0
constexpr int KEY_SHIFT = 23 - SUB;
constexpr int KEY_BASE = ((127 - OCTAVES) << SUB) - 1;       // key of 2^-OCTAVES is KEY_BASE + 1
constexpr int BUCKETS = (127 << SUB) - KEY_BASE + 1;         // the last one holds 1.0
constexpr int LO_PAD = (BUCKETS + 15) / 16 * 16;

struct Table {
    float T[T_PAD];
    uint8_t lo[LO_PAD];
};
constexpr int WORDS = sizeof(Table) / 16;
static_assert(sizeof(Table) % 16 == 0 && WORDS <= 2 * THREADS, "staging: at most two words per thread");

struct Args {
    const void *pred;
    uint8_t *out;
    const Table *tab;
    int HW, segs, items, bgr, planes16, depth;
    float scale;
    int zero;
    float g[3], m[9];
};

__device__ inline float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// step 4: the count, from the bucket's certain part in `depth` compares
__device__ inline unsigned tone(const Table &t, float o, int depth) {
    const int key = (int)((__float_as_uint(o) & 0x7fffffffu) >> KEY_SHIFT) - KEY_BASE;      // -0.0 is 0.0
    int pos = t.lo[min(max(key, 0), BUCKETS - 1)];
    for (int s = 1 << depth >> 1; s; s >>= 1) pos += o >= t.T[pos + s] ? s : 0;
    return (unsigned)pos;
}

// steps 1 .. 4 of one pixel: the three bytes in R, G, B order
__device__ inline void develop(const Args &a, const Table &t, float pr, float pg, float pb, unsigned (&b)[3]) {
    const float p[3] = {pr, pg, pb};
    float w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c] = fminf(__fmul_rn(clip01(p[c]), a.g[c]), 1.f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float o = __fadd_rn(__fadd_rn(__fmul_rn(a.m[3 * c], w[0]), __fmul_rn(a.m[3 * c + 1], w[1])), __fmul_rn(a.m[3 * c + 2], w[2]));
        b[c] = tone(t, clip01(o), a.depth);
    }
}

template <int PRED>
__global__ __launch_bounds__(THREADS) void develop_export(Args a) {
    __shared__ uint4 s_tab[WORDS];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.tab);
        for (int i = threadIdx.x; i < WORDS; i += THREADS) s_tab[i] = src[i];
    }
    __syncthreads();
    const Table &t = *reinterpret_cast<const Table *>(s_tab);
    const size_t HW = (size_t)a.HW;
    const float *pf = static_cast<const float *>(a.pred);
    const int8_t *pq = static_cast<const int8_t *>(a.pred);
    auto val = [&](int8_t q) { return __fmul_rn((float)((int)q - a.zero), a.scale); };
    const int ir = a.bgr ? 2 : 0;                         // byte position of R in a pixel (B sits at 2 - ir)

    for (int i = blockIdx.x * THREADS + threadIdx.x; i < a.items; i += gridDim.x * THREADS) {
        const int n = i / a.segs, p0 = (i - n * a.segs) * SEG;
        const size_t in0 = (size_t)n * 3 * HW + p0;       // plane R of frame n, pixel p0
        uint8_t *dst = a.out + ((size_t)n * HW + p0) * 3;
        const int npx = min(SEG, a.HW - p0);
        const bool vec = npx == SEG && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 && a.planes16 &&
                         (reinterpret_cast<uintptr_t>(PRED == SESRQ_DEVELOP_F32 ? (const void *)(pf + in0) : (const void *)(pq + in0)) & 15) == 0;
        if (vec) {
            float p[3][SEG];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (PRED == SESRQ_DEVELOP_F32) {
                    const float4 *s = reinterpret_cast<const float4 *>(pf + in0 + c * HW);
#pragma unroll
                    for (int k = 0; k < SEG / 4; ++k) {
                        const float4 v = s[k];
                        p[c][4 * k] = v.x; p[c][4 * k + 1] = v.y; p[c][4 * k + 2] = v.z; p[c][4 * k + 3] = v.w;
                    }
                } else {
                    const uint4 v = *reinterpret_cast<const uint4 *>(pq + in0 + c * HW);
                    const unsigned ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int k = 0; k < SEG; ++k) p[c][k] = val((int8_t)((ww[k >> 2] >> (8 * (k & 3))) & 0xffu));
                }
            }
            unsigned o[3 * SEG / 4];
#pragma unroll
            for (int j = 0; j < 3 * SEG / 4; ++j) o[j] = 0;
#pragma unroll
            for (int k = 0; k < SEG; ++k) {
                unsigned b[3];
                develop(a, t, p[0][k], p[1][k], p[2][k], b);
                const unsigned px[3] = {ir ? b[2] : b[0], b[1], ir ? b[0] : b[2]};
#pragma unroll
                for (int c = 0; c < 3; ++c) o[(3 * k + c) >> 2] |= px[c] << (8 * ((3 * k + c) & 3));
            }
            uint4 *d = reinterpret_cast<uint4 *>(dst);
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        } else {
            for (int k = 0; k < npx; ++k) {
                unsigned b[3];
                if (PRED == SESRQ_DEVELOP_F32) develop(a, t, pf[in0 + k], pf[in0 + HW + k], pf[in0 + 2 * HW + k], b);
                else develop(a, t, val(pq[in0 + k]), val(pq[in0 + HW + k]), val(pq[in0 + 2 * HW + k]), b);
                dst[3 * k + ir] = (uint8_t)b[0];
                dst[3 * k + 1] = (uint8_t)b[1];
                dst[3 * k + 2 - ir] = (uint8_t)b[2];
            }
        }
    }
}

}  // namespace sesrq_devk

using namespace sesrq_devk;

struct sesrq_develop_ctx_s {
    DeviceTable t;     // Table
    float g[3], m[9];
    int depth;
};

enum { K_F32 = 0, K_I8, K_COUNT };
static const char *const kNames[K_COUNT] = {"develop_export<f32>", "develop_export<i8>"};
static Counters<K_COUNT> g_count{kNames};

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// #{k : T[k] <= v} of a non-decreasing table
static int count_le(const float *T, float v) {
    int c = 0;
    while (c < LEVELS && T[c] <= v) ++c;
    return c;
}

// The device table of thresholds T[k - 1], k = 1 .. 255, and the number of search steps it needs.
static int build(const float *T, bool full, Table &tab) {
    tab.T[0] = -INFINITY;                                   // never read: pos + step >= 1
    for (int k = 1; k < T_PAD; ++k) tab.T[k] = k <= LEVELS ? T[k - 1] : INFINITY;
    memset(tab.lo, 0, sizeof tab.lo);
    if (full) return 8;
    int most = 0;
    for (int b = 0; b < BUCKETS; ++b) {
        // the floats of bucket b: bucket 0 everything below 2^-OCTAVES, bucket b >= 1 the key KEY_BASE + b
        const float first = b == 0 ? 0.f : from_bits((uint32_t)(KEY_BASE + b) << KEY_SHIFT);
        const float last = from_bits(((uint32_t)(KEY_BASE + b + 1) << KEY_SHIFT) - 1);
        const int lo = count_le(T, first), hi = count_le(T, last);
        tab.lo[b] = (uint8_t)lo;
        if (hi - lo > most) most = hi - lo;
    }
    int depth = 0;
    while ((1 << depth) - 1 < most) ++depth;
    return depth;
}

extern "C" int sesrq_develop_curve(int kind, float T[SESRQ_DEVELOP_LEVELS]) {
    g_err[0] = 0;
    if (!T) return fail("sesrq_develop_curve: T is NULL");
    if (kind != SESRQ_DEVELOP_GAMMA22 && kind != SESRQ_DEVELOP_SRGB && kind != SESRQ_DEVELOP_TRUNC255)
        return fail("sesrq_develop_curve: kind %d (0 = gamma 2.2, 1 = sRGB, 2 = trunc255)", kind);
    for (int k = 1; k <= LEVELS; ++k) {
        if (kind == SESRQ_DEVELOP_TRUNC255) {
            // the smallest t with fl(t * 255) >= k: fl(t * 255) does not decrease with t
            auto reaches = [k](float t) {
                const volatile float r = t * 255.0f;
                return r >= (float)k;
            };
            float t = (float)(k / 255.0);
            while (!reaches(t)) t = nextafterf(t, 2.f);
            while (reaches(nextafterf(t, -1.f))) t = nextafterf(t, -1.f);
            T[k - 1] = t;
            continue;
        }
        // the exact preimage in 64 significant bits, rounded once to fp32 (tests/test_develop_oracle.py checks every entry in exact
        // rational arithmetic)
        const long double v = ((long double)k - 0.5L) / 255.0L;
        long double x;
        if (kind == SESRQ_DEVELOP_GAMMA22) x = powl(v, 11.0L / 5.0L);
        else x = v > 0.04045L ? powl((v + 0.055L) / 1.055L, 12.0L / 5.0L) : v / 12.92L;
        T[k - 1] = (float)x;
    }
    return 0;
}

extern "C" int sesrq_develop_create(const float gains[3], const float ccm[9], const float T[SESRQ_DEVELOP_LEVELS], sesrq_develop_ctx *out) {
    g_err[0] = 0;
    if (!out) return fail("sesrq_develop_create: ctx is NULL");
    *out = nullptr;
    if (!gains || !ccm || !T) return fail("sesrq_develop_create: gains, ccm or T is NULL");
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(gains[c]) || gains[c] < 0.f) return fail("sesrq_develop_create: gain %d must be finite and not negative", c);
    for (int j = 0; j < 9; ++j)
        if (!std::isfinite(ccm[j])) return fail("sesrq_develop_create: matrix entry %d is not finite", j);
    for (int k = 0; k < LEVELS; ++k) {
        if (!std::isfinite(T[k])) return fail("sesrq_develop_create: threshold %d is not finite", k + 1);
        if (k && T[k] < T[k - 1]) return fail("sesrq_develop_create: threshold %d is below threshold %d: the table decreases", k + 1, k);
    }
    const char *mode = getenv("SESRQ_DEVELOP_SEARCH");
    auto *c = new sesrq_develop_ctx_s();
    memcpy(c->g, gains, sizeof c->g);
    memcpy(c->m, ccm, sizeof c->m);
    Table *host = new Table();
    c->depth = build(T, mode && !strcmp(mode, "full"), *host);
    const int rc = ctx_publish("sesrq_develop_create", c, host, sizeof(Table), out);
    delete host;
    return rc;
}

extern "C" void sesrq_develop_destroy(sesrq_develop_ctx c) { ctx_destroy(c); }

extern "C" int sesrq_develop_export(sesrq_develop_ctx c, const void *pred, int pred_dtype, float scale, int zero, int order, uint8_t *out,
                                    int N, int H, int W, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_develop_export";
    if (!c) return fail("%s: ctx is NULL", who);
    if (!pred) return fail("%s: pred is NULL", who);
    if (!out) return fail("%s: out is NULL", who);
    if (pred_dtype != SESRQ_DEVELOP_F32 && pred_dtype != SESRQ_DEVELOP_I8) return fail("%s: pred_dtype %d (0 = fp32, 1 = int8)", who, pred_dtype);
    if (pred_dtype == SESRQ_DEVELOP_I8 && (!(scale > 0.f) || !std::isfinite(scale)))
        return fail("%s: an int8 prediction needs a positive, finite output scale", who);
    if (pred_dtype == SESRQ_DEVELOP_I8 && (zero < -128 || zero > 127)) return fail("%s: zero %d outside the int8 range", who, zero);
    if (pred_dtype == SESRQ_DEVELOP_F32 && (reinterpret_cast<uintptr_t>(pred) & 3)) return fail("%s: an fp32 pred is not 4-byte aligned", who);
    if (order != SESRQ_DEVELOP_ORDER_RGB && order != SESRQ_DEVELOP_ORDER_BGR) return fail("%s: order %d (0 = RGB, 1 = BGR)", who, order);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    // the 16-pixel runs must fit an int together with one round of the grid; a generous bound on the grid (1024 CUs) keeps the check
    // independent of the device
    const long long HW = (long long)H * W, segs = (HW + SEG - 1) / SEG, items = (long long)N * segs;
    if (HW > 0x7fffffffLL || items > 0x7fffffffLL - (long long)THREADS * 1024 * BLOCKS_PER_CU)
        return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);
    if (table_on_current(who, c->t)) return 1;

    Args a;
    a.pred = pred;
    a.out = out;
    a.tab = static_cast<const Table *>(c->t.ptr);
    a.HW = (int)HW;
    a.segs = (int)segs;
    a.items = (int)items;
    a.bgr = order == SESRQ_DEVELOP_ORDER_BGR;
    a.planes16 = HW % SEG == 0;
    a.depth = c->depth;
    a.scale = scale;
    a.zero = zero;
    memcpy(a.g, c->g, sizeof a.g);
    memcpy(a.m, c->m, sizeof a.m);
    const int grid = grid_cap(items, THREADS, c->t.num_cu < 1024 ? c->t.num_cu : 1024, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int k = pred_dtype == SESRQ_DEVELOP_F32 ? K_F32 : K_I8;
    if (k == K_F32) develop_export<SESRQ_DEVELOP_F32><<<grid, THREADS, 0, st>>>(a);
    else develop_export<SESRQ_DEVELOP_I8><<<grid, THREADS, 0, st>>>(a);
    return launched(who, g_count, k);
}

extern "C" int sesrq_develop_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_develop_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_develop_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_develop_last_error(void) { return g_err; }
