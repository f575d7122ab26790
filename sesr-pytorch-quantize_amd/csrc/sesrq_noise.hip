// libsesrq_noise.so: shot and read noise on Bayer raw frames, fused into their unpack (include/sesrq_noise.h, which states the
// arithmetic): the reference's TEST_RAW_ADD_NOISE.  A library of its own: it links nothing of the other libraries and registers
// nothing in their instance tables.
//
// The stream is the Bayer unpack's (sesrq_bayer_unpack.h: a persistent grid-stride loop over row segments, 8 pixels of a U16 row, 16
// of a packed one, decoded with its load_wide / load_px), but the body is another: with noise q0 is no longer a map of the code, so
// there is no LDS table.  Per pixel one Philox4x32-10 call whose four words stay in registers, a Box-Muller pair and a half (two
// logf, one sincospif, one cospif, two sqrtf), then per channel the reference's multiply, add, sqrtf, multiply, add, the clamp and the
// forward's input quantiser (a division, an add, a round).  About 40 32-bit multiplies and a dozen transcendental or division
// sequences per pixel against 5 B/px (17 with the fp32 frame): the kernel is bound by vector instruction issue, not by memory, so the
// wide loads and stores matter less than in the plain unpack; they are kept because they are free.  A lane computes its whole segment
// into registers and then stores it, 8 / 16 bytes of q0 and 16 bytes of fp32 at a time or per pixel, from the same registers: the two
// store paths cannot differ.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_bayer_unpack.h"
#include "sesrq_noise.h"
#include "sesrq_side.h"

namespace sesrq_noisek {

using namespace sesrq_bayer;
static_assert(PACK_U16 == SESRQ_PACK_U16 && PACK_RAW10 == SESRQ_PACK_RAW10 && PACK_RAW12 == SESRQ_PACK_RAW12, "the body's packings are the header's");

constexpr int Z_BLOCKS = 2048;                // grid cap of the deviates kernel

struct NoiseArgs {
    const uint8_t *raw;
    int8_t *q0;
    float *spread;
    const float *levels;   // device, N (shot, read) pairs, or nullptr: shot / read below
    size_t stride;         // bytes between rows
    int H, W, segs, items;
    int black, white;
    float range;           // fl32(white - black), exact
    int sites;             // 2 bits per parity (py * 2 + px): its site channel
    float shot, read;
    float s0, r0, z0;      // the input domain: scale, fl(1 / scale), fl32(zero)
    int recip;             // exact_div 2: spread * r0 instead of spread / s0
    uint32_t key0, key1;   // lo32, hi32 of the seed
    uint64_t frame0;
    int in_vec, out_vec;
};

// Philox4x32-10 of Random123: counter c, key (k0, k1)
__device__ __forceinline__ void philox(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0], hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += W0;
        k1 += W1;
    }
}

// z[0 .. 2] of pixel (y, x) of frame f: the one device function behind both kernels
__device__ __forceinline__ void deviates(uint32_t x, uint32_t y, uint64_t f, uint32_t k0, uint32_t k1, float (&z)[3]) {
    uint32_t w[4] = {x, y, (uint32_t)f, (uint32_t)(f >> 32)};
    philox(w, k0, k1);
    const float ua = ((float)(w[0] >> 9) + 0.5f) * 0x1p-23f, ub = ((float)(w[2] >> 9) + 0.5f) * 0x1p-23f;      // exact
    const float ta = (float)(w[1] >> 8) * 0x1p-23f, tb = (float)(w[3] >> 8) * 0x1p-23f;                        // 2 u_t, exact
    const float ra = sqrtf(-2.0f * logf(ua)), rb = sqrtf(-2.0f * logf(ub));
    float sa, ca;
    sincospif(ta, &sa, &ca);
    z[0] = ra * ca;
    z[1] = ra * sa;
    z[2] = rb * cospif(tb);
}

__global__ __launch_bounds__(THREADS) void noise_deviates(float *z, int H, int W, size_t items, uint32_t k0, uint32_t k1, uint64_t frame0) {
    const size_t plane = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < items; i += (size_t)gridDim.x * THREADS) {
        const size_t n = i / plane, p = i - n * plane;
        const uint32_t y = (uint32_t)(p / W), x = (uint32_t)(p - (size_t)y * W);
        float v[3];
        deviates(x, y, frame0 + n, k0, k1, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) z[(n * 3 + c) * plane + p] = v[c];
    }
}

template <int OUT, int PACK>
__global__ __launch_bounds__(THREADS) void noise_unpack(NoiseArgs a) {
    constexpr int SEG = seg_px<PACK>();
    const int H = a.H, W = a.W;
    const unsigned black = (unsigned)a.black, white = (unsigned)a.white;
    const size_t plane = (size_t)H * W;
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < a.items; i += gridDim.x * THREADS) {
        const int row = i / a.segs, seg = i - row * a.segs;
        const int n = row / H, y = row - n * H, x0 = seg * SEG;
        const int npx = min(SEG, W - x0);
        const int ph = a.sites >> (4 * (y & 1));
        const int ce = ph & 3, co = (ph >> 2) & 3;      // site channel of the even / the odd columns of this row
        const uint8_t *rowp = a.raw + (size_t)row * a.stride;
        const size_t base = ((size_t)n * 3 * H + y) * W + x0;  // plane (n, c, y) starts at base + c * plane
        const float shot = a.levels ? a.levels[2 * n] : a.shot, read = a.levels ? a.levels[2 * n + 1] : a.read;
        const uint64_t f = a.frame0 + (uint64_t)n;

        unsigned d[SEG];
        if (a.in_vec && npx == SEG) {
            load_wide<PACK>(rowp + (size_t)seg * seg_bytes<PACK>(), d);
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k) d[k] = k >= npx ? 0u : load_px<PACK>(rowp, x0 + k);
        }

        float fs[3][SEG];            // the noisy fp32 frame of this segment, per channel
        unsigned qs[3][SEG / 4];     // its q0, four pixels a word
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < SEG / 4; ++j) qs[c][j] = 0u;
#pragma unroll
        for (int k = 0; k < SEG; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) fs[c][k] = 0.f;
            if (k < npx) {
                const int cs = (k & 1) ? co : ce;
                const float xs = __fdiv_rn((float)(min(max(d[k], black), white) - black), a.range);
                float z[3];
                deviates((uint32_t)(x0 + k), (uint32_t)y, f, a.key0, a.key1, z);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float xc = c == cs ? xs : 0.f;
                    const float v = xc * shot + read;          // -ffp-contract=off: a multiply, then an add
                    const float s = sqrtf(v);
                    const float yv = xc + s * z[c];
                    const float sp = fminf(fmaxf(yv, 0.f), 1.f);
                    fs[c][k] = sp;
                    if (OUT & OUT_Q) {
                        const float t = a.recip ? sp * a.r0 : __fdiv_rn(sp, a.s0);
                        const float q = fminf(fmaxf(rintf(t + a.z0), -128.f), 127.f);
                        qs[c][k >> 2] |= ((unsigned)(int)q & 0xffu) << (8 * (k & 3));
                    }
                }
            }
        }

        if (a.out_vec) {             // W % SEG == 0: every segment is whole
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (OUT & OUT_Q) {
                    if constexpr (SEG == 16)
                        *reinterpret_cast<uint4 *>(a.q0 + base + c * plane) = make_uint4(qs[c][0], qs[c][1], qs[c][2], qs[c][3]);
                    else
                        *reinterpret_cast<uint2 *>(a.q0 + base + c * plane) = make_uint2(qs[c][0], qs[c][1]);
                }
                if (OUT & OUT_F) {
                    float4 *dst = reinterpret_cast<float4 *>(a.spread + base + c * plane);
#pragma unroll
                    for (int j = 0; j < SEG / 4; ++j) dst[j] = make_float4(fs[c][4 * j], fs[c][4 * j + 1], fs[c][4 * j + 2], fs[c][4 * j + 3]);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k) {
                if (k < npx) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (OUT & OUT_Q) a.q0[base + c * plane + k] = (int8_t)(qs[c][k >> 2] >> (8 * (k & 3)));
                        if (OUT & OUT_F) a.spread[base + c * plane + k] = fs[c][k];
                    }
                }
            }
        }
    }
}

}  // namespace sesrq_noisek

using namespace sesrq_noisek;

struct sesrq_noise_ctx_s {
    DeviceTable t;     // the device and its compute units; no device memory
    sesrq_sensor_format fmt;
    InQuant q;
};

// one instantiation per (packing, output set), and the deviates kernel
enum { K_DEVIATES = 9, K_COUNT = 10 };
static const char *const kNames[K_COUNT] = {
    "noise_unpack<u16,q0>",   "noise_unpack<u16,spread>",   "noise_unpack<u16,q0+spread>",
    "noise_unpack<raw10,q0>", "noise_unpack<raw10,spread>", "noise_unpack<raw10,q0+spread>",
    "noise_unpack<raw12,q0>", "noise_unpack<raw12,spread>", "noise_unpack<raw12,q0+spread>",
    "noise_deviates"};
static Counters<K_COUNT> g_count{kNames};

static const sesrq_sensor_format kReference = {SESRQ_CFA_RGGB, 0, 4095, SESRQ_PACK_U16};

static int check_format(const char *who, const sesrq_sensor_format *f) {
    if (f->cfa < SESRQ_CFA_RGGB || f->cfa > SESRQ_CFA_BGGR) return fail("%s: cfa %d is not a Bayer order (0 .. 3)", who, f->cfa);
    if (f->packing < SESRQ_PACK_U16 || f->packing > SESRQ_PACK_RAW12) return fail("%s: packing %d (0 u16, 1 raw10, 2 raw12)", who, f->packing);
    if (f->black < 0 || f->black >= f->white || f->white > 65535)
        return fail("%s: levels need 0 <= black < white <= 65535, got black %d, white %d", who, f->black, f->white);
    const int top = f->packing == SESRQ_PACK_RAW10 ? 1023 : f->packing == SESRQ_PACK_RAW12 ? 4095 : 65535;
    if (f->white > top) return fail("%s: white %d is above the packing's range (%d)", who, f->white, top);
    return 0;
}

static size_t row_bytes(const char *who, const sesrq_sensor_format *f, int W) {
    const int group = f->packing == SESRQ_PACK_RAW10 ? 4 : f->packing == SESRQ_PACK_RAW12 ? 2 : 1;
    if (W % group) return fail("%s: W = %d is not a multiple of the %d pixels of a pack group", who, W, group), 0;
    return f->packing == SESRQ_PACK_RAW10 ? (size_t)W / 4 * 5 : f->packing == SESRQ_PACK_RAW12 ? (size_t)W / 2 * 3 : (size_t)W * 2;
}

extern "C" int sesrq_noise_create(const sesrq_sensor_format *fmt, float scale_in, int zero_in, int exact_div, sesrq_noise_ctx *out) {
    g_err[0] = 0;
    if (!out) return fail("sesrq_noise_create: ctx is NULL");
    *out = nullptr;
    if (!fmt) fmt = &kReference;
    if (check_format("sesrq_noise_create", fmt)) return 1;
    if (check_domain("sesrq_noise_create", scale_in, zero_in, exact_div)) return 1;
    auto *c = new sesrq_noise_ctx_s();
    c->fmt = *fmt;
    c->q = in_quant(scale_in, zero_in, exact_div);
    hipError_t e = hipGetDevice(&c->t.device);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&c->t.num_cu, hipDeviceAttributeMultiprocessorCount, c->t.device);
    if (e != hipSuccess) {
        delete c;
        return fail("sesrq_noise_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

extern "C" void sesrq_noise_destroy(sesrq_noise_ctx c) { ctx_destroy(c); }

static int check_level(const char *who, const char *name, float v) {
    if (!(v >= 0.f) || !std::isfinite(v)) return fail("%s: %s noise level %g must be finite and not negative", who, name, (double)v);
    return 0;
}

template <int PACK>
static void launch(int outs, int grid, hipStream_t st, const NoiseArgs &a) {
    if (outs == (OUT_Q | OUT_F))
        noise_unpack<OUT_Q | OUT_F, PACK><<<grid, THREADS, 0, st>>>(a);
    else if (outs == OUT_Q)
        noise_unpack<OUT_Q, PACK><<<grid, THREADS, 0, st>>>(a);
    else
        noise_unpack<OUT_F, PACK><<<grid, THREADS, 0, st>>>(a);
}

extern "C" int sesrq_noise_unpack(sesrq_noise_ctx c, const void *raw, size_t row_stride_bytes, int8_t *q0, float *spread, int N, int H,
                                  int W, float shot, float read, const float *levels, uint64_t seed, uint64_t frame0, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_noise_unpack";
    if (check_unpack(who, c, raw, q0, spread, N, H, W)) return 1;
    if (!levels && (check_level(who, "shot", shot) || check_level(who, "read", read))) return 1;
    if (reinterpret_cast<uintptr_t>(levels) % 4) return fail("%s: levels is not 4-byte aligned", who);
    const size_t need = row_bytes(who, &c->fmt, W);
    if (!need) return 1;
    if (row_stride_bytes < need)
        return fail("%s: row_stride_bytes %zu is less than the %zu bytes of a row of %d pixels", who, row_stride_bytes, need, W);
    if (reinterpret_cast<uintptr_t>(spread) % 4) return fail("%s: spread is not 4-byte aligned", who);
    const int pack = c->fmt.packing;
    const int SEG = pack == SESRQ_PACK_U16 ? seg_px<PACK_U16>() : seg_px<PACK_RAW10>();
    static_assert(seg_px<PACK_RAW10>() == seg_px<PACK_RAW12>(), "one segment length for the packed formats");
    NoiseArgs a;
    if (segment_items(who, N, H, W, SEG, (long long)THREADS * c->t.num_cu * BLOCKS_PER_CU, &a.segs, &a.items)) return 1;
    if (table_on_current(who, c->t)) return 1;

    const uintptr_t in_align = pack == SESRQ_PACK_U16 ? 16 : 4;
    a.raw = static_cast<const uint8_t *>(raw);
    a.q0 = q0;
    a.spread = spread;
    a.levels = levels;
    a.stride = row_stride_bytes;
    a.H = H;
    a.W = W;
    a.black = c->fmt.black;
    a.white = c->fmt.white;
    a.range = (float)(c->fmt.white - c->fmt.black);
    a.sites = SITES[c->fmt.cfa];
    a.shot = shot;
    a.read = read;
    a.s0 = c->q.s0;
    a.r0 = c->q.r0;
    a.z0 = c->q.z0;
    a.recip = c->q.recip;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    a.frame0 = frame0;
    a.in_vec = reinterpret_cast<uintptr_t>(raw) % in_align == 0 && row_stride_bytes % in_align == 0;
    a.out_vec = W % SEG == 0 && reinterpret_cast<uintptr_t>(q0) % SEG == 0 && reinterpret_cast<uintptr_t>(spread) % 16 == 0;
    const int grid = grid_cap(a.items, THREADS, c->t.num_cu, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int outs = (q0 ? OUT_Q : 0) | (spread ? OUT_F : 0);
    if (pack == SESRQ_PACK_RAW10)
        launch<PACK_RAW10>(outs, grid, st, a);
    else if (pack == SESRQ_PACK_RAW12)
        launch<PACK_RAW12>(outs, grid, st, a);
    else
        launch<PACK_U16>(outs, grid, st, a);
    return launched(who, g_count, pack * 3 + outs - 1);
}

extern "C" int sesrq_noise_deviates(float *z, int N, int H, int W, uint64_t seed, uint64_t frame0, void *stream) {
    g_err[0] = 0;
    const char *who = "sesrq_noise_deviates";
    if (!z) return fail("%s: z is NULL", who);
    if (reinterpret_cast<uintptr_t>(z) % 4) return fail("%s: z is not 4-byte aligned", who);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    const long long rows = (long long)N * H, items = rows <= 0x7fffffffLL ? rows * W : -1;
    if (items < 0 || items > 0x7fffffffLL) return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);
    const long long want = (items + THREADS - 1) / THREADS;
    noise_deviates<<<(int)(want < Z_BLOCKS ? want : Z_BLOCKS), THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        z, H, W, (size_t)items, (uint32_t)seed, (uint32_t)(seed >> 32), frame0);
    return launched(who, g_count, K_DEVIATES);
}

extern "C" int sesrq_noise_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_noise_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_noise_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_noise_last_error(void) { return g_err; }
