// libsesrq_raw.so: 12-bit RGGB Bayer raw frames into the 3-channel nets (include/sesrq_raw.h).  A library of its own: it links nothing
// of libsesrq.so and registers nothing in its instance table.
//
// The reference (self_dataset.py TestDataset.__getitem__) spreads a uint16 raw frame into a sparse 3-channel RGGB mosaic, divides by
// 4095 in fp32 and clamps to [0, 1]; its integer path then quantises that frame into q0.  Both steps are a function of the 12-bit code
// and the Bayer phase only, so q0 is one lookup in a 4096-entry table built on the host (the exact arithmetic of sesrq_forward's input
// quantiser, -ffp-contract=off), and the fp32 frame is one correctly rounded division per pixel.
//
// Kernel: a pure stream, 2 B/px read and 3 B/px written (+ 12 B/px for the fp32 frame).  Persistent grid-stride loop over row segments
// of 8 pixels; the table is staged in LDS once per workgroup.  A lane loads its segment with one 16-byte load, clamps each code to
// 4095, gathers 8 table bytes from LDS and writes 8 bytes of q0 (and 32 bytes of fp32) per plane.  Rows whose start is not 16-byte
// aligned (W % 8 != 0, or unaligned buffers) take the per-pixel path of the same kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_raw.h"
#include "sesrq_side.h"

namespace sesrq_rawk {

constexpr int THREADS = 256;
constexpr int SEG = 8;                        // pixels per lane and segment
constexpr int CODE_MAX = SESRQ_RAW_CODES - 1;
constexpr int BLOCKS_PER_CU = 8;              // 256-thread blocks: a full CU (32 waves)
enum { OUT_Q = 1, OUT_F = 2 };
static_assert(SESRQ_RAW_CODES == THREADS * 16, "one 16-byte load per thread stages the table");

struct UnpackArgs {
    const uint16_t *raw;
    const int8_t *table;   // device, SESRQ_RAW_CODES bytes
    int8_t *q0;
    float *spread;
    int H, W, segs, items, vec;
};

// x(v) for v <= 4095: the reference's fl32(v) / (2^12 - 1), already inside [0, 1]
__device__ inline float level(unsigned v) { return __fdiv_rn((float)v, (float)CODE_MAX); }

template <int OUT>
__global__ __launch_bounds__(THREADS) void raw_unpack(UnpackArgs a) {
    __shared__ uint4 s_tab4[THREADS];
    s_tab4[threadIdx.x] = reinterpret_cast<const uint4 *>(a.table)[threadIdx.x];
    __syncthreads();
    const int8_t *tab = reinterpret_cast<const int8_t *>(s_tab4);
    const int8_t t0 = tab[0];
    const unsigned z4 = (unsigned)(uint8_t)t0 * 0x01010101u;
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W;
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < a.items; i += gridDim.x * THREADS) {
        const int row = i / a.segs, seg = i - row * a.segs;
        const int n = row / H, y = row - n * H, x0 = seg * SEG;
        const int py = y & 1;
        // plane (n, c, y) starts at base + c * plane; site channel of an even column: R (py 0) / G (py 1), odd column: G / B
        const size_t base = ((size_t)n * 3 * H + y) * W;
        const int ce = py, co = py + 1;
        if (a.vec) {
            const uint4 w = *reinterpret_cast<const uint4 *>(a.raw + (size_t)row * W + x0);
            const unsigned ww[4] = {w.x, w.y, w.z, w.w};
            unsigned v[SEG];
#pragma unroll
            for (int k = 0; k < SEG; ++k) v[k] = min((ww[k >> 1] >> (16 * (k & 1))) & 0xffffu, (unsigned)CODE_MAX);
            if (OUT & OUT_Q) {
                // E: the even columns' codes, O: the odd columns', q0(0) elsewhere
                unsigned e[2] = {z4, z4}, o[2] = {z4, z4};
#pragma unroll
                for (int k = 0; k < SEG; ++k) {
                    const unsigned b = (unsigned)(uint8_t)tab[v[k]];
                    const int sh = 8 * (k & 3);
                    unsigned &d = (k & 1) ? o[k >> 2] : e[k >> 2];
                    d = (d & ~(0xffu << sh)) | (b << sh);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint2 val = c == ce ? make_uint2(e[0], e[1]) : c == co ? make_uint2(o[0], o[1]) : make_uint2(z4, z4);
                    *reinterpret_cast<uint2 *>(a.q0 + base + c * plane + x0) = val;
                }
            }
            if (OUT & OUT_F) {
                float f[SEG];
#pragma unroll
                for (int k = 0; k < SEG; ++k) f[k] = level(v[k]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float4 lo, hi;
                    if (c == ce) {
                        lo = make_float4(f[0], 0.f, f[2], 0.f); hi = make_float4(f[4], 0.f, f[6], 0.f);
                    } else if (c == co) {
                        lo = make_float4(0.f, f[1], 0.f, f[3]); hi = make_float4(0.f, f[5], 0.f, f[7]);
                    } else {
                        lo = hi = make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                    float4 *d = reinterpret_cast<float4 *>(a.spread + base + c * plane + x0);
                    d[0] = lo;
                    d[1] = hi;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k) {
                const int x = x0 + k;
                if (x >= W) break;
                const unsigned v = min((unsigned)a.raw[(size_t)row * W + x], (unsigned)CODE_MAX);
                const int cs = (k & 1) ? co : ce;
                if (OUT & OUT_Q) {
                    const int8_t q = tab[v];
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.q0[base + c * plane + x] = c == cs ? q : t0;
                }
                if (OUT & OUT_F) {
                    const float f = level(v);
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.spread[base + c * plane + x] = c == cs ? f : 0.f;
                }
            }
        }
    }
}

}  // namespace sesrq_rawk

using namespace sesrq_rawk;

struct sesrq_raw_ctx_s {
    DeviceTable t;     // SESRQ_RAW_CODES bytes of q0
};

enum { K_Q = 0, K_F, K_QF, K_COUNT };
static const char *const kNames[K_COUNT] = {"raw_unpack<q0>", "raw_unpack<spread>", "raw_unpack<q0,spread>"};
static Counters<K_COUNT> g_count{kNames};

extern "C" int sesrq_raw_table(float scale_in, int zero_in, int exact_div, int8_t table[SESRQ_RAW_CODES]) {
    g_err[0] = 0;
    if (!table) return fail("sesrq_raw_table: table is NULL");
    if (check_domain("sesrq_raw_table", scale_in, zero_in, exact_div)) return 1;
    const InQuant d = in_quant(scale_in, zero_in, exact_div);
    for (int v = 0; v < SESRQ_RAW_CODES; ++v) {
        float x = (float)v / (float)CODE_MAX;                // true IEEE quotient, as torch's CPU tensor / scalar
        x = fminf(fmaxf(x, 0.f), 1.f);
        table[v] = host_quant(x, d);
    }
    return 0;
}

extern "C" int sesrq_raw_create(float scale_in, int zero_in, int exact_div, sesrq_raw_ctx *out) {
    g_err[0] = 0;
    if (!out) return fail("sesrq_raw_create: ctx is NULL");
    *out = nullptr;
    int8_t host[SESRQ_RAW_CODES];
    if (sesrq_raw_table(scale_in, zero_in, exact_div, host)) return 1;
    auto *c = new sesrq_raw_ctx_s();
    const hipError_t e = table_create(c->t, host, SESRQ_RAW_CODES);
    if (e != hipSuccess) {
        delete c;
        return fail("sesrq_raw_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

extern "C" void sesrq_raw_destroy(sesrq_raw_ctx c) {
    if (!c) return;
    table_destroy(c->t);
    delete c;
}

extern "C" int sesrq_raw_unpack(sesrq_raw_ctx c, const uint16_t *raw, int8_t *q0, float *spread, int N, int H, int W, void *stream) {
    g_err[0] = 0;
    if (!c) return fail("sesrq_raw_unpack: ctx is NULL");
    if (!raw) return fail("sesrq_raw_unpack: raw is NULL");
    if (!q0 && !spread) return fail("sesrq_raw_unpack: neither q0 nor spread requested");
    if (N < 1 || H < 1 || W < 1) return fail("sesrq_raw_unpack: empty frame (N = %d, H = %d, W = %d)", N, H, W);
    const long long segs = (W + SEG - 1) / SEG, items = (long long)N * H * segs;
    if (items > 0x7fffffffLL - (long long)THREADS * c->t.num_cu * BLOCKS_PER_CU)
        return fail("sesrq_raw_unpack: frame of %d x %d x %d is too large", N, H, W);
    if (table_on_current("sesrq_raw_unpack", c->t)) return 1;

    UnpackArgs a;
    a.raw = raw;
    a.table = static_cast<const int8_t *>(c->t.ptr);
    a.q0 = q0;
    a.spread = spread;
    a.H = H;
    a.W = W;
    a.segs = (int)segs;
    a.items = (int)items;
    a.vec = W % SEG == 0 && reinterpret_cast<uintptr_t>(raw) % 16 == 0 && reinterpret_cast<uintptr_t>(q0) % 8 == 0 &&
            reinterpret_cast<uintptr_t>(spread) % 16 == 0;
    const int grid = grid_cap(items, THREADS, c->t.num_cu, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int k;
    if (q0 && spread) {
        k = K_QF;
        raw_unpack<OUT_Q | OUT_F><<<grid, THREADS, 0, st>>>(a);
    } else if (q0) {
        k = K_Q;
        raw_unpack<OUT_Q><<<grid, THREADS, 0, st>>>(a);
    } else {
        k = K_F;
        raw_unpack<OUT_F><<<grid, THREADS, 0, st>>>(a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("sesrq_raw_unpack: kernel launch: %s", hipGetErrorString(e));
    ++g_count.launches[k];
    return 0;
}

extern "C" int sesrq_raw_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_raw_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_raw_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_raw_last_error(void) { return g_err; }
