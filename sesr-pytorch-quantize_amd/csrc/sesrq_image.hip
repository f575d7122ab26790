// libsesrq_image.so: 8-bit images into and out of the super-resolution nets (include/sesrq_image.h).  A library of its own: it links
// nothing of libsesrq.so and registers nothing in its instance table.
//
// The reference (self_dataset_sr.py TestDataset.__getitem__) reads a uint8 image, divides by 255 in float64 and, for MFLAG 5, forms
// the luma (65.481 R + 128.553 G + 24.966 B + 16) / 255 in float64 before it casts to fp32; its integer path then quantises that
// frame into q0.  Its PNG export (sim.py) clips the fp32 output to [0, 1], scales by 255 in fp32 and truncates to uint8.
//
// Decode: a pure stream, 3 B/px read; 1 or 3 B/px of q0 and 4 or 12 B/px of fp32 written.  A lane owns a run of 16 pixels of a frame
// (pixel index y * W + x: the interleaved image and every plane are contiguous over the whole frame, so rows do not matter) and loads
// its 48 bytes as three 16-byte words; it writes 16 bytes of q0 and 64 bytes of fp32 per plane.  The RGB form is a lookup: 256 codes,
// a table of x and q0 built on the host.  The Y form is a float64 sum of three per-code products (65.481 d(v) etc., tables built on
// the host, each product rounded as the reference rounds it), one correctly rounded float64 division per pixel, the cast to fp32 and
// the input quantiser.  The tables are staged in LDS after the lane's first run has been requested, so the load and the staging
// overlap.  Runs that are partial (the last one of a frame) or not 16-byte aligned (H * W % 16 != 0, unaligned buffers) take the
// per-pixel path of the same kernel.
//
// Export: the transpose.  A lane reads 16 pixels of each of the C planes (fp32: four 16-byte words a plane; int8: one) and writes
// them interleaved as whole 16-byte words (48 bytes for C = 3, 16 for C = 1).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_image.h"
#include "sesrq_side.h"
#include "sesrq_image_decode.h"

namespace sesrq_imgk {

constexpr int THREADS = 128;
constexpr int SEG = 16;                       // pixels per lane and run
constexpr int BLOCKS_PER_CU = 16;             // 128-thread blocks: a full CU (32 waves)
constexpr int CODES = sesrq_imgdec::CODES;
enum { OUT_Q = 1, OUT_F = 2 };

using sesrq_imgdec::Tables;
using sesrq_imgdec::Y_WORDS;
using sesrq_imgdec::RGB_WORDS;
using sesrq_imgdec::Quant;
using sesrq_imgdec::quant;
using sesrq_imgdec::luma;
static_assert(Y_WORDS % THREADS == 0 && RGB_WORDS <= THREADS, "staging: whole words per thread");

struct DecodeArgs {
    const uint8_t *img;
    const Tables *tab;
    int8_t *q0;
    float *x;
    int HW, segs, items, bgr, planes16;
    Quant q;              // the input quantiser
};

struct ExportArgs {
    const void *pred;
    uint8_t *out;
    int HW, segs, items, bgr, planes16;
    float scale;
    int zero;
};

__device__ inline unsigned byte_of(const unsigned (&w)[12], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }

template <int FORM, int OUT>
__global__ __launch_bounds__(THREADS) void image_decode(DecodeArgs a) {
    constexpr int C = FORM == SESRQ_IMAGE_Y ? 1 : 3;
    constexpr int WORDS = sesrq_imgdec::table_words<FORM>();
    __shared__ uint4 s_tab[WORDS];
    const int stride = gridDim.x * THREADS;
    const size_t HW = (size_t)a.HW;
    int i = blockIdx.x * THREADS + threadIdx.x;

    // the run of item i: source, first output index, pixel count, and whether it takes the 16-byte path
    auto run = [&](int it, const uint8_t *&src, size_t &o, int &npx, bool &vec) {
        const int n = it / a.segs, p0 = (it - n * a.segs) * SEG;
        src = a.img + ((size_t)n * HW + p0) * 3;
        o = (size_t)n * C * HW + p0;
        npx = min(SEG, a.HW - p0);
        vec = npx == SEG && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (C == 1 || a.planes16) &&
              (!(OUT & OUT_Q) || (reinterpret_cast<uintptr_t>(a.q0 + o) & 15) == 0) &&
              (!(OUT & OUT_F) || (reinterpret_cast<uintptr_t>(a.x + o) & 15) == 0);
    };
    const uint8_t *src = nullptr;
    size_t o = 0;
    int npx = 0;
    bool vec = false;
    unsigned w[12];
    auto load = [&]() {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint4 v = s4[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    };
    if (i < a.items) {                                    // requested before the table is staged
        run(i, src, o, npx, vec);
        if (vec) load();
    }
    sesrq_imgdec::stage_tables<FORM, THREADS>(s_tab, a.tab);
    __syncthreads();
    const double(*ty)[CODES] = sesrq_imgdec::table_y(s_tab);
    const float *tx = sesrq_imgdec::table_x(s_tab);
    const int8_t *tq = sesrq_imgdec::table_q(s_tab);
    // byte position of R in a pixel (B sits at 2 - ir); RGB form: plane c takes byte c (RGB) or 2 - c (BGR)
    const int ir = a.bgr ? 2 : 0;

    for (; i < a.items; i += stride) {
        if (vec) {
            if (FORM == SESRQ_IMAGE_Y) {
                float f[SEG];
#pragma unroll
                for (int k = 0; k < SEG; ++k) {
                    const unsigned b0 = byte_of(w, 3 * k), b1 = byte_of(w, 3 * k + 1), b2 = byte_of(w, 3 * k + 2);
                    f[k] = luma(ty, ir ? b2 : b0, b1, ir ? b0 : b2);
                }
                if (OUT & OUT_Q) {
                    unsigned qq[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int k = 0; k < SEG; ++k) qq[k >> 2] |= (unsigned)(uint8_t)quant(f[k], a.q) << (8 * (k & 3));
                    *reinterpret_cast<uint4 *>(a.q0 + o) = make_uint4(qq[0], qq[1], qq[2], qq[3]);
                }
                if (OUT & OUT_F) {
                    float4 *d = reinterpret_cast<float4 *>(a.x + o);
#pragma unroll
                    for (int k = 0; k < SEG / 4; ++k) d[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const size_t oc = o + (size_t)(a.bgr ? 2 - c : c) * HW;     // byte c of a pixel goes to this plane
                    if (OUT & OUT_Q) {
                        unsigned qq[4] = {0, 0, 0, 0};
#pragma unroll
                        for (int k = 0; k < SEG; ++k) qq[k >> 2] |= (unsigned)(uint8_t)tq[byte_of(w, 3 * k + c)] << (8 * (k & 3));
                        *reinterpret_cast<uint4 *>(a.q0 + oc) = make_uint4(qq[0], qq[1], qq[2], qq[3]);
                    }
                    if (OUT & OUT_F) {
                        float4 *d = reinterpret_cast<float4 *>(a.x + oc);
#pragma unroll
                        for (int k = 0; k < SEG / 4; ++k)
                            d[k] = make_float4(tx[byte_of(w, 12 * k + c)], tx[byte_of(w, 12 * k + 3 + c)],
                                               tx[byte_of(w, 12 * k + 6 + c)], tx[byte_of(w, 12 * k + 9 + c)]);
                    }
                }
            }
        } else {
            for (int k = 0; k < npx; ++k) {
                const unsigned b0 = src[3 * k], b1 = src[3 * k + 1], b2 = src[3 * k + 2];
                if (FORM == SESRQ_IMAGE_Y) {
                    const float f = luma(ty, ir ? b2 : b0, b1, ir ? b0 : b2);
                    if (OUT & OUT_Q) a.q0[o + k] = quant(f, a.q);
                    if (OUT & OUT_F) a.x[o + k] = f;
                } else {
                    const unsigned v[3] = {b0, b1, b2};
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const size_t oc = o + (size_t)(a.bgr ? 2 - c : c) * HW + k;
                        if (OUT & OUT_Q) a.q0[oc] = tq[v[c]];
                        if (OUT & OUT_F) a.x[oc] = tx[v[c]];
                    }
                }
            }
        }
        const int nx = i + stride;
        if (nx < a.items) {
            run(nx, src, o, npx, vec);
            if (vec) load();
        }
    }
}

// u = trunc(fl32(clip(p, 0, 1) * 255)); an int8 prediction is first dequantised as sesrq_forward forms out_f
__device__ inline unsigned to_byte(float p) { return (unsigned)__fmul_rn(fminf(fmaxf(p, 0.f), 1.f), 255.f); }

template <int PRED, int C>
__global__ __launch_bounds__(THREADS) void image_export(ExportArgs a) {
    const size_t HW = (size_t)a.HW;
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < a.items; i += gridDim.x * THREADS) {
        const int n = i / a.segs, p0 = (i - n * a.segs) * SEG;
        const size_t in0 = (size_t)n * C * HW + p0;       // plane 0 of frame n, pixel p0
        uint8_t *dst = a.out + ((size_t)n * HW + p0) * C;
        const int npx = min(SEG, a.HW - p0);
        // output byte c of a pixel comes from plane c (RGB) or 2 - c (BGR)
        size_t pl[C];
#pragma unroll
        for (int c = 0; c < C; ++c) pl[c] = in0 + (size_t)(C == 3 && a.bgr ? 2 - c : c) * HW;
        const float *pf = static_cast<const float *>(a.pred);
        const int8_t *pq = static_cast<const int8_t *>(a.pred);
        auto val = [&](int8_t q) { return __fmul_rn((float)((int)q - a.zero), a.scale); };
        const bool vec = npx == SEG && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (C == 1 || a.planes16) &&
                         (reinterpret_cast<uintptr_t>(PRED == SESRQ_IMAGE_F32 ? (const void *)(pf + in0) : (const void *)(pq + in0)) & 15) == 0;
        if (vec) {
            unsigned u[C][SEG];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (PRED == SESRQ_IMAGE_F32) {
                    const float4 *s = reinterpret_cast<const float4 *>(pf + pl[c]);
#pragma unroll
                    for (int k = 0; k < SEG / 4; ++k) {
                        const float4 v = s[k];
                        u[c][4 * k] = to_byte(v.x); u[c][4 * k + 1] = to_byte(v.y);
                        u[c][4 * k + 2] = to_byte(v.z); u[c][4 * k + 3] = to_byte(v.w);
                    }
                } else {
                    const uint4 v = *reinterpret_cast<const uint4 *>(pq + pl[c]);
                    const unsigned ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int k = 0; k < SEG; ++k) u[c][k] = to_byte(val((int8_t)((ww[k >> 2] >> (8 * (k & 3))) & 0xffu)));
                }
            }
            unsigned o[C * SEG / 4];
#pragma unroll
            for (int j = 0; j < C * SEG / 4; ++j) o[j] = 0;
#pragma unroll
            for (int j = 0; j < C * SEG; ++j) o[j >> 2] |= u[j % C][j / C] << (8 * (j & 3));
            uint4 *d = reinterpret_cast<uint4 *>(dst);
#pragma unroll
            for (int k = 0; k < C; ++k) d[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        } else {
            for (int k = 0; k < npx; ++k) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    dst[C * k + c] = (uint8_t)to_byte(PRED == SESRQ_IMAGE_F32 ? pf[pl[c] + k] : val(pq[pl[c] + k]));
            }
        }
    }
}

}  // namespace sesrq_imgk

using namespace sesrq_imgk;

struct sesrq_image_ctx_s {
    DeviceTable t;     // Tables
    InQuant q;
};

enum { K_YQ = 0, K_YF, K_YQF, K_RQ, K_RF, K_RQF, K_EF1, K_EF3, K_EQ1, K_EQ3, K_COUNT };
static const char *const kNames[K_COUNT] = {
    "image_decode<Y,q0>", "image_decode<Y,x>", "image_decode<Y,q0,x>", "image_decode<RGB,q0>", "image_decode<RGB,x>",
    "image_decode<RGB,q0,x>", "image_export<f32,C1>", "image_export<f32,C3>", "image_export<i8,C1>", "image_export<i8,C3>"};
static Counters<K_COUNT> g_count{kNames};

using sesrq_imgdec::build;

extern "C" int sesrq_image_table(float scale_in, int zero_in, int exact_div, int8_t q[SESRQ_IMAGE_CODES], float x[SESRQ_IMAGE_CODES]) {
    g_err[0] = 0;
    if (!q || !x) return fail("sesrq_image_table: q or x is NULL");
    if (check_domain("sesrq_image_table", scale_in, zero_in, exact_div)) return 1;
    static thread_local Tables t;
    build(in_quant(scale_in, zero_in, exact_div), t);
    for (int v = 0; v < CODES; ++v) {
        q[v] = t.q[v];
        x[v] = t.x[v];
    }
    return 0;
}

extern "C" int sesrq_image_create(float scale_in, int zero_in, int exact_div, sesrq_image_ctx *out) {
    g_err[0] = 0;
    if (!out) return fail("sesrq_image_create: ctx is NULL");
    *out = nullptr;
    if (check_domain("sesrq_image_create", scale_in, zero_in, exact_div)) return 1;
    auto *c = new sesrq_image_ctx_s();
    c->q = in_quant(scale_in, zero_in, exact_div);
    Tables *host = new Tables();
    build(c->q, *host);
    const hipError_t e = table_create(c->t, host, sizeof(Tables));
    delete host;
    if (e != hipSuccess) {
        delete c;
        return fail("sesrq_image_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

extern "C" void sesrq_image_destroy(sesrq_image_ctx c) {
    if (!c) return;
    table_destroy(c->t);
    delete c;
}

// items of 16-pixel runs, checked to fit an int together with the grid stride
static int runs(const char *who, int N, int H, int W, int num_cu, int &segs, int &items) {
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    const long long HW = (long long)H * W;
    const long long sg = (HW + SEG - 1) / SEG, it = (long long)N * sg;
    if (HW > 0x7fffffffLL || it > 0x7fffffffLL - (long long)THREADS * num_cu * BLOCKS_PER_CU)
        return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);
    segs = (int)sg;
    items = (int)it;
    return 0;
}

extern "C" int sesrq_image_decode(sesrq_image_ctx c, const uint8_t *img, int form, int order, int8_t *q0, float *x, int N, int H, int W,
                                  void *stream) {
    g_err[0] = 0;
    if (!c) return fail("sesrq_image_decode: ctx is NULL");
    if (!img) return fail("sesrq_image_decode: img is NULL");
    if (!q0 && !x) return fail("sesrq_image_decode: neither q0 nor x requested");
    if (form != SESRQ_IMAGE_Y && form != SESRQ_IMAGE_RGB) return fail("sesrq_image_decode: form %d (0 = Y, 1 = RGB)", form);
    if (order != SESRQ_IMAGE_ORDER_RGB && order != SESRQ_IMAGE_ORDER_BGR) return fail("sesrq_image_decode: order %d (0 = RGB, 1 = BGR)", order);
    int segs, items;
    if (runs("sesrq_image_decode", N, H, W, c->t.num_cu, segs, items)) return 1;
    if (table_on_current("sesrq_image_decode", c->t)) return 1;

    DecodeArgs a;
    a.img = img;
    a.tab = static_cast<const Tables *>(c->t.ptr);
    a.q0 = q0;
    a.x = x;
    a.HW = H * W;
    a.segs = segs;
    a.items = items;
    a.bgr = order == SESRQ_IMAGE_ORDER_BGR;
    a.planes16 = a.HW % SEG == 0;
    a.q = sesrq_imgdec::quant_of(c->q);
    const int grid = grid_cap(items, THREADS, c->t.num_cu, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int out = (q0 ? OUT_Q : 0) | (x ? OUT_F : 0);
    int k;
#define SESRQ_IMAGE_DECODE(F, O, K)                                \
    if (form == F && out == (O)) {                                 \
        k = K;                                                     \
        image_decode<F, O><<<grid, THREADS, 0, st>>>(a);           \
    }
    SESRQ_IMAGE_DECODE(SESRQ_IMAGE_Y, OUT_Q, K_YQ)
    else SESRQ_IMAGE_DECODE(SESRQ_IMAGE_Y, OUT_F, K_YF)
    else SESRQ_IMAGE_DECODE(SESRQ_IMAGE_Y, OUT_Q | OUT_F, K_YQF)
    else SESRQ_IMAGE_DECODE(SESRQ_IMAGE_RGB, OUT_Q, K_RQ)
    else SESRQ_IMAGE_DECODE(SESRQ_IMAGE_RGB, OUT_F, K_RF)
    else SESRQ_IMAGE_DECODE(SESRQ_IMAGE_RGB, OUT_Q | OUT_F, K_RQF)
    else return fail("sesrq_image_decode: unreachable output set %d", out);
#undef SESRQ_IMAGE_DECODE
    return launched("sesrq_image_decode", g_count, k);
}

extern "C" int sesrq_image_export(const void *pred, int pred_dtype, float scale, int zero, int C, int order, uint8_t *out, int N, int H,
                                  int W, void *stream) {
    g_err[0] = 0;
    if (!pred) return fail("sesrq_image_export: pred is NULL");
    if (!out) return fail("sesrq_image_export: out is NULL");
    if (pred_dtype != SESRQ_IMAGE_F32 && pred_dtype != SESRQ_IMAGE_I8)
        return fail("sesrq_image_export: pred_dtype %d (0 = fp32, 1 = int8)", pred_dtype);
    if (pred_dtype == SESRQ_IMAGE_I8 && (!(scale > 0.f) || !std::isfinite(scale)))
        return fail("sesrq_image_export: an int8 prediction needs a positive, finite output scale");
    if (pred_dtype == SESRQ_IMAGE_I8 && (zero < -128 || zero > 127)) return fail("sesrq_image_export: zero %d outside the int8 range", zero);
    if (C != 1 && C != 3) return fail("sesrq_image_export: %d channels (1 or 3)", C);
    if (order != SESRQ_IMAGE_ORDER_RGB && order != SESRQ_IMAGE_ORDER_BGR) return fail("sesrq_image_export: order %d (0 = RGB, 1 = BGR)", order);
    int dev = -1, num_cu = 0;
    // the size check needs the grid cap; a generous bound (1024 CUs) keeps it before any HIP call
    int segs, items;
    if (runs("sesrq_image_export", N, H, W, 1024, segs, items)) return 1;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return fail("sesrq_image_export: no current device");
    if (num_cu > 1024) num_cu = 1024;

    ExportArgs a;
    a.pred = pred;
    a.out = out;
    a.HW = H * W;
    a.segs = segs;
    a.items = items;
    a.bgr = order == SESRQ_IMAGE_ORDER_BGR;
    a.planes16 = a.HW % SEG == 0;
    a.scale = scale;
    a.zero = zero;
    const int grid = grid_cap(items, THREADS, num_cu, BLOCKS_PER_CU);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int k;
    if (pred_dtype == SESRQ_IMAGE_F32) {
        k = C == 1 ? K_EF1 : K_EF3;
        if (C == 1) image_export<SESRQ_IMAGE_F32, 1><<<grid, THREADS, 0, st>>>(a);
        else image_export<SESRQ_IMAGE_F32, 3><<<grid, THREADS, 0, st>>>(a);
    } else {
        k = C == 1 ? K_EQ1 : K_EQ3;
        if (C == 1) image_export<SESRQ_IMAGE_I8, 1><<<grid, THREADS, 0, st>>>(a);
        else image_export<SESRQ_IMAGE_I8, 3><<<grid, THREADS, 0, st>>>(a);
    }
    return launched("sesrq_image_export", g_count, k);
}

extern "C" int sesrq_image_instance_count(void) { return g_count.count(); }

extern "C" const char *sesrq_image_instance_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_image_instance_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_image_last_error(void) { return g_err; }
