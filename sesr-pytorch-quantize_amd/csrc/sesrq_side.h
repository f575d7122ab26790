// Host scaffold of the side libraries (libsesrq_eval.so, libsesrq_raw.so, libsesrq_image.so): the error buffer, the launch counters
// behind their exported instance lists and the end of an entry that launched one of them, the input-domain check and host q0
// quantiser, and a context that keeps one host table on a device.  For the two Bayer unpack libraries (raw, sensor; their device
// body is sesrq_bayer_unpack.h) also the q0 table of a level count, the shared argument checks of their unpack entries and a
// context's publish / destroy; for the colour and the video export (their chroma upscale is sesrq_chroma_upscale.h) the check of
// the luma arguments and the frame size.
// Each library stays a library of its own; only this host code is shared.  Everything here has internal
// linkage (static, or the anonymous namespace), so a library exports exactly what its own header declares.  No device code.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

static thread_local char g_err[512];

static int fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return 1;
}

namespace {

// A library's fixed list of kernel instantiations: its exported *_count / *_name / *_launches forward here.
template <int N>
struct Counters {
    const char *const (&names)[N];
    std::atomic<long long> launches[N];
    int count() const { return N; }
    const char *name(int i) const { return i >= 0 && i < N ? names[i] : nullptr; }
    long long get(int i) const { return i >= 0 && i < N ? launches[i].load() : -1; }
};

// The input quantiser of sesrq_forward on the host: clamp8(rint(x / s0 + z0)); exact_div 2 forms x * fl(1 / s0) instead.
struct InQuant {
    float s0, r0, z0;
    int recip;
};

// A context's host table on the device that was current at create; launches are checked against that device.
struct DeviceTable {
    void *ptr = nullptr;
    int device = -1;
    int num_cu = 0;
};

}  // namespace

[[maybe_unused]] static int check_domain(const char *who, float scale_in, int zero_in, int exact_div) {
    if (!(scale_in > 0.f) || !std::isfinite(scale_in)) return fail("%s: scale_in must be positive and finite", who);
    if (zero_in < -(1 << 24) || zero_in > (1 << 24)) return fail("%s: zero_in %d is not exact in fp32", who, zero_in);
    if (exact_div < 0 || exact_div > 2) return fail("%s: exact_div %d (0, 1 or 2)", who, exact_div);
    return 0;
}

[[maybe_unused]] static InQuant in_quant(float scale_in, int zero_in, int exact_div) {
    const volatile float r = 1.0f / scale_in;             // exact_div 2: fl(1 / s0), formed once
    return {scale_in, r, (float)zero_in, exact_div == 2};
}

[[maybe_unused]] static int8_t host_quant(float x, const InQuant &d) {
    const float t = d.recip ? x * d.r0 : x / d.s0;         // true IEEE quotient, as torch's CPU tensor / scalar
    const float q = rintf(t + d.z0);                      // round half to even, as torch.round
    return (int8_t)fminf(fmaxf(q, -128.f), 127.f);
}

// q0 of every level d = 0 .. D of a raw format with D + 1 levels: x = clamp(fl32(d) / fl32(D), 0, 1), quantised as the net's input.
[[maybe_unused]] static void level_table(int D, const InQuant &q, int8_t *table) {
    for (int d = 0; d <= D; ++d) {
        float x = (float)d / (float)D;                       // true IEEE quotient, as torch's CPU tensor / scalar
        x = fminf(fmaxf(x, 0.f), 1.f);
        table[d] = host_quant(x, q);
    }
}

// What every Bayer unpack entry refuses first.
[[maybe_unused]] static int check_unpack(const char *who, const void *ctx, const void *raw, const void *q0, const void *spread, int N, int H,
                                         int W) {
    if (!ctx) return fail("%s: ctx is NULL", who);
    if (!raw) return fail("%s: raw is NULL", who);
    if (!q0 && !spread) return fail("%s: neither q0 nor spread requested", who);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    return 0;
}

// The N H ceil(W / seg) items of a grid-stride launch over row segments, which must fit an int together with one grid round.
[[maybe_unused]] static int segment_items(const char *who, int N, int H, int W, int seg, long long round, int *segs, int *items) {
    const long long s = (W + seg - 1) / seg, n = (long long)N * H * s;
    if (n > 0x7fffffffLL - round) return fail("%s: frame of %d x %d x %d is too large", who, N, H, W);
    *segs = (int)s;
    *items = (int)n;
    return 0;
}

// What the colour and the video export refuse of the net's luma (y_dtype: LUMA_F32 or LUMA_I8 with its output domain), of r and
// of the LR frame; then the tiles of out_w x out_h output pixels that cover the r H x r W frame, N frames of which must fit a grid.
enum { LUMA_F32 = 0, LUMA_I8 = 1 };
[[maybe_unused]] static int check_luma_export(const char *who, const void *y, int y_dtype, float scale, int zero, int r, int N, int H, int W,
                                              int out_w, int out_h, int *tiles_x, int *tiles_y) {
    if (!y) return fail("%s: y is NULL", who);
    if (y_dtype != LUMA_F32 && y_dtype != LUMA_I8) return fail("%s: y_dtype %d (0 = fp32, 1 = int8)", who, y_dtype);
    if (y_dtype == LUMA_I8 && (!(scale > 0.f) || !std::isfinite(scale)))
        return fail("%s: an int8 luma needs a positive, finite output scale", who);
    if (y_dtype == LUMA_I8 && (zero < -128 || zero > 127)) return fail("%s: zero %d outside the int8 range", who, zero);
    if (y_dtype == LUMA_F32 && (reinterpret_cast<uintptr_t>(y) & 3)) return fail("%s: an fp32 y is not 4-byte aligned", who);
    if (r != 2 && r != 4) return fail("%s: r = %d (2 or 4)", who, r);
    if (N < 1 || H < 1 || W < 1) return fail("%s: empty frame (N = %d, H = %d, W = %d)", who, N, H, W);
    const long long rW = (long long)r * W, rH = (long long)r * H, tx = (rW + out_w - 1) / out_w, ty = (rH + out_h - 1) / out_h;
    if (rH > 0x7fffffffLL || rW > 0x7fffffffLL || (long long)N * tx * ty > 0x7fffffffLL)
        return fail("%s: frame of %d x %d x %d at r = %d is too large", who, N, H, W, r);
    *tiles_x = (int)tx;
    *tiles_y = (int)ty;
    return 0;
}

// The end of an entry that launched kernel k of its library's list: the launch's error, or one more launch counted.
template <int N>
[[maybe_unused]] static int launched(const char *who, Counters<N> &count, int k) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: kernel launch: %s", who, hipGetErrorString(e));
    ++count.launches[k];
    return 0;
}

// Upload `bytes` of `host` to the current device; on failure nothing stays allocated.
[[maybe_unused]] static hipError_t table_create(DeviceTable &t, const void *host, size_t bytes) {
    hipError_t e = hipGetDevice(&t.device);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&t.num_cu, hipDeviceAttributeMultiprocessorCount, t.device);
    if (e == hipSuccess) e = hipMalloc(&t.ptr, bytes);
    if (e == hipSuccess) e = hipMemcpy(t.ptr, host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess && t.ptr) {
        (void)hipFree(t.ptr);
        t.ptr = nullptr;
    }
    return e;
}

[[maybe_unused]] static void table_destroy(DeviceTable &t) {
    if (t.ptr) (void)hipFree(t.ptr);
    t.ptr = nullptr;
}

// The end of a <library>_create whose context `c` (new, with a DeviceTable t) keeps `bytes` of `host`: *out = c, or c is deleted.
template <class Ctx>
[[maybe_unused]] static int ctx_publish(const char *who, Ctx *c, const void *host, size_t bytes, Ctx **out) {
    const hipError_t e = table_create(c->t, host, bytes);
    if (e != hipSuccess) {
        delete c;
        return fail("%s: %s", who, hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

template <class Ctx>
[[maybe_unused]] static void ctx_destroy(Ctx *c) {
    if (!c) return;
    table_destroy(c->t);
    delete c;
}

[[maybe_unused]] static int table_on_current(const char *who, const DeviceTable &t) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != t.device)
        return fail("%s: the context lives on device %d, device %d is current", who, t.device, dev);
    return 0;
}

// A persistent grid-stride launch: one block per `threads` items, at most `blocks_per_cu` blocks per CU.
[[maybe_unused]] static int grid_cap(long long items, int threads, int num_cu, int blocks_per_cu) {
    const long long want = (items + threads - 1) / threads, cap = (long long)num_cu * blocks_per_cu;
    return (int)(want < cap ? want : cap);
}
