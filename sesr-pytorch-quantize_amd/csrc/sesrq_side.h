// Host scaffold of the side libraries (libsesrq_eval.so, libsesrq_raw.so, libsesrq_image.so): the error buffer, the launch counters
// behind their exported instance lists, the input-domain check and host q0 quantiser, and a context that keeps one host table on a
// device.  Each library stays a library of its own; only this host code is shared.  Everything here has internal
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
