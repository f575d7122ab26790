// Calibration pass (the reference's exe_mode 0; test.py:79-113,141-217): the float net is
// run with fake-quantised weights and activations while the running min/max of every conv input is
// observed.  It produces the activation domains (scale, zero) the integer path consumes; it is not a
// throughput path, so the kernels are simple (one lane = one pixel, all output channels).
//
// Per conv (reference: quantize_asymmetrical_by_tensor mode 0 -> reshape_input_for_hardware_pe -> Conv2d
// with Wq*sw -> PEs_and_bias_adder mode 0 -> activation), with this batch's (scale, zero) of the input:
//   q      = clamp_b(rint(x/scale + zero)) - zero            integer; outside the frame 0     (quan_func.py:207,215)
//            (clamp_b = clamp(., -2^(b-1), 2^(b-1) - 1), the width b of sesrq_calib_conv_q; b = 8 for sesrq_calib_conv)
//   pe_p   = sum_{ic = p mod 4, taps} Wq * q                  exact in int64                   (quan_func.py:298-318)
//   v_p    = clamp(f32(pe_p) * f32(scale*sw), fmin18, fmax18)                                  (quan_func.py:330-333)
//   v      = clamp(v_0 + v_1 + v_2 + v_3, fmin20, fmax20) + bias_q * f32(scale*sw)             (quan_func.py:431-434,459)
// q and pe_p are exact for every zero derive_domain can produce (|zero| <= 2^30): q is staged as int32 and the PE sums are formed in
// int64 -- a domain far from zero (min / span above ~127 at b = 8) has |q| far beyond 16 bits and |pe_p| beyond 32.
// The reference forms the same sums in fp32 (fl(Wq*sw) * fl(q*scale) accumulated by oneDNN in an
// unspecified order); here the integer sum is exact and scaled once, so results agree to fp32 rounding
// -- calibration is pinned to the reference within a tolerance, not bit for bit, and to
// oracle/calib_oracle.py (the definition above) bit for bit.
//
// Quantised long-skip merge (QADD; the reference's QuantAdd, models/quantize_utils_pt.py:654-711, which quantize.prepare() puts in
// place of the long skip's AddOp of a QAT net): with the constant 8-bit symmetric scale s of the net (a launch argument),
//   fq(t) = clamp(sign(t/s) * floor(|t/s| + 0.5), -128, 127) * s        fp32, round half away from zero (Round, :150-166)
//   v     = fq(v) + fq(skip)                                            in place of v + skip
// fused into the same epilogue; tests/qat_calib_oracle.py is its definition, bit for bit.
#include <algorithm>
#include <cmath>

#include "sesrq_common.h"

namespace sesrq {

struct CalibArgs {
    const float *in;        // (N, IC, H, W) fp32
    const float *skip;      // (N, OC, H, W) added after the activation (long residual) or NULL
    float *out;             // (N, OC, H, W)
    const int *w;           // [oc][ic][k][k] int32 (quantised weights)
    const float *qbias;     // [oc]  bias_q * f32(scale*sw)
    int N, H, W, ic, oc;
    float scale, zero;      // this batch's input domain (zero: f32 of izero)
    int izero;
    float qlo, qhi;         // activation range of the width: -2^(b-1), 2^(b-1) - 1
    float ss;               // f32(scale * sw)
    float acc_lo, acc_hi, add_lo, add_hi;
    int relu;
    const sesrq_calib_slot *slot;   // device-resident pass: scale, zero, ss, the bounds and qbias come from here (NULL: the fields above)
    float skip_s;           // QADD instantiations only: the QuantAdd's scale s
};

// The QuantAdd's 8-bit symmetric fake-quantiser at scale s (NaN takes the lower clamp, as fmaxf(NaN, lo) = lo)
__device__ __forceinline__ float skip_fakequant(float t, float s) {
    const float u = __fdiv_rn(t, s), r = floorf(__fadd_rn(fabsf(u), 0.5f));
    return __fmul_rn(fminf(fmaxf(u < 0.f ? -r : r, -128.f), 127.f), s);
}

template <int K, bool QADD>
__device__ __forceinline__ void calib_conv_body(const CalibArgs a) {
    constexpr int R = K / 2, TW = 32, TH = 8, SW = TW + K - 1, SH = TH + K - 1;
    __shared__ int tile[SESRQ_MAX_CH][SH * SW];     // q = r - zero: |q| <= 2^30 + 2^7 (K = 5: 27 KiB)
    const int tid = threadIdx.x, lx = tid & 31, ly = tid >> 5;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, n = blockIdx.z;
    const size_t HW = (size_t)a.H * a.W;
    const sesrq_calib_slot *d = a.slot;
    const float scale = d ? d->scale32 : a.scale, zero = d ? d->zero32 : a.zero, ss = d ? d->ss : a.ss;
    const int izero = d ? d->zero : a.izero;
    const float acc_lo = d ? d->acc_lo : a.acc_lo, acc_hi = d ? d->acc_hi : a.acc_hi;
    const float add_lo = d ? d->add_lo : a.add_lo, add_hi = d ? d->add_hi : a.add_hi;
    const float *qbias = d ? d->qbias : a.qbias;
    for (int c = 0; c < a.ic; ++c)
        for (int i = tid; i < SH * SW; i += 256) {
            const int ty = i / SW, tx = i - ty * SW, gy = y0 - R + ty, gx = x0 - R + tx;
            int q = 0;
            if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
                const float xv = a.in[((size_t)n * a.ic + c) * HW + (size_t)gy * a.W + gx];
                const float r = fminf(fmaxf(rintf(__fadd_rn(__fdiv_rn(xv, scale), zero)), a.qlo), a.qhi);
                q = (int)r - izero;
            }
            tile[c][i] = q;
        }
    __syncthreads();
    const int gx = x0 + lx, gy = y0 + ly;
    if (gx >= a.W || gy >= a.H) return;
    for (int o = 0; o < a.oc; ++o) {
        float sum = 0.f;
        for (int p = 0; p < 4; ++p) {
            long long acc = 0;
            for (int c = p; c < a.ic; c += 4) {
                const int *wp = a.w + ((size_t)o * a.ic + c) * K * K;
#pragma unroll
                for (int ky = 0; ky < K; ++ky)
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) acc += (long long)wp[ky * K + kx] * tile[c][(ly + ky) * SW + lx + kx];
            }
            const float v = fminf(fmaxf(__fmul_rn((float)acc, ss), acc_lo), acc_hi);
            sum = (p == 0) ? v : __fadd_rn(sum, v);
        }
        float v = __fadd_rn(fminf(fmaxf(sum, add_lo), add_hi), qbias[o]);
        if (a.relu) v = fmaxf(v, 0.f);
        const size_t off = ((size_t)n * a.oc + o) * HW + (size_t)gy * a.W + gx;
        if constexpr (QADD) v = __fadd_rn(skip_fakequant(v, a.skip_s), skip_fakequant(a.skip[off], a.skip_s));
        else if (a.skip) v = __fadd_rn(v, a.skip[off]);
        a.out[off] = v;
    }
}
template <int K>
__global__ __launch_bounds__(256) void calib_conv_kernel(const CalibArgs a) { calib_conv_body<K, false>(a); }
// the same conv with the QuantAdd merge in its epilogue: kernels of their own (list REG_QADD), so that the plain ones stay as they are
template <int K>
__global__ __launch_bounds__(256) void calib_conv_qadd_kernel(const CalibArgs a) { calib_conv_body<K, true>(a); }

// order-preserving float <-> uint map so that min/max can use integer atomics
__device__ __forceinline__ unsigned f2ord(float f) { const unsigned u = __builtin_bit_cast(unsigned, f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__global__ void calib_minmax_kernel(const float *x, size_t n, unsigned *mm) {
    float lo = INFINITY, hi = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        lo = fminf(lo, v); hi = fmaxf(hi, v);
    }
    for (int s = 32; s > 0; s >>= 1) { lo = fminf(lo, __shfl_xor(lo, s)); hi = fmaxf(hi, __shfl_xor(hi, s)); }
    if ((threadIdx.x & 63) == 0) { atomicMin(&mm[0], f2ord(lo)); atomicMax(&mm[1], f2ord(hi)); }
}
// The quantiser's domain from a batch's extrema (test.py's mode-0 quantiser, quan_func.py:175-215, and the per-layer constants of the
// host pass, sesrq/calibrate.py): fp64 where the host computes in Python floats, fp32 where it uses numpy float32, same order.
struct DomainArgs {
    int quan_bits, oc;
    const float *bias;
    double sw;
    int acc_bits, add_bits, bias_bits;
};

__device__ inline void derive_domain(sesrq_calib_slot *s, const DomainArgs &d, float mn32, float mx32, int lane) {
    if (lane == 0) {               // fold, as the host does: a strictly larger max / smaller min replaces the running one
        if (s->batches == 0 || s->run_max < mx32) s->run_max = mx32;
        if (s->batches == 0 || s->run_min > mn32) s->run_min = mn32;
        s->batches += 1;
    }
    const double mn = mn32, mx = mx32;
    if (!(mx != mn)) {             // the host pass asserts here; the pass goes on with a harmless domain and the flag is raised at readback
        if (lane == 0) {
            s->degenerate = 1;
            s->scale = 0.0; s->zero = 0; s->scale32 = 1.f; s->zero32 = 0.f; s->ss = 1.f;
            s->acc_lo = s->add_lo = -INFINITY; s->acc_hi = s->add_hi = INFINITY;
        }
        if (lane < d.oc) s->qbias[lane] = 0.f;
        return;
    }
    const double scale = (mx - mn) / (double)((1 << d.quan_bits) - 1);
    // Python's round is half-to-even: rint in the default rounding mode; clamped so that a far-off range cannot overflow the int
    const double zd = fmin(fmax(-(double)(1 << (d.quan_bits - 1)) - rint(mn / scale), -1073741824.0), 1073741824.0);
    const int zero = (int)zd;
    const double ssd = scale * d.sw;
    const float ss = (float)ssd;
    if (lane == 0) {
        s->scale = scale;
        s->zero = zero;
        s->scale32 = (float)scale;
        s->zero32 = (float)zero;
        s->ss = ss;
        const double lo_a = -(double)(1 << (d.acc_bits - 1)), hi_a = (double)(1 << (d.acc_bits - 1)) - 1.0;
        const double lo_s = -(double)(1 << (d.add_bits - 1)), hi_s = (double)(1 << (d.add_bits - 1)) - 1.0;
        s->acc_lo = (float)(((lo_a - zero) * scale) * d.sw);
        s->acc_hi = (float)(((hi_a - zero) * scale) * d.sw);
        s->add_lo = (float)(((lo_s - zero) * scale) * d.sw);
        s->add_hi = (float)(((hi_s - zero) * scale) * d.sw);
    }
    if (lane < d.oc) {             // numpy: clip(rint(f32 bias / f32(scale * sw)), lo, hi) in float32, then * f32(scale * sw)
        const float lo16 = -(float)(1 << (d.bias_bits - 1)), hi16 = (float)((1 << (d.bias_bits - 1)) - 1);
        const float bq = fminf(fmaxf(rintf(__fdiv_rn(d.bias[lane], ss)), lo16), hi16);
        s->qbias[lane] = __fmul_rn(bq, ss);
    }
}

// Decodes the reduction's keys into out[0..1].  With a slot (the device-resident pass; mm = slot->ord, out = &slot->min) it also
// folds the extrema into the running ones, derives this batch's domain (one wave: lane o forms bias constant o) and leaves the keys
// at their initial value for the slot's next batch.
__global__ void calib_minmax_finish(const unsigned *mm, float *out, sesrq_calib_slot *slot, DomainArgs dom) {
    const int lane = threadIdx.x;
    float v[2];
    for (int i = 0; i < 2; ++i) {
        const unsigned o = mm[i], u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
        v[i] = __builtin_bit_cast(float, u);
    }
    __syncthreads();               // every lane has read the keys before lane 0 resets them
    if (lane == 0) { out[0] = v[0]; out[1] = v[1]; }
    if (!slot) return;
    if (lane == 0) { slot->ord[0] = 0xffffffffu; slot->ord[1] = 0u; }
    derive_domain(slot, dom, v[0], v[1], lane);
}
// With a slot the domain is the slot's and the output is written pixel-shuffled by r (input (N, C, H, W), C = c r^2:
// out[n][c][h r + i][w r + j] = in[n][c r^2 + i r + j][h][w], torch's pixel_shuffle); without one, scale / zero / out[i] as given.
__global__ void calib_fakequant_kernel(const float *in, float *out, size_t n, float scale, float zero, float qlo, float qhi,
                                       const sesrq_calib_slot *slot, int C, int H, int W, int r) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        if (slot) { scale = slot->scale32; zero = slot->zero32; }
        const float q = fminf(fmaxf(rintf(__fadd_rn(__fdiv_rn(in[i], scale), zero)), qlo), qhi);
        size_t o = i;
        if (r > 1) {
            const size_t HW = (size_t)H * W, p = i % HW, nc = i / HW;
            const int h = (int)(p / W), w = (int)(p - (size_t)h * W), ch = (int)(nc % C), rr = r * r, c = ch / rr, ij = ch - c * rr;
            const size_t nn = nc / C;
            o = ((nn * (C / rr) + c) * ((size_t)H * r) + (size_t)h * r + ij / r) * ((size_t)W * r) + (size_t)w * r + ij % r;
        }
        out[o] = __fmul_rn(q - zero, scale);
    }
}

// Histogram of a tensor over [lo, hi) in `bins` equal bins (bin = floor((x - lo) * bins / (hi - lo)), clamped to the range: values
// outside count in the edge bins), accumulated INTO hist.  One private copy per workgroup in LDS, merged with one atomic per
// non-empty bin: the entropy calibration variant's second pass (no reference counterpart).
constexpr int CALIB_MAX_BINS = 4096;
__global__ __launch_bounds__(256) void calib_hist_kernel(const float *x, size_t n, float lo, float inv_w, int bins, unsigned *hist) {
    __shared__ unsigned h[CALIB_MAX_BINS];
    for (int i = threadIdx.x; i < bins; i += 256) h[i] = 0;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = x[i];
        if (v == v) {                    // NaNs are not counted
            int b = (int)floorf(__fmul_rn(__fsub_rn(v, lo), inv_w));
            b = min(max(b, 0), bins - 1);
            atomicAdd(&h[b], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

}  // namespace sesrq

using namespace sesrq;

extern "C" {

int sesrq_calib_minmax(const float *x, size_t n, float *out_min_max, void *scratch8, void *stream) {
    if (!x || !out_min_max || !scratch8 || n == 0) { set_error("sesrq_calib_minmax: bad argument"); return 1; }
    hipStream_t st = (hipStream_t)stream;
    static const unsigned init[2] = {0xffffffffu, 0u};
    if (hipMemcpyAsync(scratch8, init, sizeof(init), hipMemcpyHostToDevice, st) != hipSuccess) { set_error("sesrq_calib_minmax: memcpy failed"); return 1; }
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 2048);
    launch_kernel<calib_minmax_kernel>(dim3(blocks), dim3(256), 0, st, x, n, (unsigned *)scratch8);
    launch_kernel<calib_minmax_finish>(dim3(1), dim3(1), 0, st, (const unsigned *)scratch8, out_min_max, (sesrq_calib_slot *)nullptr,
                                       DomainArgs{});
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// One launch of the conv: the plain instantiation, or -- qadd -- the one whose epilogue merges the skip through the QuantAdd.
static int launch_conv(const CalibArgs &a, int k, bool qadd, void *stream, const char *who) {
    dim3 grid((a.W + 31) / 32, (a.H + 7) / 8, a.N);
    hipStream_t st = (hipStream_t)stream;
    if (qadd) {
        if (k == 3) launch_kernel<calib_conv_qadd_kernel<3>, REG_QADD>(grid, dim3(256), 0, st, a);
        else launch_kernel<calib_conv_qadd_kernel<5>, REG_QADD>(grid, dim3(256), 0, st, a);
    } else {
        if (k == 3) launch_kernel<calib_conv_kernel<3>>(grid, dim3(256), 0, st, a);
        else launch_kernel<calib_conv_kernel<5>>(grid, dim3(256), 0, st, a);
    }
    if (hipGetLastError() != hipSuccess) { set_error(std::string(who) + ": launch failed"); return 1; }
    return 0;
}

// The QuantAdd arguments of the _qadd entry points, refused before any launch
static bool bad_skip_scale(const float *skip, float skip_scale, const char *who) {
    if (!skip) { set_error(std::string(who) + ": the quantised merge needs a skip tensor"); return true; }
    if (!(skip_scale > 0.f) || !std::isfinite(skip_scale)) { set_error(std::string(who) + ": skip_scale must be positive and finite"); return true; }
    return false;
}

static int calib_conv_host(const sesrq_calib_conv_desc *d, const float *in, const float *skip, float *out, int N, int H, int W, int quan_bits,
                           bool qadd, float skip_scale, void *stream) {
    if (quan_bits < 2 || quan_bits > 8) { set_error("sesrq_calib_conv_q: quan_bits must be 2..8"); return 1; }
    if (!d || !in || !out || !d->w || !d->qbias) { set_error("sesrq_calib_conv: null argument"); return 1; }
    if ((d->k != 3 && d->k != 5) || d->ic < 1 || d->ic > SESRQ_MAX_CH || d->oc < 1 || d->oc > SESRQ_MAX_CH) { set_error("sesrq_calib_conv: unsupported layer shape"); return 1; }
    if (N < 1 || H < 1 || W < 1 || !(d->in_scale > 0.f)) { set_error("sesrq_calib_conv: bad size or scale"); return 1; }
    if (d->in_zero < -(1 << 30) || d->in_zero > (1 << 30)) { set_error("sesrq_calib_conv: |in_zero| must be <= 2^30"); return 1; }
    CalibArgs a;
    a.in = in; a.skip = skip; a.out = out; a.w = d->w; a.qbias = d->qbias;
    a.N = N; a.H = H; a.W = W; a.ic = d->ic; a.oc = d->oc;
    a.scale = d->in_scale; a.zero = (float)d->in_zero; a.izero = d->in_zero; a.ss = d->ss;
    a.qlo = -(float)(1 << (quan_bits - 1)); a.qhi = (float)((1 << (quan_bits - 1)) - 1);
    a.acc_lo = d->acc_lo; a.acc_hi = d->acc_hi; a.add_lo = d->add_lo; a.add_hi = d->add_hi; a.relu = d->relu;
    a.slot = nullptr;
    a.skip_s = skip_scale;
    return launch_conv(a, d->k, qadd, stream, "sesrq_calib_conv");
}

int sesrq_calib_conv_q(const sesrq_calib_conv_desc *d, const float *in, const float *skip, float *out, int N, int H, int W, int quan_bits,
                       void *stream) {
    return calib_conv_host(d, in, skip, out, N, H, W, quan_bits, false, 0.f, stream);
}

int sesrq_calib_conv_qadd(const sesrq_calib_conv_desc *d, const float *in, const float *skip, float *out, int N, int H, int W, int quan_bits,
                          float skip_scale, void *stream) {
    if (bad_skip_scale(skip, skip_scale, "sesrq_calib_conv_qadd")) return 1;
    return calib_conv_host(d, in, skip, out, N, H, W, quan_bits, true, skip_scale, stream);
}

int sesrq_calib_conv(const sesrq_calib_conv_desc *d, const float *in, const float *skip, float *out, int N, int H, int W, void *stream) {
    return sesrq_calib_conv_q(d, in, skip, out, N, H, W, 8, stream);
}

int sesrq_calib_histogram(const float *x, size_t n, float lo, float hi, int bins, uint32_t *hist, void *stream) {
    if (!x || !hist || n == 0) { set_error("sesrq_calib_histogram: bad argument"); return 1; }
    if (bins < 2 || bins > CALIB_MAX_BINS) { set_error("sesrq_calib_histogram: bins must be 2..4096"); return 1; }
    if (!(hi > lo) || !std::isfinite(lo) || !std::isfinite(hi)) { set_error("sesrq_calib_histogram: need finite lo < hi"); return 1; }
    const float inv_w = (float)bins / (hi - lo);
    const int blocks = (int)std::min<size_t>((n + 256 * 16 - 1) / (256 * 16), 2048);
    launch_kernel<calib_hist_kernel>(dim3(std::max(blocks, 1)), dim3(256), 0, (hipStream_t)stream, x, n, lo, inv_w, bins, (unsigned *)hist);
    if (hipGetLastError() != hipSuccess) { set_error("sesrq_calib_histogram: launch failed"); return 1; }
    return 0;
}

int sesrq_calib_fakequant_q(const float *in, float *out, size_t n, float scale, int zero, int quan_bits, void *stream) {
    if (!in || !out || n == 0 || !(scale > 0.f)) { set_error("sesrq_calib_fakequant: bad argument"); return 1; }
    if (quan_bits < 2 || quan_bits > 8) { set_error("sesrq_calib_fakequant_q: quan_bits must be 2..8"); return 1; }
    const float qlo = -(float)(1 << (quan_bits - 1)), qhi = (float)((1 << (quan_bits - 1)) - 1);
    launch_kernel<calib_fakequant_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, n, scale, (float)zero, qlo, qhi,
                                          (const sesrq_calib_slot *)nullptr, 0, 0, 0, 1);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int sesrq_calib_fakequant(const float *in, float *out, size_t n, float scale, int zero, void *stream) {
    return sesrq_calib_fakequant_q(in, out, n, scale, zero, 8, stream);
}

static_assert(sizeof(sesrq_calib_slot) == 136, "sesrq_calib_slot: the layout the bindings mirror");
size_t sesrq_calib_slot_bytes(void) { return sizeof(sesrq_calib_slot); }

int sesrq_calib_slots_init(sesrq_calib_slot *host_slots, int n) {
    if (!host_slots || n < 1) { set_error("sesrq_calib_slots_init: bad argument"); return 1; }
    for (int i = 0; i < n; ++i) {
        sesrq_calib_slot s = {};
        s.ord[0] = 0xffffffffu;
        s.run_min = INFINITY;
        s.run_max = -INFINITY;
        host_slots[i] = s;
    }
    return 0;
}

int sesrq_calib_observe_slot(const float *x, size_t n, sesrq_calib_slot *slot, const sesrq_calib_domain_desc *d, void *stream) {
    if (!x || !slot || !d || n == 0) { set_error("sesrq_calib_observe_slot: bad argument"); return 1; }
    if (d->quan_bits < 2 || d->quan_bits > 8) { set_error("sesrq_calib_observe_slot: quan_bits must be 2..8"); return 1; }
    if (d->oc < 0 || d->oc > SESRQ_MAX_CH || (d->oc > 0 && !d->bias)) { set_error("sesrq_calib_observe_slot: oc must be 0..16 with a bias"); return 1; }
    if (d->acc_bits < 2 || d->acc_bits > 30 || d->add_bits < 2 || d->add_bits > 30 || d->bias_bits < 2 || d->bias_bits > 24) {
        set_error("sesrq_calib_observe_slot: PE / bias widths out of range");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    const DomainArgs dom{d->quan_bits, d->oc, d->bias, d->sw, d->acc_bits, d->add_bits, d->bias_bits};
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 2048);
    launch_kernel<calib_minmax_kernel>(dim3(blocks), dim3(256), 0, st, x, n, (unsigned *)slot->ord);
    launch_kernel<calib_minmax_finish>(dim3(1), dim3(64), 0, st, (const unsigned *)slot->ord, &slot->min, slot, dom);
    if (hipGetLastError() != hipSuccess) { set_error("sesrq_calib_observe_slot: launch failed"); return 1; }
    return 0;
}

static int calib_conv_slot(const sesrq_calib_conv_desc *d, const sesrq_calib_slot *slot, const float *in, const float *skip, float *out,
                           int N, int H, int W, int quan_bits, bool qadd, float skip_scale, void *stream) {
    if (quan_bits < 2 || quan_bits > 8) { set_error("sesrq_calib_conv_slot: quan_bits must be 2..8"); return 1; }
    if (!d || !slot || !in || !out || !d->w) { set_error("sesrq_calib_conv_slot: null argument"); return 1; }
    if ((d->k != 3 && d->k != 5) || d->ic < 1 || d->ic > SESRQ_MAX_CH || d->oc < 1 || d->oc > SESRQ_MAX_CH) { set_error("sesrq_calib_conv_slot: unsupported layer shape"); return 1; }
    if (N < 1 || H < 1 || W < 1) { set_error("sesrq_calib_conv_slot: bad size"); return 1; }
    CalibArgs a = {};
    a.in = in; a.skip = skip; a.out = out; a.w = d->w; a.qbias = nullptr;
    a.N = N; a.H = H; a.W = W; a.ic = d->ic; a.oc = d->oc;
    a.qlo = -(float)(1 << (quan_bits - 1)); a.qhi = (float)((1 << (quan_bits - 1)) - 1);
    a.relu = d->relu;
    a.slot = slot;
    a.skip_s = skip_scale;
    return launch_conv(a, d->k, qadd, stream, "sesrq_calib_conv_slot");
}

int sesrq_calib_conv_slot(const sesrq_calib_conv_desc *d, const sesrq_calib_slot *slot, const float *in, const float *skip, float *out,
                          int N, int H, int W, int quan_bits, void *stream) {
    return calib_conv_slot(d, slot, in, skip, out, N, H, W, quan_bits, false, 0.f, stream);
}

int sesrq_calib_conv_slot_qadd(const sesrq_calib_conv_desc *d, const sesrq_calib_slot *slot, const float *in, const float *skip, float *out,
                               int N, int H, int W, int quan_bits, float skip_scale, void *stream) {
    if (bad_skip_scale(skip, skip_scale, "sesrq_calib_conv_slot_qadd")) return 1;
    return calib_conv_slot(d, slot, in, skip, out, N, H, W, quan_bits, true, skip_scale, stream);
}

int sesrq_calib_fakequant_slot(const float *in, float *out, int N, int C, int H, int W, int r, const sesrq_calib_slot *slot, int quan_bits,
                               void *stream) {
    if (!in || !out || !slot || N < 1 || C < 1 || H < 1 || W < 1 || r < 1 || C % (r * r) != 0) {
        set_error("sesrq_calib_fakequant_slot: bad argument");
        return 1;
    }
    if (quan_bits < 2 || quan_bits > 8) { set_error("sesrq_calib_fakequant_slot: quan_bits must be 2..8"); return 1; }
    const size_t n = (size_t)N * C * H * W;
    const float qlo = -(float)(1 << (quan_bits - 1)), qhi = (float)((1 << (quan_bits - 1)) - 1);
    launch_kernel<calib_fakequant_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, n, 1.f, 0.f, qlo,
                                          qhi, slot, C, H, W, r);
    if (hipGetLastError() != hipSuccess) { set_error("sesrq_calib_fakequant_slot: launch failed"); return 1; }
    return 0;
}

}  // extern "C"
