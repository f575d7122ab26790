// libsesrq_eval.so: PSNR / SSIM of output frames on the device (include/sesrq_eval.h, include/sesrq_eval_anchor.h).  A library of its own: it links nothing of
// libsesrq.so and registers nothing in its instance table.
//
// One pass over the bytes.  A frame is cut into tiles of BAND input columns x (RH + 6) input rows, one block per tile and one wave per
// channel of it (the waves of a block read the same rows at about the same time); every lane owns
// KC consecutive columns and walks down the tile's rows.  Per row it loads its columns of pred and gt (clip, dequantisation and luma
// on chip), takes the three halo columns on each side from its neighbour lanes, and keeps the 7x7 box sums of the five SSIM moments
// (x, y, x^2, y^2, xy) of its own columns as running sums: row r enters, row r - 7 (re-read, a cache hit) leaves.  Nothing goes back
// to memory but two doubles per tile (sum of squared errors, sum of the SSIM map); a second launch adds them up in a fixed order.
//
// Accuracy.  The variance is E[x^2] - E[x]^2 over a window: in fp32 that difference cancels to an absolute error of ~1e-7, which
// against C2 = 9e-4 is a relative error of ~1e-4 in a flat window.  The moments are therefore formed and summed in fp64: x^2 of an
// fp32 x is exact in fp64, as is the difference of two fp32 values, and the running sums over at most RH + 6 rows drift by ~1e-16.
// Only the final SSIM quotient is fp32 (five inputs rounded once: ~3e-7 relative per pixel), and it divides exactly, so an identical
// pair gives 1.0.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "sesrq_eval.h"
#include "sesrq_eval_anchor.h"
#include "sesrq_eval_tile.h"
#include "sesrq_side.h"

namespace sesrq_evalk {

using namespace sesrq_tile;      // the tile geometry and the row-window core (csrc/sesrq_eval_tile.h)

struct TileArgs {
    const void *pred;
    const float *gt;
    double *part;        // [N][ntiles][C][2]
    const float *anchor; // x2 form, fp32 pred only: the LR frame (N, C, H/2, W/2) whose nearest upsampling is added to pred, or NULL
    int H, W, nbx, nby, ntiles, vec;
    float scale;
    int zero;
};

// np.clip on the float64 luma: a NaN passes through, as clip01
__device__ inline double clip255(double x) { return x != x ? x : fmin(fmax(x, 0.0), 255.0); }

// pred: clip(pred) to [0, 1]; an int8 frame is first dequantised exactly as sesrq_forward forms out_f: (q - zero_L) * scale_out in fp32
__device__ inline void load_pred(const float *row, int col, int W, bool vec, float, int, float v[KC]) {
    load4(row, col, W, vec, v);
#pragma unroll
    for (int k = 0; k < KC; ++k) v[k] = clip01(v[k]);
}

__device__ inline void load_pred(const int8_t *row, int col, int W, bool vec, float scale, int zero, float v[KC]) {
    int q[KC];
    if (vec) {
        const int t = col < W ? *reinterpret_cast<const int *>(row + col) : 0;
#pragma unroll
        for (int k = 0; k < KC; ++k) q[k] = (int)(int8_t)(t >> (8 * k));
    } else {
#pragma unroll
        for (int k = 0; k < KC; ++k) q[k] = col + k < W ? (int)row[col + k] : 0;
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) v[k] = col + k < W ? clip01(__fmul_rn((float)(q[k] - zero), scale)) : 0.f;
}

// pred + up2(anchor) in fp32, then clipped: the bits of scoring a frame the anchor was added to beforehand (torch: pred + up2(x))
__device__ inline void load_pred_anchored(const float *row, const float *arow, int col, int W, bool vec, float v[KC]) {
    load4(row, col, W, vec, v);
#pragma unroll
    for (int k = 0; k < KC; ++k) v[k] = clip01(__fadd_rn(v[k], col + k < W ? arow[(col + k) >> 1] : 0.f));
}

template <typename T, int FORM>
__global__ __launch_bounds__(64 * 3) void eval_tile(TileArgs a) {
    constexpr int C = FORM == SESRQ_EVAL_Y255 ? 1 : 3;
    const int lane = threadIdx.x & 63;
    const int c = threadIdx.x >> 6;                                 // one wave per channel of the tile: they read the same rows at once
    const int tile = blockIdx.x, n = blockIdx.y, H = a.H, W = a.W;
    const int by = tile / a.nbx, bx = tile - by * a.nbx;
    const int c0 = bx * OW, col = c0 + lane * KC;
    const int o0 = PAD + by * RH, o1 = min(o0 + RH, H - PAD);       // SSIM output rows of the tile
    const int s_c0 = c0 + PAD, s_c1 = min(c0 + PAD + OW, W - PAD);  // SSIM output columns of the tile
    // squared errors: every pixel in exactly one tile (the border rows / columns go to the first and last tiles)
    const int m_r0 = by * RH, m_r1 = by == a.nby - 1 ? H : m_r0 + RH;
    const int m_c1 = bx == a.nbx - 1 ? W : c0 + OW;
    const bool vec = a.vec != 0;
    const size_t plane = (size_t)H * W;
    const T *pred = static_cast<const T *>(a.pred) + (size_t)n * C * plane;
    const float *gt = a.gt + (size_t)n * C * plane;
    // SESRQ_EVAL_X2: the squared luma error needs all three channels of a pixel; the channel-0 wave forms it (the other two waves
    // read the same rows in the same block, so those bytes come from cache)
    const bool luma = FORM == SESRQ_EVAL_X2 && c == 0;
    // one row of channel cc of pred, clipped (anchored first when the launch carries an anchor)
    auto pred_row = [&](int cc, int rr, float v[KC]) {
        if constexpr (FORM == SESRQ_EVAL_X2 && std::is_same<T, float>::value) {
            if (a.anchor) {
                const int Wl = W >> 1;
                const float *arow = a.anchor + ((size_t)n * C + cc) * (size_t)(H >> 1) * Wl + (size_t)(rr >> 1) * Wl;
                load_pred_anchored(pred + cc * plane + (size_t)rr * W, arow, col, W, vec, v);
                return;
            }
        }
        load_pred(pred + cc * plane + (size_t)rr * W, col, W, vec, a.scale, a.zero, v);
    };

    double S[KC][5];
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int m = 0; m < 5; ++m) S[k][m] = 0.0;
    double sse = 0.0, ssim = 0.0;

    for (int r = o0 - PAD; r < o1 + PAD; ++r) {
        const bool leave = r - 2 * PAD - 1 >= o0 - PAD;     // row r - 7 leaves the window
        const bool own_row = r >= m_r0 && r < m_r1;
        const bool emit = r >= o0 + PAD;                    // the window of output row r - 3 is complete
        const size_t off = c * plane + (size_t)r * W;
        float x[KC], y[KC], xo[KC] = {0.f, 0.f, 0.f, 0.f}, yo[KC] = {0.f, 0.f, 0.f, 0.f};
        pred_row(c, r, x);
        load4(gt + off, col, W, vec, y);
        if (leave) {
            const size_t offo = off - (size_t)(2 * PAD + 1) * W;
            pred_row(c, r - (2 * PAD + 1), xo);
            load4(gt + offo, col, W, vec, yo);
        }
        if (FORM != SESRQ_EVAL_X2 && own_row) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const double d = (double)y[k] - (double)x[k];
                if (col + k >= c0 && col + k < m_c1) sse += d * d;
            }
        }
        if (luma && own_row) {
            double lp[KC], lg[KC];
#pragma unroll
            for (int k = 0; k < KC; ++k) lp[k] = lg[k] = 0.0;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                const double wc = cc == 0 ? 65.481 : cc == 1 ? 128.553 : 24.966;
                float xc[KC], yc[KC];
                pred_row(cc, r, xc);
                load4(gt + cc * plane + (size_t)r * W, col, W, vec, yc);
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    lp[k] += (double)xc[k] * wc;
                    lg[k] += (double)yc[k] * wc;
                }
            }
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const double yp = clip255(lp[k] + 16.0), yg = clip255(lg[k] + 16.0);
                const double d = yg - yp;
                if (col + k >= c0 && col + k < m_c1) sse += d * d;
            }
        }
        window_step(x, y, xo, yo, S);
        if (emit) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const float s = window_ssim(S[k]);
                if (col + k >= s_c0 && col + k < s_c1) ssim += (double)s;
            }
        }
    }
    wave_sum2(sse, ssim);
    if (lane == 0) {
        double *p = a.part + (((size_t)n * a.ntiles + tile) * C + c) * 2;
        p[0] = sse;
        p[1] = ssim;
    }
}

// one block per frame: the frame's tile partials in a fixed order, then mse / psnr / ssim
__global__ __launch_bounds__(FIN_THREADS) void eval_finish(const double *part, int ntiles, int form, int C, int H, int W, double *out) {
    __shared__ double s_sse[FIN_THREADS], s_ssim[FIN_THREADS];
    const int n = blockIdx.x, t = threadIdx.x;
    const int nparts = ntiles * C;                  // (tile, channel) partials of the frame
    frame_sum2(part + (size_t)n * nparts * 2, nparts, s_sse, s_ssim);
    if (t == 0) {
        const double px = (double)H * W;
        double mse, psnr;
        if (form == SESRQ_EVAL_RGB) {
            mse = s_sse[0] / (C * px);
            psnr = mse == 0.0 ? INFINITY : 10.0 * log10(1.0 / mse);
        } else {
            mse = form == SESRQ_EVAL_Y255 ? 65025.0 * (s_sse[0] / px) : s_sse[0] / px;
            psnr = 10.0 * log10(65025.0 / (mse + 1e-8));
        }
        out[3 * n + 0] = mse;
        out[3 * n + 1] = psnr;
        out[3 * n + 2] = s_ssim[0] / ((double)C * (H - 2 * PAD) * (W - 2 * PAD));
    }
}

// ---------------------------------------------------------------------------------------------------------------------- host side
enum { K_F32_RGB, K_I8_RGB, K_F32_Y255, K_I8_Y255, K_F32_X2, K_FINISH, K_COUNT };
static const char *const kNames[K_COUNT] = {"eval_tile<f32,rgb>", "eval_tile<i8,rgb>", "eval_tile<f32,y255>",
                                            "eval_tile<i8,y255>", "eval_tile<f32,x2>", "eval_finish"};
static Counters<K_COUNT> g_count{kNames};

static int expected_channels(int form) { return form == SESRQ_EVAL_Y255 ? 1 : 3; }

}  // namespace sesrq_evalk

using namespace sesrq_evalk;

extern "C" size_t sesrq_eval_workspace_bytes(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || H < 2 * PAD + 1 || W < 2 * PAD + 1) return 0;
    return (size_t)N * geometry(H, W).ntiles * C * 2 * sizeof(double);
}

static int eval_launch(const sesrq_eval_desc *d, const void *pred, const float *anchor, const float *gt, int N, int C, int H, int W,
                       double *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!d) return fail("sesrq_eval: desc is NULL");
    if (d->form < SESRQ_EVAL_RGB || d->form > SESRQ_EVAL_X2) return fail("sesrq_eval: unknown form %d", d->form);
    if (d->pred_dtype != SESRQ_EVAL_F32 && d->pred_dtype != SESRQ_EVAL_I8)
        return fail("sesrq_eval: unknown pred_dtype %d", d->pred_dtype);
    if (d->pred_dtype == SESRQ_EVAL_I8 && d->form == SESRQ_EVAL_X2)
        return fail("sesrq_eval: an int8 prediction cannot be scored in the x2 form (the anchor exists only in the fp32 output)");
    if (d->pred_dtype == SESRQ_EVAL_I8 && !(d->pred_scale > 0.f && std::isfinite(d->pred_scale)))
        return fail("sesrq_eval: int8 prediction needs a positive finite pred_scale");
    if (d->pred_dtype == SESRQ_EVAL_I8 && (d->pred_zero < -128 || d->pred_zero > 127))
        return fail("sesrq_eval: pred_zero %d outside the int8 range", d->pred_zero);
    if (C != expected_channels(d->form))
        return fail("sesrq_eval: form %d scores %d-channel frames, got C = %d", d->form, expected_channels(d->form), C);
    if (N < 1 || N > 65535) return fail("sesrq_eval: N = %d (1 ... 65535 frames)", N);
    if (H < 2 * PAD + 1 || W < 2 * PAD + 1)
        return fail("sesrq_eval: frame %dx%d is smaller than the 7x7 SSIM window", H, W);
    if (!pred || !gt || !out || !workspace) return fail("sesrq_eval: NULL pred, gt, out or workspace");
    const size_t need = sesrq_eval_workspace_bytes(N, C, H, W);
    if (workspace_bytes < need) return fail("sesrq_eval: workspace of %zu bytes, %zu needed", workspace_bytes, need);

    const Geometry g = geometry(H, W);
    const bool i8 = d->pred_dtype == SESRQ_EVAL_I8;
    TileArgs a;
    a.pred = pred;
    a.gt = gt;
    a.part = static_cast<double *>(workspace);
    a.anchor = anchor;
    a.H = H;
    a.W = W;
    a.nbx = g.nbx;
    a.nby = g.nby;
    a.ntiles = g.ntiles;
    a.vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(gt) % 16 == 0 && reinterpret_cast<uintptr_t>(pred) % (i8 ? 4 : 16) == 0;
    a.scale = d->pred_scale;
    a.zero = d->pred_zero;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(g.ntiles, N), block(64 * C);
    int k;
    if (d->form == SESRQ_EVAL_RGB) {
        k = i8 ? K_I8_RGB : K_F32_RGB;
        if (i8) eval_tile<int8_t, SESRQ_EVAL_RGB><<<grid, block, 0, st>>>(a);
        else eval_tile<float, SESRQ_EVAL_RGB><<<grid, block, 0, st>>>(a);
    } else if (d->form == SESRQ_EVAL_Y255) {
        k = i8 ? K_I8_Y255 : K_F32_Y255;
        if (i8) eval_tile<int8_t, SESRQ_EVAL_Y255><<<grid, block, 0, st>>>(a);
        else eval_tile<float, SESRQ_EVAL_Y255><<<grid, block, 0, st>>>(a);
    } else {
        k = K_F32_X2;
        eval_tile<float, SESRQ_EVAL_X2><<<grid, block, 0, st>>>(a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("sesrq_eval: tile kernel launch: %s", hipGetErrorString(e));
    ++g_count.launches[k];
    eval_finish<<<N, FIN_THREADS, 0, st>>>(a.part, g.ntiles, d->form, C, H, W, out);
    e = hipGetLastError();
    if (e != hipSuccess) return fail("sesrq_eval: finish kernel launch: %s", hipGetErrorString(e));
    ++g_count.launches[K_FINISH];
    return 0;
}

extern "C" int sesrq_eval(const sesrq_eval_desc *d, const void *pred, const float *gt, int N, int C, int H, int W, double *out,
                          void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    return eval_launch(d, pred, nullptr, gt, N, C, H, W, out, workspace, workspace_bytes, stream);
}

extern "C" int sesrq_eval_anchored(const sesrq_eval_desc *d, const float *pred, const float *lr, const float *gt, int N, int C, int H,
                                   int W, double *out, void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (!d) return fail("sesrq_eval_anchored: desc is NULL");
    if (d->form != SESRQ_EVAL_X2 || d->pred_dtype != SESRQ_EVAL_F32)
        return fail("sesrq_eval_anchored: the anchor is added to an fp32 prediction in the x2 form (form %d, pred_dtype %d)", d->form,
                    d->pred_dtype);
    if (!lr) return fail("sesrq_eval_anchored: NULL lr");
    if (H % 2 || W % 2) return fail("sesrq_eval_anchored: frame %dx%d is not twice an LR frame", H, W);
    return eval_launch(d, pred, lr, gt, N, C, H, W, out, workspace, workspace_bytes, stream);
}

extern "C" int sesrq_eval_kernel_count(void) { return g_count.count(); }

extern "C" const char *sesrq_eval_kernel_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_eval_kernel_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_eval_last_error(void) { return g_err; }
