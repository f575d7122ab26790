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
#include "sesrq_side.h"

namespace sesrq_evalk {

constexpr int KC = 4;              // columns per lane
constexpr int BAND = 64 * KC;      // input columns of one tile
constexpr int OW = 248;            // SSIM output columns per tile (BAND - 6, rounded down to a multiple of 4: tiles start 16-B aligned)
constexpr int RH = 32;             // SSIM output rows per tile
constexpr int PAD = 3;             // window radius
constexpr int FIN_THREADS = 256;
static_assert(OW % 4 == 0 && OW <= BAND - 2 * PAD, "a tile's SSIM columns need their halo inside the band");

struct Geometry {
    int nbx, nby, ntiles;
};

// A function of (H, W) only: a frame's partial sums, and so its result, do not depend on N, the stream or the other frames.
static inline Geometry geometry(int H, int W) {
    Geometry g;
    g.nbx = (W - 2 * PAD + OW - 1) / OW;
    g.nby = (H - 2 * PAD + RH - 1) / RH;
    g.ntiles = g.nbx * g.nby;
    return g;
}

struct TileArgs {
    const void *pred;
    const float *gt;
    double *part;        // [N][ntiles][C][2]
    const float *anchor; // x2 form, fp32 pred only: the LR frame (N, C, H/2, W/2) whose nearest upsampling is added to pred, or NULL
    int H, W, nbx, nby, ntiles, vec;
    float scale;
    int zero;
};

// four consecutive columns of one row; zeros past the right edge (they reach only SSIM outputs that are never used)
__device__ inline void load4(const float *row, int col, int W, bool vec, float v[KC]) {
    if (vec) {
        float4 t = col < W ? *reinterpret_cast<const float4 *>(row + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < KC; ++k) v[k] = col + k < W ? row[col + k] : 0.f;
    }
}

// np.clip of the reference: a NaN passes through (fminf / fmaxf alone would return the bound), so a NaN in a frame reaches its scores
__device__ inline float clip01(float x) { return x != x ? x : fminf(fmaxf(x, 0.f), 1.f); }
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

// the 10 columns col-3 .. col+6 of one row: three from the lane on the left, four own, three from the lane on the right
// (lanes 0 and 63 receive their own values; they reach only SSIM outputs outside the tile)
__device__ inline void halo(const float own[KC], float out[KC + 2 * PAD]) {
#pragma unroll
    for (int k = 0; k < PAD; ++k) out[k] = __shfl_up(own[KC - PAD + k], 1);
#pragma unroll
    for (int k = 0; k < KC; ++k) out[PAD + k] = own[k];
#pragma unroll
    for (int k = 0; k < PAD; ++k) out[PAD + KC + k] = __shfl_down(own[k], 1);
}

__device__ inline double moment(int m, double x, double y) {
    return m == 0 ? x : m == 1 ? y : m == 2 ? x * x : m == 3 ? y * y : x * y;
}

template <typename T, int FORM>
__global__ __launch_bounds__(64 * 3) void eval_tile(TileArgs a) {
    constexpr int C = FORM == SESRQ_EVAL_Y255 ? 1 : 3;
    constexpr int NC = KC + 2 * PAD;
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
        float hx[NC], hy[NC], hxo[NC], hyo[NC];
        halo(x, hx);
        halo(y, hy);
        halo(xo, hxo);
        halo(yo, hyo);
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            double d[NC];
#pragma unroll
            for (int i = 0; i < NC; ++i) d[i] = moment(m, hx[i], hy[i]) - moment(m, hxo[i], hyo[i]);
            double h = d[0] + d[1] + d[2] + d[3] + d[4] + d[5] + d[6];
            S[0][m] += h;
#pragma unroll
            for (int k = 1; k < KC; ++k) {
                h = h + d[k + 6] - d[k - 1];
                S[k][m] += h;
            }
        }
        if (emit) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const double ux = S[k][0] * (1.0 / 49.0), uy = S[k][1] * (1.0 / 49.0);
                const double cov = 49.0 / 48.0;
                const float fux = (float)ux, fuy = (float)uy;
                const float vx = (float)(cov * (S[k][2] * (1.0 / 49.0) - ux * ux));
                const float vy = (float)(cov * (S[k][3] * (1.0 / 49.0) - uy * uy));
                const float vxy = (float)(cov * (S[k][4] * (1.0 / 49.0) - ux * uy));
                const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
                const float A1 = 2.f * fux * fuy + C1, A2 = 2.f * vxy + C2;
                const float B1 = fux * fux + fuy * fuy + C1, B2 = vx + vy + C2;
                const float s = (A1 * A2) / (B1 * B2);
                if (col + k >= s_c0 && col + k < s_c1) ssim += (double)s;
            }
        }
    }
    // fixed-order butterfly over the wave: the same bits on every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sse += __shfl_xor(sse, o);
        ssim += __shfl_xor(ssim, o);
    }
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
    const double *p = part + (size_t)n * nparts * 2;
    double a = 0.0, b = 0.0;
    for (int i = t; i < nparts; i += FIN_THREADS) {
        a += p[2 * i];
        b += p[2 * i + 1];
    }
    s_sse[t] = a;
    s_ssim[t] = b;
    __syncthreads();
    for (int s = FIN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            s_sse[t] += s_sse[t + s];
            s_ssim[t] += s_ssim[t + s];
        }
        __syncthreads();
    }
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
