// What the metric libraries share (csrc/sesrq_eval.hip, csrc/sesrq_mosaic.hip).  Device side: the tile geometry, the loads of a
// lane's four columns, np.clip's clip, the int8 dequantisation, the lane-shuffled halo, the five SSIM moments, the running 7x7 box
// sums, the SSIM quotient, the two fixed-order sums, the walk down a tile's rows (tile_walk) and the frame's finish (frame_finish).
// Host side: the checks every scoring entry makes and the filling of TileArgs (tile_args), and the launch of a tile kernel and its
// finish kernel (launch_pair).  Each library compiles its own copy (they share no symbol), with -ffp-contract=off: one definition of
// every expression, so a single-channel frame scores to the same bits in either library (tests/test_mosaic_quality.py compares them).
//
// A tile is BAND input columns x (RH + 6) input rows, walked by one wave: lane l owns the KC columns c0 + KC l ... and keeps, per
// column, the box sums of the moments (x, y, x^2, y^2, xy) in fp64; only the final quotient is fp32 (csrc/sesrq_eval.hip, "Accuracy").
// A library's kernel says how a row is loaded (row) and what its squared error is (err); everything else is here.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_side.h"

namespace sesrq_tile {

constexpr int KC = 4;              // columns per lane
constexpr int BAND = 64 * KC;      // input columns of one tile
constexpr int OW = 248;            // SSIM output columns per tile (BAND - 6, rounded down to a multiple of 4: tiles start 16-B aligned)
constexpr int RH = 32;             // SSIM output rows per tile
constexpr int PAD = 3;             // window radius
constexpr int NC = KC + 2 * PAD;   // a lane's columns with their halo
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

// an int8 sample dequantised exactly as sesrq_forward forms out_f, (q - zero_L) * scale_out in fp32, then clipped
__device__ inline float dequant_clip01(int q, int zero, float scale) { return clip01(__fmul_rn((float)(q - zero), scale)); }

// the 10 columns col-3 .. col+6 of one row: three from the lane on the left, four own, three from the lane on the right
// (lanes 0 and 63 receive their own values; they reach only SSIM outputs outside the tile)
__device__ inline void halo(const float own[KC], float out[NC]) {
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

// One row (x, y) enters the box sums of a lane's columns and one row (xo, yo) leaves them (zeros while the window fills).
__device__ inline void window_step(const float x[KC], const float y[KC], const float xo[KC], const float yo[KC], double S[KC][5]) {
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
}

// SSIM of one complete window from its box sums: skimage's defaults (K1 = 0.01, K2 = 0.03, covariance scaled by 49 / 48, data_range 1)
__device__ inline float window_ssim(const double S[5]) {
    const double ux = S[0] * (1.0 / 49.0), uy = S[1] * (1.0 / 49.0);
    const double cov = 49.0 / 48.0;
    const float fux = (float)ux, fuy = (float)uy;
    const float vx = (float)(cov * (S[2] * (1.0 / 49.0) - ux * ux));
    const float vy = (float)(cov * (S[3] * (1.0 / 49.0) - uy * uy));
    const float vxy = (float)(cov * (S[4] * (1.0 / 49.0) - ux * uy));
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float A1 = 2.f * fux * fuy + C1, A2 = 2.f * vxy + C2;
    const float B1 = fux * fux + fuy * fuy + C1, B2 = vx + vy + C2;
    return (A1 * A2) / (B1 * B2);
}

// fixed-order butterfly over the wave: the same bits on every run
__device__ inline void wave_sum2(double &a, double &b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
}

// A frame's `nparts` partials (pairs of doubles) in a fixed order, by one block of FIN_THREADS threads: the two sums are left in
// s_a[0] and s_b[0] for thread 0.
__device__ inline void frame_sum2(const double *p, int nparts, double s_a[FIN_THREADS], double s_b[FIN_THREADS]) {
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = t; i < nparts; i += FIN_THREADS) {
        a += p[2 * i];
        b += p[2 * i + 1];
    }
    s_a[t] = a;
    s_b[t] = b;
    __syncthreads();
    for (int s = FIN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            s_a[t] += s_a[t + s];
            s_b[t] += s_b[t + s];
        }
        __syncthreads();
    }
}

// What a tile kernel gets: the frames, the slab of partials and the launch's geometry.
struct TileArgs {
    const void *pred;
    const float *gt;
    double *part;        // [N][ntiles][slots][2]
    const float *anchor; // sesrq_eval_anchored only: the LR frame (N, C, H/2, W/2) whose nearest upsampling is added to pred; else NULL
    int H, W, nbx, nby, ntiles, vec;
    float scale;
    int zero;
};

// One lane's share of one tile
struct Tile {
    int lane;
    int c0, col;           // the tile's first column, the lane's first column
    int o0, o1;            // SSIM output rows of the tile
    int s_c0, s_c1;        // SSIM output columns of the tile
    int m_r0, m_r1, m_c1;  // squared errors: every pixel in exactly one tile (the border rows / columns go to the first and last tiles)
};

__device__ inline Tile tile_of(const TileArgs &a, int tile, int lane) {
    Tile t;
    const int by = tile / a.nbx, bx = tile - by * a.nbx;
    t.lane = lane;
    t.c0 = bx * OW;
    t.col = t.c0 + lane * KC;
    t.o0 = PAD + by * RH;
    t.o1 = min(t.o0 + RH, a.H - PAD);
    t.s_c0 = t.c0 + PAD;
    t.s_c1 = min(t.c0 + PAD + OW, a.W - PAD);
    t.m_r0 = by * RH;
    t.m_r1 = by == a.nby - 1 ? a.H : t.m_r0 + RH;
    t.m_c1 = bx == a.nbx - 1 ? a.W : t.c0 + OW;
    return t;
}

// the default err of tile_walk: the squared difference of a lane's columns of one row, in fp64
__device__ inline bool sq_err(int, const float x[KC], const float y[KC], double d2[KC]) {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const double d = (double)y[k] - (double)x[k];
        d2[k] = d * d;
    }
    return true;
}

// The walk down a tile's rows, by one wave: row r enters the box sums, row r - 7 (re-read, a cache hit) leaves them; the wave's sum of
// squared errors and of the SSIM map go to p[0] and p[1].
//   row(r, x, y)       loads the lane's columns of row r: the prediction, dequantised and clipped, and the ground truth
//   err(r, x, y, d2)   fills the squared errors of those columns; false when this wave contributes none
template <class Row, class Err>
__device__ inline void tile_walk(const Tile &t, Row row, Err err, double *p) {
    double S[KC][5];
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int m = 0; m < 5; ++m) S[k][m] = 0.0;
    double sse = 0.0, ssim = 0.0;

    for (int r = t.o0 - PAD; r < t.o1 + PAD; ++r) {
        const bool leave = r - 2 * PAD - 1 >= t.o0 - PAD;     // row r - 7 leaves the window
        const bool own_row = r >= t.m_r0 && r < t.m_r1;
        const bool emit = r >= t.o0 + PAD;                    // the window of output row r - 3 is complete
        float x[KC], y[KC], xo[KC] = {0.f, 0.f, 0.f, 0.f}, yo[KC] = {0.f, 0.f, 0.f, 0.f};
        row(r, x, y);
        if (leave) row(r - (2 * PAD + 1), xo, yo);
        if (own_row) {
            double d2[KC];
            if (err(r, x, y, d2)) {
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    if (t.col + k >= t.c0 && t.col + k < t.m_c1) sse += d2[k];
            }
        }
        window_step(x, y, xo, yo, S);
        if (emit) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const float s = window_ssim(S[k]);
                if (t.col + k >= t.s_c0 && t.col + k < t.s_c1) ssim += (double)s;
            }
        }
    }
    wave_sum2(sse, ssim);
    if (t.lane == 0) {
        p[0] = sse;
        p[1] = ssim;
    }
}

// How a frame's sum of squared errors becomes (mse, psnr): the forms of include/sesrq_eval.h, by their values there
enum { FIN_RGB = 0, FIN_Y255 = 1, FIN_X2 = 2 };

// One block of FIN_THREADS threads per frame: the frame's (tile, channel) partials in a fixed order, then mse / psnr / ssim of its C
// scored channels.
__device__ inline void frame_finish(const double *part, int ntiles, int form, int C, int H, int W, double *out) {
    __shared__ double s_sse[FIN_THREADS], s_ssim[FIN_THREADS];
    const int n = blockIdx.x;
    const int nparts = ntiles * C;
    frame_sum2(part + (size_t)n * nparts * 2, nparts, s_sse, s_ssim);
    if (threadIdx.x == 0) {
        const double px = (double)H * W;
        double mse, psnr;
        if (form == FIN_RGB) {
            mse = s_sse[0] / (C * px);
            psnr = mse == 0.0 ? INFINITY : 10.0 * log10(1.0 / mse);
        } else {
            mse = form == FIN_Y255 ? 65025.0 * (s_sse[0] / px) : s_sse[0] / px;
            psnr = 10.0 * log10(65025.0 / (mse + 1e-8));
        }
        out[3 * n + 0] = mse;
        out[3 * n + 1] = psnr;
        out[3 * n + 2] = s_ssim[0] / ((double)C * (H - 2 * PAD) * (W - 2 * PAD));
    }
}

// ---------------------------------------------------------------------------------------------------------------------- host side
// `slots` pairs of doubles per tile: one per wave of the tile kernel's block
static inline size_t partials_bytes(int N, int slots, int H, int W) {
    if (N < 1 || slots < 1 || H < 2 * PAD + 1 || W < 2 * PAD + 1) return 0;
    return (size_t)N * geometry(H, W).ntiles * slots * 2 * sizeof(double);
}

// What every scoring entry refuses, in `who`'s name, and the arguments of its tile kernel.  pred_dtype: 0 fp32, 1 int8 (both headers).
static int tile_args(const char *who, int pred_dtype, float pred_scale, int pred_zero, const void *pred, const float *anchor,
                     const float *gt, int N, int slots, int H, int W, const double *out, void *workspace, size_t workspace_bytes,
                     TileArgs &a) {
    const bool i8 = pred_dtype == 1;
    if (pred_dtype != 0 && !i8) return fail("%s: unknown pred_dtype %d", who, pred_dtype);
    if (i8 && !(pred_scale > 0.f && std::isfinite(pred_scale))) return fail("%s: int8 prediction needs a positive finite pred_scale", who);
    if (i8 && (pred_zero < -128 || pred_zero > 127)) return fail("%s: pred_zero %d outside the int8 range", who, pred_zero);
    if (N < 1 || N > 65535) return fail("%s: N = %d (1 ... 65535 frames)", who, N);
    if (H < 2 * PAD + 1 || W < 2 * PAD + 1) return fail("%s: frame %dx%d is smaller than the 7x7 SSIM window", who, H, W);
    if (!pred || !gt || !out || !workspace) return fail("%s: NULL pred, gt, out or workspace", who);
    const size_t need = partials_bytes(N, slots, H, W);
    if (workspace_bytes < need) return fail("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);

    const Geometry g = geometry(H, W);
    a = {};
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
    a.scale = pred_scale;
    a.zero = pred_zero;
    return 0;
}

// tile(): the launch of tile kernel k_tile; finish(): that of the finish kernel k_finish
template <int K, class TileLaunch, class FinishLaunch>
static int launch_pair(const char *who, Counters<K> &count, int k_tile, int k_finish, TileLaunch tile, FinishLaunch finish) {
    tile();
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: tile kernel launch: %s", who, hipGetErrorString(e));
    ++count.launches[k_tile];
    finish();
    e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: finish kernel launch: %s", who, hipGetErrorString(e));
    ++count.launches[k_finish];
    return 0;
}

}  // namespace sesrq_tile
