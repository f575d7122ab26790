// The row-window core of the metric kernels (csrc/sesrq_eval.hip, csrc/sesrq_mosaic.hip): the tile geometry, the loads of a lane's four
// columns, np.clip's clip, the lane-shuffled halo, the five SSIM moments, the running 7x7 box sums, the SSIM quotient and the two
// fixed-order sums.  Device code and the geometry only; each library compiles its own copy (they share no symbol), with
// -ffp-contract=off: one text, the same expressions in the same order, so a single-channel frame scores to the same bits in either
// library (tests/test_mosaic_quality.py compares them).
//
// A tile is BAND input columns x (RH + 6) input rows, walked by one wave: lane l owns the KC columns c0 + KC l ... and keeps, per
// column, the box sums of the moments (x, y, x^2, y^2, xy) in fp64; only the final quotient is fp32 (csrc/sesrq_eval.hip, "Accuracy").
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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

}  // namespace sesrq_tile
