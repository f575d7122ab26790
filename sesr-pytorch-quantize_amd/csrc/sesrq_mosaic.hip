// libsesrq_mosaic.so: PSNR / SSIM of the Bayer mosaics of output frames on the device -- the reference's MFLAG 1 (nr) metric
// (include/sesrq_mosaic.h).  A library of its own: it links nothing of libsesrq.so or libsesrq_eval.so.
//
// One pass over the bytes, no mosaic frame in memory.  The walk is eval_tile's (csrc/sesrq_eval.hip, csrc/sesrq_eval_tile.h): tiles of
// BAND input columns x (RH + 6) input rows, every lane owns KC consecutive columns and walks down the tile's rows with running 7x7
// box sums; here one wave per tile, since the mosaic has one channel.  Tile origins (multiples of OW and RH) and a lane's first
// column (a multiple of KC) are even, so column k of a lane in row r takes channel (r & 1) + (k & 1): a row reads the two planes
// r & 1 and (r & 1) + 1 and keeps the even columns of the first and the odd columns of the second.  The samples not selected are
// dropped straight after the load and enter no arithmetic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_eval_tile.h"
#include "sesrq_mosaic.h"
#include "sesrq_side.h"

namespace sesrq_mosaick {

using namespace sesrq_tile;
static_assert(OW % 2 == 0 && RH % 2 == 0 && KC % 2 == 0, "the parity of a lane's column k and of a tile's row must be that of k and of the row");

struct TileArgs {
    const void *pred;
    const float *gt;
    double *part;        // [N][ntiles][2]
    int H, W, nbx, nby, ntiles, vec;
    float scale;
    int zero;
};

// The selected samples of a lane's four columns of one row: `a` is the row in plane (r & 1), `b` the row in the next plane; column
// col + k takes a for even k and b for odd k.  Zeros past the right edge, as load4.
__device__ inline void load_sel(const float *a, const float *b, int col, int W, bool vec, float v[KC]) {
    if (vec) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 ta = col < W ? *reinterpret_cast<const float4 *>(a + col) : z;
        const float4 tb = col < W ? *reinterpret_cast<const float4 *>(b + col) : z;
        v[0] = ta.x; v[1] = tb.y; v[2] = ta.z; v[3] = tb.w;
    } else {
#pragma unroll
        for (int k = 0; k < KC; ++k) v[k] = col + k < W ? ((k & 1) ? b : a)[col + k] : 0.f;
    }
}

// pred: clip(pred) to [0, 1]; an int8 frame is first dequantised exactly as sesrq_forward forms out_f: (q - zero_L) * scale_out in fp32
__device__ inline void load_pred_sel(const float *a, const float *b, int col, int W, bool vec, float, int, float v[KC]) {
    load_sel(a, b, col, W, vec, v);
#pragma unroll
    for (int k = 0; k < KC; ++k) v[k] = clip01(v[k]);
}

__device__ inline void load_pred_sel(const int8_t *a, const int8_t *b, int col, int W, bool vec, float scale, int zero, float v[KC]) {
    int q[KC];
    if (vec) {
        const int ta = col < W ? *reinterpret_cast<const int *>(a + col) : 0;
        const int tb = col < W ? *reinterpret_cast<const int *>(b + col) : 0;
#pragma unroll
        for (int k = 0; k < KC; ++k) q[k] = (int)(int8_t)(((k & 1) ? tb : ta) >> (8 * k));
    } else {
#pragma unroll
        for (int k = 0; k < KC; ++k) q[k] = col + k < W ? (int)((k & 1) ? b : a)[col + k] : 0;
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) v[k] = col + k < W ? clip01(__fmul_rn((float)(q[k] - zero), scale)) : 0.f;
}

template <typename T>
__global__ __launch_bounds__(64) void mosaic_tile(TileArgs a) {
    const int lane = threadIdx.x;
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
    const T *pred = static_cast<const T *>(a.pred) + (size_t)n * 3 * plane;
    const float *gt = a.gt + (size_t)n * 3 * plane;
    // the mosaic's row rr of pred (clipped) and of gt: planes rr & 1 and (rr & 1) + 1, never the third
    auto row = [&](int rr, float x[KC], float y[KC]) {
        const size_t off = (size_t)(rr & 1) * plane + (size_t)rr * W;
        load_pred_sel(pred + off, pred + off + plane, col, W, vec, a.scale, a.zero, x);
        load_sel(gt + off, gt + off + plane, col, W, vec, y);
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
        float x[KC], y[KC], xo[KC] = {0.f, 0.f, 0.f, 0.f}, yo[KC] = {0.f, 0.f, 0.f, 0.f};
        row(r, x, y);
        if (leave) row(r - (2 * PAD + 1), xo, yo);
        if (own_row) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const double d = (double)y[k] - (double)x[k];
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
        double *p = a.part + ((size_t)n * a.ntiles + tile) * 2;
        p[0] = sse;
        p[1] = ssim;
    }
}

// one block per frame: the frame's tile partials in a fixed order, then mse / psnr / ssim
__global__ __launch_bounds__(FIN_THREADS) void mosaic_finish(const double *part, int ntiles, int H, int W, double *out) {
    __shared__ double s_sse[FIN_THREADS], s_ssim[FIN_THREADS];
    const int n = blockIdx.x;
    frame_sum2(part + (size_t)n * ntiles * 2, ntiles, s_sse, s_ssim);
    if (threadIdx.x == 0) {
        const double px = (double)H * W;
        const double mse = s_sse[0] / px;
        out[3 * n + 0] = mse;
        out[3 * n + 1] = mse == 0.0 ? INFINITY : 10.0 * log10(1.0 / mse);
        out[3 * n + 2] = s_ssim[0] / ((double)(H - 2 * PAD) * (W - 2 * PAD));
    }
}

// ---------------------------------------------------------------------------------------------------------------------- host side
enum { K_F32, K_I8, K_FINISH, K_COUNT };
static const char *const kNames[K_COUNT] = {"mosaic_tile<f32>", "mosaic_tile<i8>", "mosaic_finish"};
static Counters<K_COUNT> g_count{kNames};

}  // namespace sesrq_mosaick

using namespace sesrq_mosaick;

extern "C" size_t sesrq_mosaic_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 2 * PAD + 1 || W < 2 * PAD + 1) return 0;
    return (size_t)N * geometry(H, W).ntiles * 2 * sizeof(double);
}

extern "C" int sesrq_mosaic_score(const sesrq_mosaic_desc *d, const void *pred, const float *gt, int N, int H, int W, double *out,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (!d) return fail("sesrq_mosaic: desc is NULL");
    if (d->pred_dtype != SESRQ_MOSAIC_F32 && d->pred_dtype != SESRQ_MOSAIC_I8)
        return fail("sesrq_mosaic: unknown pred_dtype %d", d->pred_dtype);
    if (d->pred_dtype == SESRQ_MOSAIC_I8 && !(d->pred_scale > 0.f && std::isfinite(d->pred_scale)))
        return fail("sesrq_mosaic: int8 prediction needs a positive finite pred_scale");
    if (d->pred_dtype == SESRQ_MOSAIC_I8 && (d->pred_zero < -128 || d->pred_zero > 127))
        return fail("sesrq_mosaic: pred_zero %d outside the int8 range", d->pred_zero);
    if (N < 1 || N > 65535) return fail("sesrq_mosaic: N = %d (1 ... 65535 frames)", N);
    if (H < 2 * PAD + 1 || W < 2 * PAD + 1)
        return fail("sesrq_mosaic: frame %dx%d is smaller than the 7x7 SSIM window", H, W);
    if (!pred || !gt || !out || !workspace) return fail("sesrq_mosaic: NULL pred, gt, out or workspace");
    const size_t need = sesrq_mosaic_workspace_bytes(N, H, W);
    if (workspace_bytes < need) return fail("sesrq_mosaic: workspace of %zu bytes, %zu needed", workspace_bytes, need);

    const Geometry g = geometry(H, W);
    const bool i8 = d->pred_dtype == SESRQ_MOSAIC_I8;
    TileArgs a;
    a.pred = pred;
    a.gt = gt;
    a.part = static_cast<double *>(workspace);
    a.H = H;
    a.W = W;
    a.nbx = g.nbx;
    a.nby = g.nby;
    a.ntiles = g.ntiles;
    a.vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(gt) % 16 == 0 && reinterpret_cast<uintptr_t>(pred) % (i8 ? 4 : 16) == 0;
    a.scale = d->pred_scale;
    a.zero = d->pred_zero;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(g.ntiles, N), block(64);
    if (i8) mosaic_tile<int8_t><<<grid, block, 0, st>>>(a);
    else mosaic_tile<float><<<grid, block, 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("sesrq_mosaic: tile kernel launch: %s", hipGetErrorString(e));
    ++g_count.launches[i8 ? K_I8 : K_F32];
    mosaic_finish<<<N, FIN_THREADS, 0, st>>>(a.part, g.ntiles, H, W, out);
    e = hipGetLastError();
    if (e != hipSuccess) return fail("sesrq_mosaic: finish kernel launch: %s", hipGetErrorString(e));
    ++g_count.launches[K_FINISH];
    return 0;
}

extern "C" int sesrq_mosaic_kernel_count(void) { return g_count.count(); }

extern "C" const char *sesrq_mosaic_kernel_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_mosaic_kernel_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_mosaic_last_error(void) { return g_err; }
