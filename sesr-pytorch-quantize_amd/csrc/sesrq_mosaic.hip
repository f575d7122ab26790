// libsesrq_mosaic.so: PSNR / SSIM of the Bayer mosaics of output frames on the device -- the reference's MFLAG 1 (nr) metric
// (include/sesrq_mosaic.h).  A library of its own: it links nothing of libsesrq.so or libsesrq_eval.so.
//
// One pass over the bytes, no mosaic frame in memory.  The walk, the finish and the checks of a call are sesrq_eval's, defined once in
// csrc/sesrq_eval_tile.h: tiles of BAND input columns x (RH + 6) input rows, every lane owns KC consecutive columns and walks down the
// tile's rows with running 7x7 box sums; here one wave per tile, since the mosaic has one channel.  Tile origins (multiples of OW and
// RH) and a lane's first column (a multiple of KC) are even, so column k of a lane in row r takes channel (r & 1) + (k & 1): a row
// reads the two planes r & 1 and (r & 1) + 1 and keeps the even columns of the first and the odd columns of the second.  The samples
// not selected are dropped straight after the load and enter no arithmetic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sesrq_eval_tile.h"
#include "sesrq_mosaic.h"
#include "sesrq_side.h"

namespace sesrq_mosaick {

using namespace sesrq_tile;
static_assert(SESRQ_MOSAIC_F32 == 0 && SESRQ_MOSAIC_I8 == 1, "tile_args takes pred_dtype as it is");
static_assert(OW % 2 == 0 && RH % 2 == 0 && KC % 2 == 0, "the parity of a lane's column k and of a tile's row must be that of k and of the row");

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

// pred: clip(pred) to [0, 1]; an int8 frame is first dequantised (dequant_clip01)
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
    for (int k = 0; k < KC; ++k) v[k] = col + k < W ? dequant_clip01(q[k], zero, scale) : 0.f;
}

template <typename T>
__global__ __launch_bounds__(64) void mosaic_tile(TileArgs a) {
    const int lane = threadIdx.x;
    const int tile = blockIdx.x, n = blockIdx.y, H = a.H, W = a.W;
    const Tile t = tile_of(a, tile, lane);
    const int col = t.col;
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
    tile_walk(t, row, sq_err, a.part + ((size_t)n * a.ntiles + tile) * 2);
}

// one block per frame: the single-channel case of the data_range-1 form
__global__ __launch_bounds__(FIN_THREADS) void mosaic_finish(const double *part, int ntiles, int H, int W, double *out) {
    frame_finish(part, ntiles, FIN_RGB, 1, H, W, out);
}

// ---------------------------------------------------------------------------------------------------------------------- host side
enum { K_F32, K_I8, K_FINISH, K_COUNT };
static const char *const kNames[K_COUNT] = {"mosaic_tile<f32>", "mosaic_tile<i8>", "mosaic_finish"};
static Counters<K_COUNT> g_count{kNames};

}  // namespace sesrq_mosaick

using namespace sesrq_mosaick;

extern "C" size_t sesrq_mosaic_workspace_bytes(int N, int H, int W) { return partials_bytes(N, 1, H, W); }

extern "C" int sesrq_mosaic_score(const sesrq_mosaic_desc *d, const void *pred, const float *gt, int N, int H, int W, double *out,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (!d) return fail("sesrq_mosaic: desc is NULL");
    TileArgs a = {};
    if (tile_args("sesrq_mosaic", d->pred_dtype, d->pred_scale, d->pred_zero, pred, nullptr, gt, N, 1, H, W, out, workspace, workspace_bytes, a))
        return 1;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(a.ntiles, N), block(64);
    const bool i8 = d->pred_dtype == SESRQ_MOSAIC_I8;
    return launch_pair(
        "sesrq_mosaic", g_count, i8 ? K_I8 : K_F32, K_FINISH,
        [&] {
            if (i8) mosaic_tile<int8_t><<<grid, block, 0, st>>>(a);
            else mosaic_tile<float><<<grid, block, 0, st>>>(a);
        },
        [&] { mosaic_finish<<<N, FIN_THREADS, 0, st>>>(a.part, a.ntiles, H, W, out); });
}

extern "C" int sesrq_mosaic_kernel_count(void) { return g_count.count(); }

extern "C" const char *sesrq_mosaic_kernel_name(int i) { return g_count.name(i); }

extern "C" long long sesrq_mosaic_kernel_launches(int i) { return g_count.get(i); }

extern "C" const char *sesrq_mosaic_last_error(void) { return g_err; }
