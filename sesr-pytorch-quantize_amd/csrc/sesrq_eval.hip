// libsesrq_eval.so: PSNR / SSIM of output frames on the device (include/sesrq_eval.h, include/sesrq_eval_anchor.h).  A library of its own: it links nothing of
// libsesrq.so and registers nothing in its instance table.
//
// One pass over the bytes.  A frame is cut into tiles of BAND input columns x (RH + 6) input rows, one block per tile and one wave per
// channel of it (the waves of a block read the same rows at about the same time); every lane owns
// KC consecutive columns and walks down the tile's rows.  Per row it loads its columns of pred and gt (clip, dequantisation and luma
// on chip), takes the three halo columns on each side from its neighbour lanes, and keeps the 7x7 box sums of the five SSIM moments
// (x, y, x^2, y^2, xy) of its own columns as running sums: row r enters, row r - 7 (re-read, a cache hit) leaves.  Nothing goes back
// to memory but two doubles per tile (sum of squared errors, sum of the SSIM map); a second launch adds them up in a fixed order.
// The walk, the finish and the checks of a call are defined once, in csrc/sesrq_eval_tile.h, for this library and libsesrq_mosaic.so;
// here are the wave-per-channel indexing, the row loads (anchored or not), the luma error of the x2 form and the form-specific refusals.
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

using namespace sesrq_tile;      // the tile geometry, the walk, the finish and the host path (csrc/sesrq_eval_tile.h)

// np.clip on the float64 luma: a NaN passes through, as clip01
__device__ inline double clip255(double x) { return x != x ? x : fmin(fmax(x, 0.0), 255.0); }

// pred: clip(pred) to [0, 1]; an int8 frame is first dequantised (dequant_clip01)
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
    for (int k = 0; k < KC; ++k) v[k] = col + k < W ? dequant_clip01(q[k], zero, scale) : 0.f;
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
    const Tile t = tile_of(a, tile, lane);
    const int col = t.col;
    const bool vec = a.vec != 0;
    const size_t plane = (size_t)H * W;
    const T *pred = static_cast<const T *>(a.pred) + (size_t)n * C * plane;
    const float *gt = a.gt + (size_t)n * C * plane;
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
    // gt first: the clip of pred then waits on both loads, not on one of them before the other is issued
    auto row = [&](int rr, float x[KC], float y[KC]) {
        load4(gt + c * plane + (size_t)rr * W, col, W, vec, y);
        pred_row(c, rr, x);
    };
    // SESRQ_EVAL_X2: the squared luma error needs all three channels of a pixel; the channel-0 wave forms it (the other two waves
    // read the same rows in the same block, so those bytes come from cache)
    auto err = [&](int r, const float x[KC], const float y[KC], double d2[KC]) {
        if constexpr (FORM != SESRQ_EVAL_X2) {
            return sq_err(r, x, y, d2);
        } else {
            if (c != 0) return false;
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
                d2[k] = d * d;
            }
            return true;
        }
    };
    tile_walk(t, row, err, a.part + (((size_t)n * a.ntiles + tile) * C + c) * 2);
}

static_assert(SESRQ_EVAL_F32 == 0 && SESRQ_EVAL_I8 == 1, "tile_args takes pred_dtype as it is");
static_assert(SESRQ_EVAL_RGB == FIN_RGB && SESRQ_EVAL_Y255 == FIN_Y255 && SESRQ_EVAL_X2 == FIN_X2, "frame_finish takes the form as it is");

// one block per frame: the frame's tile partials in a fixed order, then mse / psnr / ssim
__global__ __launch_bounds__(FIN_THREADS) void eval_finish(const double *part, int ntiles, int form, int C, int H, int W, double *out) {
    frame_finish(part, ntiles, form, C, H, W, out);
}

// ---------------------------------------------------------------------------------------------------------------------- host side
enum { K_F32_RGB, K_I8_RGB, K_F32_Y255, K_I8_Y255, K_F32_X2, K_FINISH, K_COUNT };
static const char *const kNames[K_COUNT] = {"eval_tile<f32,rgb>", "eval_tile<i8,rgb>", "eval_tile<f32,y255>",
                                            "eval_tile<i8,y255>", "eval_tile<f32,x2>", "eval_finish"};
static Counters<K_COUNT> g_count{kNames};

static int expected_channels(int form) { return form == SESRQ_EVAL_Y255 ? 1 : 3; }

}  // namespace sesrq_evalk

using namespace sesrq_evalk;

extern "C" size_t sesrq_eval_workspace_bytes(int N, int C, int H, int W) { return partials_bytes(N, C, H, W); }

static int eval_launch(const sesrq_eval_desc *d, const void *pred, const float *anchor, const float *gt, int N, int C, int H, int W,
                       double *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!d) return fail("sesrq_eval: desc is NULL");
    if (d->form < SESRQ_EVAL_RGB || d->form > SESRQ_EVAL_X2) return fail("sesrq_eval: unknown form %d", d->form);
    if (d->pred_dtype == SESRQ_EVAL_I8 && d->form == SESRQ_EVAL_X2)
        return fail("sesrq_eval: an int8 prediction cannot be scored in the x2 form (the anchor exists only in the fp32 output)");
    if (C != expected_channels(d->form))
        return fail("sesrq_eval: form %d scores %d-channel frames, got C = %d", d->form, expected_channels(d->form), C);
    TileArgs a = {};
    if (tile_args("sesrq_eval", d->pred_dtype, d->pred_scale, d->pred_zero, pred, anchor, gt, N, C, H, W, out, workspace, workspace_bytes, a))
        return 1;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(a.ntiles, N), block(64 * C);
    const bool i8 = d->pred_dtype == SESRQ_EVAL_I8;
    const int k = d->form == SESRQ_EVAL_RGB ? (i8 ? K_I8_RGB : K_F32_RGB) : d->form == SESRQ_EVAL_Y255 ? (i8 ? K_I8_Y255 : K_F32_Y255) : K_F32_X2;
    return launch_pair(
        "sesrq_eval", g_count, k, K_FINISH,
        [&] {
            switch (k) {
            case K_F32_RGB: eval_tile<float, SESRQ_EVAL_RGB><<<grid, block, 0, st>>>(a); break;
            case K_I8_RGB: eval_tile<int8_t, SESRQ_EVAL_RGB><<<grid, block, 0, st>>>(a); break;
            case K_F32_Y255: eval_tile<float, SESRQ_EVAL_Y255><<<grid, block, 0, st>>>(a); break;
            case K_I8_Y255: eval_tile<int8_t, SESRQ_EVAL_Y255><<<grid, block, 0, st>>>(a); break;
            default: eval_tile<float, SESRQ_EVAL_X2><<<grid, block, 0, st>>>(a);
            }
        },
        [&] { eval_finish<<<N, FIN_THREADS, 0, st>>>(a.part, a.ntiles, d->form, C, H, W, out); });
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
