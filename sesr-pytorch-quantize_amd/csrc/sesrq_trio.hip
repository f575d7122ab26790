// sesrq fused hidden trio: three consecutive 3x3 16->16 layers (the reference's conv 1..3, the last one with
// the long-residual merge, myQL/quan_func.py:244-280) in ONE launch.  The two intermediate activation tensors
// never leave the CU: 2 x 66 MB of HBM traffic per 1080p frame and two synchronised kernel starts less than the
// per-layer kernels (sesrq_mfma.hip), and no global staging / transpose / 16-byte store work for the two inner
// layers (their MFMA results go to LDS as they come out: lane (n, g) owns word g of pixel n).
//
// Geometry: a workgroup (4 waves = 4 groups of 16 columns) owns a strip of 64 COMPUTED columns of which
// TV = 60 are valid outputs (a 3x3 layer eats one column per side; the two outermost computed columns of the
// inner layers are never read by a valid output) and walks down it in steps of TH = 8 rows.  Three LDS
// windows of TH + 2 rows each (IN, A, B; row pitch 66 pixels: columns -1 .. 64) hold
//      IN: input rows  Y+1 .. Y+10        A: layer-a rows Y .. Y+9        B: layer-b rows Y-1 .. Y+8
// while the step produces output rows Y .. Y+7: every layer lags the one before by one row, so all three
// phases have the same access pattern (window position 2+i from positions i .. i+2) and NO row is computed
// twice inside a chunk; between steps the last two rows of each window move to its top (132 pixels each).
// A chunk starts cold with a partial step (4 rows of layer a, 2 rows of layer b, nothing stored).
// Pixels outside the frame are the NEXT layer's pad value zc = max(zero, -128), exactly as the per-layer
// kernels pad (myQL/quan_func.py:351-356): the inner epilogues select the pad word there.
// Only the merged accumulation mode (load-time proof: no 18-/20-bit clamp can fire) is fused; anything else
// runs on the per-layer kernels.
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <type_traits>

#include "sesrq_mfma_common.h"

namespace sesrq {

// Diagnostic build only (-DSESRQ_STAMPS, make stamps): EVERY wave of every workgroup records s_memtime at the phase boundaries of its
// first 12 full steps into a device array no other code reads (tools/trio_stamps.py) -- where a step's cycles go, barrier waits included.
#ifdef SESRQ_STAMPS
__device__ unsigned long long g_trio_stamps[1024 * 4 * 12 * 8];
#define TSTAMP(k)                                                                                                         \
    if (l == 0 && stamp_step < 12) {                                                                                      \
        const unsigned wg_ = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;                              \
        if (wg_ < 1024) g_trio_stamps[((wg_ * 4 + w) * 12 + stamp_step) * 8 + (k)] = __builtin_amdgcn_s_memtime();          \
    }
#else
#define TSTAMP(k)
#endif

constexpr int TV = 60;            // valid output columns per strip
constexpr int TH = 8;             // rows per step
constexpr int TP = 66;            // LDS row pitch (pixels): computed columns -1 .. 64
constexpr int TR = TH + 2;        // rows per LDS window
constexpr int OOB = (int)0x80000000;
constexpr int TRIO_WIN = TR * TP + 2;      // pixels per LDS window (+ 2: lane group 3 over-reads one pixel)
constexpr int TRIO_LUT_I4 = 32;               // 512-byte table of the residual merge behind the three windows
constexpr int TRIO_LDS_BYTES = 3 * TRIO_WIN * 16;      // dynamic part (the windows); the table is static LDS, TRIO_LUT_I4 * 16 bytes more

struct TrioStage {
    static constexpr int NIT = 3;         // 660 pixels (cold: 10 rows) or 528 (steady: 8 rows) over 256 threads
    v4u v[NIT];
    bool ok[NIT];
    int voff[NIT], ty[NIT], tx[NIT];
    int voff2s;                           // steady form of iteration 2: rows 8, 9 are not loaded
    __amdgpu_buffer_rsrc_t rs;
    int row_bytes;
    __device__ __forceinline__ void init(const TrioArgs &a, int n_img, int x0, int tid) {
        const size_t img = (size_t)a.H * a.W * 16;
        rs = __builtin_amdgcn_make_buffer_rsrc((char *)const_cast<void *>(a.in) + (size_t)n_img * img, 0, (int)img, 0x00020000);
        row_bytes = a.W * 16;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * 256;
            ty[it] = i / TP;
            tx[it] = i - ty[it] * TP;
            const int gx = x0 - 1 + tx[it];
            const bool okx = (gx >= 0) & (gx < a.W) & (i < TR * TP);
            voff[it] = okx ? (ty[it] * a.W + gx) * 16 : OOB;
            if (!okx) ty[it] = NO_ROW;          // never a valid row -> pad
        }
        voff2s = (ty[2] < TH) ? voff[2] : OOB;
    }
    // rows [y, y + nrows) of the frame.  COLD: any y (lane-form offsets, rows above the frame pushed out of range);
    // steady: y > 0, one scalar offset per step (gfx950 range-checks voffset + soffset)
    template <bool COLD>
    __device__ __forceinline__ void load(const TrioArgs &a, int y) {
        constexpr int nrows = COLD ? TR : TH;
        const int lo = -y, hi = min(a.H - y, nrows);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            ok[it] = (ty[it] >= lo) & (ty[it] < hi);
            if constexpr (COLD) v[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, ok[it] ? voff[it] + y * row_bytes : OOB, 0, 0);
            else v[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, it == 2 ? voff2s : voff[it], y * row_bytes, 0);
        }
    }
    template <bool COLD>
    __device__ __forceinline__ void store(int4 *win, int pad_word, int tid) const {
        constexpr int nrows = COLD ? TR : TH, pos0 = COLD ? 0 : 2;
        const unsigned pw = (unsigned)pad_word;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * 256;
            const v4u pad = {pw, pw, pw, pw};
            const v4u t = ok[it] ? v[it] : pad;
            if (i < nrows * TP) win[pos0 * TP + i] = make_int4((int)t[0], (int)t[1], (int)t[2], (int)t[3]);
        }
    }
};

struct TrioEpiC {           // the field names the shared epilogues read
    float Mf, sh, z_next, Mres, shres, z_merge, Md, Cd;
};

// U8, a bit mask: 1 = every zero point of the three epilogues is -128 (the launch checks): round_pack_u8 (sesrq_mfma_common.h);
// 2 = the requants of layers a and b passed prove_direct_requant: the one-fma form of epi_mid; 4 = so did the third layer's
// (residual merge: its first requant, into the fixed -128 domain of ic); 8 = the residual operand IS the trio's input tensor (the
// 5-conv nets: layer 0's output, zero[1] == -128): it is read out of the input window in LDS, already in compute layout (word g of pixel
// n), instead of being loaded again from global memory and transposed (2 loads + 8 v_permlane*_swap per step, and 33 MB per 1080p
// frame off the L2 / MALL).  Instances: 0, 1, 3, 7, 15
// The kernel's text is sesrq_trio_kernel.inc, included twice: the 8-bit kernel and its width-aware flavour mfma_trio_kernel_q
// (SESRQ_ENGINE_MFMA_Q at b < 8): the generic epilogues with the width's range (TrioArgsQ), U8 = 0 only
struct TrioArgsQ : TrioArgs {
    float qlo, qhi, qhalf, qspan;      // ConvArgs::qlo .. qspan
};
#define SESRQ_KERNEL mfma_trio_kernel
#define SESRQ_NARROW 0
#define SESRQ_TRIO_ARGS TrioArgs
#define SESRQ_TRIO_TEMPLATE template <int EPI_C, int U8>
#include "sesrq_trio_kernel.inc"
#undef SESRQ_KERNEL
#undef SESRQ_NARROW
#undef SESRQ_TRIO_ARGS
#undef SESRQ_TRIO_TEMPLATE
#define SESRQ_KERNEL mfma_trio_kernel_q
#define SESRQ_NARROW 1
#define SESRQ_TRIO_ARGS TrioArgsQ
#define SESRQ_TRIO_TEMPLATE template <int EPI_C, int U8 = 0>      // generic epilogues only: the reduced forms are proven for the 8-bit clamp
#include "sesrq_trio_kernel.inc"
#undef SESRQ_KERNEL
#undef SESRQ_NARROW
#undef SESRQ_TRIO_ARGS
#undef SESRQ_TRIO_TEMPLATE

// Launch geometry: the chip is filled EVENLY.  A workgroup lives for tens of microseconds here, so a compute unit that holds
// one workgroup more than its neighbours sets the kernel time while the others idle (measured: 864 workgroups on 1024 slots,
// SQ busy 1.47 x the average wave lifetime).  The dynamic LDS size is padded so that exactly `occ` workgroups fit a CU, and a
// strip is cut into floor(occ * CUs / (strips * N)) runs whose lengths differ by at most one step.
template <auto KERN, int REG = REG_MAIN, class ARGS = TrioArgs>
static void launch_trio_k(ARGS a, hipStream_t st) {
    // 4 workgroups per CU: the LDS size a plain launch accepts and the kernel's registers allow (3 and 5 measured slower, rounds 2-3)
    constexpr int occ = 4;
    const int lds = std::max(TRIO_LDS_BYTES, ((160 * 1024 / occ) & ~1023) - TRIO_LUT_I4 * 16);      // static + dynamic: exactly occ workgroups per 160 KiB
    const int strips = (a.W + TV - 1) / TV, steps = (a.H + TH - 1) / TH;
    const RunCut c = cut_runs(strips, steps, a.N, a.wg_budget, occ * device_cu_count());      // a run is at least one full step on average
    a.chunk_steps = c.chunk; a.inv_nx = c.inv_nx;
    a.run_unit = (steps < 3 * c.k) ? TH / 2 : TH;                         // short runs (< 3 steps) are cut in half-step units,
    const int units = (a.H + a.run_unit - 1) / a.run_unit;                // ... the same k runs (whole steps: c.run_q, c.run_rem)
    a.run_q = units / c.k; a.run_rem = units % c.k;
    dim3 grid(strips, c.k, a.N);
    launch_kernel<KERN, REG>(grid, dim3(256), (unsigned)lds, st, a);
}

#ifdef SESRQ_STAMPS
extern "C" int sesrq_debug_fetch_trio_stamps(void *host, size_t bytes) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_trio_stamps), std::min(bytes, sizeof(g_trio_stamps)), 0, hipMemcpyDeviceToHost);
}
#endif

// The instances the library builds: epilogue mode U8 = 0 / 1 / 3 / 7 (select_trio) for a plain and for the residual-merging trio, 15 for
// the latter only
constexpr bool trio_built(int epi, int u8) {
    return (epi == EPI_MID || epi == EPI_PRERES) && (u8 == 0 || u8 == 1 || u8 == 3 || u8 == 7 || (u8 == 15 && epi == EPI_PRERES));
}
// Which epilogue mode a launch runs: the reduced forms whose precondition holds AND sesrq_options.reduced_forms (TrioArgs::allow) admits,
// each on top of the one before.  1 = the cvt_pk_u8 epilogues, 2 = one-fma requants of layers a and b, 4 = of the third layer, 8 = the
// residual operand out of the input window
static int select_trio(const TrioArgs &a, int epi_c) {
    // zero points all -128 (and ReLU's clamp therefore the int8 clamp): the cvt_pk_u8 epilogues
    bool u8 = a.l[0].z_next == -128.f && a.l[1].z_next == -128.f && a.l[0].zlo == -128.f && a.l[1].zlo == -128.f;
    if (epi_c == EPI_PRERES) u8 = u8 && a.z_merge == -128.f;
    else u8 = u8 && a.l[2].z_next == -128.f && a.l[2].zlo == -128.f;
    u8 = u8 && (a.allow & 1);
    const bool ab = u8 && (a.allow & 2) && a.l[0].direct && a.l[1].direct, abc = ab && (a.allow & 4) && a.l[2].direct;      // one-fma requants (proof per layer)
    if (abc && epi_c == EPI_PRERES && a.rc_in == a.in && (a.allow & 8)) return 15;
    return abc ? 7 : (ab ? 3 : (u8 ? 1 : 0));
}

int launch_trio(const TrioArgs &a, int epi_c, hipStream_t st) {
    if (!frame_fits_32bit_offsets(a.H, a.W)) { set_error("trio: frame too large for 32-bit buffer offsets (H*W must stay below 2^24 pixels)"); return 1; }
    const bool built = pick([&](auto E, auto U) {
        if constexpr (trio_built(E, U)) return launch_trio_k<mfma_trio_kernel<E, U>>(a, st), true; else return false;
    }, Of<EPI_MID, EPI_PRERES>{}, epi_c, Of<0, 1, 3, 7, 15>{}, select_trio(a, epi_c));
    // select_trio returns built modes only, so the one way to get here is an epi_c outside the list
    if (!built) { set_error("trio: the third layer must be a hidden layer"); return 1; }
    return check_launch("trio");
}

// a trio of a net of width b < 8 (SESRQ_ENGINE_MFMA_Q): the plain and the residual-merging form, generic epilogues
int launch_trio_q(const TrioArgs &a, const ConvArgs &width, int epi_c, hipStream_t st) {
    if (!frame_fits_32bit_offsets(a.H, a.W)) { set_error("trio: frame too large for 32-bit buffer offsets (H*W must stay below 2^24 pixels)"); return 1; }
    TrioArgsQ q;
    static_cast<TrioArgs &>(q) = a;
    q.qlo = width.qlo; q.qhi = width.qhi; q.qhalf = width.qhalf; q.qspan = width.qspan;
    const bool built = pick([&](auto E) { return launch_trio_k<mfma_trio_kernel_q<E>, REG_NARROW, TrioArgsQ>(q, st), true; }, Of<EPI_MID, EPI_PRERES>{}, epi_c);
    if (!built) { set_error("trio: the third layer must be a hidden layer"); return 1; }
    return check_launch("trio");
}

}  // namespace sesrq
