// Included twice by sesrq_mfma.hip: SESRQ_KERNEL = mfma_h3_kernel with SESRQ_NARROW 0 (the 8-bit kernel, the text it always had) and mfma_h3_kernel_q with
// SESRQ_NARROW 1 (the width-aware flavour of SESRQ_ENGINE_MFMA_Q: activation range from the arguments, epilogues epi_*_q).  One text, two
// kernels of their own name: a shared body function changed the code of the 8-bit kernels (kernel arguments reached through a reference).
template <int MODE, int EPI>
__global__ __launch_bounds__(256) void SESRQ_KERNEL(const ConvArgs a) {
    constexpr bool NARROW = SESRQ_NARROW != 0;
    constexpr bool GENERAL = mode_general(MODE);
    constexpr int SW = H3_SW;
    constexpr int SH = h3_sh(MODE);
    constexpr int PW = GENERAL ? SW : 0;             // planar image: row pitch 4*68 = 272 dwords = 16 mod 64 banks
    __shared__ int4 buf0[SH * SW], buf1[SH * SW];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    kernarg_warm<ConvArgs>();
    const BlockXY bxy = xcd_block(a.inv_nx);
    const int x0 = bxy.x * MTW, n_img = blockIdx.z;
    const int4 *fr = a.afrag;
    constexpr bool BIASED = mode_biased(MODE);     // requant without v_cvt: sums carry + MAGIC_I (needs |s| < 2^22)
    int4 ac = fr[g];
    if constexpr (BIASED) { ac.x += MAGIC_I; ac.y += MAGIC_I; ac.z += MAGIC_I; ac.w += MAGIC_I; }
    v4i A[GENERAL ? 4 : 3];
#pragma unroll
    for (int f = 0; f < (GENERAL ? 4 : 3); ++f) A[f] = ld_frag(fr + 4 + f * 64 + l);
    v4i AR = {0, 0, 0, 0};
    if constexpr (MODE == HYB) AR = ld_frag(a.afrag2 + 4 + a.risky_pe * 64 + l);
    const float qlo = NARROW ? a.qlo : -128.f;
    const float zlo = a.relu ? fmaxf(a.z_next, qlo) : qlo;
    QRange qr = {};
    if constexpr (NARROW) qr = qrange(a);
    const int gx = x0 + 16 * w + n;
    auto compute = [&](const int4 *tile, int y0) __attribute__((always_inline)) {
        const RowIO io = make_rowio(a, n_img, y0, gx, g);
        if constexpr (!GENERAL) {
            const int col = 16 * w + n + g;
            const v4i zero = {0, 0, 0, 0};
            const v4i acc0 = {ac.x, ac.y, ac.z, ac.w};
            const int *t32 = reinterpret_cast<const int *>(tile);
            const int rbase = (g * SW + 16 * w + n) * 4 + a.risky_pe;      // HYB: word risky_pe of pixel (row g, col)
            v4i B0 = ld_frag(tile + col), B1 = ld_frag(tile + SW + col);
#pragma unroll
            for (int y4 = 0; y4 < MTH; y4 += 4) {
                int s4[4][4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const v4i B2 = ld_frag(tile + (y4 + r + 2) * SW + col);
                    v4i acc[MODE == HYB ? 2 : 1];
                    acc[0] = mfma(A[0], B0, acc0);
                    acc[0] = mfma(A[1], B1, acc[0]);
                    acc[0] = mfma(A[2], B2, acc[0]);
                    B0 = B1; B1 = B2;
                    if constexpr (MODE == HYB) {
                        const int o = rbase + (y4 + r) * SW * 4;
                        const v4i br = {t32[o], t32[o + 4], t32[o + 8], t32[o + 12]};
                        acc[1] = mfma(AR, br, zero);
                    }
                    finish_sums<MODE>(s4[r], acc, ac, a);
                }
                if constexpr (NARROW) emit_rows4_q<EPI, false, BIASED>(s4, a, io, y4, zlo, qr); else emit_rows4<EPI, false, BIASED>(s4, a, io, y4, zlo);
            }
        } else {
            const int col = 16 * w + n;
#pragma unroll 1
            for (int y4 = 0; y4 < MTH; y4 += 4) {
                int s4[4][4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int *row = reinterpret_cast<const int *>(tile) + (y4 + r + g) * (4 * PW) + col;   // lane group g = kernel row ky
                    const v4i zero = {0, 0, 0, 0};
                    v4i acc[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int *q = row + p * PW;                       // plane p: 4 horizontally adjacent pixels of PE p
                        const v4i b = {q[0], q[1], q[2], q[3]};
                        acc[p] = mfma(A[p], b, zero);
                    }
                    if constexpr (MODE == GEN_TAP) tap_sums<4>(acc, a, n_img, y0 + y4 + r, gx, g, 0);
                    finish_sums<MODE>(s4[r], acc, ac, a);
                }
                if constexpr (NARROW) emit_rows4_q<EPI, false, BIASED>(s4, a, io, y4, zlo, qr); else emit_rows4<EPI, false, BIASED>(s4, a, io, y4, zlo);
            }
        }
    };
#define SESRQ_COMPUTE(B) compute(B, y0);
    using Stage = StageNHWC16<SH, SW, 1, PW>;
    SESRQ_TILE_WALK(Stage, buf0, buf1, SESRQ_COMPUTE)
#undef SESRQ_COMPUTE
}
