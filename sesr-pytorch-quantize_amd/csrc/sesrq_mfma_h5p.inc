// Included twice by sesrq_mfma.hip: SESRQ_KERNEL = mfma_h5p_kernel with SESRQ_NARROW 0 (the 8-bit kernel, the text it always had) and mfma_h5p_kernel_q with
// SESRQ_NARROW 1 (the width-aware flavour of SESRQ_ENGINE_MFMA_Q: activation range from the arguments, epilogues epi_*_q).  One text, two
// kernels of their own name: a shared body function changed the code of the 8-bit kernels (kernel arguments reached through a reference).
template <int MODE>
__global__ __launch_bounds__(256) void SESRQ_KERNEL(const ConvArgs a) {
    constexpr bool NARROW = SESRQ_NARROW != 0;
    constexpr int SW = H5_SW;
    constexpr int SH = H5_SH;
    __shared__ int4 buf0[SH * SW], buf1[SH * SW];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    kernarg_warm<ConvArgs>();
    const BlockXY bxy = xcd_block(a.inv_nx);
    const int x0 = bxy.x * MTW, n_img = blockIdx.z;
    const int4 *fr = a.afrag;
    constexpr bool BIASED = mode_biased(MODE);
    int4 ac = fr[0];
    if constexpr (BIASED) { ac.x += MAGIC_I; ac.y += MAGIC_I; ac.z += MAGIC_I; ac.w += MAGIC_I; }
    const float qlo = NARROW ? a.qlo : -128.f;
    const float zlo = a.relu ? fmaxf(a.z_out, qlo) : qlo;
    const int gx = x0 + 16 * w + n;
    v4i A[7];
#pragma unroll
    for (int f = 0; f < 7; ++f) A[f] = ld_frag(fr + 4 + f * 64 + l);
    LastStore ls;
    ls.init(a, n_img, 0, gx, g);
    auto compute = [&](const int4 *tile, int y0) __attribute__((always_inline)) {
        const int col = 16 * w + n + g, colc = 16 * w + n + 4;
        const v4i zero = {0, 0, 0, 0};
        // merged: nothing can clamp -> the add constant rides in PE 0's accumulator rows
        const v4i acc0 = (MODE == MERGED && g == 0) ? (v4i){ac.x, ac.y, ac.z, ac.w} : zero;
        v4i B[5];
#pragma unroll
        for (int r = 0; r < 4; ++r) B[r] = ld_frag(tile + r * SW + col);
#pragma unroll
        for (int y4 = 0; y4 < MTH; y4 += 4) {
            unsigned s[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = y4 + r;
                B[(y + 4) % 5] = ld_frag(tile + (y + 4) * SW + col);
                const v4i C5 = ld_frag(tile + (y + g) * SW + colc);
                const v4i C6 = ld_frag(tile + (y + 4) * SW + colc);
                v4i acc = acc0;
#pragma unroll
                for (int ky = 0; ky < 5; ++ky) acc = mfma(A[ky], B[(y + ky) % 5], acc);
                acc = mfma(A[5], C5, acc);
                acc = mfma(A[6], C6, acc);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (MODE == MERGED) s[r][i] = (unsigned)acc[i];
                    else if constexpr (MODE == GEN_ANY) s[r][i] = (unsigned)clampi3(acc[i], a.acc_lo, a.acc_hi);
                    else s[r][i] = (unsigned)clampi3(acc[i], -131072, 131071);
                }
            }
            int t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // lane halves trade rows {0,1} against {2,3}: u0 = row 0 | row 2, u1 = row 1 | row 3 (PE g + PE g^2)
                v2u x = __builtin_amdgcn_permlane32_swap(s[0][i], s[2][i], false, false);
                const unsigned u0 = x[0] + x[1];
                x = __builtin_amdgcn_permlane32_swap(s[1][i], s[3][i], false, false);
                const unsigned u1 = x[0] + x[1];
                // odd lane groups trade with even ones: lane group r ends up with row r, all four PEs
                x = __builtin_amdgcn_permlane16_swap(u0, u1, false, false);
                t[i] = (int)(x[0] + x[1]);
            }
            int sf[4];
            const int acv[4] = {ac.x, ac.y, ac.z, ac.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (MODE == MERGED) sf[i] = t[i];
                else if constexpr (MODE == GEN_ANY) sf[i] = clampi3(t[i], a.add_lo, a.add_hi) + acv[i];
                else sf[i] = clampi3(t[i], -524288, 524287) + acv[i];
            }
            if (y0 + y4 < a.H) ls.template store<BIASED, 0, 4, 0, NARROW>(sf, a, y0 + y4, zlo, y0 + y4 + g < a.H);
        }
    };
#define SESRQ_COMPUTE(B) compute(B, y0);
    using Stage = StageNHWC16<SH, SW, 2>;
    SESRQ_TILE_WALK(Stage, buf0, buf1, SESRQ_COMPUTE)
#undef SESRQ_COMPUTE
}
