// Included twice by sesrq_mfma.hip: SESRQ_KERNEL = mfma_h5_kernel with SESRQ_NARROW 0 (the 8-bit kernel, the text it always had) and mfma_h5_kernel_q with
// SESRQ_NARROW 1 (the width-aware flavour of SESRQ_ENGINE_MFMA_Q: activation range from the arguments, epilogues epi_*_q).  One text, two
// kernels of their own name: a shared body function changed the code of the 8-bit kernels (kernel arguments reached through a reference).
template <int MODE, int EPI, int FAST = 0, int NV = 4, int OUTF = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void SESRQ_KERNEL(const ConvArgs a) {
    constexpr bool NARROW = SESRQ_NARROW != 0;
    constexpr bool GENERAL = mode_general(MODE);
    constexpr int SW = H5_SW;
    constexpr int SH = H5_SH;
    // per-PE (general) kernels: column-major PE-planar image [PE][col][row] (StageNHWC16, CP > 0), column pitch CS = 12 dwords (the tile's
    // rows), plane pitch CP = 72 columns.  A lane's operand per PE and K-chunk = two vertical pixel pairs that start on EVEN tile rows
    // (h5_pair, sesrq_common.h): 8-byte-aligned LDS accesses straight into the four operand registers -- K-chunk 0 one ds_read2_b64 of four
    // consecutive rows, K-chunk 1 two ds_read_b64 (round 3: four ds_read2_b32 of pairs of any alignment, 1.75 x the LDS cycles).  That needs
    // output rows of one parity per wave: wave w works on rows (w & 1) + 2t, t = 0..3, of TWO 16-column groups (w >> 1), with the A
    // fragments of its parity.  All 4 PEs x 4 rows of a column group are reached by immediate offsets from three lane-constant addresses;
    // the planes are more than a ds_read2_b64's offset range apart, so hipcc cannot pair reads of different PEs (it did, and then moved
    // 192 registers per tile into operand order).  Banks: h5_pair; the staging writes (dword stores 12 apart) are 4-way.
    constexpr int CS = GENERAL ? SH : 0;
    constexpr int CP = SW * CS;
    static_assert(!GENERAL || (CS % 8 == 4 && CP * 4 > 2040), "aligned pairs / bank rule / no ds_read2 across PE planes");
    constexpr int SHB = SH + (MODE == HYB ? 1 : 0);      // hybrid: the risky PE's pairs reach one row below the tile (zero weights)
    __shared__ int4 buf0[GENERAL ? CP : SHB * SW], buf1[GENERAL ? CP : SHB * SW];      // general: 4 planes of CP dwords
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    kernarg_warm<ConvArgs>();
    const BlockXY bxy = xcd_block(a.inv_nx);
    const int x0 = bxy.x * MTW, n_img = blockIdx.z;
    using Stage = StageNHWC16<SH, SW, 2, 0, CP, CS>;
    SESRQ_TILE_WALK_BEGIN(MTH, Stage)
    const int4 *fr = a.afrag;
    constexpr bool BIASED = mode_biased(MODE);     // requant without v_cvt: sums carry + MAGIC_I (needs |s| < 2^22)
    int4 ac = fr[g];
    if constexpr (BIASED) { ac.x += MAGIC_I; ac.y += MAGIC_I; ac.z += MAGIC_I; ac.w += MAGIC_I; }
    const float qlo = NARROW ? a.qlo : -128.f;
    const float zlo = a.relu ? fmaxf(EPI == EPI_LAST ? a.z_out : a.z_next, qlo) : qlo;
    QRange qr = {};
    if constexpr (NARROW) qr = qrange(a);
    const int gx = x0 + 16 * w + n;
    // merged: K-chunks 0..4 = kernel row f, lane group g = kx 0..3;  5 = column 4, lane group g = ky 0..3;  6 = tap (4,4)
    // general, per PE p two K-chunks of two vertical pixel pairs per lane group (h5_pair; pack_mfma_frags, MFMA_H5), one set per row parity
    constexpr int NF = GENERAL ? 8 : 7;
    // general: this wave's row parity and pair of 16-column groups -- wave-uniform, and TOLD so (readfirstlane): everything derived from
    // them (row offsets of the stores, column bases) is then scalar arithmetic instead of VALU + v_readfirstlane per row
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const int par = GENERAL ? (wu & 1) : 0, cg = wu >> 1;
    v4i A[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) A[f] = ld_frag(fr + 4 + (par * 8 + f) * 64 + l);
    // per-PE chains (general, and the risky PE's chain of the hybrid mode); must match pack_mfma_frags (MFMA_H5 general)
    int pcol[2][2], prow[2][2];                         // [chunk][pair]: column and first row of lane group g's pixel pair
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < 2; ++q) h5_pair(c, g, q, pcol[c][q], prow[c][q]);
    LastStore ls, ls1;                                  // general: one per column group of the wave
    if constexpr (EPI == EPI_LAST) {
        if constexpr (GENERAL) { ls.template init<NV, FAST % 10>(a, n_img, g, x0 + 32 * cg + n); ls1.template init<NV, FAST % 10>(a, n_img, g, x0 + 32 * cg + 16 + n); }
        else ls.template init<NV, FAST % 10>(a, n_img, g, gx);
    }
    v4i AR[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if constexpr (MODE == HYB) {
        AR[0] = ld_frag(a.afrag2 + 4 + (0 * 4 + a.risky_pe) * 64 + l);
        AR[1] = ld_frag(a.afrag2 + 4 + (1 * 4 + a.risky_pe) * 64 + l);
    }
    // lane-constant byte offsets of the four pixel pairs inside a tile for both column groups, computed ONCE (pinned: hipcc re-derived them
    // -- 8 v_mul_lo + a dozen adds -- at the top of every tile)
    unsigned pboff[2][2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                pboff[j][c][q] = GENERAL ? (unsigned)(((32 * cg + 16 * j + n + pcol[c][q]) * CS + prow[c][q]) * 4) : 0u;      // [0][1] unused: pair 1 of K-chunk 0 = pair 0 + 2 rows
                asm volatile("" : "+v"(pboff[j][c][q]));
            }
    auto compute = [&](const int4 *tile, int y0) __attribute__((always_inline)) {
        RowIO io;
        if constexpr (EPI != EPI_LAST) io = make_rowio(a, n_img, y0, gx, g);
        if constexpr (!GENERAL) {
            const int col = 16 * w + n + g, colc = 16 * w + n + 4;
            const v4i zero = {0, 0, 0, 0};
            const v4i acc0 = {ac.x, ac.y, ac.z, ac.w};
            const int *t32 = reinterpret_cast<const int *>(tile);
            const int cb = (16 * w + n) * 4 + a.risky_pe;       // HYB: word risky_pe of column (16w + n), row 0
            v4i B[5];
#pragma unroll
            for (int r = 0; r < 4; ++r) B[r] = ld_frag(tile + r * SW + col);
#pragma unroll
            for (int y4 = 0; y4 < MTH; y4 += 4) {
                int s4[4][4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int y = y4 + r;
                    float x01 = 0.f, x2 = 0.f;
                    if constexpr (OUTF == 2) ls.fetch_anchor(a, y0 + y, x01, x2);
                    B[(y + 4) % 5] = ld_frag(tile + (y + 4) * SW + col);
                    const v4i C5 = ld_frag(tile + (y + g) * SW + colc);      // column 4: lane group g = kernel row g
                    const v4i C6 = ld_frag(tile + (y + 4) * SW + colc);      // tap (4,4)
                    v4i acc[MODE == HYB ? 2 : 1];
                    acc[0] = acc0;
#pragma unroll
                    for (int ky = 0; ky < 5; ++ky) acc[0] = mfma(A[ky], B[(y + ky) % 5], acc[0]);
                    acc[0] = mfma(A[5], C5, acc[0]);
                    acc[0] = mfma(A[6], C6, acc[0]);
                    if constexpr (MODE == HYB) {
                        int o[2][2];                                   // word risky_pe of the first pixel of pair [chunk][pair]
#pragma unroll
                        for (int c = 0; c < 2; ++c)
#pragma unroll
                            for (int q = 0; q < 2; ++q) o[c][q] = cb + ((y + prow[c][q]) * SW + pcol[c][q]) * 4;
                        const v4i b0 = {t32[o[0][0]], t32[o[0][0] + SW * 4], t32[o[0][1]], t32[o[0][1] + SW * 4]};
                        const v4i b1 = {t32[o[1][0]], t32[o[1][0] + SW * 4], t32[o[1][1]], t32[o[1][1] + SW * 4]};
                        acc[1] = mfma(AR[0], b0, zero);
                        acc[1] = mfma(AR[1], b1, acc[1]);
                    }
                    finish_sums<MODE, NV>(s4[r], acc, ac, a);
                    if constexpr (EPI == EPI_LAST) {
                        // a row below the frame is dropped by its offsets (FAST: the scalar one, else the lanes'), not by a
                        // branch: the four rows stay one basic block
                        ls.template store<BIASED, FAST, NV, OUTF, NARROW>(s4[r], a, y0 + y, zlo, y0 + y < a.H, x01, x2);
                    }
                }
                if constexpr (EPI != EPI_LAST) if constexpr (NARROW) emit_rows4_q<EPI, false, BIASED>(s4, a, io, y4, zlo, qr); else emit_rows4<EPI, false, BIASED>(s4, a, io, y4, zlo);
            }
        } else {
            typedef int v2ia __attribute__((ext_vector_type(2)));                  // two adjacent dwords, 8-byte aligned: ds_read_b64
            typedef const v2ia __attribute__((address_space(3))) *lds_pair_t;
            const unsigned tb = (unsigned)(size_t)(const __attribute__((address_space(3))) void *)tile;     // LDS byte address of the tile
#pragma unroll
            for (int j = 0; j < 2; ++j) {                                // the wave's two 16-column groups
                const int gxj = x0 + 32 * cg + 16 * j + n;
                // LDS byte addresses (row 0, PE 0) of the four pairs.  K-chunk 0's second pair is the first one two rows down, but it gets an
                // address register of its own: reads off ONE register 8 bytes apart become a ds_read2_b64, which the LDS serves 16 lanes at a
                // time over 32 banks (column pitch 12: two-way conflicts, half the rate) where a ds_read_b64 goes 32 lanes at a time over 64
                unsigned pa0 = tb + pboff[j][0][0], pa1 = tb + pboff[j][0][0] + 8, p0 = tb + pboff[j][1][0], p1 = tb + pboff[j][1][1];
                int s4[4][4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {                            // tile rows par + 2t
                    const int gy = y0 + par + 2 * t;
                    float x01 = 0.f, x2 = 0.f;
                    if constexpr (OUTF == 2) { if (j == 0) ls.fetch_anchor(a, gy, x01, x2); else ls1.fetch_anchor(a, gy, x01, x2); }
                    const v4i zero = {0, 0, 0, 0};
                    v4i acc[4];
                    // a pair of row t + 1 is a pair of row t in another operand slot: hide the relation between the rows' addresses from the
                    // compiler, which otherwise keeps the pair and MOVES it into place (the reads are not what bounds this loop, vector issue is)
                    asm("" : "+v"(pa0), "+v"(pa1), "+v"(p0), "+v"(p1));
                    v4i b0[4], b1[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int o = 4 * (2 * t + p * CP);
                        const v2ia a0 = *(lds_pair_t)(size_t)(pa0 + o), a1 = *(lds_pair_t)(size_t)(pa1 + o);
                        const v2ia c0 = *(lds_pair_t)(size_t)(p0 + o), c1 = *(lds_pair_t)(size_t)(p1 + o);
                        b0[p] = (v4i){a0[0], a0[1], a1[0], a1[1]};
                        b1[p] = (v4i){c0[0], c0[1], c1[0], c1[1]};
                    }
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        acc[p] = mfma(A[p], b0[p], zero);
                        acc[p] = mfma(A[4 + p], b1[p], acc[p]);
                    }
                    if constexpr (MODE == GEN_TAP) tap_sums<NV>(acc, a, n_img, gy, gxj, g, EPI == EPI_LAST ? NV : 0);
                    finish_sums<MODE, NV>(s4[t], acc, ac, a);
                    if constexpr (EPI == EPI_LAST) {
                        // a row below the frame is dropped by its offsets (FAST: the scalar one, else the lanes'), not by a branch
                        if (j == 0) ls.template store<BIASED, FAST, NV, OUTF, NARROW>(s4[t], a, gy, zlo, gy < a.H, x01, x2);
                        else ls1.template store<BIASED, FAST, NV, OUTF, NARROW>(s4[t], a, gy, zlo, gy < a.H, x01, x2);
                    }
                }
                if constexpr (EPI != EPI_LAST) {
                    // hidden 5x5 layer: the wave's four rows are two apart: lane (n, r' = g) stores pixel row y0 + par + 2g
                    RowIO ioj = make_rowio(a, n_img, y0, gxj, g);
                    ioj.voff = (gxj < a.W) ? ((y0 + par + 2 * g) * a.W + gxj) * 16 : (int)0x80000000;
                    if constexpr (NARROW) emit_rows4_q<EPI, false, BIASED>(s4, a, ioj, 0, zlo, qr); else emit_rows4<EPI, false, BIASED>(s4, a, ioj, 0, zlo);
                }
            }
        }
    };
#define SESRQ_COMPUTE(B) compute(B, y0);
    SESRQ_TILE_WALK_REST(MTH, buf0, buf1, SESRQ_COMPUTE)
#undef SESRQ_COMPUTE
}
