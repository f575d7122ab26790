// sesrq C ABI, part 1 of 4: bundle validation + weight repacking (sesrq_create / sesrq_destroy), the error channel.
// The other parts: sesrq_plan.hip (workspace layout + launch planner = the forwards), sesrq_submit.hip (sesrq_forward_many and its
// submission threads), sesrq_scalar.hip (host scalar code of the path); load-time proofs: sesrq_verify.hip; the kernel-instance
// registry: sesrq_registry.hip.  See include/sesrq.h for the contract.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>

#include "sesrq_common.h"

namespace sesrq {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

// Packed weights for the dot4 engine: [tap][ocp][4] dwords.
//  16-channel input (IN_DW = 4): dword p = bytes j=0..3 -> W[oc][p + 4j][tap]
//  first layer (IC <= 4, IN_DW = 1): input dword byte c = channel c
//     general: dword p = W[oc][p][tap] in byte p only (each channel is its own PE)
//     merged : dword 0 = all channels
static void pack_weights(const sesrq_layer_desc &d, int ocp, bool first, std::vector<int> &gen, std::vector<int> &mer) {
    const int k = d.k, taps = k * k;
    gen.assign((size_t)taps * ocp * 4, 0);
    mer.assign((size_t)taps * ocp * 4, 0);
    for (int t = 0; t < taps; ++t)
        for (int o = 0; o < d.oc; ++o)
            for (int c = 0; c < d.ic; ++c) {
                const int w = d.w[((size_t)o * d.ic + c) * taps + t];
                const size_t base = ((size_t)t * ocp + o) * 4;
                if (!first) {
                    const int p = c & 3, j = c >> 2;
                    gen[base + p] |= (w & 0xff) << (8 * j);
                    mer[base + p] |= (w & 0xff) << (8 * j);
                } else {
                    gen[base + c] |= (w & 0xff) << (8 * c);
                    mer[base + 0] |= (w & 0xff) << (8 * c);
                }
            }
}

// PE-major order of 16 channels / accumulator rows: slot x holds channel (x >> 2) + 4 * (x & 3), so that a dword is one PE's four
static int pe_major(int x) { return (x >> 2) + 4 * (x & 3); }
// 5x5 merged chains (MFMA_H5 merged, MFMA_H5P): K-chunks 0..4 = kernel row f, lane group g = kx 0..3 (the row operands are re-used
// across rows); chunk 5: column 4, lane group g = ky 0..3; chunk 6: tap (4,4) in lane group 0.  ky = -1: the slot carries no weight
static void h5_merged_tap(int f, int g, int &ky, int &kx) {
    ky = kx = -1;
    if (f < 5) { ky = f; kx = g; }
    else if (f == 5) { ky = g; kx = 4; }
    else if (g == 0) { ky = 4; kx = 4; }
}

// A-operand fragments of the MFMA engine.  Layout: 4 x int4 header = add constants in output-row
// order, then F fragments of 64 lanes x 16 bytes.  Lane (m = lane & 15, g = lane >> 4), byte b of
// fragment f carries W[ocmap(m)][ch][ky][kx] for the (ky, kx, ch) the kernel's B operand puts in
// the same (g, b) slot -- the tap rules (above; h5_tap, f5_tap, last_slot_oc: sesrq_common.h) are the single source of truth for
// both sides (kernels: sesrq_mfma.hip).
// zero_pe >= 0: the channels of that PE carry no weights (hybrid kernels: the chain of the other three PEs)
// lastnv: 0 = hidden / first layer (PE-major channel order); 3 / 4 = last layer with that many real rows per lane group
// (last_slot_oc, sesrq_common.h), ps = its PixelShuffle factor
static void pack_mfma_frags(const sesrq_layer_desc &d, int kind, bool general, int lastnv, int ps, std::vector<int> &out, int zero_pe = -1) {
    const int taps = d.k * d.k;
    int F = 0;
    switch (kind) {
        case MFMA_H3: F = general ? 4 : 3; break;
        case MFMA_H5: F = general ? 16 : 7; break;      // general: two sets of 8, one per row parity (h5_pair, sesrq_common.h)
        case MFMA_F5: F = general ? 8 : 2; break;
        case MFMA_H5P: F = 7; break;
    }
    out.assign((size_t)16 + (size_t)F * 64 * 4, 0);
    // MFMA_H5P (last layer, OC <= 4): accumulator row m = (PE m/4, output channel m%4); a row only carries
    // the weights of its PE's channels, so one chain over the full K yields the four per-PE sums
    auto ocmap = [&](int m) { return kind == MFMA_H5P ? (m & 3) : (lastnv ? last_slot_oc(lastnv, m >> 2, m & 3, d.oc, ps) : pe_major(m)); };
    for (int m = 0; m < 16; ++m) out[m] = (ocmap(m) < d.oc && !(kind == MFMA_H5P && m > 3)) ? d.add_const[ocmap(m)] : 0;
    signed char *bytes = reinterpret_cast<signed char *>(out.data() + 16);
    for (int f = 0; f < F; ++f)
        for (int lane = 0; lane < 64; ++lane)
            for (int b = 0; b < 16; ++b) {
                const int m = lane & 15, g = lane >> 4, i = b >> 2, j = b & 3;
                int ky = -1, kx = -1, ch = -1;
                if (kind == MFMA_H3 && !general) { ky = f; kx = g; ch = pe_major(b); if (g > 2) ky = -1; }
                else if (kind == MFMA_H3) { const int p = f; ky = g; kx = i; ch = p + 4 * j; if (g > 2 || i > 2) ky = -1; }
                else if (kind == MFMA_H5P || (kind == MFMA_H5 && !general)) {
                    ch = pe_major(b);
                    h5_merged_tap(f, g, ky, kx);
                    if (kind == MFMA_H5P && i != (m >> 2)) ky = -1;      // byte group i = PE of the channel
                } else if (kind == MFMA_H5) {
                    // per row parity and PE p two K-chunks of two vertical pixel pairs per lane group: dword i = pair i / 2, element i % 2 (h5_tap)
                    const int par = f >> 3, fi = (f >> 2) & 1, p = f & 3;
                    ch = p + 4 * j;
                    if (!h5_tap(fi, g, i >> 1, i & 1, par, ky, kx)) ky = -1;
                } else if (kind == MFMA_F5) {
                    // K-chunk 0: lane group g = kernel row g, dwords = kx 0..3.  K-chunk 1: the 9 remaining taps (row 4 and
                    // column 4) are covered by FOUR translates f5_tr(g) of ONE 4-pixel pattern f5_pt(i) (f5_tap, sesrq_common.h), so a
                    // single pair of ds_read2_b32 (same immediate offsets in every lane) fetches every lane group's operand.
                    const int npe = general ? 4 : 1, fi = f / npe, p = f % npe;
                    ch = j;
                    if (!f5_tap(fi, g, i, ky, kx) || (general && ch != p)) ky = -1;
                }
                const int oc = ocmap(m);
                int w = 0;
                if (ky >= 0 && ky < d.k && kx >= 0 && kx < d.k && ch >= 0 && ch < d.ic && oc < d.oc && (ch & 3) != zero_pe)
                    w = d.w[((size_t)oc * d.ic + ch) * taps + ky * d.k + kx];
                bytes[((size_t)f * 64 + lane) * 16 + b] = (signed char)w;
            }
}

// Sparse hybrid images of a 3-channel first layer (HYBS, sesrq_mfma_common.h): header = add constants in row order, then the
// "other two channels" image and the risky channel's image, 64 lanes x 16 stored bytes each.  Stored byte 2j + e of lane (m, ga)
// = weight of channel ch_e at the tap that B lane group gb = 2 (ga & 1) + (j >> 2) holds in register r = 4 (ga >> 1) + (j & 3):
// f5_tap(r >> 2, gb, r & 3)  (the dense MFMA_F5 scheme, K-chunks 0 and 1 side by side).
static void pack_f5_sparse(const sesrq_layer_desc &d, int risky_pe, std::vector<int> &out) {
    const int taps = d.k * d.k;
    out.assign((size_t)16 + 2 * 64 * 4, 0);
    for (int m = 0; m < 16; ++m) out[m] = pe_major(m) < d.oc ? d.add_const[pe_major(m)] : 0;
    int others[2], no = 0;
    for (int c = 0; c < 3; ++c) if (c != risky_pe) others[no++] = c;
    signed char *bytes = reinterpret_cast<signed char *>(out.data() + 16);
    for (int img = 0; img < 2; ++img)
        for (int lane = 0; lane < 64; ++lane)
            for (int s = 0; s < 16; ++s) {
                const int m = lane & 15, ga = lane >> 4, j = s >> 1, e = s & 1;
                const int gb = 2 * (ga & 1) + (j >> 2), r = 4 * (ga >> 1) + (j & 3);
                int ky, kx;
                if (!f5_tap(r >> 2, gb, r & 3, ky, kx)) ky = -1;
                const int ch = img == 0 ? others[e] : (e == 0 ? risky_pe : -1);
                const int oc = pe_major(m);
                int w = 0;
                if (ky >= 0 && ky < d.k && kx >= 0 && kx < d.k && ch >= 0 && ch < d.ic && oc < d.oc)
                    w = d.w[((size_t)oc * d.ic + ch) * taps + ky * d.k + kx];
                bytes[((size_t)img * 64 + lane) * 16 + s] = (signed char)w;
            }
}

static int replicate_byte(int v) {
    const int b = v & 0xff;
    return b | (b << 8) | (b << 16) | (b << 24);
}

// ---- sesrq_create, step by step.  Validation first: every refusal is decided before anything is allocated.

// The first fault of a descriptor, in a fixed order (a descriptor with one fault always gets the same message), or "" if it is valid.
static std::string validate_desc(const sesrq_net_desc *d, int quan_bits) {
    // width b: activations and weights live in [qlo, qhi] (myQL/quan_func.py:67-70,201-202,218-219)
    const int qlo = -(1 << (quan_bits - 1)), qhi = (1 << (quan_bits - 1)) - 1;
    const bool narrow = quan_bits < 8;
    const int L = d->n_layers;
    if (L < 3 || L > SESRQ_MAX_LAYERS) return "sesrq_create: n_layers must be in [3,16]";
    if (d->pe_num != 4) return "sesrq_create: only pe_num == 4 is supported (define.py PE)";
    if (d->pe_acc_bits < 9 || d->pe_acc_bits > 31 || d->pe_add_bits < d->pe_acc_bits || d->pe_add_bits > 31)
        return "sesrq_create: pe_acc_bits/pe_add_bits out of range";
    if (d->pixel_shuffle < 1 || d->pixel_shuffle > 4) return "sesrq_create: pixel_shuffle must be 1..4";
    if (!d->layers || !d->zero) return "sesrq_create: null layers/zero";
    if (d->M_res >= (1u << 16) || d->n_res > 32) return "sesrq_create: residual requant constant out of range";
    if (!(d->scale_in > 0.f) || !(d->scale_out > 0.f)) return "sesrq_create: scales must be positive";
    for (int k = 0; k <= L; ++k)
        if (d->zero[k] < -32768 || d->zero[k] > qhi) return "sesrq_create: zero point out of range [-32768," + std::to_string(qhi) + "]";
    for (int k = 0; k < L; ++k) {
        const sesrq_layer_desc &l = d->layers[k];
        if (l.k != 3 && l.k != 5) return "sesrq_create: kernel size must be 3 or 5";
        if (l.ic < 1 || l.ic > SESRQ_MAX_CH || l.oc < 1 || l.oc > SESRQ_MAX_CH) return "sesrq_create: channels must be 1..16";
        if (!l.w || !l.add_const) return "sesrq_create: null weight/add_const";
        for (size_t i = 0, nw = (size_t)l.oc * l.ic * l.k * l.k; narrow && i < nw; ++i)
            if (l.w[i] < qlo || l.w[i] > qhi) return "sesrq_create: weight outside the " + std::to_string(quan_bits) + "-bit range";
        if (l.M >= (1u << 16) || l.n > 32) return "sesrq_create: requant constant out of range (M < 2^16, n <= 32)";
        if (narrow && l.M_oc) return "sesrq_create: per-channel requant constants need quan_bits == 8";
        if ((l.M_oc != nullptr) != (l.n_oc != nullptr)) return "sesrq_create: per-channel requant constants need both M_oc and n_oc";
        for (int o = 0; l.M_oc && o < l.oc; ++o)
            if (l.M_oc[o] >= (1u << 16) || l.n_oc[o] > 32) return "sesrq_create: per-channel requant constant out of range (M < 2^16, n <= 32)";
        if (k > 0 && l.ic != d->layers[k - 1].oc) return "sesrq_create: channel mismatch between consecutive layers";
        for (int o = 0; o < l.oc; ++o)
            if (l.add_const[o] < -(1 << 24) || l.add_const[o] > (1 << 24)) return "sesrq_create: add_const out of range";
    }
    if (d->layers[0].ic > 4) return "sesrq_create: first layer supports 1..4 input channels";
    if (d->layers[0].oc != d->layers[L - 2].oc) return "sesrq_create: residual source/destination width mismatch";
    if (d->layers[L - 1].oc % (d->pixel_shuffle * d->pixel_shuffle)) return "sesrq_create: last layer channels not divisible by pixel_shuffle^2";
    return "";
}

// ... and of the options, given a valid descriptor
static std::string validate_options(const sesrq_options &o, const sesrq_net_desc *d, bool narrow) {
    if (o.exact_div < 0 || o.exact_div > 2) return "sesrq_create: exact_div must be 0, 1 or 2";
    if (o.fuse_hidden < 0 || o.fuse_hidden > 1) return "sesrq_create: fuse_hidden must be 0 or 1";
    if (o.wg_budget < 0) return "sesrq_create: wg_budget must be >= 0";
    if (o.reduced_forms < -1 || o.reduced_forms > 63) return "sesrq_create: reduced_forms must be -1 or a mask of bits 1 | 2 | 4 | 8 | 16 | 32";
    // the int8 hand-off domain is an upstream net's OUTPUT domain (scale_L, zero[L]): an int8-range zero point
    if (!(o.i8_in_scale >= 0.f) || o.i8_in_zero < -128 || o.i8_in_zero > 127) return "sesrq_create: bad int8 input domain (zero point must be in [-128, 127])";
    if (narrow && o.i8_in_scale > 0.f) return "sesrq_create: an int8 upstream hand-off needs quan_bits == 8";
    if (o.anchor_add && d->layers[0].ic * d->pixel_shuffle * d->pixel_shuffle != d->layers[d->n_layers - 1].oc)
        return "sesrq_create: anchor add needs as many output as input channels";
    if (o.exact_div == 2 && !reciprocal_form(d->scale_in, d->zero[0]).ok) return "sesrq_create: exact_div = 2 needs a finite positive scale_in";
    return "";
}

static int pad_value(const sesrq_net_desc *d, int k) { return std::max(d->zero[k], -128); }
// exactly one PE of an MFMA layer can saturate: its image is packed apart (d_afrag_others), the hybrid kernels may apply
static bool one_risky_pe(const LayerPlan &lp) { return lp.mfma_kind != MFMA_NONE && lp.general && __builtin_popcount(lp.risky_mask) == 1; }
// the last layer with OC <= 4 runs the MFMA_H5P kernel: one chain whose 16 rows are (PE, channel)
static bool pe_split(const LayerPlan &lp, bool last) { return last && lp.mfma_kind == MFMA_H5 && lp.oc <= 4; }

// Step 1, per layer: what its weights can do to the accumulators (load-time proofs, sesrq_verify.hip), and the kernel family that follows.
// Per-channel layers: the dot4 kernels only (the MFMA kernels hold one (M, n)).  A net of width b < 8 too -- the dot4 kernels' clamps are
// run-time arguments, the MFMA kernels and the fused trio keep the 8-bit literals -- unless the net asks for SESRQ_ENGINE_MFMA_Q: its
// layers then get their MFMA kinds and run on the width-aware flavours (mfma_*_kernel_q).  Those have no unbiased hybrid and no
// literal-bounds form: a layer with one risky PE is a general one there, and a wide layer (reach >= 2^22) stays on the dot4 kernels.
static void analyse_layer(const sesrq_net_desc *d, int k, bool narrow, int engine, LayerPlan &lp) {
    const sesrq_layer_desc &l = d->layers[k];
    const bool last = k == d->n_layers - 1;
    lp.k = l.k; lp.ic = l.ic; lp.oc = l.oc;
    lp.ocp = last ? ((l.oc + 3) & ~3) : 16;
    lp.general = !saturation_free(l, pad_value(d, k), d->pe_acc_bits, d->pe_add_bits, lp.worst_pe, lp.worst_sum, lp.risky_mask, &lp.risky_oc);
    // the biased accumulator of the MFMA kernels is exact for |s| < 2^22 only (never reached at 18 / 20 bits with a 16-bit constant)
    lp.reach = reachable_sum(lp.worst_sum, d->pe_add_bits, l.add_const, l.oc);
    lp.wide = lp.reach >= BIASED_LIMIT;
    const bool narrow_dot4 = narrow && (engine != SESRQ_ENGINE_MFMA_Q || lp.wide);
    lp.mfma_kind = (narrow_dot4 || l.M_oc) ? MFMA_NONE
                 : k == 0             ? (l.k == 5 && l.ic <= 4 ? MFMA_F5 : MFMA_NONE)
                 : l.k == 3           ? (last ? MFMA_NONE : MFMA_H3)
                                      : MFMA_H5;
    // the hybrid kernels hold the reference's 18 / 20-bit clamps as literals
    lp.hybrid = one_risky_pe(lp) && d->pe_acc_bits == 18 && d->pe_add_bits == 20 && !lp.wide && !narrow;
    // hidden-layer rows: channel o sits in register o >> 2 of lane group o & 3.  If every channel that can saturate lives in
    // ONE register, the hybrid first layer clamps that register only (risky_reg), else all four (4)
    for (int i = 0; i < 4; ++i)
        if (lp.risky_oc && (lp.risky_oc & ~(0xf << (4 * i))) == 0) lp.risky_reg = i;
}

// Step 2, per layer: its weight images, one upload each.  false = the device refused one.
static bool upload_images(const sesrq_layer_desc &l, bool first, bool last, int ps, bool narrow, LayerPlan &lp) {
    std::vector<int> gen, mer, fr;
    pack_weights(l, lp.ocp, first, gen, mer);
    if (!lp.d_wpk_general.upload(gen) || !lp.d_wpk_merged.upload(mer)) return false;
    if (l.M_oc) {      // per-output-channel requant constants: a device table for the dot4 kernels
        float2 mn[SESRQ_MAX_CH];
        for (int o = 0; o < SESRQ_MAX_CH; ++o) mn[o] = o < l.oc ? make_float2((float)l.M_oc[o], ldexpf(1.0f, -(int)l.n_oc[o])) : make_float2(0.f, 0.f);
        if (!lp.d_mn_oc.upload(mn, sizeof(mn))) return false;
    }
    if (lp.mfma_kind == MFMA_NONE) return true;
    const int lastnv = last ? last_nv(l.oc) : 0;
    auto frags = [&](DevBuf<int4> &dst, int kind, bool general, int nv, int zero_pe) {
        pack_mfma_frags(l, kind, general, nv, ps, fr, zero_pe);
        return dst.upload(fr);
    };
    if (!frags(lp.d_afrag_merged, lp.mfma_kind, false, lastnv, -1) || !frags(lp.d_afrag_general, lp.mfma_kind, true, lastnv, -1)) return false;
    if (one_risky_pe(lp) && !narrow) {      // (the width-aware kernels run such a layer on the per-PE image)      // hybrid kernels: merged chain without the risky PE; a 3-channel first layer: the sparse images too
        const int risky = __builtin_ctz(lp.risky_mask);
        if (!frags(lp.d_afrag_others, lp.mfma_kind, false, lastnv, risky)) return false;
        if (lp.mfma_kind == MFMA_F5 && l.ic == 3 && risky < 3) {
            pack_f5_sparse(l, risky, fr);
            if (!lp.d_afrag_sparse.upload(fr)) return false;
        }
    }
    return !pe_split(lp, last) || frags(lp.d_afrag_pesplit, MFMA_H5P, true, 4, -1);
}

// Which one-fma requant form layer k may use (ConvArgs::direct): it requantises into a -128 domain (z_next; the output layer: zero[L])
// and (M, n) passes the proof.  The residual-merging layer L-2: its FIRST requant, into the fixed -128 domain of ic (quan_func.py:250),
// whatever the zero points.  The output layer has a second choice, form 2 (LastStore, FASTD 2x): one fma that also subtracts the 128,
// and the add back.  rf = sesrq_options.reduced_forms: bit 2 gates the first layer here, bits 16 / 32 the output layer's two forms; the
// hidden layers keep their proof -- only the fused trio uses it, and applies bits 2 / 4 at launch (launch_trio).
// The forms are proven for the 8-bit clamp with one (M, n), and for |s| < 2^22 (biased sums), which a wide layer can leave.
static int requant_form(const sesrq_net_desc *d, int k, int rf, bool narrow, bool wide) {
    const sesrq_layer_desc &l = d->layers[k];
    const int L = d->n_layers;
    const int zt = (k == L - 1) ? d->zero[L] : d->zero[(k == 0) ? 1 : k + 1];
    if (l.M_oc || narrow || wide || (k != L - 2 && zt != -128)) return 0;
    if (k == L - 1) return ((rf & 16) && prove_direct_requant(l.M, l.n)) ? 1 : ((rf & 32) && prove_single_requant(l.M, l.n)) ? 2 : 0;
    return (k > 0 || (rf & 2)) ? sesrq_requant_form(l.M, l.n, 0) : 0;
}

// Step 3, per layer: the constant fields of its launch arguments
static void prefill_args(const sesrq_net_desc *d, int k, int quan_bits, int rf, LayerPlan &lp) {
    const sesrq_layer_desc &l = d->layers[k];
    const int L = d->n_layers;
    ConvArgs &a = lp.base;
    memset(&a, 0, sizeof(a));
    a.ic = l.ic; a.oc = l.oc;
    a.pad_word = replicate_byte(pad_value(d, k));
    a.acc_lo = -(1 << (d->pe_acc_bits - 1)); a.acc_hi = (1 << (d->pe_acc_bits - 1)) - 1;
    a.add_lo = -(1 << (d->pe_add_bits - 1)); a.add_hi = (1 << (d->pe_add_bits - 1)) - 1;
    a.Mf = (float)l.M;
    a.sh = ldexpf(1.0f, -(int)l.n);
    a.relu = l.relu;
    a.z_next = (float)d->zero[(k == 0 || k == L - 2) ? 1 : k + 1];
    a.Md = a.Mf * a.sh; a.Cd = -(12582912.f * a.Mf) * a.sh; a.Cs = a.Cd - 128.f;
    a.direct = requant_form(d, k, rf, quan_bits < 8, lp.wide);
    a.qlo = (float)-(1 << (quan_bits - 1)); a.qhi = (float)((1 << (quan_bits - 1)) - 1); a.qhalf = (float)(1 << (quan_bits - 1)); a.qspan = (float)(1 << quan_bits);
    a.mn_oc = lp.d_mn_oc.get();
    a.Mres = (float)d->M_res; a.shres = ldexpf(1.0f, -(int)d->n_res);
    a.z_merge = (float)d->zero[L - 1];
    a.s_in = d->scale_in; a.z_in = (float)d->zero[0];
    a.s_out = d->scale_out; a.z_out = (float)d->zero[L];
    a.ps = d->pixel_shuffle;
    for (int o = 0; o < l.oc; ++o) a.add_const[o] = l.add_const[o];
}

// Step 4, per layer: what it runs on, as layer_engines() reports it.  dot4-{merged|general}[-perchannel][-qB]; on the MFMA engine
// {mfma-h3|mfma-h5|mfma-f5|mfma-h5p}-{merged|hybrid|general|unbiased} (the pe-split kernel has no hybrid; a sum that can leave the biased
// range: the per-PE kernel with run-time bounds, GEN_ANY, whatever the saturation verdict says).  on_dot4: the net's engine option, or a
// first layer that divides (no 3-instruction form for its (scale, zero), or exact_div = 1)
static void engine_name(LayerPlan &lp, bool per_channel, int quan_bits, bool on_dot4) {
    static const char *kn[] = {"", "mfma-h3", "mfma-h5", "mfma-f5"};
    const bool pesplit = lp.d_afrag_pesplit.get();
    lp.engine_dot4 = std::string(lp.general ? "dot4-general" : "dot4-merged") + (per_channel ? "-perchannel" : "") +
                     (quan_bits < 8 ? "-q" + std::to_string(quan_bits) : "");
    lp.engine_mfma = lp.mfma_kind == MFMA_NONE ? lp.engine_dot4 : std::string(pesplit ? "mfma-h5p" : kn[lp.mfma_kind]) +
                     (lp.wide ? "-unbiased" : (lp.hybrid && !pesplit) ? "-hybrid" : lp.general ? "-general" : "-merged") +
                     (quan_bits < 8 ? "-q" + std::to_string(quan_bits) : "");      // the width-aware flavours (SESRQ_ENGINE_MFMA_Q)
    lp.engine = on_dot4 ? lp.engine_dot4 : lp.engine_mfma;
}

// Step 5: residual merge (myQL/quan_func.py:256-270): q4 = clamp8(rint(fl(fl(u * M_res) * 2^-n_res + zero[L-1]))) is a function of the
// 9-bit integer u = rc + ic + 256 alone: a 511-entry byte table (512 bytes = 128 dwords) replaces the second requant of the fused trio's
// last phase (2 fma + add + cvt per value) by one LDS byte read.  Same fp32 operations, same order, as requant4<true> + round_pack.
// Width b < 8: u = rc + ic + 2^b and the clamp is the width's.  The kernels keep the table's index rc + ic + 256, so entry i holds
// q4(u = i - 256 + 2^b); a width reaches i in [256 - 2^b, 254 + 2^b] only, entries below 256 - 2^b (u < 0) stay 0.
static std::vector<int> merge_table(uint32_t M_res, uint32_t n_res, int zero_merge, int quan_bits) {
    std::vector<int> lut(128);
    unsigned char *bytes = reinterpret_cast<unsigned char *>(lut.data());
    const float Mres = (float)M_res, shres = ldexpf(1.0f, -(int)n_res), zm = (float)zero_merge;
    const float qlo = (float)-(1 << (quan_bits - 1)), qhi = (float)((1 << (quan_bits - 1)) - 1);
    for (int i = 0; i < 512; ++i) {
        const int u = i - 256 + (1 << quan_bits);
        if (u < 0) continue;
        const float prod = (float)u * Mres;              // one rounding of the exact product, as fma(MAGIC + u, M, -MAGIC * M)
        float v = prod * shres;                          // exact (power of two)
        v = v + zm;                                      // one rounding, as fma(prod, 2^-n, z)
        v = fminf(fmaxf(v, qlo), qhi);
        bytes[i] = (unsigned char)(signed char)(int)nearbyintf(v);
    }
    return lut;
}

// Step 6: fused hidden trios, greedy from the residual-merging layer L-2 backwards: three consecutive 3x3 16->16 layers whose
// load-time proof allows the merged accumulation mode.  trio_len[k] == 3 marks a trio's first layer; that layer's LayerPlan::trio gets
// the constant fields of the trio's launch arguments (the forward adds in / out / rc_in / N / H / W, launch_trio_k the run geometry)
static std::vector<int> plan_trios(sesrq_net &net) {
    std::vector<LayerPlan> &layers = net.layers;
    const int L = (int)layers.size();
    std::vector<int> trio_len(L, 0);
    auto trio_ok = [&](int k) {
        const LayerPlan &lp = layers[k];
        return k >= 1 && k <= L - 2 && lp.mfma_kind == MFMA_H3 && !lp.general && !lp.wide && lp.ic == 16 && lp.oc == 16;
    };
    for (int k = L - 4; k >= 1 && trio_ok(k) && trio_ok(k + 1) && trio_ok(k + 2); k -= 3) {
        trio_len[k] = 3;
        const ConvArgs &b0 = layers[k].base;
        TrioArgs &t = layers[k].trio;
        memset(&t, 0, sizeof(t));
        t.merge_lut = net.d_merge_lut.get();
        t.wg_budget = net.wg_budget;
        t.allow = net.reduced_forms;
        t.pad_in = b0.pad_word;
        t.Mres = b0.Mres; t.shres = b0.shres; t.z_merge = b0.z_merge;
        for (int j = 0; j < 3; ++j) {
            const ConvArgs &b = layers[k + j].base;
            TrioLayer &tl = t.l[j];
            tl.afrag = layers[k + j].d_afrag_merged.get();
            tl.Mf = b.Mf; tl.sh = b.sh; tl.z_next = b.z_next; tl.Md = b.Md; tl.Cd = b.Cd; tl.direct = b.direct;
            tl.zlo = b.relu ? fmaxf(b.z_next, b.qlo) : b.qlo;      // qlo = -128 at 8 bits
            tl.pad_next = layers[k + j + 1].base.pad_word;
        }
    }
    return trio_len;
}

}  // namespace sesrq

using namespace sesrq;

// The steps in order, for a net whose scalars are set.  false = a device upload failed.
static bool build_layers(sesrq_net &net, const sesrq_net_desc *d) {
    const int L = net.L;
    net.layers.resize(L);
    for (int k = 0; k < L; ++k) {
        const sesrq_layer_desc &l = d->layers[k];
        LayerPlan &lp = net.layers[k];
        analyse_layer(d, k, net.quan_bits < 8, net.engine, lp);
        if (!upload_images(l, k == 0, k == L - 1, d->pixel_shuffle, net.quan_bits < 8, lp)) return false;
        prefill_args(d, k, net.quan_bits, net.reduced_forms, lp);
        engine_name(lp, l.M_oc != nullptr, net.quan_bits, net.engine == SESRQ_ENGINE_DOT4 || (k == 0 && !net.fd.ok));
    }
    net.layers[0].base.fd = net.fd;
    if (!net.d_merge_lut.upload(merge_table(d->M_res, d->n_res, d->zero[L - 1], net.quan_bits))) return false;
    net.trio_engine = "mfma-trio-merged" + (net.quan_bits < 8 ? "-q" + std::to_string(net.quan_bits) : std::string());
    net.trio_len = plan_trios(net);
    return true;
}

extern "C" {

const char *sesrq_last_error(void) { return g_err.c_str(); }
int sesrq_version(void) { return SESRQ_VERSION; }

void sesrq_default_options(sesrq_options *o) {
    if (!o) return;
    o->engine = SESRQ_ENGINE_AUTO;
    o->force_general = 0;
    o->exact_div = 0;
    o->anchor_add = 0;
    o->fuse_hidden = 1;
    o->wg_budget = 0;
    o->i8_in_scale = 0.f;
    o->i8_in_zero = 0;
    o->reduced_forms = -1;
}

int sesrq_create(const sesrq_net_desc *d, const sesrq_options *opts, sesrq_net **out) { return sesrq_create_q(d, opts, 8, out); }

int sesrq_create_q(const sesrq_net_desc *d, const sesrq_options *opts, int quan_bits, sesrq_net **out) {
    if (!d || !out) { set_error("sesrq_create: null argument"); return 1; }
    *out = nullptr;
    sesrq_options o;
    sesrq_default_options(&o);
    if (opts) o = *opts;
    std::string err;
    if (quan_bits < 2 || quan_bits > 8) err = "sesrq_create: quan_bits must be 2..8 (define.py QUAN_BIT)";
    else if (o.engine < SESRQ_ENGINE_AUTO || o.engine > SESRQ_ENGINE_MFMA_Q) err = "sesrq_create: bad engine option";
    else err = validate_desc(d, quan_bits);
    if (err.empty()) err = validate_options(o, d, quan_bits < 8);
    if (!err.empty()) { set_error(err); return 1; }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { set_error("sesrq_create: no HIP device"); return 1; }
    std::unique_ptr<sesrq_net> net(new (std::nothrow) sesrq_net());      // from here on every failure frees the net and what it uploaded
    if (!net) { set_error("sesrq_create: out of memory"); return 1; }

    const int L = d->n_layers, qlo = -(1 << (quan_bits - 1));
    net->L = L;
    net->zero.assign(d->zero, d->zero + L + 1);
    net->scale_in = d->scale_in;
    net->scale_out = d->scale_out;
    net->M_res = d->M_res;
    net->n_res = d->n_res;
    net->ps = d->pixel_shuffle;
    net->acc_bits = d->pe_acc_bits;
    net->add_bits = d->pe_add_bits;
    net->quan_bits = quan_bits;
    net->rc_separate = (d->zero[1] != qlo);      // layer 0's output IS the residual operand only in the domain zero[1] == -2^(b-1)
    net->device = device;
    // MFMA_Q at 8 bits IS the MFMA engine: same kinds, same instantiations, same names
    net->engine = (o.engine == SESRQ_ENGINE_MFMA_Q && quan_bits == 8) ? SESRQ_ENGINE_MFMA : o.engine;
    net->force_general = o.force_general ? 1 : 0;
    net->div_mode = o.exact_div;
    net->fuse_hidden = o.fuse_hidden;
    net->wg_budget = o.wg_budget;
    // which proven reduced forms the kernels may select: all by default; SESRQ_DIRECT=0 leaves the cvt_pk_u8 epilogues only
    static const int knob = env_knob("SESRQ_DIRECT", 1, 0, 1);
    net->reduced_forms = o.reduced_forms >= 0 ? o.reduced_forms : (knob ? 63 : (1 | 8));
    net->i8_in_scale = o.i8_in_scale;
    net->i8_in_zero = o.i8_in_zero;
    net->anchor_add = o.anchor_add ? 1 : 0;
    // The input quantiser's division.  The proof compares clamp8(rint(.)) of the two quotient forms; it holds for every width b <= 8 as
    // it stands, because clamp_b(v) = clamp_b(clamp8(v)): two forms that agree after clamp8 agree after clamp_b.
    net->fd_proof = prove_fastdiv(d->scale_in, d->zero[0]);
    net->fd = net->div_mode == 2 ? reciprocal_form(d->scale_in, d->zero[0]) : net->fd_proof;
    if (net->div_mode == 1) net->fd.ok = 0;

    if (!build_layers(*net, d)) { set_error("sesrq_create: device upload failed"); return 1; }
    *out = net.release();
    return 0;
}

void sesrq_destroy(sesrq_net *net) { delete net; }

}  // extern "C"
