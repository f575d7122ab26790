// sesrq C ABI, part 2 of 4: workspace layout and the launch planner -- sesrq_forward / _debug / _timed are one walk over the net's layers
// (forward_impl) that picks, per layer or fused trio, the kernel family and fills its arguments.  See include/sesrq.h.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "sesrq_common.h"

namespace sesrq {

thread_local KernelEvents tl_kernel_events;

WsLayout ws_layout(const sesrq_net *net, int N, int H, int W) {
    WsLayout l;
    l.act_bytes = (((size_t)N * H * W * 16) + 255) & ~(size_t)255;
    l.off_s = 0;
    l.off_a = l.act_bytes;
    l.off_b = 2 * l.act_bytes;
    l.off_rc = 3 * l.act_bytes;
    l.total = (net->rc_separate ? 4 : 3) * l.act_bytes;
    return l;
}


// the fused hidden trio runs in the production forward (no debug taps), on the MFMA kernels, unless the per-PE path is forced
static bool trio_active(const sesrq_net *net, const sesrq_taps *taps) {
    return net->fuse_hidden && net->engine != SESRQ_ENGINE_DOT4 && !net->force_general && !taps;
}

// Can the frames of several caller buffers be the images of one launch (ConvArgs::ft)?  Only the MFMA first- and last-layer kernels read
// the table: the first layer needs its MFMA kernel (the proven division form), the last layer an MFMA shape.
bool groupable(const sesrq_net *net) {
    const LayerPlan &l0 = net->layers[0], &ll = net->layers[net->L - 1];
    return net->engine != SESRQ_ENGINE_DOT4 && l0.mfma_kind != MFMA_NONE && net->fd.ok && ll.mfma_kind != MFMA_NONE;
}

}  // namespace sesrq

using namespace sesrq;

extern "C" {

int sesrq_fast_division_proven(const sesrq_net *net) { return net ? net->fd_proof.ok : 0; }

int sesrq_net_quan_bits(const sesrq_net *net) { return net ? net->quan_bits : 0; }

const char *sesrq_layer_engine(const sesrq_net *net, int k) {
    if (!net || k < 0 || k >= net->L) return "";
    for (int j = std::max(1, k - 2); j <= k; ++j)
        if (trio_active(net, nullptr) && net->trio_len[j] == 3 && k < j + 3) return net->trio_engine.c_str();
    return net->layers[k].engine.c_str();
}

int sesrq_layer_one_fma(const sesrq_net *net, int k) {
    if (!net || k < 0 || k >= net->L) return 0;
    // 1 = one fma, 2 = one fma + the add of 128 (output layer only).  First and output layer: sesrq_create has applied
    // sesrq_options.reduced_forms already; a hidden layer's proof is used by the fused trio only, under bit 2 (layers a, b) / bit 4 (third layer)
    int d = net->layers[k].base.direct;
    if (k > 0 && k < net->L - 1) {
        int bit = 2;
        for (int j = std::max(1, k - 2); j <= k; ++j)
            if (net->trio_len[j] == 3 && k == j + 2) bit = 4;
        if (!(net->reduced_forms & bit)) d = 0;
    }
    return d;
}

int sesrq_launch_plan(const sesrq_net *net, int *first, int *count) {
    if (!net) return 0;
    int n = 0;
    for (int k = 0; k < net->L;) {
        const int c = (trio_active(net, nullptr) && net->trio_len[k] == 3) ? 3 : 1;
        if (first) first[n] = k;
        if (count) count[n] = c;
        ++n;
        k += c;
    }
    return n;
}

int sesrq_net_shape(const sesrq_net *net, int *cin, int *cout, int *pixel_shuffle) {
    if (!net) { set_error("sesrq_net_shape: null net"); return 1; }
    if (cin) *cin = net->layers[0].ic;
    if (cout) *cout = net->layers[net->L - 1].oc;
    if (pixel_shuffle) *pixel_shuffle = net->ps;
    return 0;
}

size_t sesrq_workspace_bytes(const sesrq_net *net, int N, int H, int W) {
    if (!net || N < 1 || H < 1 || W < 1) return 0;
    return ws_layout(net, N, H, W).total;
}

}  // extern "C"

namespace sesrq {

// Step 1: the checks of the call's arguments, before anything is enqueued; wl = the workspace layout they needed
static int validate_forward(const sesrq_net *net, const Call &c, void *workspace, size_t workspace_bytes, WsLayout &wl) {
    if (!net || !c.in || !workspace) { set_error("sesrq_forward: null argument"); return 1; }
    if (c.ft && (c.taps || !groupable(net) || c.ft->n != c.N || c.N > SESRQ_GROUP_MAX)) { set_error("sesrq_forward: frame table not applicable"); return 1; }
    if (!c.out_q && !c.out_f) { set_error("sesrq_forward: both outputs are NULL"); return 1; }
    if (net->anchor_add && c.in_dtype != SESRQ_F32) { set_error("sesrq_forward: anchor add needs the fp32 input frame"); return 1; }
    if (c.N < 1 || c.H < 1 || c.W < 1) { set_error("sesrq_forward: N, H, W must be positive"); return 1; }
    if ((size_t)c.N * c.H * c.W > (size_t)1 << 31) { set_error("sesrq_forward: frame batch too large (N*H*W > 2^31)"); return 1; }
    if (c.in_dtype != SESRQ_F32 && c.in_dtype != SESRQ_I8) { set_error("sesrq_forward: in_dtype must be SESRQ_F32 or SESRQ_I8"); return 1; }
    if ((uintptr_t)workspace & 15) { set_error("sesrq_forward: workspace must be 16-byte aligned"); return 1; }
    wl = ws_layout(net, c.N, c.H, c.W);
    if (workspace_bytes < wl.total) { set_error("sesrq_forward: workspace too small (see sesrq_workspace_bytes)"); return 1; }
    // the net's device copy of the bundle lives on net->device: a launch from another current device would read foreign pointers
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != net->device) {
        set_error("sesrq_forward: the current HIP device (" + std::to_string(dev) + ") is not the device the net was created on (" +
                  std::to_string(net->device) + ")");
        return 1;
    }
    return 0;
}

// Step 2: the activation tensors inside the caller's workspace.  S = layer 0's output (kept for the residual), A / B = the hidden layers'
// ping-pong, RC = the residual operand: S itself unless layer 0 writes a separate one (sesrq_net::rc_separate)
struct WsBuffers {
    void *S, *A, *B, *RC;
    WsBuffers(const sesrq_net *net, void *workspace, const WsLayout &wl)
        : S((char *)workspace + wl.off_s), A((char *)workspace + wl.off_a), B((char *)workspace + wl.off_b),
          RC(net->rc_separate ? (void *)((char *)workspace + wl.off_rc) : S) {}
    void *next(const void *cur) const { return cur == A ? B : A; }      // where a hidden layer reading `cur` writes
};

// Step 3, per layer that runs on its own: kernel family, accumulation mode and weight images.  Pure: no HIP call, nothing written.
static LayerChoice choose_layer(const sesrq_net *net, int k, const sesrq_taps *taps, int in_dtype) {
    const LayerPlan &lp = net->layers[k];
    const int L = net->L;
    const bool pesplit = lp.d_afrag_pesplit.get() != nullptr;      // last layer with OC <= 4: the MFMA_H5P image exists
    // any debug tap of this layer's PE sums; the taps only the dot4 kernels write: the overflow counters, layer 0's quantised input
    // (input.0.pt) and un-rounded output (shortcut_tensor.pt), the merging layer's ic (input.4.spcial.pt)
    const bool dbg = taps && (taps->pe_out[k] || taps->pe_add[k] || taps->overflow);
    const bool dot4_tap = taps && (taps->overflow || (k == 0 && (taps->act[0] || taps->shortcut)) || (k == L - 2 && taps->ic));
    // the layer has an MFMA kernel: the engine option, its shape, and for the first layer the proven division form
    // a net of width b < 8 has MFMA kinds under SESRQ_ENGINE_MFMA_Q only (analyse_layer); its debug forward runs on the dot4 kernels
    // (the width-aware flavours write no taps)
    const bool mfma_ok = net->engine != SESRQ_ENGINE_DOT4 && lp.mfma_kind != MFMA_NONE && (k > 0 || net->fd.ok) && !(net->quan_bits < 8 && taps);
    LayerChoice c{};
    c.tap = dbg && !dot4_tap && mfma_ok && !pesplit;      // PE taps the per-PE MFMA kernels write themselves; the pe-split kernel has none
    c.mfma = mfma_ok && !dot4_tap && (!dbg || c.tap);     // every other tapped layer runs on the dot4 kernels
    c.general = lp.general || net->force_general || dbg || (lp.wide && c.mfma);      // a wide layer has no merged MFMA kernel (LayerPlan::wide)
    c.one_pe = c.mfma && lp.hybrid && !net->force_general && !dbg;      // the hybrid unless something forces the full per-PE path
    c.src = k > 0 ? SRC_NHWC16 : in_dtype == SESRQ_F32 ? SRC_F32 : net->i8_in_scale > 0.f ? SRC_I8D : SRC_I8;      // I8D: an upstream net's domain
    c.epi = k == L - 1 ? EPI_LAST : k == L - 2 ? EPI_PRERES : EPI_MID;
    c.wpk = (c.general ? lp.d_wpk_general : lp.d_wpk_merged).get();
    if (!c.mfma) return c;
    c.afrag = pesplit ? lp.d_afrag_pesplit.get() : c.one_pe ? lp.d_afrag_others.get() : (c.general ? lp.d_afrag_general : lp.d_afrag_merged).get();
    if (c.one_pe) {
        c.afrag2 = lp.d_afrag_general.get(); c.afrag_sp = lp.d_afrag_sparse.get();
        c.risky_pe = __builtin_ctz(lp.risky_mask); c.risky_reg = lp.risky_reg;
    }
    return c;
}

// Step 4, per layer: the per-call fields of its arguments (LayerPlan::base holds the constant ones).  cur -> dst: the layer's activations
static ConvArgs fill_conv_args(const sesrq_net *net, int k, const LayerChoice &ch, const Call &c, const WsBuffers &buf, const void *cur, void *dst) {
    const int L = net->L;
    ConvArgs a = net->layers[k].base;
    a.wpk = ch.wpk; a.afrag = ch.afrag; a.afrag2 = ch.afrag2; a.afrag_sp = ch.afrag_sp; a.risky_pe = ch.risky_pe; a.risky_reg = ch.risky_reg;
    a.N = c.N; a.H = c.H; a.W = c.W;
    a.wg_budget = net->wg_budget;
    a.s_prev = net->i8_in_scale; a.z_prev = (float)net->i8_in_zero;
    a.in = cur; a.out = dst;
    a.rc_in = buf.RC;
    if (k == 0 && net->rc_separate) a.rc_out = buf.RC;
    a.out_q = c.out_q; a.out_f = (float *)c.out_f;
    a.anchor = (net->anchor_add && c.in_dtype == SESRQ_F32) ? (const float *)c.in : nullptr;
    if (c.ft && (k == 0 || k == L - 1)) a.ft = *c.ft;
    if (const sesrq_taps *t = c.taps) {
        a.dbg_pe = (int *)t->pe_out[k];
        a.dbg_add = (int *)t->pe_add[k];
        a.dbg_ovf = t->overflow ? (int *)t->overflow + 2 * k : nullptr;
        if (k == L - 2) a.dbg_ic = (signed char *)t->ic;
        if (k == 0) { a.dbg_q0 = (signed char *)t->act[0]; a.dbg_t = (float *)t->shortcut; }
    }
    return a;
}

// One kernel launch of the forward: refuses a launch sesrq_launch_plan does not announce (ev[] holds two events per announced launch),
// and makes ev's pair the begin / end events of exactly this launch (launch_kernel reads tl_kernel_events) -- cleared on every way out
struct LaunchSlot {
    const bool ok;
    LaunchSlot(int launch, int announced, hipEvent_t *ev) : ok(launch < announced) {
        if (!ok) set_error("sesrq_forward: more launches than sesrq_launch_plan reports");
        else if (ev) tl_kernel_events = KernelEvents{ev[2 * launch], ev[2 * launch + 1]};
    }
    ~LaunchSlot() { tl_kernel_events = KernelEvents{}; }
};

int forward_impl(const sesrq_net *net, const Call &c, void *workspace, size_t workspace_bytes, void *stream, hipEvent_t *ev) {
    WsLayout wl;
    if (validate_forward(net, c, workspace, workspace_bytes, wl)) return 1;
    const sesrq_taps *taps = c.taps;
    const int L = net->L, N = c.N, H = c.H, W = c.W;
    hipStream_t st = (hipStream_t)stream;
    if (taps && taps->overflow && hipMemsetAsync(taps->overflow, 0, (size_t)L * 2 * sizeof(int), st) != hipSuccess) {
        set_error("sesrq_forward: clearing the overflow counters failed"); return 1;
    }
    const WsBuffers buf(net, workspace, wl);
    const int announced = taps ? L : sesrq_launch_plan(net, nullptr, nullptr);
    const void *cur = c.in;
    for (int k = 0, launch = 0; k < L; ++launch) {
        if (trio_active(net, taps) && net->trio_len[k] == 3) {
            // ---- fused hidden trio: layers k, k+1, k+2 in one launch (sesrq_trio.hip)
            TrioArgs t = net->layers[k].trio;
            t.in = cur; t.out = buf.next(cur); t.rc_in = buf.RC;
            t.N = N; t.H = H; t.W = W;
            LaunchSlot slot(launch, announced, ev);
            const int epi_c = (k + 2 == L - 2) ? EPI_PRERES : EPI_MID;
            if (!slot.ok || (net->quan_bits < 8 ? launch_trio_q(t, net->layers[k].base, epi_c, st) : launch_trio(t, epi_c, st))) return 1;
            cur = t.out;
            k += 3;
            continue;
        }
        const LayerChoice ch = choose_layer(net, k, taps, c.in_dtype);
        void *dst = k == 0 ? buf.S : k < L - 1 ? buf.next(cur) : nullptr;      // the last layer writes the caller's frames
        const ConvArgs a = fill_conv_args(net, k, ch, c, buf, cur, dst);
        if (taps && k > 0 && taps->act[k] && launch_unpack_nhwc16(cur, (signed char *)taps->act[k], N, net->layers[k].ic, H, W, st)) {
            set_error("sesrq_forward: debug unpack launch failed"); return 1;
        }
        LaunchSlot slot(launch, announced, ev);
        if (!slot.ok || (ch.mfma ? launch_mfma(net->layers[k], ch, a, st) : launch_dot4(net->layers[k], ch, a, st))) return 1;
        cur = dst;
        ++k;
    }
    return 0;
}

}  // namespace sesrq

extern "C" {

int sesrq_forward_debug(const sesrq_net *net, const void *in, int in_dtype, void *out_q, void *out_f, int N, int H, int W,
                        void *workspace, size_t workspace_bytes, void *stream, const sesrq_taps *taps) {
    return forward_impl(net, {in, in_dtype, out_q, out_f, N, H, W, taps, nullptr}, workspace, workspace_bytes, stream, nullptr);
}

int sesrq_forward(const sesrq_net *net, const void *in, int in_dtype, void *out_q, void *out_f, int N, int H, int W,
                  void *workspace, size_t workspace_bytes, void *stream) {
    return forward_impl(net, {in, in_dtype, out_q, out_f, N, H, W, nullptr, nullptr}, workspace, workspace_bytes, stream, nullptr);
}

int sesrq_forward_timed(const sesrq_net *net, const void *in, int in_dtype, void *out_q, void *out_f, int N, int H, int W,
                        void *workspace, size_t workspace_bytes, void *stream, int iters, float *launch_ms, float *forward_ms) {
    if (!net || iters < 1 || !launch_ms) { set_error("sesrq_forward_timed: bad argument"); return 1; }
    const int NL = sesrq_launch_plan(net, nullptr, nullptr);
    std::vector<hipEvent_t> ev((size_t)2 * NL * iters, nullptr);
    int rc = 0;
    for (auto &e : ev)
        if (hipEventCreate(&e) != hipSuccess) { set_error("sesrq_forward_timed: hipEventCreate failed"); e = nullptr; rc = 1; break; }
    for (int it = 0; it < iters && !rc; ++it)
        rc = forward_impl(net, {in, in_dtype, out_q, out_f, N, H, W, nullptr, nullptr}, workspace, workspace_bytes, stream, ev.data() + (size_t)2 * NL * it);
    if (!rc && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { set_error("hipStreamSynchronize failed"); rc = 1; }
    if (!rc) {
        for (int k = 0; k < NL; ++k) launch_ms[k] = 0.f;
        double fw = 0;
        for (int it = 0; it < iters; ++it) {
            hipEvent_t *e = ev.data() + (size_t)2 * NL * it;
            for (int k = 0; k < NL; ++k) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, e[2 * k], e[2 * k + 1]);
                launch_ms[k] += ms / iters;
            }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e[0], e[2 * NL - 1]);
            fw += ms;
        }
        if (forward_ms) *forward_ms = (float)(fw / iters);
    }
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

}  // extern "C"
