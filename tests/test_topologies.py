"""The topologies sesrq_create accepts, off the 16-wide depth-5 / depth-8 path every other module runs: depths 3..16, hidden widths 1..15.

sesrq_create validates n_layers 3..16, 1..16 channels per layer, 3x3 / 5x5 anywhere, PixelShuffle 1..4.  What only runs when a hidden
width is below 16 or the depth is not 5 or 8 -- the zero-fill of the weight images, the requant constants and the downstream reads of the
padding lanes of an NHWC16 tensor, PEs with fewer (or no) channels, trio planning with single layers in front -- is compared here, bit for
bit, with the C oracle (tests/topologies.py builds the nets):

  id     L  kernel sizes    hidden widths  cin->cout, ps   what it reaches
  t3     3  5,3,5           16,16          3->12, 2        layer 1 is first-hidden and residual-merging at once; no trio
  t3n    3  3,3,3           8,8            1->4, 2         dot4 first / last by kernel size, narrow, 4-channel output
  t4     4  5,3,3,5         12,9,12        2->8, 2         unequal widths, widths not 0 mod 4
  t4s    4  5,3,5,5         5,7,5          1->16, 4        PEs with 2/1/1/1 and 2/2/2/1 channels, 5x5 hidden
  t6     6  5,3,3,3,3,5     16 x 5         3->3, 1         one single layer in front of the trio
  t7     7  5,3 x 5,5       16 x 6         3->12, 2        two single layers in front of the trio
  t16    16 5,3 x 14,5      16 x 15        3->12, 2        four trios + two singles: the SESRQ_MAX_LAYERS bound
  t16n   16 5,3 x 14,5      13 x 15        4->9, 3         deepest accepted net, no trio, PixelShuffle 3
  t1     5  5,3,3,3,5       1,1,1,1        1->1, 1         one channel everywhere: PEs 1..3 empty in every hidden layer
  t15    5  5,3,3,3,5       15 x 4         3->12, 2        one padding lane: the closest miss of the trio condition
  tmix   5  5,3,3,3,5       16,4,16,16     3->12, 2        a 4-wide bottleneck: stale lanes 4..15 of the NHWC16 slot must not leak

The CPU part pins the two oracles to each other on every case, shows that every case is live (an output that is one constant would
equal the oracle's whatever the kernels did with the padding lanes), pins sesrq_saturation_verdict on layers whose PEs own unequal
numbers of channels or none, and the refusals of sesrq_create at the edges of the family.  Every comparison is exact.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import Arena, bundle_from_oracle, device, fixture_case, rand_frame, same, stream_ptr, to_device
from oracle import c_oracle as CO
from oracle import sesrq_oracle as O
from planner import expected_plan_and_engines, np_verdict, verdicts
from topologies import NARROW, RISKY, SEAM_FRAMES as SIZES, TOPOLOGIES, case_net, risky_net, topo_net
import sesrq
from sesrq import _lib

IDS = list(TOPOLOGIES)
CASES = [(t, h) for t in IDS for h in (False, True)]
CASE_IDS = [f"{t}-{'hard' if h else 'plain'}" for t, h in CASES]
FRAMES = ((1, 1, 1),) + SIZES          # SIZES: (2, 21, 70), (1, 41, 130) cross a 64-column strip, a row tile and a frame seam
TAP_FRAME = (1, 13, 37)
GROUP_FRAME, GROUP_COUNT = (1, 9, 61), 6
PLANS = [("default", dict()), ("per-layer", dict(fuse_hidden=0)), ("dot4", dict(engine=_lib.ENGINE_DOT4)), ("general", dict(force_general=True))]
# launch plans the issue states in full; t16: two singles, then trios at 3, 6, 9, 12
STATED_PLANS = {"t6": [(0, 1), (1, 1), (2, 3), (5, 1)], "t7": [(0, 1), (1, 1), (2, 1), (3, 3), (6, 1)],
                "t16": [(0, 1), (1, 1), (2, 1), (3, 3), (6, 3), (9, 3), (12, 3), (15, 1)],
                "t15": [(k, 1) for k in range(5)], "tmix": [(k, 1) for k in range(5)]}
# ... and what the reference's three 5-layer nets run by default (tests/golden/<name>.crop.npz): one trio, and the first / last kernels
GOLDEN_PLANS = {"nrdm_3": ("mfma-f5-merged", "mfma-h5p-merged"), "sesr_x4": ("mfma-f5-merged", "mfma-h5-merged"),
                "sesr_x2_rand": ("mfma-f5-hybrid", "mfma-h5-general")}


def _cin(net):
    return net.layers[0].wq.shape[1]


def _frame(net, shape, k=0):
    """The case's frame of a shape: one seeded draw per (channels, shape, k), the same in the CPU and the GPU part."""
    N, H, W = shape
    return rand_frame((N, _cin(net), H, W), 1000 + H * W + 7919 * k)


@functools.lru_cache(maxsize=None)
def _want(net_key, shape, k=0):
    """The C oracle's q_out and y of a case on its frame: computed once, shared, read-only."""
    net = _net(net_key)
    x = _frame(net, shape, k)
    res = CO.forward(net, x)
    res = dict(x=x, q0=O.quantize_input(x, net.scale[0], net.zero[0], quan_bits=net.quan_bits), q_out=res["q_out"], y=res["y"])
    for v in res.values():
        v.setflags(write=False)
    return res


def _net(key):
    """key: (id, hard) | (id, hard, quan_bits) | ("risky", id, layer, pe, seed)."""
    if key[0] == "risky":
        return risky_net(*key[1:])
    return case_net(*key)


# ================================================================================================================== CPU part
def _liveness(q):
    vals, counts = np.unique(q, return_counts=True)
    return len(vals), counts.max() / q.size


@pytest.mark.parametrize("tid,hard", CASES, ids=CASE_IDS)
def test_oracles_agree_off_the_16_wide_path(tid, hard):
    """oracle.forward == c_oracle.forward, every stage, on a 2 x cin x 9 x 21 frame (stages of the first image: what the taps hold)."""
    net = case_net(tid, hard)
    x = rand_frame((2, _cin(net), 9, 21), 5)
    a, c = O.forward(net, x), CO.forward(net, x)
    np.testing.assert_array_equal(c["q_out"], a["q_out"])
    np.testing.assert_array_equal(c["y"].view(np.uint32), a["y"].view(np.uint32))
    a, c = O.forward(net, x[:1], keep=True), CO.forward(net, x[:1], keep=True)
    for k, l in enumerate(net.layers):
        oc, ic = l.wq.shape[:2]
        assert a[f"input{k}"].shape == (1, ic, 9, 21) and a[f"pe_out{k}"].shape == (4, oc, 9, 21)
        np.testing.assert_array_equal(c[f"input{k}"], a[f"input{k}"])
        np.testing.assert_array_equal(c[f"pe_out{k}"], a[f"pe_out{k}"])
        np.testing.assert_array_equal(c[f"pe_add{k}"], a[f"pe_add{k}"])


@pytest.mark.parametrize("tid,hard", CASES, ids=CASE_IDS)
def test_cases_are_live(tid, hard):
    """Every frame the GPU part compares (but the single pixel) carries at least 32 distinct output bytes, none on more than 60 % of the
    pixels -- shown on the oracle alone.  (1, 1, 1) has cout * ps^2 bytes: it checks the walk, not the arithmetic."""
    net = case_net(tid, hard)
    for shape, k in [(s, 0) for s in SIZES + (TAP_FRAME,)] + [(GROUP_FRAME, k) for k in range(GROUP_COUNT) if tid in ("t3", "t7", "t15")]:
        n, top = _liveness(_want((tid, hard), shape, k)["q_out"])
        assert n >= 32 and top <= 0.6, (tid, hard, shape, k, n, top)
    assert _want((tid, hard), (1, 1, 1))["q_out"].size == net.layers[-1].wq.shape[0]


def test_narrow_and_risky_cases_are_live():
    """The nets of the narrow-datapath and hybrid tests.  A width b has 2^b codes: both clamp ends and more than half of the codes are
    present, none on more than 60 % of the pixels.  The risky nets: the 8-bit condition, exactly one risky PE, and only in its layer."""
    for tid, b, hard in NARROW:
        net = case_net(tid, hard, b)
        for shape in SIZES:
            q = _want((tid, hard, b), shape)["q_out"]
            n, top = _liveness(q)
            assert q.min() == net.qlo and q.max() == net.qhi and n > (1 << (b - 1)) and top <= 0.6, (tid, b, hard, shape, n, top)
            np.testing.assert_array_equal(O.forward(net, _frame(net, shape))["q_out"], q)         # the numpy oracle at the width
    assert set(NARROW) == {(t, b, h) for t in ("t3", "t4", "t6") for b in (4, 2) for h in (False, True)}
    for tid, layer, pe, seed, _ in RISKY:
        net = risky_net(tid, layer, pe, seed)
        for shape in SIZES:
            n, top = _liveness(_want(("risky", tid, layer, pe, seed), shape)["q_out"])
            assert n >= 32 and top <= 0.6, (tid, layer, pe, shape, n, top)
        for k, v in enumerate(verdicts(net)):
            assert v["risky_mask"] == ((1 << pe) if k == layer else 0) and v["biased_ok"], (tid, layer, pe, k, v)
        assert len(range(pe, net.layers[layer].wq.shape[1], 4)) >= 1
    ic9, ic15 = case_net("t4").layers[2].wq.shape[1], case_net("t15").layers[2].wq.shape[1]
    assert [len(range(p, ic9, 4)) for p in range(4)] == [3, 2, 2, 2] and [len(range(p, ic15, 4)) for p in range(4)] == [4, 4, 4, 3]


def test_saturation_verdict_on_layers_with_unequal_and_empty_pes():
    """sesrq_saturation_verdict == the numpy restatement for ic in {1, 2, 3, 5, 9, 13} x oc in {1, 5, 16} x k in {3, 5}, narrow weights
    (provably safe), wide ones, and wide ones on one PE only; a PE that owns no channel is never risky."""
    rng = np.random.default_rng(11)
    seen = set()
    for ic in (1, 2, 3, 5, 9, 13):
        for oc in (1, 5, 16):
            for k in (3, 5):
                draws = [("narrow", rng.integers(-2, 3, size=(oc, ic, k, k))), ("wide", rng.choice(np.array([-128, -100, 90, 127]), size=(oc, ic, k, k)))]
                for p in range(4):
                    w = rng.integers(-1, 2, size=(oc, ic, k, k))
                    w[:, p::4] = rng.choice(np.array([-128, -110, 100, 127]), size=w[:, p::4].shape)
                    draws.append((f"pe{p}", w))
                for tag, w in draws:
                    w = w.astype(np.int8)
                    ac = rng.integers(-32768, 32768, oc).astype(np.int32)
                    for zero in (-128, -140, 0):
                        got = sesrq.saturation_verdict(w, ac, zero)
                        assert got == np_verdict(w, ac, zero, 18, 20), (ic, oc, k, tag, zero, got)
                        assert got["risky_mask"] >> min(ic, 4) == 0, (ic, oc, k, tag, got)
                        if tag == "narrow":
                            assert got["saturation_free"] and got["risky_mask"] == 0
                        if tag.startswith("pe"):      # every other PE holds weights in [-1, 1]: at most 128 * 100 per sum
                            p = int(tag[2])
                            owns = len(range(p, ic, 4)) * k * k
                            assert got["risky_mask"] & ~(1 << p) == 0 and (owns or got["risky_mask"] == 0), (ic, oc, k, tag, got)
                            if 127 * 100 * owns > 131071:      # |w| >= 100 on the PE's `owns` weights, all of one sign at the extreme
                                assert got["risky_mask"] == 1 << p, (ic, oc, k, tag, got)
                        seen.add((tag, got["risky_mask"]))
    assert ("wide", 1) in seen and ("wide", 15) in seen and ("pe1", 2) in seen and ("pe3", 0) in seen        # ic = 1: PE 0 alone; ic <= 3: PE 3 empty


def _create_raw(shapes, ps=1, zeros=None):
    """sesrq_create on a descriptor of zero weights with layers [(k, ic, oc)]: its return code and message.  No device is touched
    before the descriptor is validated."""
    L = len(shapes)
    layers = (_lib.LayerDesc * max(L, 1))()
    keep = []
    for i, (k, ic, oc) in enumerate(shapes):
        w = np.zeros(max(1, oc * ic * k * k), np.int8)
        ac = np.zeros(max(1, oc), np.int32)
        keep += [w, ac]
        layers[i] = _lib.LayerDesc(k=k, ic=ic, oc=oc, w=w.ctypes.data_as(C.POINTER(C.c_int8)), add_const=ac.ctypes.data_as(C.POINTER(C.c_int32)),
                                   M=1 << 15, n=20, relu=int(i != L - 1))
    zero = (C.c_int32 * (L + 1))(*(zeros or [-128] * (L + 1)))
    desc = _lib.NetDesc(n_layers=L, layers=layers, zero=zero, scale_in=1.0 / 255.0, scale_out=0.01, M_res=1 << 15, n_res=16, pixel_shuffle=ps,
                        pe_num=4, pe_acc_bits=18, pe_add_bits=20)
    h = C.c_void_p()
    rc = _lib.lib().sesrq_create(C.byref(desc), None, C.byref(h))
    assert rc != 0 and not h.value, "the descriptor was accepted"
    return _lib.last_error()


def test_create_refuses_what_lies_outside_the_family():
    """The edges of the accepted family stay refusals, with their messages."""
    mid = [(5, 3, 16), (3, 16, 16), (3, 16, 16), (3, 16, 16), (5, 16, 12)]
    assert _create_raw([(5, 3, 16), (3, 16, 17), (3, 17, 16), (5, 16, 12)]) == "sesrq_create: channels must be 1..16"
    assert _create_raw([(5, 0, 16)] + mid[1:]) == "sesrq_create: channels must be 1..16"
    assert _create_raw([mid[0], mid[4]]) == "sesrq_create: n_layers must be in [3,16]"
    assert _create_raw([mid[0]] + [mid[1]] * 15 + [mid[4]]) == "sesrq_create: n_layers must be in [3,16]"
    assert _create_raw([(5, 3, 16), (3, 16, 12), (5, 12, 12)]) == "sesrq_create: residual source/destination width mismatch"
    assert _create_raw(mid[:4] + [(5, 16, 9)], ps=2) == "sesrq_create: last layer channels not divisible by pixel_shuffle^2"
    assert _create_raw([(5, 5, 16)] + mid[1:]) == "sesrq_create: first layer supports 1..4 input channels"
    assert _create_raw([(5, 3, 16), (3, 15, 16), (5, 16, 12)]) == "sesrq_create: channel mismatch between consecutive layers"


def test_planner_restatement_on_the_stated_plans():
    """The restatement the GPU part compares launch_plan() with gives the plans the topology table states, and no trio off 16 channels."""
    for tid, plan in STATED_PLANS.items():
        for hard in (False, True):
            net = case_net(tid, hard)
            got, names = expected_plan_and_engines(net)
            if all(v["saturation_free"] for v in verdicts(net)[1:-1]):
                assert got == plan, (tid, hard, got)
            if tid in ("t15", "tmix"):
                assert got == plan and not any("trio" in n for n in names)
    for tid in ("t6", "t7", "t16"):       # the plain draws are saturation-free in every hidden layer: the stated plans are what runs
        assert all(v["saturation_free"] for v in verdicts(case_net(tid))[1:-1]), tid
        assert expected_plan_and_engines(case_net(tid))[0] == STATED_PLANS[tid]
        assert expected_plan_and_engines(case_net(tid), fuse_hidden=0)[0] == [(k, 1) for k in range(case_net(tid).L)]
    for tid in ("t3", "t3n", "t4", "t4s", "t16n", "t1"):
        assert all(n == 1 for _, n in expected_plan_and_engines(case_net(tid))[0]), tid
    for name, (first, last) in GOLDEN_PLANS.items():
        net = fixture_case(os.path.join(GOLDEN, f"{name}.crop.npz"))[2]
        assert expected_plan_and_engines(net) == ([(0, 1), (1, 3), (4, 1)], [first] + ["mfma-trio-merged"] * 3 + [last]), name
        for kw in (dict(fuse_hidden=0), dict(force_general=True), dict(engine=_lib.ENGINE_DOT4)):
            plan, names = expected_plan_and_engines(net, **kw)
            assert plan == [(k, 1) for k in range(5)] and not any("trio" in n for n in names), (name, kw)
        assert expected_plan_and_engines(net, fuse_hidden=0)[1] == [first] + ["mfma-h3-merged"] * 3 + [last], name


def test_topo_net_draws_are_seeded_and_shaped():
    a, b = case_net("t4s", True), topo_net((5, 7, 5), (5, 3, 5, 5), 1, 16, 4, 1, hard=True)
    assert [l.wq.shape for l in a.layers] == [(5, 1, 5, 5), (7, 5, 3, 3), (5, 7, 5, 5), (16, 5, 5, 5)]
    for la, lb in zip(a.layers, b.layers):
        assert np.array_equal(la.wq, lb.wq) and np.array_equal(la.add_const, lb.add_const) and (la.M, la.n) == (lb.M, lb.n)
    assert a.zero == b.zero and all(-150 <= z < -100 for z in a.zero) and case_net("t4s").zero == [-128] * 5
    assert topo_net((8, 8), (3, 3, 3), 1, 4, 2, 3, zeros=[-140, -120, -131, -128]).zero == [-140, -120, -131, -128]
    with pytest.raises(ValueError, match="equal widths"):
        topo_net((8, 9), (3, 3, 3), 1, 4, 2, 1)
    with pytest.raises(ValueError, match="hidden widths"):
        topo_net((8,), (3, 3, 3), 1, 4, 2, 1)


# ================================================================================================================== GPU part
def _engine(net, **kw):
    """An engine and the proof that it runs the kernels its topology is planned for: launch_plan() and layer_engines() by name."""
    e = sesrq.Engine(bundle_from_oracle(net), device(), **kw)
    plan, names = expected_plan_and_engines(net, fast_division=e.fast_division_proven(), **kw)
    assert e.launch_plan() == plan, (net.name, kw, e.launch_plan(), plan)
    assert e.layer_engines() == names, (net.name, kw, e.layer_engines(), names)
    return e


def _check_forward(tag, e, key, shape, int8_too=True):
    w = _want(key, shape)
    q, y = e.forward(to_device(w["x"]))
    same(f"{tag} {shape} q_out", q, w["q_out"])
    same(f"{tag} {shape} y", y, w["y"])
    q, y = e.forward(to_device(w["x"]), want_f=False)
    assert y is None
    same(f"{tag} {shape} q_out (int8 only)", q, w["q_out"])
    if int8_too:
        q, y = e.forward(to_device(w["q0"]))
        same(f"{tag} {shape} q_out (int8 q0 in)", q, w["q_out"])
        same(f"{tag} {shape} y (int8 q0 in)", y, w["y"])


@pytest.mark.gpu
@pytest.mark.parametrize("tid,hard", CASES, ids=CASE_IDS)
def test_engine_plans_against_the_c_oracle(tid, hard):
    """a.  Default engine, per-layer MFMA, dot4 and force_general: the planned kernels by name, q_out and y (fp32 and int8 q0 frames,
    with and without the fp32 output) equal the C oracle's on (1, 1, 1), (2, 21, 70) and (1, 41, 130)."""
    net = case_net(tid, hard)
    for tag, kw in PLANS:
        e = _engine(net, **kw)
        if tid in STATED_PLANS and not hard:
            assert e.launch_plan() == (STATED_PLANS[tid] if tag == "default" else [(k, 1) for k in range(net.L)]), (tid, tag, e.launch_plan())
        for shape in FRAMES:
            _check_forward(f"{net.name} [{tag}]", e, (tid, hard), shape)
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tid,hard", [(t, h) for t in ("t3", "t4", "t1", "tmix") for h in (False, True)],
                         ids=[f"{t}-{'hard' if h else 'plain'}" for t in ("t3", "t4", "t1", "tmix") for h in (False, True)])
def test_stage_taps_carry_the_real_channel_counts(tid, hard):
    """b.  forward_debug: every input{k}, pe_out{k}, pe_add{k}, shortcut and input4_special equals the oracle's stage of the layer's
    real width -- a wrong byte is localised to a layer, and padding lanes that cancel further down do not hide."""
    net = case_net(tid, hard)
    L = net.L
    x = _frame(net, TAP_FRAME)
    st = O.forward(net, x, keep=True)
    same("numpy oracle == C oracle", st["q_out"], _want((tid, hard), TAP_FRAME)["q_out"])
    b = bundle_from_oracle(net)
    for tag, kw, acts in (("per-layer", dict(fuse_hidden=0), True), ("per-layer, PE taps only", dict(fuse_hidden=0), False), ("dot4", dict(engine=_lib.ENGINE_DOT4), True)):
        e = sesrq.Engine(b, device(), **kw)
        res = e.forward_debug(to_device(x), pe=True, acts=acts, special=acts)
        for k, l in enumerate(net.layers):
            oc, ic = l.wq.shape[:2]
            assert tuple(res[f"pe_out{k}"].shape) == (1, 4, oc, *TAP_FRAME[1:]) and tuple(res[f"pe_add{k}"].shape) == (1, oc, *TAP_FRAME[1:])
            same(f"{net.name} [{tag}] pe_out{k}", res[f"pe_out{k}"][0], st[f"pe_out{k}"])
            same(f"{net.name} [{tag}] pe_add{k}", res[f"pe_add{k}"], st[f"pe_add{k}"])
            if acts:
                assert tuple(res[f"input{k}"].shape) == (1, ic, *TAP_FRAME[1:])
                same(f"{net.name} [{tag}] input{k}", res[f"input{k}"], st[f"input{k}"])
        if acts:
            same(f"{net.name} [{tag}] shortcut", res["shortcut"], st["shortcut"].astype(np.float32))
            same(f"{net.name} [{tag}] input4_special", res["input4_special"], st["input4_special"].astype(np.int8))
            assert res["shortcut"].shape[1] == net.layers[0].wq.shape[0] == res["input4_special"].shape[1] == net.layers[L - 2].wq.shape[0]
        same(f"{net.name} [{tag}] q_out (debug)", res["q_out"], st["q_out"])
        same(f"{net.name} [{tag}] y (debug)", res["y"], st["y"])
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tid,layer,pe,seed,owns", RISKY, ids=[f"{t}-layer{l}-pe{p}" for t, l, p, _, _ in RISKY])
def test_one_risky_pe_in_a_narrow_hidden_layer(tid, layer, pe, seed, owns):
    """c.  Exactly one PE of a hidden layer narrower than 16 channels can saturate: the layer is named -hybrid on the MFMA plans, and the
    bytes are the oracle's on all four plans (force_general is one of them)."""
    net = risky_net(tid, layer, pe, seed)
    key = ("risky", tid, layer, pe, seed)
    for tag, kw in PLANS:
        e = _engine(net, **kw)
        want = "dot4-general" if tag == "dot4" else f"mfma-h{net.layers[layer].wq.shape[2]}-hybrid"
        assert e.layer_engines()[layer] == want, (tag, e.layer_engines())
        for shape in SIZES:
            _check_forward(f"{net.name} ({owns}) [{tag}]", e, key, shape)
        e.close()


def _pe_major(a16):
    """(N, 16, H, W) channels -> (N, H, W, 16) bytes of an NHWC16 slot: byte x of a pixel holds channel (x >> 2) + 4 (x & 3)."""
    return np.ascontiguousarray(a16[:, [(x >> 2) + 4 * (x & 3) for x in range(16)]].transpose(0, 2, 3, 1))


@functools.lru_cache(maxsize=None)
def _hidden_slots(net_key, shape):
    """The 16-lane hidden tensors of the case on its frame, from the numpy oracle: {layer k: (N, H, W, 16) int8 output of layer k as the
    next layer reads it}, and "rc": the residual operand.  Lanes the layer does not have hold what a zero weight row with a zero add
    constant requantises to: t = 0 (ReLU keeps it), q = clamp8(0 + zero of the next domain) = max(zero, -128); the residual operand
    clamp8(0 - 128) = -128, and the merge of two such lanes u = -128 - 128 + 256 = 0 -> max(zero[L-1], -128)."""
    net = _net(net_key)
    L = net.L
    st = O.forward(net, _frame(net, shape), keep=True)
    out = {}
    for k in range(L - 1):
        real = st[f"input{k + 1}"]
        full = np.full((real.shape[0], 16) + real.shape[2:], max(net.zero[k + 1], -128), np.int8)
        full[:, :real.shape[1]] = real
        out[k] = _pe_major(full)
    rc = O._qb(st["shortcut"] - np.float32(128)).astype(np.int8)
    full = np.full((rc.shape[0], 16) + rc.shape[2:], -128, np.int8)
    full[:, :rc.shape[1]] = rc
    out["rc"] = _pe_major(full)
    for v in out.values():
        v.setflags(write=False)
    return out


def _check_hidden_slots(e, net, key, shape, ws, what):
    """The workspace after a forward: every hidden tensor a launch left there (layer 0's output, the last two a hidden launch wrote, the
    separate residual operand) holds the oracle's bytes in its real lanes AND the zero row's value in the lanes the layer does not have --
    the zero-fill of every weight image's output rows and the add-constant slots of the padding channels, observed where they land."""
    N, H, W = shape
    L = net.L
    slot = -(-N * H * W * 16 // 256) * 256
    want = _hidden_slots(key, shape)
    where, cur = {0: 0}, 0                       # slot index (S = 0, A = 1, B = 2) <- the layer whose output it holds last
    for first, n in e.launch_plan():
        if 0 < first < L - 1:
            cur = 2 if cur == 1 else 1
            where = {k: s_ for k, s_ in where.items() if s_ != cur}
            where[first + n - 1] = cur
    got = ws.cpu().numpy()
    assert len(where) == min(3, L - 1)
    for k, s_ in sorted(where.items()):
        view = got[s_ * slot:s_ * slot + N * H * W * 16].view(np.int8).reshape(N, H, W, 16)
        same(f"{what}: 16-lane output of layer {k} ({net.layers[k].wq.shape[0]} channels; byte x = channel (x >> 2) + 4 (x & 3))", view, want[k])
    if net.zero[1] != -128:      # layer 0 writes the residual operand apart
        assert len(got) == 4 * slot
        same(f"{what}: 16-lane residual operand", got[3 * slot:3 * slot + N * H * W * 16].view(np.int8).reshape(N, H, W, 16), want["rc"])
    else:
        assert len(got) == 3 * slot


def _forward_in_arena(e, net, key, shape, ws_fill, canary, what):
    """sesrq_forward through the C ABI with a workspace of exactly sesrq_workspace_bytes, pre-filled, inside a canary arena."""
    w = _want(key, shape)
    import torch
    N, H, W = shape
    lib = _lib.lib()
    ws_bytes = lib.sesrq_workspace_bytes(e._h, N, H, W)
    assert ws_bytes >= 3 * N * H * W * 16
    oshape = e.out_shape(N, H, W)
    n_out = int(np.prod(oshape))
    arena = Arena(device(), Arena.room(n_out, 4 * n_out, ws_bytes), canary)
    q = arena.place(oshape, torch.int8, 0, name="out_q")
    y = arena.place(oshape, torch.float32, 0, name="out_f")
    ws = arena.place(ws_bytes, torch.uint8, 16, fill=ws_fill, name="workspace")
    x = to_device(w["x"])
    rc = lib.sesrq_forward(e._h, x.data_ptr(), _lib.F32, q.data_ptr(), y.data_ptr(), N, H, W, ws.data_ptr(), ws_bytes,
                           stream_ptr())
    assert rc == 0, (what, _lib.last_error())
    torch.cuda.synchronize()
    stray = arena.check()
    assert not stray, f"{what}: bytes outside the caller's buffers changed: {stray[:6]}"
    same(f"{what} q_out", q, w["q_out"])
    same(f"{what} y", y, w["y"])
    _check_hidden_slots(e, net, key, shape, ws, what)


STALE = [(t, h) for t in ("t1", "t15", "tmix", "t3n", "t4", "t4s", "t6", "t16n") for h in (False, True)] + [("risky", "t15", 0, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("key", STALE, ids=["-".join(str(x) for x in k).replace("True", "hard").replace("False", "plain") for k in STALE])
def test_stale_workspace_and_the_padding_lanes_of_hidden_tensors(key):
    """d.  Every plan with the workspace (exactly sesrq_workspace_bytes) full of 0xFF and of 0x00 before the call: the oracle's bytes
    out -- a padding lane nobody wrote would be read as -1 or as 0, it must meet a zero weight -- and, read back from the workspace,
    every hidden tensor with all 16 lanes: the lanes a layer does not have hold what a zero row requantises to (_hidden_slots), so
    a weight image or an add-constant slot that is not zero for a channel oc <= o < 16 shows although no later layer weighs it.
    t1, t15, tmix as the issue asks; the other narrow topologies for their packers (3x3 first layer, 5x5 hidden, 13 of 16); t6 for the
    slots behind a trio; t15 with a risky PE in its 3-channel first layer for the sparse hybrid image."""
    net = _net(key)
    if key[0] == "risky":
        assert verdicts(net)[0]["risky_mask"] == 2 and _cin(net) == 3
    for tag, kw in PLANS:
        e = _engine(net, **kw)
        for shape in ((1, 1, 1), SIZES[0]):
            for ws_fill, canary in ((0xFF, 0x5A), (0x00, 0xA5)):
                _forward_in_arena(e, net, key, shape, ws_fill, canary, f"{net.name} [{tag}] {shape} workspace 0x{ws_fill:02X}")
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tid,hard", [(t, h) for t in ("t3", "t7", "t15") for h in (False, True)],
                         ids=[f"{t}-{'hard' if h else 'plain'}" for t in ("t3", "t7", "t15") for h in (False, True)])
def test_grouped_launches_equal_single_forwards(tid, hard):
    """e.  sesrq_forward_many on six (1, 9, 61) frames, group 1 and group 4: each frame's bytes are the C oracle's, which a single
    forward gives too.  On the dot4 engine grouping stays refused, with its message."""
    import torch
    net = case_net(tid, hard)
    wants = [_want((tid, hard), GROUP_FRAME, k) for k in range(GROUP_COUNT)]
    N, H, W = GROUP_FRAME
    stream = [torch.cuda.Stream(device=device())]
    for tag, kw in PLANS[:2]:
        e = _engine(net, **kw)
        frames = [to_device(w["x"]) for w in wants]
        q1, y1 = e.forward(frames[0])
        same(f"{net.name} [{tag}] single forward q", q1, wants[0]["q_out"])
        same(f"{net.name} [{tag}] single forward y", y1, wants[0]["y"])
        for group in (1, 4):
            oq = [torch.zeros(e.out_shape(N, H, W), dtype=torch.int8, device=device()) for _ in frames]
            of = [torch.zeros(e.out_shape(N, H, W), dtype=torch.float32, device=device()) for _ in frames]
            torch.cuda.synchronize()
            e.submission(frames, oq, stream, outs_f=of, group=group).enqueue(GROUP_COUNT)
            torch.cuda.synchronize()
            for k, w in enumerate(wants):
                same(f"{net.name} [{tag}] group {group} frame {k} q", oq[k], w["q_out"])
                same(f"{net.name} [{tag}] group {group} frame {k} y", of[k], w["y"])
        e.close()
    e = sesrq.Engine(bundle_from_oracle(net), device(), engine=_lib.ENGINE_DOT4)
    frames = [to_device(w["x"]) for w in wants]
    oq = [torch.zeros(e.out_shape(N, H, W), dtype=torch.int8, device=device()) for _ in frames]
    with pytest.raises(RuntimeError, match=r"group > 1 needs the MFMA first- and last-layer kernels \(this net / engine option runs them on dot4\)"):
        e.submission(frames, oq, stream, group=4).enqueue(GROUP_COUNT)
    torch.cuda.synchronize()
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tid,b,hard", NARROW, ids=[f"{t}-q{b}-{'hard' if h else 'plain'}" for t, b, h in NARROW])
def test_narrow_datapaths_on_both_engines(tid, b, hard):
    """f.  QUAN_BIT 4 and 2 on the default engine (the dot4 kernels) and on ENGINE_MFMA_Q (the width-aware MFMA kernels; t6: its trio)."""
    net = case_net(tid, hard, b)
    for tag, kw in (("default", dict()), ("mfma-q", dict(engine=_lib.ENGINE_MFMA_Q)), ("mfma-q per-layer", dict(engine=_lib.ENGINE_MFMA_Q, fuse_hidden=0))):
        e = _engine(net, **kw)
        assert e.quan_bits == b and all(n.endswith(f"-q{b}") for n in e.layer_engines())
        if tag != "default":
            assert sum(n.startswith("mfma-") for n in e.layer_engines()) >= net.L - 1, e.layer_engines()
        for shape in FRAMES:
            _check_forward(f"{net.name} [{tag}]", e, (tid, hard, b), shape)
        e.close()
    if tid == "t6":
        assert "mfma-trio-merged-q%d" % b in expected_plan_and_engines(net, engine=_lib.ENGINE_MFMA_Q)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("tid,hard", [(t, h) for t in ("t3", "t15") for h in (False, True)],
                         ids=[f"{t}-{'hard' if h else 'plain'}" for t in ("t3", "t15") for h in (False, True)])
def test_anchor_add_on_other_depths_and_widths(tid, hard):
    """g.  anchor_add (3 -> 12 channels, PixelShuffle 2): the fp32 frame is the oracle's plus the nearest-upsampled input, one fp32 add;
    the int8 frame is unaffected."""
    net = case_net(tid, hard)
    for tag, kw in PLANS:
        e2 = _engine(net, anchor_add=True, **kw)
        for shape in SIZES:
            w = _want((tid, hard), shape)
            ya = (w["y"] + np.repeat(np.repeat(w["x"], 2, axis=2), 2, axis=3)).astype(np.float32)
            q, y = e2.forward(to_device(w["x"]))
            same(f"{net.name} [{tag}] anchor {shape} q_out", q, w["q_out"])
            same(f"{net.name} [{tag}] anchor {shape} y", y, ya)
            _, y = e2.forward(to_device(w["x"]), want_q=False)
            same(f"{net.name} [{tag}] anchor {shape} y (fp32 only)", y, ya)
        e2.close()
