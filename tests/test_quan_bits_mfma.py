"""define.py QUAN_BIT = b < 8 on the MFMA kernels: the opt-in engine ENGINE_MFMA_Q (sesrq_options.engine = SESRQ_ENGINE_MFMA_Q).

A narrow net's layers get their MFMA kinds and run on width-aware kernel flavours (mfma_*_kernel_q, the fused trio included), bit for
bit with the reference's fixtures (tests/golden/quan_bits/), with the dot4 kernels every other engine value lands on, and with the
width-aware oracles.  The flavours sit in a registry of their own (sesrq_narrow_instance_*): the last test of this file fails, by
name, for any of them that no checked case above launched.

Pad value: max(zero, -128) at every width (quan_func.py:290 tests the zero point against the literal; oracle.sesrq_oracle.conv_pe) --
not max(zero, -2^(b-1)): the hard synthetic nets (zero points down to -170) pin it.
"""
import dataclasses
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_fixture
from helpers import device, full_input, same, sha256, to_device

QB = os.path.join(GOLDEN, "quan_bits")
CROPS = sorted(glob.glob(os.path.join(QB, "*.crop.npz")))
STAGE_FILES = CROPS + sorted(glob.glob(os.path.join(QB, "*.zeros.npz")))
HIT = set()          # narrow instantiations launched inside a checked case


def _id(p):
    return os.path.basename(p)[:-4]


class Checked:
    """The narrow instantiations launched inside the block count as covered -- if the block's comparisons passed."""

    def __enter__(self):
        from sesrq import _lib
        self.before = _lib.narrow_instances()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            import torch
            from sesrq import _lib
            torch.cuda.synchronize()
            HIT.update(k for k, v in _lib.narrow_instances().items() if v > self.before.get(k, 0))
        return False


def _engine(bundle, **kw):
    import sesrq
    from sesrq import _lib
    kw.setdefault("engine", _lib.ENGINE_MFMA_Q)
    return sesrq.Engine(bundle, device(), **kw)


def _bundle(path):
    from sesrq.bundle import Bundle
    return Bundle.load(path)


def _names_ok(e, b):
    names = e.layer_engines()
    assert all(n.startswith("mfma-") and n.endswith(f"-q{b}") for n in names), names
    assert e.one_fma_layers() == [0] * len(names)          # generic epilogues only


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_the_narrow_registry_is_a_list_of_its_own():
    """Non-empty, nothing launched without a device, and none of its names in the list tests/test_instances.py drives."""
    from sesrq import _lib
    assert _lib.ENGINE_MFMA_Q == 3 and _lib.ENGINE_NAMES["mfma-q"] == 3 and _lib.lib().sesrq_version() == 4
    narrow, main = _lib.narrow_instances(), _lib.instances()
    assert len(main) == 258
    assert narrow and all(n.endswith(">") and "_q<" in n for n in narrow), sorted(narrow)
    assert not set(narrow) & set(main)
    import torch
    if not torch.cuda.is_available():
        assert all(v == 0 for v in narrow.values())


# ------------------------------------------------------------------------------------------------------------- 1. reference fixtures

@pytest.mark.gpu
@pytest.mark.parametrize("fuse", [1, 0], ids=["trio", "per-layer"])
@pytest.mark.parametrize("path", STAGE_FILES, ids=_id)
def test_reference_fixtures_on_the_narrow_engine(path, fuse):
    fx, meta = load_fixture(path)
    b = meta["quan_bits"]
    e = _engine(_bundle(path), fuse_hidden=fuse)
    assert e.quan_bits == b
    _names_ok(e, b)
    assert e.launch_plan() == ([(0, 1), (1, 3), (4, 1)] if fuse else [(k, 1) for k in range(5)])
    if fuse:
        assert e.layer_engines()[1:4] == [f"mfma-trio-merged-q{b}"] * 3
    with Checked():
        q, y = e.forward(to_device(fx["x"]))
        same("q_out", q, fx["q_out"])
        same("y", y, fx["out"])
        if meta["tag"] == "crop":          # the reference's 80 x 960 frame
            x = full_input(meta)
            assert sha256(x) == meta["full"]["x_sha256"]
            q, y = e.forward(to_device(x))
            assert list(y.shape) == meta["full"]["shape"]
            assert sha256(q.cpu().numpy()) == meta["full"]["q_out"] and sha256(y.cpu().numpy()) == meta["full"]["y"]


# ------------------------------------------------------------------------------------------------------------- 2. against the dot4 engine

DOT4_CASES = [f"{c}.q{b}.{t}" for c in ("sesr_x4", "nrdm_3", "sesr_x2_rand") for b, t in ((4, "crop"), (7, "zeros"))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DOT4_CASES)
def test_every_accepted_option_gives_the_dot4_bits(case):
    import sesrq
    from sesrq import _lib
    path = os.path.join(QB, case + ".npz")
    fx, meta = load_fixture(path)
    b, bun = meta["quan_bits"], _bundle(path)
    x = fx["x"]
    rng = np.random.default_rng(b)
    wild = rng.integers(-128, 128, size=fx["input0"].shape).astype(np.int8)          # int8 input with bytes outside the width
    opts = [dict(), dict(fuse_hidden=0), dict(force_general=True), dict(pe=(17, 17)), dict(pe=(16, 18))]
    if meta["mflag"] == 6:
        opts.append(dict(anchor_add=True))
    for kw in opts:
        kw = dict(kw)
        pe = kw.pop("pe", None)
        bb = dataclasses.replace(bun, pe_acc_bits=pe[0], pe_add_bits=pe[1]) if pe else bun
        d4 = sesrq.Engine(bb, device(), engine=_lib.ENGINE_DOT4, **kw)
        mq = _engine(bb, **kw)
        assert all(n.endswith(f"-q{b}") for n in mq.layer_engines()) and any(n.startswith("mfma-") for n in mq.layer_engines())
        inputs = [("f32", to_device(x))] + ([] if kw.get("anchor_add") else [("i8 beyond the width", to_device(wild))])
        with Checked():
            for lbl, xt in inputs:
                for wq, wf in ((True, False), (False, True), (True, True)):
                    q0, y0 = d4.forward(xt, want_q=wq, want_f=wf)
                    q1, y1 = mq.forward(xt, want_q=wq, want_f=wf)
                    if wq:
                        same(f"{case} {kw} pe={pe} [{lbl}] q", q1, q0)
                    if wf:
                        same(f"{case} {kw} pe={pe} [{lbl}] y", y1, y0)


# ------------------------------------------------------------------------------------------------------------- 3. the walk, against the oracles

SHAPES = [(1, 1, 1), (1, 7, 59), (1, 8, 60), (1, 9, 61), (2, 16, 119), (1, 17, 120), (1, 64, 180), (1, 130, 62)]


@pytest.mark.gpu
@pytest.mark.parametrize("hard", [False, True], ids=["plain", "hard"])
@pytest.mark.parametrize("b", [2, 4, 6, 7])
@pytest.mark.parametrize("kind", ["sesr_x4", "sesr_x2", "nrdm"])
def test_strip_and_step_borders_against_the_oracle(kind, b, hard):
    """test_gpu_parity.py's trio shapes (strips of 60 valid columns, 8-row steps, borders inside the 3-layer halo), wg_budget 0 and 1."""
    from helpers import bundle_from_oracle, rand_frame
    from oracle import c_oracle as CO
    from oracle import sesrq_oracle as O
    net = O.synth_net(kind, 10 * b + hard, quan_bits=b, hard=hard)
    bun = bundle_from_oracle(net)
    cin = net.layers[0].wq.shape[1]
    engines = [_engine(bun, wg_budget=w) for w in (0, 1)]
    for e in engines:
        names = e.layer_engines()
        assert all(n.endswith(f"-q{b}") for n in names) and sum(n.startswith("mfma-") for n in names) >= 4, names
    for (N, H, W) in SHAPES:
        x = rand_frame((N, cin, H, W), 7 * H + W)
        want = CO.forward(net, x, threads=4)
        if H * W < 500:          # the C oracle itself against the numpy oracle, where that is cheap
            ref = O.forward(net, x)
            same("c_oracle q", want["q_out"], ref["q_out"])
            same("c_oracle y", want["y"], ref["y"])
        with Checked():
            for w, e in zip((0, 1), engines):
                q, y = e.forward(to_device(x))
                same(f"{kind} b={b} hard={hard} {N}x{H}x{W} budget {w} q", q, want["q_out"])
                same(f"{kind} b={b} hard={hard} {N}x{H}x{W} budget {w} y", y, want["y"])
                assert int(q.min()) >= net.qlo and int(q.max()) <= net.qhi


def _variant(net, cin=None, ks=None, seed=0):
    """A synth net with its first layer cut to `cin` input channels and / or hidden layers re-drawn with kernel size ks[k] (weights in the
    width's range, the layer's requant factor scaled by the tap count): what no reference topology has, for the oracle to arbitrate."""
    from oracle import sesrq_oracle as O
    rng = np.random.default_rng(seed)
    layers = list(net.layers)
    if cin is not None:
        l = layers[0]
        layers[0] = O.Layer(**{**l.__dict__, "wq": np.ascontiguousarray(l.wq[:, :cin])})
    for k, kk in (ks or {}).items():
        l = layers[k]
        oc, ic, k0, _ = l.wq.shape
        w = rng.integers(net.qlo, net.qhi + 1, size=(oc, ic, kk, kk)).astype(np.int8)
        M, n = O.qconst(float(l.M) * 2.0 ** -int(l.n) * (k0 * k0) / (kk * kk))
        layers[k] = O.Layer(**{**l.__dict__, "wq": w, "M": M, "n": n})
    return O.Net(**{**net.__dict__, "layers": layers, "name": net.name + "_variant"})


@pytest.mark.gpu
def test_first_hidden_and_last_layer_flavours_against_the_oracle():
    """What the matrix above does not select: 1 / 2 / 3 input channels x {merged, per-PE} x {fp32, int8 frame} x {with, without the
    separate residual tensor}; 5x5 hidden layers (plain and residual-merging); an 8-conv net (two trios); every store flavour of the
    last layer."""
    import sesrq
    from helpers import bundle_from_oracle, rand_frame
    from oracle import sesrq_oracle as O
    b = 4
    cases = []
    for cin, kind in ((1, "sesr_x4"), (2, "sesr_x2"), (3, "sesr_x2"), (3, "nrdm")):
        for hard in (False, True):          # hard: zero[1] != -2^(b-1) -> the separate residual tensor
            net = O.synth_net(kind, 40 + cin, quan_bits=b, hard=hard)
            cases.append((f"{kind} cin={cin} hard={hard}", _variant(net, cin=cin) if cin == 2 else net))
    net5 = O.synth_net("sesr_x2", 50, quan_bits=b)
    cases.append(("5x5 hidden layers", _variant(net5, ks={1: 5, 3: 5}, seed=1)))
    cases.append(("8 convs: a plain trio and the residual-merging one", O.synth_net("nrdm", 70, n_blocks=6, quan_bits=b)))
    for tag, net in cases:
        bun = bundle_from_oracle(net)
        cin = net.layers[0].wq.shape[1]
        x = rand_frame((2, cin, 21, 70), 11)
        want = O.forward(net, x)
        q0 = O.quantize_input(x, net.scale[0], net.zero[0], quan_bits=net.quan_bits)
        for kw in (dict(), dict(fuse_hidden=0), dict(force_general=True)):
            e = _engine(bun, **kw)
            assert all(n.startswith("mfma-") for n in e.layer_engines()), (tag, e.layer_engines())
            with Checked():
                for lbl, xt in (("f32", to_device(x)), ("i8", to_device(q0))):
                    for wq, wf in ((True, False), (False, True), (True, True)):
                        q, y = e.forward(xt, want_q=wq, want_f=wf)
                        if wq:
                            same(f"{tag} {kw} [{lbl}] q", q, want["q_out"])
                        if wf:
                            same(f"{tag} {kw} [{lbl}] y", y, want["y"])
    # the x2 anchor add (fp32 frame out): the oracle's frame + the nearest-upsampled input, one fp32 add
    net = O.synth_net("sesr_x2", 60, quan_bits=b)
    x = rand_frame((1, 3, 21, 70), 12)
    ya = (O.forward(net, x)["y"] + np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)).astype(np.float32)
    for kw in (dict(), dict(force_general=True)):
        with Checked():
            _, y = _engine(bundle_from_oracle(net), anchor_add=True, **kw).forward(to_device(x), want_q=False, want_f=True)
            same(f"anchor {kw}", y, ya)


# ------------------------------------------------------------------------------------------------------------- 4. grouped launches

@pytest.mark.gpu
def test_grouped_launches_equal_single_frames():
    import torch
    path = os.path.join(QB, "sesr_x4.q4.crop.npz")
    fx, _ = load_fixture(path)
    e = _engine(_bundle(path))
    frames = [to_device(fx["x"] * np.float32(0.5 + 0.1 * k)) for k in range(6)]
    N, _, H, W = frames[0].shape
    want = [tuple(t.clone() for t in e.forward(f)) for f in frames]
    torch.cuda.synchronize()
    for group in (1, 2, 4):
        oq = [torch.zeros(e.out_shape(N, H, W), dtype=torch.int8, device=device()) for _ in frames]
        of = [torch.zeros(e.out_shape(N, H, W), dtype=torch.float32, device=device()) for _ in frames]
        with Checked():
            e.submission(frames, oq, [torch.cuda.Stream(device=device())], outs_f=of, group=group).enqueue(len(frames))
            torch.cuda.synchronize()
            for k in range(len(frames)):
                same(f"group {group} frame {k} q", oq[k], want[k][0])
                same(f"group {group} frame {k} y", of[k], want[k][1])


# ------------------------------------------------------------------------------------------------------------- 5. caller buffers

@pytest.mark.gpu
@pytest.mark.parametrize("q_off", [1, 7])
def test_odd_output_addresses_inside_a_canary_arena(q_off):
    import torch
    from helpers import Arena
    path = os.path.join(QB, "sesr_x2_rand.q4.crop.npz")
    fx, _ = load_fixture(path)
    e = _engine(_bundle(path))
    x = to_device(fx["x"])
    N, _, H, W = x.shape
    oshape = e.out_shape(N, H, W)
    n_out = int(np.prod(oshape))
    arena = Arena(device(), Arena.room(n_out, 4 * n_out), canary=0xA5)
    q = arena.place(oshape, torch.int8, q_off, name="out_q")
    y = arena.place(oshape, torch.float32, 4, name="out_f")
    with Checked():
        e.forward(x, out_q=q, out_f=y)
        torch.cuda.synchronize()
        same("q", q, fx["q_out"])
        same("y", y, fx["out"])
        assert arena.check() == []


# ------------------------------------------------------------------------------------------------------------- 6. b = 8

@pytest.mark.gpu
def test_at_8_bits_the_narrow_engine_is_the_mfma_engine():
    import sesrq
    from sesrq import _lib
    path = os.path.join(GOLDEN, "sesr_x4.crop.npz")
    fx, _ = load_fixture(path)
    bun = _bundle(path)
    before = _lib.narrow_instances()
    a, m = sesrq.Engine(bun, device(), engine=_lib.ENGINE_MFMA), _engine(bun)
    assert m.layer_engines() == a.layer_engines() and m.launch_plan() == a.launch_plan() and m.one_fma_layers() == a.one_fma_layers()
    assert not any("-q8" in n for n in m.layer_engines())
    qa, ya = a.forward(to_device(fx["x"]))
    qm, ym = m.forward(to_device(fx["x"]))
    same("q", qm, qa)
    same("y", ym, ya)
    same("y (reference)", ym, fx["out"])
    assert _lib.narrow_instances() == before          # no narrow instantiation launched


@pytest.mark.gpu
def test_other_engine_values_and_the_debug_forward_stay_on_dot4():
    """AUTO / DOT4 / MFMA keep landing on dot4 at b < 8 (tests/test_quan_bits.py pins it); the debug forward of a narrow-engine net runs
    on the dot4 kernels (the width-aware flavours write no taps) and gives the fixture's stages."""
    from sesrq import _lib
    path = os.path.join(QB, "nrdm_3.q4.crop.npz")
    fx, _ = load_fixture(path)
    before = _lib.narrow_instances()
    r = _engine(_bundle(path)).forward_debug(to_device(fx["x"]), pe=True, acts=True, special=True)
    for k in range(5):
        same(f"pe_out{k}", r[f"pe_out{k}"], fx[f"pe_out{k}"], reshape=True)      # stored without the batch axis
    same("q_out", r["q_out"], fx["q_out"])
    assert _lib.narrow_instances() == before
    with pytest.raises(ValueError, match="bad engine option"):
        _engine(_bundle(path), engine=4)


# ------------------------------------------------------------------------------------------------------------- 7. registry (LAST)

@pytest.mark.gpu
def test_zz_every_narrow_instance_ran():
    """LAST in this file: every width-aware instantiation the library can launch was launched by a checked case above."""
    from sesrq import _lib
    inst = _lib.narrow_instances()
    assert inst
    missing = sorted(n for n, v in inst.items() if v == 0 or n not in HIT)
    assert not missing, f"{len(missing)} of {len(inst)} narrow instantiations were never launched by a checked case:\n  " + "\n  ".join(missing)
