"""Caller-buffer contracts of every device entry (include/sesrq*.h, "Caller buffers"): what a kernel does BESIDE the tensors it is handed.

Every buffer a case passes is a placement of an arena (tests/helpers.py Arena; its self-tests: tests/test_arena.py): a 256-byte aligned
block filled with a canary, the placement at a chosen address modulo 256 with at least 256 canary bytes of its own on either side.
A case runs twice, in surroundings that differ in every byte:

                         run 1          run 2
  outputs, workspace     0x5A canary    0xA5 canary       outputs pre-filled with the canary
  fp32 inputs            NaN            -3e38             what lies around (and between) the input frames
  int8 / byte inputs     127            -128              (0x7f / 0x80 bytes around uint8 and uint16 inputs)
  workspace contents     0x00           0xFF

Both runs must equal the ORACLE (oracle/sesrq_oracle.py, oracle/calib_oracle.py, tests/image_oracle.py, tests/quality_oracle.py; never
an aligned run of the library) bit for bit -- the quality scores within the tolerance tests/test_quality.py applies to them -- and
arena.check() must find every byte outside the placements untouched.  That catches a store that spills past a frame (into the slack, the
next frame of a grouped launch, the gap between two frames), an output byte nobody wrote (it would hold the canary: two canaries, so a
value cannot equal both), a read of workspace nobody wrote, and an out-of-frame input value used where the pad value belongs.

Addresses: frames are only aligned to their element type.  int8 / uint8 buffers sit at 0, 1, 2, 3 and 7 modulo 16, fp32 buffers at 0, 4,
8 and 12, uint16 at even offsets; the workspace at 16 modulo 256 (the alignment the library asks for, and no more).  Each (engine) case
asserts that every one of its buffers saw every residue class.  In the side libraries the pointer half of each 16-byte-path predicate
(csrc/sesrq_raw.hip, sesrq_image.hip, sesrq_eval.hip `vec`) is flipped by the address alone: the same shape, aligned and misaligned.

Shapes are the smallest at which each mechanism is live: (1, 1, 1); (1, 9, 61): one column past a 60-column trio strip, one row past a
step; (2, 17, 70): the second image of a batch, ragged in both directions, across the 64-column tile."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from helpers import (Arena, bundle_from_oracle, calib_params, device, pass_equals, rand_frame, reference_levels, same, spread_like,
                     stream_ptr)
from planner import expected_plan_and_engines
from oracle import calib_oracle as CO
from oracle import sesrq_oracle as O
import image_oracle as IO
import quality_oracle as Q
import sesrq
from sesrq import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = np.array([np.nan], F32).tobytes()
NEG = np.array([-3e38], F32).tobytes()
# (canary of outputs and workspace, what surrounds fp32 inputs, what surrounds int8 / byte inputs, workspace contents)
ROUNDS = ((0x5A, NAN, bytes([0x7F]), 0x00), (0xA5, NEG, bytes([0x80]), 0xFF))
I8_OFFS = (0, 1, 2, 3, 7)
F32_OFFS = (0, 4, 8, 12)
SHAPES = ((1, 1, 1), (1, 9, 61), (2, 17, 70))
TORCH = {np.dtype(np.int8): torch.int8, np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8,
         np.dtype(np.uint16): torch.uint16, np.dtype(np.int32): torch.int32, np.dtype(np.float64): torch.float64}


class Offsets:
    """The next address class of each buffer of a case, cycling through the classes of its element size at a pace of its own (so that
    input, int8 output and fp32 output do not move in step), and the record that every class was seen."""

    def __init__(self):
        self.it, self.seen, self.classes = {}, {}, {}

    def next(self, who, classes, step=1):
        if who not in self.it:
            order = [classes[(i * step) % len(classes)] for i in range(len(classes))]
            assert sorted(order) == sorted(classes)
            self.it[who], self.seen[who], self.classes[who] = itertools.cycle(order), set(), set(classes)
        o = next(self.it[who])
        self.seen[who].add(o % 16)
        return o

    def assert_all_seen(self):
        for who, seen in self.seen.items():
            assert seen == {c % 16 for c in self.classes[who]}, (who, sorted(seen))


def _clean(what, *arenas):
    torch.cuda.synchronize()
    for a in arenas:
        stray = a.check()
        assert not stray, f"{what}: bytes outside the caller's buffers changed: {stray[:6]}"


def _put(arena, a, off, name):
    a = np.array(a, order="C", copy=True)          # the shared cases are read-only
    return arena.place(a.shape, TORCH[a.dtype], off, fill=a, name=name)


# =============================================================================================================== libsesrq: sesrq_forward
@functools.lru_cache(maxsize=None)
def _net(kind, hard=False):
    return O.synth_net(kind, 7, hard=hard)


@functools.lru_cache(maxsize=None)
def _case(kind, hard, shape, seed=0):
    """The frame, its q0 and the oracle's outputs: computed once, shared by every engine, never modified."""
    net = _net(kind, hard)
    N, H, W = shape
    x = rand_frame((N, net.layers[0].wq.shape[1], H, W), 4242 + 17 * seed + H * W)
    want = O.forward(net, x)
    res = dict(x=x, q0=O.quantize_input(x, net.scale[0], net.zero[0]), q_out=want["q_out"], y=want["y"],
               y_anchor=(want["y"] + IO.upsample2(x)).astype(F32) if net.pixel_shuffle == 2 else None)
    for v in res.values():
        if v is not None:
            v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _engine(kind, hard=False, **kw):
    return sesrq.Engine(bundle_from_oracle(_net(kind, hard)), device(), **kw)


CONFIGS = {
    "x2-default": ("sesr_x2", False, {}), "x4-default": ("sesr_x4", False, {}), "nrdm-default": ("nrdm", False, {}),
    "x2-perlayer": ("sesr_x2", False, dict(fuse_hidden=0)), "x4-perlayer": ("sesr_x4", False, dict(fuse_hidden=0)),
    "nrdm-perlayer": ("nrdm", False, dict(fuse_hidden=0)),
    "x2-dot4": ("sesr_x2", False, dict(engine=_lib.ENGINE_DOT4)), "x4-dot4": ("sesr_x4", False, dict(engine=_lib.ENGINE_DOT4)),
    "nrdm-dot4": ("nrdm", False, dict(engine=_lib.ENGINE_DOT4)),
    "x2-hard": ("sesr_x2", True, {}),
    "x2-anchor": ("sesr_x2", False, dict(anchor_add=True)),
    "x2-budget1": ("sesr_x2", False, dict(wg_budget=1)),
}


def _expect_kernels(cfg, names):
    """The case runs the kernels it is named after."""
    if cfg.endswith("dot4"):
        assert all(s.startswith("dot4") for s in names), names
    elif cfg.endswith("perlayer"):
        assert any(s.startswith("mfma") for s in names) and not any("trio" in s for s in names), names
    elif cfg.endswith("hard"):
        assert any("general" in s or "hybrid" in s for s in names), names
    else:
        assert any("trio" in s for s in names), names


def _forward_in_arenas(e, want, shape, in_kind, want_q, want_f, offs, rnd, what):
    """One sesrq_forward through the C ABI, every buffer an arena placement; the outputs and the arenas for the caller to judge."""
    canary, around_f32, around_i8, ws_fill = rnd
    N, H, W = shape
    lib = _lib.lib()
    src = want["x"] if in_kind == "f32" else want["q0"]
    ain = Arena(device(), Arena.room(src.nbytes), around_f32 if in_kind == "f32" else around_i8)
    xin = _put(ain, src, offs.next("in_" + in_kind, F32_OFFS if in_kind == "f32" else I8_OFFS), "in")
    ws_bytes = lib.sesrq_workspace_bytes(e._h, N, H, W)
    assert ws_bytes > 0
    oshape = e.out_shape(N, H, W)
    n_out = int(np.prod(oshape))
    aout = Arena(device(), Arena.room(n_out, 4 * n_out, ws_bytes), canary)
    q = aout.place(oshape, torch.int8, offs.next("out_q", I8_OFFS, 2), name="out_q") if want_q else None
    y = aout.place(oshape, torch.float32, offs.next("out_f", F32_OFFS, 3), name="out_f") if want_f else None
    ws = aout.place(ws_bytes, torch.uint8, 16, fill=ws_fill, name="workspace")      # exactly sesrq_workspace_bytes, 16-byte aligned
    rc = lib.sesrq_forward(e._h, xin.data_ptr(), _lib.F32 if in_kind == "f32" else _lib.I8, q.data_ptr() if want_q else None,
                           y.data_ptr() if want_f else None, N, H, W, ws.data_ptr(), ws_bytes, stream_ptr())
    assert rc == 0, (what, _lib.last_error())
    _clean(what, ain, aout)
    same(what + " input untouched", xin, src)
    return q, y


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_forward_in_hostile_surroundings(cfg):
    """sesrq_forward on each kernel family: every shape x output kind (int8 only, fp32 only, both: the FAST, OUTF and generic store
    flavours of the last layer) x input kind, the buffers walking through the address classes."""
    kind, hard, kw = CONFIGS[cfg]
    e = _engine(kind, hard, **kw)
    _expect_kernels(cfg, e.layer_engines())
    plan, names = expected_plan_and_engines(_net(kind, hard), fast_division=e.fast_division_proven(), **kw)
    assert e.launch_plan() == plan and e.layer_engines() == names, (cfg, e.launch_plan(), plan, e.layer_engines(), names)
    anchored = bool(kw.get("anchor_add"))
    offs = Offsets()
    for shape in SHAPES:
        want = _case(kind, hard, shape)
        for want_q, want_f in ((True, False), (False, True), (True, True)):
            for in_kind in (("f32",) if anchored else ("f32", "i8")):      # the anchor is the fp32 frame itself
                for r, rnd in enumerate(ROUNDS):
                    what = f"{cfg} {shape} in={in_kind} q={want_q} f={want_f} run {r + 1}"
                    q, y = _forward_in_arenas(e, want, shape, in_kind, want_q, want_f, offs, rnd, what)
                    if want_q:
                        same(what + " out_q", q, want["q_out"])
                    if want_f:
                        same(what + " out_f", y, want["y_anchor"] if anchored else want["y"])
    offs.assert_all_seen()


# =============================================================================================================== sesrq_forward_many
MANY = {"x2": ("sesr_x2", {}), "x4": ("sesr_x4", {}), "x2-anchor": ("sesr_x2", dict(anchor_add=True))}


@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("cfg", list(MANY))
def test_forward_many_frames_packed_in_one_pool(cfg, group):
    """Six frames' inputs in one arena at mixed addresses, their outputs in another: frame k must not spill into frame k + 1 or into
    the gap between them, grouped (a pointer table: ConvArgs::ft) or not; the anchored engine adds each frame's OWN input."""
    kind, kw = MANY[cfg]
    e = _engine(kind, False, **kw)
    lib = _lib.lib()
    shape, F = (1, 9, 61), 6
    N, H, W = shape
    wants = [_case(kind, False, shape, seed=k) for k in range(F)]
    ws_bytes = lib.sesrq_workspace_bytes(e._h, N * group, H, W)
    oshape = e.out_shape(N, H, W)
    n_out = int(np.prod(oshape))
    offs = Offsets()
    for in_kind in (("f32",) if kw else ("f32", "i8")):
        for r, (canary, around_f32, around_i8, ws_fill) in enumerate(ROUNDS):
            what = f"forward_many {cfg} group {group} in={in_kind} run {r + 1}"
            srcs = [w["x"] if in_kind == "f32" else w["q0"] for w in wants]
            ain = Arena(device(), Arena.room(*[s.nbytes for s in srcs]), around_f32 if in_kind == "f32" else around_i8)
            xs = [_put(ain, s, offs.next("in_" + in_kind, F32_OFFS if in_kind == "f32" else I8_OFFS), f"in{k}") for k, s in enumerate(srcs)]
            aout = Arena(device(), Arena.room(*([n_out, 4 * n_out] * F + [ws_bytes])), canary)
            qs, ys = [], []
            for k in range(F):
                qs.append(aout.place(oshape, torch.int8, offs.next("out_q", I8_OFFS, 2), name=f"out_q{k}"))
                ys.append(aout.place(oshape, torch.float32, offs.next("out_f", F32_OFFS, 3), name=f"out_f{k}"))
            ws = aout.place(ws_bytes, torch.uint8, 16, fill=ws_fill, name="workspace")
            io = (_lib.FrameIO * F)(*[_lib.FrameIO(xs[k].data_ptr(), qs[k].data_ptr(), ys[k].data_ptr()) for k in range(F)])
            rc = lib.sesrq_forward_many(e._h, io, F, _lib.F32 if in_kind == "f32" else _lib.I8, N, H, W,
                                        (C.c_void_p * 1)(ws.data_ptr()), ws_bytes, (C.c_void_p * 1)(stream_ptr().value), 1, group)
            assert rc == 0, (what, _lib.last_error())
            _clean(what, ain, aout)
            for k in range(F):
                same(f"{what} frame {k} out_q", qs[k], wants[k]["q_out"])
                same(f"{what} frame {k} out_f", ys[k], wants[k]["y_anchor"] if kw else wants[k]["y"])
    offs.assert_all_seen()


# =============================================================================================================== sesrq_forward_debug
def test_forward_debug_taps_in_hostile_surroundings():
    """Every tap buffer of a dot4-tapped net (the taps are stores through raw pointers) an arena placement."""
    kind, shape = "sesr_x2", (1, 9, 33)
    N, H, W = shape
    net = _net(kind)
    e = _engine(kind, False, engine=_lib.ENGINE_DOT4)
    lib = _lib.lib()
    x = rand_frame((N, 3, H, W), 99)
    st = O.forward(net, x, keep=True)
    L = net.L
    want = {"q_out": st["q_out"], "y": st["y"], "shortcut": st["shortcut"].astype(F32), "input4_special": st["input4_special"].astype(np.int8)}
    ovf = np.zeros((L, 2), np.int32)
    for k in range(L):
        want[f"input{k}"] = st[f"input{k}"].astype(np.int8)
        want[f"pe_out{k}"] = st[f"pe_out{k}"][None].astype(np.int32)
        want[f"pe_add{k}"] = st[f"pe_add{k}"].astype(np.int32)
        lo, hi = -(1 << (net.acc_bits - 1)), (1 << (net.acc_bits - 1)) - 1
        ovf[k] = int((st[f"pe_raw{k}"] > hi).sum()), int((st[f"pe_raw{k}"] < lo).sum())
    want["overflow"] = ovf
    ws_bytes = lib.sesrq_workspace_bytes(e._h, N, H, W)
    offs = Offsets()
    for r, (canary, around_f32, around_i8, ws_fill) in enumerate(ROUNDS):
        what = f"forward_debug run {r + 1}"
        ain = Arena(device(), Arena.room(x.nbytes), around_f32)
        xin = _put(ain, x, (4, 12)[r], "in")
        aout = Arena(device(), Arena.room(*([v.nbytes for v in want.values()] + [ws_bytes])), canary)
        bufs = {}
        for name, v in want.items():
            classes, step = (I8_OFFS, 2) if v.dtype == np.int8 else (F32_OFFS, 3)
            bufs[name] = aout.place(v.shape, TORCH[v.dtype], offs.next(str(v.dtype), classes, step), name=name)
        ws = aout.place(ws_bytes, torch.uint8, 16, fill=ws_fill, name="workspace")
        taps = _lib.Taps()
        for k in range(L):
            taps.act[k], taps.pe_out[k], taps.pe_add[k] = (bufs[f"{n}{k}"].data_ptr() for n in ("input", "pe_out", "pe_add"))
        taps.shortcut, taps.ic, taps.overflow = bufs["shortcut"].data_ptr(), bufs["input4_special"].data_ptr(), bufs["overflow"].data_ptr()
        rc = lib.sesrq_forward_debug(e._h, xin.data_ptr(), _lib.F32, bufs["q_out"].data_ptr(), bufs["y"].data_ptr(), N, H, W,
                                     ws.data_ptr(), ws_bytes, stream_ptr(), C.byref(taps))
        assert rc == 0, _lib.last_error()
        _clean(what, ain, aout)
        for name, v in want.items():
            same(f"{what} {name}", bufs[name], v)
    offs.assert_all_seen()


# =============================================================================================================== libsesrq_raw
def _spread(raw, per_code, fill):
    return np.stack([spread_like(f, per_code, fill) for f in raw])


# (raw, q0, spread) address classes: all on 16 bytes (the 16-byte path when W % 8 == 0), each buffer off it in turn (the per-pixel arm
# because of that pointer alone), q0 on 8 but not 16 (still the 16-byte path), all off
RAW_PLACES = ((0, 0, 0), (2, 0, 0), (0, 4, 0), (0, 1, 0), (0, 0, 4), (0, 8, 0), (6, 3, 12), (14, 7, 8))


@pytest.mark.parametrize("hw", [(6, 16), (6, 10)])
def test_raw_unpack_in_hostile_surroundings(hw):
    """sesrq_raw_unpack against what tests/test_raw.py compares with: the reference's per-code fp32 levels at the site channel (0 at
    the non-sites) and the oracle's input quantiser of those levels."""
    from sesrq import raw as R
    H, W = hw
    s0, z0 = 0.0038037779284458536, -128
    lv = reference_levels()
    tq = O.quantize_input(lv, s0, z0)
    rng = np.random.default_rng(H * W)
    raw = rng.integers(0, 4096, (2, H, W)).astype(np.uint16)
    raw[0, 1, 3], raw[1, 0, 0], raw[1, H - 1, W - 1], raw[0, 2, 2] = 4095, 4096, 65535, 0
    want_q, want_sp = _spread(raw, tq, tq[0]), _spread(raw, lv, F32(0))
    ctx = R._so.context(device(), s0, z0, 0)
    for i, (ro, qo, so) in enumerate(RAW_PLACES):
        for outs in ((True, True), (True, False), (False, True)) if i in (0, 6) else ((True, True),):
            for r, (canary, _, around_i8, _) in enumerate(ROUNDS):
                what = f"raw {H}x{W} at ({ro}, {qo}, {so}) q0={outs[0]} spread={outs[1]} run {r + 1}"
                ain = Arena(device(), Arena.room(raw.nbytes), around_i8)
                rin = _put(ain, raw, ro, "raw")
                aout = Arena(device(), Arena.room(want_q.nbytes, want_sp.nbytes), canary)
                q = aout.place(want_q.shape, torch.int8, qo, name="q0") if outs[0] else None
                sp = aout.place(want_sp.shape, torch.float32, so, name="spread") if outs[1] else None
                rc = R.lib().sesrq_raw_unpack(ctx, rin.data_ptr(), q.data_ptr() if q is not None else None,
                                              sp.data_ptr() if sp is not None else None, 2, H, W, stream_ptr())
                assert rc == 0, (what, R.last_error())
                _clean(what, ain, aout)
                if outs[0]:
                    same(what + " q0", q, want_q)
                if outs[1]:
                    same(what + " spread", sp, want_sp)


# =============================================================================================================== libsesrq_image
# (source / prediction, q0 / destination, x) address classes
IMG_PLACES = ((0, 0, 0), (1, 0, 0), (0, 3, 0), (0, 0, 4), (0, 2, 8), (5, 7, 12))


@pytest.mark.parametrize("form", ["y", "rgb"])
@pytest.mark.parametrize("hw", [(8, 16), (7, 9)])
def test_image_decode_in_hostile_surroundings(hw, form):
    """sesrq_image_decode against tests/image_oracle.py.  At 7 x 9 the second frame's runs are off 16 bytes whatever the base: one
    launch mixes the 16-byte and the per-pixel path."""
    from sesrq import image as I
    H, W = hw
    s0, z0 = 1.0 / 255.0 * 1.07, -121
    rng = np.random.default_rng(H * W + len(form))
    img = rng.integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    img[0, 0, 0], img[1, H - 1, W - 1] = 255, 0
    ctx = I._so.context(device(), s0, z0, 0)
    for i, (so, qo, xo) in enumerate(IMG_PLACES):
        order = ("rgb", "bgr")[i % 2]
        want_x = np.ascontiguousarray(IO.decode(img, form, order))
        want_q = IO.q0(want_x, s0, z0)
        for outs in ((True, True), (True, False), (False, True)) if i in (0, 5) else ((True, True),):
            for r, (canary, _, around_i8, _) in enumerate(ROUNDS):
                what = f"decode {form} {order} {H}x{W} at ({so}, {qo}, {xo}) q0={outs[0]} x={outs[1]} run {r + 1}"
                ain = Arena(device(), Arena.room(img.nbytes), around_i8)
                src = _put(ain, img, so, "img")
                aout = Arena(device(), Arena.room(want_q.nbytes, want_x.nbytes), canary)
                q = aout.place(want_q.shape, torch.int8, qo, name="q0") if outs[0] else None
                x = aout.place(want_x.shape, torch.float32, xo, name="x") if outs[1] else None
                rc = I.lib().sesrq_image_decode(ctx, src.data_ptr(), I._form(form), I._order(order), q.data_ptr() if q is not None else None,
                                                x.data_ptr() if x is not None else None, 2, H, W, stream_ptr())
                assert rc == 0, (what, I.last_error())
                _clean(what, ain, aout)
                if outs[0]:
                    same(what + " q0", q, want_q)
                if outs[1]:
                    same(what + " x", x, want_x)


@pytest.mark.parametrize("dtype", ["f32", "i8"])
@pytest.mark.parametrize("Ch", [1, 3])
@pytest.mark.parametrize("hw", [(8, 16), (7, 9)])
def test_image_export_in_hostile_surroundings(hw, Ch, dtype):
    """sesrq_image_export of fp32 and int8 predictions against tests/image_oracle.py."""
    from sesrq import image as I
    H, W = hw
    scale, zero = 0.0047, -119
    rng = np.random.default_rng(H * W + Ch)
    if dtype == "f32":
        pred = (rng.random((2, Ch, H, W)) * 1.4 - 0.2).astype(F32)
        pred[0, 0, 0, :4] = (0.0, 1.0, F32(1.0 / 255.0), F32(254.999 / 255.0))
        deq = pred
    else:
        pred = rng.integers(-128, 128, (2, Ch, H, W)).astype(np.int8)
        deq = IO.dequant(pred, scale, zero)
    for i, (po, do, _) in enumerate(IMG_PLACES):
        po = po * 4 if dtype == "f32" and po % 4 else po            # fp32 predictions at 4-byte classes
        order = ("rgb", "bgr")[i % 2]
        want = IO.export(deq, order)
        for r, (canary, around_f32, around_i8, _) in enumerate(ROUNDS):
            what = f"export {dtype} C={Ch} {order} {H}x{W} at ({po}, {do}) run {r + 1}"
            ain = Arena(device(), Arena.room(pred.nbytes), around_f32 if dtype == "f32" else around_i8)
            src = _put(ain, pred, po, "pred")
            aout = Arena(device(), Arena.room(want.nbytes), canary)
            out = aout.place(want.shape, torch.uint8, do, name="out")
            rc = I.lib().sesrq_image_export(src.data_ptr(), I.PRED_F32 if dtype == "f32" else I.PRED_I8, scale, zero, Ch, I._order(order),
                                            out.data_ptr(), 2, H, W, stream_ptr())
            assert rc == 0, (what, I.last_error())
            _clean(what, ain, aout)
            same(what, out, want)


# =============================================================================================================== libsesrq_eval
def _scores_ok(what, got, want):
    """The tolerance of tests/test_quality.py (_check): |psnr| <= 1e-5, |ssim| <= 1e-6."""
    assert got.shape == want.shape and np.isfinite(got).all(), (what, got)
    for n in range(len(want)):
        assert abs(got[n, 1] - want[n, 1]) <= 1e-5, (what, n, got[n, 1], want[n, 1])
        assert abs(got[n, 2] - want[n, 2]) <= 1e-6, (what, n, got[n, 2], want[n, 2])


# (pred, gt, anchor) address classes; an int8 prediction takes the first modulo its own classes
EVAL_PLACES = ((0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (8, 12, 8), (12, 8, 12))
EVAL_I8 = (0, 4, 1, 2, 3, 7)


@pytest.mark.parametrize("form", ["rgb-f32", "rgb-i8", "y255-f32", "y255-i8", "x2-f32", "x2-anchored"])
@pytest.mark.parametrize("wide", [True, False], ids=["w%4==0", "w%4!=0"])
def test_quality_score_in_hostile_surroundings(wide, form):
    """sesrq_eval / sesrq_eval_anchored at the smallest frame the entry accepts, once with W % 4 == 0 (the 16-byte loads when the
    pointers allow) and once without, against tests/quality_oracle.py; the partial-sum workspace and the result in the arena too."""
    from sesrq import quality as QL
    kind, dt = form.split("-")
    anchored = dt == "anchored"
    H, W = ((8, 8) if wide else (8, 10)) if anchored else ((7, 8) if wide else (7, 7))
    mflag, Ch, fcode = {"rgb": (3, 3, QL.FORM_RGB), "y255": (5, 1, QL.FORM_Y255), "x2": (6, 3, QL.FORM_X2)}[kind]
    scale, zero = 0.0051, -117
    rng = np.random.default_rng(H * W + Ch)
    gt = rng.random((2, Ch, H, W)).astype(F32)
    lr = None
    if dt == "i8":
        pred = rng.integers(-128, 128, (2, Ch, H, W)).astype(np.int8)
        seen = IO.dequant(pred, scale, zero)
    else:
        pred = (gt + rng.normal(0, 0.05, gt.shape)).astype(F32)
        pred[0, 0, 0, 0], pred[1, -1, -1, -1] = 1.3, -0.2          # clipped
        seen = pred
        if anchored:
            lr = (rng.random((2, Ch, H // 2, W // 2)) * 0.5).astype(F32)
            seen = (pred + IO.upsample2(lr)).astype(F32)
    want = Q.metrics(seen, gt, mflag)
    ws_bytes = QL.lib().sesrq_eval_workspace_bytes(2, Ch, H, W)
    assert ws_bytes > 0
    desc = QL.EvalDesc(form=fcode, pred_dtype=QL.PRED_I8 if dt == "i8" else QL.PRED_F32, pred_scale=scale if dt == "i8" else 0.0,
                       pred_zero=zero if dt == "i8" else 0)
    for i, (po, go, ao) in enumerate(EVAL_PLACES):
        po = EVAL_I8[i] if dt == "i8" else po
        for r, (canary, around_f32, around_i8, ws_fill) in enumerate(ROUNDS):
            what = f"eval {form} {H}x{W} at ({po}, {go}, {ao}) run {r + 1}"
            af = Arena(device(), Arena.room(gt.nbytes, gt.nbytes, gt.nbytes), around_f32)
            g = _put(af, gt, go, "gt")
            a8 = Arena(device(), Arena.room(gt.nbytes), around_i8)
            p = _put(a8 if dt == "i8" else af, pred, po, "pred")
            a = _put(af, lr, ao, "lr") if anchored else None
            aout = Arena(device(), Arena.room(48, ws_bytes), canary)
            out = aout.place((2, 3), torch.float64, 8 + 16 * (i % 2), name="out")
            ws = aout.place(ws_bytes, torch.uint8, 16, fill=ws_fill, name="workspace")
            if anchored:
                rc = QL.anchored_lib().sesrq_eval_anchored(C.byref(desc), p.data_ptr(), a.data_ptr(), g.data_ptr(), 2, Ch, H, W,
                                                           out.data_ptr(), ws.data_ptr(), ws_bytes, stream_ptr())
            else:
                rc = QL.lib().sesrq_eval(C.byref(desc), p.data_ptr(), g.data_ptr(), 2, Ch, H, W, out.data_ptr(), ws.data_ptr(), ws_bytes,
                                         stream_ptr())
            assert rc == 0, (what, QL.last_error())
            _clean(what, af, a8, aout)
            _scores_ok(what, out.cpu().numpy(), want)


# =============================================================================================================== calibration front end
@pytest.mark.parametrize("entry,case", [("enqueue", "nrdm_3"), ("enqueue", "sesr_x4"), ("enqueue_raw", "nrdm_3"),
                                        ("enqueue_image", "sesr_x4"), ("enqueue_image", "sesr_x2_rand")])
def test_calibrator_frames_at_odd_offsets(entry, case):
    """Calibrator.enqueue / enqueue_raw / enqueue_image on one tiny frame at an odd element offset, its output at another: ranges and
    output equal calib_oracle.forward, as tests/test_calib_kernels.py requires of the aligned frame."""
    from sesrq.calibrate import Calibrator
    Wf, bf, ps = calib_params(case)
    cin = Wf[0].shape[1]
    H, W = 9, 33
    rng = np.random.default_rng(len(entry) + cin)
    if entry == "enqueue":
        src = (rng.random((1, cin, H, W)) * 1.2 - 0.1).astype(F32)
        x, off = src, 4
    elif entry == "enqueue_raw":
        src = rng.integers(0, 4200, (1, H, W)).astype(np.uint16)
        x, off = _spread(src, reference_levels(), F32(0)), 6
    else:
        src = rng.integers(0, 256, (1, H, W, 3)).astype(np.uint8)
        x, off = np.ascontiguousarray(IO.decode(src, "y" if cin == 1 else "rgb", "bgr")), 3
    want = CO.forward(Wf, bf, ps, [x], 8)
    for r, (canary, around_f32, around_i8, _) in enumerate(ROUNDS):
        what = f"{entry} {case} run {r + 1}"
        cal = Calibrator(Wf, bf, ps, device(), quan_bits=8)
        ain = Arena(device(), Arena.room(src.nbytes), around_f32 if entry == "enqueue" else around_i8)
        xin = _put(ain, src, off, "frame")
        aout = Arena(device(), Arena.room(want.outputs[0].nbytes), canary)
        out = aout.place(want.outputs[0].shape, torch.float32, 12, name="out")
        got = cal.enqueue(xin, out=out) if entry == "enqueue" else cal.enqueue_raw(xin, out=out) if entry == "enqueue_raw" \
            else cal.enqueue_image(xin, order="bgr", out=out)
        assert got.data_ptr() == out.data_ptr()
        _clean(what, ain, aout)
        cal.sync()
        same(what + " output", out, np.asarray(want.outputs[0], F32))
        pass_equals(what, cal, want)


# =============================================================================================================== Engine: caller outputs
def test_engine_refuses_unusable_caller_outputs():
    """Engine.forward / forward_raw / forward_image write caller outputs through data_ptr(): a short buffer, a wrong dtype, a strided
    view or another device's tensor is a ValueError before any launch, never a device-memory overrun."""
    dev = device()
    e2 = _engine("sesr_x2")
    e4 = _engine("sesr_x4")
    en = _engine("nrdm")
    x = torch.from_numpy(_case("sesr_x2", False, (1, 9, 61))["x"].copy()).to(dev)
    shp = e2.out_shape(1, 9, 61)
    st = torch.cuda.current_stream(dev)
    launches = sum(_lib.instances().values())

    def bad_outputs(shp):
        good_q, good_f = torch.empty(shp, dtype=torch.int8, device=dev), torch.empty(shp, dtype=torch.float32, device=dev)
        short = (shp[0], shp[1], shp[2] - 1, shp[3])
        wide = (shp[0], shp[1], shp[2], 2 * shp[3])
        yield "short int8", dict(out_q=torch.empty(short, dtype=torch.int8, device=dev), out_f=good_f)
        yield "short fp32", dict(out_q=good_q, out_f=torch.empty(short, dtype=torch.float32, device=dev))
        yield "flat int8 of the right size", dict(out_q=torch.empty(int(np.prod(shp)), dtype=torch.int8, device=dev))
        yield "fp32 where int8 belongs", dict(out_q=torch.empty(shp, dtype=torch.float32, device=dev))
        yield "int8 where fp32 belongs", dict(out_f=torch.empty(shp, dtype=torch.int8, device=dev))
        yield "uint8", dict(out_q=torch.empty(shp, dtype=torch.uint8, device=dev))
        yield "strided int8", dict(out_q=torch.empty(wide, dtype=torch.int8, device=dev)[..., ::2])
        yield "strided fp32", dict(out_f=torch.empty(wide, dtype=torch.float32, device=dev)[..., ::2])
        yield "host tensor", dict(out_q=torch.empty(shp, dtype=torch.int8))

    for name, kw in bad_outputs(shp):
        with pytest.raises(ValueError, match="output must be a contiguous tensor of the forward's output shape"):
            e2.forward(x, **kw)
        full = dict(out_q=torch.empty(shp, dtype=torch.int8, device=dev), out_f=torch.empty(shp, dtype=torch.float32, device=dev))
        full.update(kw)
        with pytest.raises(ValueError, match="output must be a contiguous tensor of the forward's output shape"):
            e2.forward(x, stream=st, assume_ordered=True, **full)
    raw = torch.zeros((1, 9, 61), dtype=torch.uint16, device=dev)
    for name, kw in bad_outputs(en.out_shape(1, 9, 61)):
        with pytest.raises(ValueError, match="output must be a contiguous tensor of the forward's output shape"):
            en.forward_raw(raw, **kw)
    img = torch.zeros((1, 9, 61, 3), dtype=torch.uint8, device=dev)
    for eng in (e2, e4):
        for name, kw in bad_outputs(eng.out_shape(1, 9, 61)):
            with pytest.raises(ValueError, match="output must be a contiguous tensor of the forward's output shape"):
                eng.forward_image(img, **kw)
    torch.cuda.synchronize()
    assert sum(_lib.instances().values()) == launches, "a refused call launched a kernel"
    # and the buffers the contract names are taken: the same bytes as the oracle's
    want = _case("sesr_x2", False, (1, 9, 61))
    q, y = torch.empty(shp, dtype=torch.int8, device=dev), torch.empty(shp, dtype=torch.float32, device=dev)
    rq, ry = e2.forward(x, out_q=q, out_f=y)
    torch.cuda.synchronize()
    assert rq is q and ry is y
    same("caller out_q", q, want["q_out"])
    same("caller out_f", y, want["y"])
