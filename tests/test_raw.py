"""12-bit RGGB raw frames into the 3-channel nets (sesrq.raw, libsesrq_raw.so, Engine.forward_raw, quality.evaluate_raw, sim.py --input
*.raw) against the reference's own dataset class and integer simulation (tests/golden/raw/, made by make_raw_golden.py).

CPU: the q0 table against the reference's input.0 at every site of a frame that holds every code at every Bayer phase; raw file
naming; the C ABI.  GPU: the unpacked q0 / fp32 frame against the reference's, the raw forward against the reference's outputs and
against forward() on the fp32 frame, evaluate_raw, sim.py, the refusals, a side stream, and that every kernel instantiation ran."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import (device, raw_frame, raw_frames, raw_frames_sha, ref_gt, ref_inp, reference_levels, sha256, sites,
                     spread_like)

RAW = os.path.join(GOLDEN, "raw")
HEADER = os.path.join(ROOT, "include", "sesrq_raw.h")
NETS = ("nrdm_3", "nrdm_3_qat")
FRAMES = ("a", "b", "c")


def net_fixture(net):
    z = np.load(os.path.join(RAW, net + ".npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_frame_a_holds_every_code_at_every_phase():
    raw = raw_frame("a")[0]
    assert raw.shape[0] >= 128 and raw.shape[1] >= 128
    for py in (0, 1):
        for px in (0, 1):
            ph = raw[py::2, px::2].ravel()
            assert set(range(4096)) <= set(ph.tolist()), (py, px)
            assert {4095, 4096, 4097, 65535} <= set(ph.tolist())


@pytest.mark.parametrize("net", NETS)
def test_table_equals_reference_input0_at_every_site(net):
    from sesrq import raw as R
    z, meta = net_fixture(net)
    t = R.table(meta["scale"][0], meta["zero"][0])
    for f in FRAMES:
        assert sha256(spread_like(raw_frame(f)[0], t, t[0])[None]) == meta["sha"][f"input0_{f}"], (net, f)
    assert np.array_equal(spread_like(raw_frame("a")[0], t, t[0]), z["input0_a"][0])
    # frame (a) pins every entry: each code's q0 sits at some site of it
    raw = raw_frame("a")[0]
    ref = np.take_along_axis(z["input0_a"][0], sites(*raw.shape)[None], 0)[0]
    got = np.full(4096, 999, np.int32)
    got[np.minimum(raw, 4095)] = ref
    assert np.array_equal(got, t.astype(np.int32))


def test_table_division_forms_match_the_oracle():
    from sesrq import raw as R
    from oracle import sesrq_oracle as O
    lv = reference_levels()
    assert np.array_equal(lv, raw_frames()["levels_gt"])        # inp and gt: one quotient per code
    for f in FRAMES:
        ref_inp(f), ref_gt(f)                                  # the per-code values rebuild the reference's frames exactly
    for s0, z0 in ((0.0038037779284458536, -128), (0.0031, -140), (0.0052, -120), (1.7e-3, -128)):
        for ed, recip in ((0, False), (1, False), (2, True)):
            assert np.array_equal(R.table(s0, z0, ed), O.quantize_input(lv, s0, z0, reciprocal=recip)), (s0, z0, ed)


def test_table_refuses_bad_domains():
    from sesrq import raw as R
    for s0, z0, ed in ((0.0, -128, 0), (float("inf"), -128, 0), (-1.0, 0, 0), (0.01, -128, 3), (0.01, 1 << 25, 0)):
        with pytest.raises(ValueError, match="sesrq_raw_table"):
            R.table(s0, z0, ed)


def test_load_raw_naming_shape_and_errors(tmp_path):
    from sesrq import raw as R
    a = (np.arange(5 * 7, dtype=np.uint16) * 1999).reshape(5, 7)
    d = tmp_path / "shots_day1"
    d.mkdir()
    p = d / "scene_take_2_5_7.raw"               # '_' in the directory and the name: only the basename's last two fields count
    a.astype("<u2").tofile(p)
    got = R.load_raw(str(p))
    assert got.dtype == np.uint16 and got.shape == (5, 7) and np.array_equal(got, a)
    assert R.raw_size("x/frame_1080_1920.raw") == (1080, 1920)
    a[:4].astype("<u2").tofile(d / "short_5_7.raw")
    with pytest.raises(ValueError, match="bytes"):
        R.load_raw(str(d / "short_5_7.raw"))
    for bad in ("frame.raw", "frame_12.raw", "frame_a_7.raw", "frame_5_7.png", "frame_0_7.raw"):
        with pytest.raises(ValueError):
            R.raw_size(bad)


def test_raw_library_exports_exactly_the_header():
    from sesrq import raw as R
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_raw[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 8, names
    assert sorted(R.SYMBOLS) == names, "python binding and header disagree"
    nm = subprocess.run(["nm", "-D", "--defined-only", R.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" T (sesrq\w*)", nm)))
    assert exported == names


def test_libsesrq_instances_unchanged_by_the_raw_library():
    from sesrq import _lib, raw as R
    before = _lib.instances()
    assert len(R.instances()) == 3
    after = _lib.instances()
    assert sorted(before) == sorted(after)
    assert not any("raw" in n for n in after)


def test_unpack_argument_checks_without_a_device():
    import ctypes as C
    from sesrq import raw as R
    lib = R.lib()
    fake = C.c_void_p(4096)                       # never dereferenced: the NULL-context check comes first
    assert lib.sesrq_raw_unpack(None, fake, fake, fake, 1, 8, 8, None) != 0 and R.last_error().startswith("sesrq_raw_unpack")
    assert lib.sesrq_raw_create(1.0, 0, 0, None) != 0 and "NULL" in R.last_error()
    assert lib.sesrq_raw_instance_name(3) is None and lib.sesrq_raw_instance_launches(-1) == -1


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _engine(net, **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(os.path.join(RAW, net + ".npz")), device(), **kw)


def _u16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16)).to(device())


def _batch(f, n):
    """n frames of frame f's size: frame f itself first, then its codes shuffled (seeded)."""
    raw = raw_frame(f)[0]
    rng = np.random.default_rng(7)
    return np.stack([raw] + [rng.permutation(raw.ravel()).reshape(raw.shape) for _ in range(n - 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("f", FRAMES)
def test_unpack_equals_reference_inp_and_input0(f, N):
    import torch
    from sesrq import raw as R
    from sesrq.bundle import Bundle
    lv = reference_levels()
    b = Bundle.load(os.path.join(RAW, "nrdm_3.npz"))
    z, meta = net_fixture("nrdm_3")
    t = R.table(meta["scale"][0], meta["zero"][0])
    raws = _batch(f, N)
    x = _u16(raws)
    q_both, sp_both = R.unpack(b, x, want_q=True, want_spread=True)
    q_only, _ = R.unpack(b, x.unsqueeze(1), want_q=True, want_spread=False)
    _, sp_only = R.unpack(None, x, want_q=False, want_spread=True)
    torch.cuda.synchronize()
    for q in (q_both, q_only):
        q = q.cpu().numpy()
        assert q.shape == (N, 3) + raws.shape[1:]
        assert sha256(q[:1]) == meta["sha"][f"input0_{f}"], f
        for n in range(1, N):
            assert np.array_equal(q[n], spread_like(raws[n], t, t[0])), (f, n)
    for sp in (sp_both, sp_only):
        sp = sp.cpu().numpy()
        assert sha256(sp[:1]) == raw_frames_sha()[f"inp_{f}"], f
        for n in range(1, N):
            assert spread_like(raws[n], lv, np.float32(0)).tobytes() == sp[n].tobytes(), (f, n)


@pytest.mark.gpu
def test_load_gt_equals_reference_gt():
    from sesrq import raw as R
    for f in FRAMES:
        g = R.load_gt(raw_frame(f)[1], device()).cpu().numpy()
        assert g.dtype == np.float32 and sha256(g) == raw_frames_sha()[f"gt_{f}"], f


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["auto", "dot4"])
@pytest.mark.parametrize("net", NETS)
def test_forward_raw_equals_reference_outputs(net, engine):
    import torch
    from sesrq import _lib
    z, meta = net_fixture(net)
    e = _engine(net, engine=_lib.ENGINE_AUTO if engine == "auto" else _lib.ENGINE_DOT4)
    for f in FRAMES:
        q, y = e.forward_raw(_u16(raw_frame(f)[0])[None, None])
        torch.cuda.synchronize()
        assert sha256(q.cpu().numpy()) == meta["sha"][f"out_q_{f}"], (net, engine, f)
        assert sha256(y.cpu().numpy()) == meta["sha"][f"out_{f}"], (net, engine, f)


@pytest.mark.gpu
def test_forward_raw_equals_forward_on_the_spread_1080p():
    import torch
    from sesrq import raw as R
    rng = np.random.default_rng(1080)
    raws = rng.integers(0, 4096, (1, 1080, 1920)).astype(np.uint16)
    raws[0, ::97, ::89] = 65535
    e = _engine("nrdm_3")
    x = _u16(raws)
    q, y = e.forward_raw(x)
    _, sp = R.unpack(e, x, want_q=False, want_spread=True)
    q2, y2 = e.forward(sp)
    torch.cuda.synchronize()
    assert torch.equal(q, q2)
    assert q.cpu().numpy().tobytes() == q2.cpu().numpy().tobytes() and y.cpu().numpy().tobytes() == y2.cpu().numpy().tobytes()
    # only one output asked for, and a second slot: the same bytes
    q3, none = e.forward_raw(x, want_f=False, slot=1)
    torch.cuda.synchronize()
    assert none is None and torch.equal(q3, q)


@pytest.mark.gpu
def test_evaluate_raw_equals_evaluate_on_the_spread():
    import torch
    from sesrq import quality
    raws = [raw_frame(f) for f in FRAMES]
    for net in NETS:
        e = _engine(net)
        got = quality.evaluate_raw(e, [r for r, _ in raws], [g for _, g in raws], 3)
        want = quality.evaluate(e, [torch.from_numpy(ref_inp(f)) for f in FRAMES], [torch.from_numpy(ref_gt(f)) for f in FRAMES], 3)
        assert got.shape == (3, 3) and got.tobytes() == want.tobytes(), net
    with pytest.raises(ValueError, match="MFLAG 5"):
        quality.evaluate_raw(e, [raws[0][0]], [raws[0][1]], 5)


@pytest.mark.gpu
def test_sim_raw_input_prints_the_fp32_route_mean_line(capsys, tmp_path):
    import sim
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "nrdm_3_nat.params.npz")
    raw, gt16 = raw_frame("b")
    rawp = str(tmp_path / "frameb_80_960.raw")
    raw.astype("<u2").tofile(rawp)
    np.save(str(tmp_path / "gt16.npy"), gt16)
    np.save(str(tmp_path / "inp.npy"), ref_inp("b"))
    np.save(str(tmp_path / "gt.npy"), ref_gt("b"))
    STORE.clear()
    y_raw = sim.main(["--mflag", "3", "--params", params, "--input", rawp, "--gt", str(tmp_path / "gt16.npy")])
    out_raw = capsys.readouterr().out.strip().split("\n")
    STORE.clear()
    y_f32 = sim.main(["--mflag", "3", "--params", params, "--input", str(tmp_path / "inp.npy"), "--gt", str(tmp_path / "gt.npy")])
    out_f32 = capsys.readouterr().out.strip().split("\n")
    assert out_raw[-1].startswith("nrdm_small mean psnr is: ")
    assert out_raw[-1] == out_f32[-1] and out_raw[-2] == out_f32[-2]
    assert y_raw.cpu().numpy().tobytes() == y_f32.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_forward_raw_refusals():
    import sesrq
    from sesrq.bundle import Bundle
    x = _u16(raw_frame("c")[0])[None]
    one = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "sesr_x4.crop.npz")), device())
    with pytest.raises(ValueError, match="3-channel"):
        one.forward_raw(x)
    nrdm = Bundle.load(os.path.join(RAW, "nrdm_3.npz"))
    chained = sesrq.Engine(nrdm, device(), upstream=nrdm)
    with pytest.raises(ValueError, match="upstream"):
        chained.forward_raw(x)
    anchored = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "sesr_x2_rand.crop.npz")), device(), anchor_add=True)
    with pytest.raises(ValueError, match="anchor_add"):
        anchored.forward_raw(x)
    e = _engine("nrdm_3")
    with pytest.raises(ValueError, match="uint16"):
        e.forward_raw(x.to(dtype=__import__("torch").int32))
    with pytest.raises(ValueError, match="one channel"):
        e.forward_raw(x.unsqueeze(1).expand(1, 2, *x.shape[1:]).contiguous())


@pytest.mark.gpu
def test_forward_raw_on_a_side_stream():
    import torch
    e = _engine("nrdm_3")
    want = net_fixture("nrdm_3")[1]["sha"]["out_q_b"]
    dev = device()
    side = torch.cuda.Stream(device=dev)
    src = torch.from_numpy(raw_frame("b")[0].astype(np.int32)).to(dev)
    for _ in range(3):
        x = (src * 1).to(torch.uint16)[None]          # produced on the current stream just before the call
        q, y = e.forward_raw(x, stream=side)
        side.synchronize()
        assert sha256(q.cpu().numpy()) == want
        del x


@pytest.mark.gpu
def test_zz_every_raw_instance_ran():
    """LAST in this file: every kernel instantiation libsesrq_raw.so can launch was launched by a checked case above."""
    from sesrq import raw as R
    k = R.instances()
    assert len(k) == 3, k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
