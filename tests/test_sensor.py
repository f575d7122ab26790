"""Bayer raw frames in a sensor's own format (sesrq.sensor, libsesrq_sensor.so, the fmt= argument of Engine.forward_raw,
Calibrator.enqueue_raw, quality.evaluate_raw and the --cfa / --black / --white / --packing flags of sim.py and test.py).

The reference has no format knob, so formats other than (rggb, 0, 4095, u16) are pinned to tests/sensor_oracle.py, a numpy restatement
of include/sesrq_sensor.h, and the restatement is pinned to the reference at that format.  Every comparison is exact: bytes for q0, bit
patterns for fp32.

CPU: the default format against the reference's fixtures and sesrq.raw; the q0 table of shallow, deep and two-level formats against the
oracle's input quantiser; the MIPI byte layouts; the C ABI; every refusal.  GPU: every code at every Bayer phase under every CFA order,
the default format against libsesrq_raw.so and the reference's SHAs, ties that need no oracle, packed against unpacked, a launch whose
loop wraps, the routes that take fmt=, and that every kernel instantiation ran."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sensor_oracle as SO
from conftest import GOLDEN, ROOT
from helpers import device, raw_frame, raw_frames, raw_frames_sha, same, sha256, spread_like

RAW = os.path.join(GOLDEN, "raw")
HEADER = os.path.join(ROOT, "include", "sesrq_sensor.h")
FRAMES = ("a", "b", "c")
F32 = np.float32
CFAS = ("rggb", "grbg", "gbrg", "bggr")
# input domains: the nrdm_3 fixture's, and one whose zero point lies below -128
DOMAINS = ((0.0038037779284458536, -128), (0.0031, -140))
DEEP_LEVELS = ((0, 4095), (64, 1023), (1024, 16383), (4096, 65535))


def net_fixture(net="nrdm_3"):
    z = np.load(os.path.join(RAW, net + ".npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def Format(*a, **kw):
    from sesrq import sensor
    return sensor.Format(*a, **kw)


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_default_format_reproduces_the_reference_and_sesrq_raw():
    from sesrq import raw as R, sensor as S
    z, meta = net_fixture()
    assert meta["scale"][0] == DOMAINS[0][0] and meta["zero"][0] == DOMAINS[0][1]
    fmt = S.Format()
    assert (fmt.cfa, fmt.black, fmt.white, fmt.packing) == ("rggb", 0, 4095, "u16")
    lv = raw_frames()["levels_inp"]
    same("oracle levels", SO.levels(0, 4095), lv)
    same("sensor.levels", S.levels(fmt), lv)
    t = S.table(fmt, meta["scale"][0], meta["zero"][0])
    same("table", t, SO.q_table(0, 4095, meta["scale"][0], meta["zero"][0]))
    for f in FRAMES:
        codes = raw_frame(f)[0][None]
        assert sha256(SO.spread(codes, t, t[0], "rggb", 0, 4095)) == meta["sha"][f"input0_{f}"], f
        assert sha256(SO.spread(codes, lv, F32(0), "rggb", 0, 4095)) == raw_frames_sha()[f"inp_{f}"], f
        same(f"oracle spread {f}", SO.spread(codes, t, t[0], "rggb", 0, 4095)[0], spread_like(codes[0], t, t[0]))
    for s0, z0 in ((0.0038037779284458536, -128), (0.0031, -140), (0.0052, -120), (1.7e-3, -128)):
        for ed in (0, 1, 2):
            same(f"table {s0} {z0} {ed}", S.table(fmt, s0, z0, ed), R.table(s0, z0, ed))


@pytest.mark.parametrize("levels", [(0, 1023), (64, 1023), (256, 4095), (0, 16383), (1024, 16383), (0, 65535), (4096, 65535), (7, 8),
                                    (0, 1)], ids=lambda l: f"{l[0]}-{l[1]}")
def test_table_equals_the_oracle_quantiser(levels):
    from sesrq import sensor as S
    black, white = levels
    fmt = S.Format(black=black, white=white)
    assert fmt.levels == white - black + 1
    same("levels", S.levels(fmt), SO.levels(black, white))
    for s0 in (DOMAINS[0][0], 1.7e-3):
        for z0 in (-128, -140, -120):
            for ed in (0, 1, 2):
                t = S.table(fmt, s0, z0, ed)
                same(f"{levels} {s0} {z0} {ed}", t, SO.q_table(black, white, s0, z0, ed))
                assert t.shape == (white - black + 1,) and np.all(np.diff(t.astype(np.int32)) >= 0), (levels, s0, z0, ed)


def test_pack_round_trips_every_code_at_every_position():
    from sesrq import sensor as S
    for packing, bits, group in (("raw10", 10, 4), ("raw12", 12, 2), ("u16", 16, 1)):
        fmt = S.Format(white=(1 << bits) - 1, packing=packing)
        codes = np.arange(1 << bits, dtype=np.uint16)
        frame = np.stack([np.roll(codes, k) for k in range(group)])           # row k: code c sits at position (c + k) % group
        for pos in range(group):
            assert set(frame[:, pos::group].ravel().tolist()) == set(codes.tolist())
        for stride, pad in ((None, 0), (fmt.row_bytes(codes.size) + 3, 0xFF)):
            rows = S.pack(frame, fmt, stride, pad)
            assert rows.dtype == np.uint8 and rows.shape == (group, stride or fmt.row_bytes(codes.size))
            same(packing + " layout", rows, SO.pack_rows(frame[None], packing, stride, pad)[0])
            same(packing + " round trip", S.unpack_host(rows, fmt, codes.size), frame)
        same(packing + " unpadded", S.unpack_host(S.pack(frame, fmt), fmt), frame)


def test_pack_byte_layout_by_hand():
    from sesrq import sensor as S
    px10 = np.array([[0x3FF, 0x000, 0x155, 0x2AA, 0x001, 0x002, 0x003, 0x204]], np.uint16)
    by10 = bytes([0xFF, 0x00, 0x55, 0xAA, 0x93, 0x00, 0x00, 0x00, 0x81, 0x39])
    px12 = np.array([[0xFFF, 0x000, 0x123, 0x456, 0xABC, 0xDEF, 0x001, 0x800]], np.uint16)
    by12 = bytes([0xFF, 0x00, 0x0F, 0x12, 0x45, 0x63, 0xAB, 0xDE, 0xFC, 0x00, 0x80, 0x01])
    for packing, white, px, by in (("raw10", 1023, px10, by10), ("raw12", 4095, px12, by12)):
        fmt = S.Format(white=white, packing=packing)
        assert S.pack(px, fmt).tobytes() == by, packing
        assert SO.pack_rows(px[None], packing).tobytes() == by, packing
        same(packing, S.unpack_host(np.frombuffer(by, np.uint8)[None], fmt), px)
        assert fmt.row_bytes(8) == len(by)
    assert S.pack(np.array([[0x1234, 0xFFFE]], np.uint16), S.Format(white=65535)).tobytes() == bytes([0x34, 0x12, 0xFE, 0xFF])


def test_sensor_library_exports_exactly_the_header():
    from sesrq import _lib, raw as R, sensor as S
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_sensor_[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 9, names
    assert sorted(S.SYMBOLS) == names, "python binding and header disagree"
    nm = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r" [TDBW] (sesrq\w*)", nm))) == names
    before, raw_before = _lib.instances(), R.instances()
    k = S.instances()
    assert len(k) == 12 and all(n.startswith("sensor_unpack<") for n in k), k
    assert sorted(_lib.instances()) == sorted(before) and sorted(R.instances()) == sorted(raw_before) and len(raw_before) == 3
    assert S.lib().sesrq_sensor_instance_name(12) is None and S.lib().sesrq_sensor_instance_launches(-1) == -1


def test_c_abi_refusals_without_a_device():
    from sesrq import sensor as S
    lib = S.lib()
    ok = S.Format().c()
    fake = C.c_void_p(4096)                       # never dereferenced: the NULL-context check comes first
    assert lib.sesrq_sensor_unpack(None, fake, 64, fake, fake, 1, 8, 8, None) != 0 and S.last_error().startswith("sesrq_sensor_unpack")
    assert lib.sesrq_sensor_create(C.byref(ok), 1.0, 0, 0, None) != 0 and "NULL" in S.last_error()
    h = C.c_void_p()
    assert lib.sesrq_sensor_create(None, 1.0, 0, 0, C.byref(h)) != 0 and "NULL" in S.last_error() and not h
    t = np.zeros(70000, np.int8)
    assert lib.sesrq_sensor_table(None, 1.0, 0, 0, t.ctypes.data, 4096) != 0 and "NULL" in S.last_error()
    assert lib.sesrq_sensor_table(C.byref(ok), 1.0, 0, 0, None, 4096) != 0 and "NULL" in S.last_error()
    assert lib.sesrq_sensor_table(C.byref(ok), 1.0, 0, 0, t.ctypes.data, 4095) != 0 and "entries" in S.last_error()
    assert lib.sesrq_sensor_table(C.byref(ok), 1.0, 0, 0, t.ctypes.data, 4096) == 0 and S.last_error() == ""
    for s0, z0, ed in ((0.0, -128, 0), (float("inf"), -128, 0), (-1.0, 0, 0), (0.01, -128, 3), (0.01, 1 << 25, 0)):
        with pytest.raises(ValueError, match="sesrq_sensor_table"):
            S.table(S.Format(), s0, z0, ed)
    # formats: (cfa, black, white, packing) as the C struct takes them
    for bad, word in (((4, 0, 4095, 0), "cfa"), ((-1, 0, 4095, 0), "cfa"), ((0, 0, 4095, 3), "packing"), ((0, -1, 4095, 0), "black"),
                      ((0, 100, 100, 0), "black"), ((0, 200, 100, 0), "black"), ((0, 0, 65536, 0), "white"), ((0, 0, 1024, 1), "white"),
                      ((0, 0, 4096, 2), "white")):
        cf = S.CFormat(*bad)
        for rc in (lib.sesrq_sensor_create(C.byref(cf), 1.0, 0, 0, C.byref(h)),
                   lib.sesrq_sensor_table(C.byref(cf), 1.0, 0, 0, t.ctypes.data, t.size)):
            assert rc != 0 and word in S.last_error() and not h, (bad, S.last_error())
        assert lib.sesrq_sensor_row_bytes(C.byref(cf), 8) == 0 and word in S.last_error(), bad
    # rows: a whole number of pack groups
    r10, r12 = S.Format(white=1023, packing="raw10").c(), S.Format(packing="raw12").c()
    assert [lib.sesrq_sensor_row_bytes(C.byref(ok), w) for w in (1, 7, 1920)] == [2, 14, 3840]
    assert [lib.sesrq_sensor_row_bytes(C.byref(r10), w) for w in (4, 40, 1920)] == [5, 50, 2400]
    assert [lib.sesrq_sensor_row_bytes(C.byref(r12), w) for w in (2, 6, 1920)] == [3, 9, 2880]
    for cf, w in ((r10, 6), (r10, 1), (r12, 3), (ok, 0), (r12, -2)):
        assert lib.sesrq_sensor_row_bytes(C.byref(cf), w) == 0 and "W = " in S.last_error(), w
    assert lib.sesrq_sensor_row_bytes(None, 8) == 0 and "NULL" in S.last_error()


def test_python_refusals_without_a_device(tmp_path):
    import torch
    from sesrq import quality, sensor as S
    for kw, word in ((dict(cfa="rgbg"), "cfa"), (dict(packing="raw14"), "packing"), (dict(black=-1), "levels"),
                     (dict(black=4095), "levels"), (dict(white=65536), "levels"), (dict(white=1024, packing="raw10"), "above the range"),
                     (dict(white=4096, packing="raw12"), "above the range"), (dict(black=1.5), "integer"), (dict(white=True), "integer")):
        with pytest.raises(ValueError, match=word):
            S.Format(**kw)
    assert S.Format(cfa="BGGR", packing="RAW10", white=1023) == S.Format("bggr", 0, 1023, "raw10")
    with pytest.raises(dataclasses_error()):
        S.Format().black = 3
    r10, r12, u16 = S.Format(white=1023, packing="raw10"), S.Format(packing="raw12"), S.Format()
    cpu = torch.device("cpu")
    for fmt, w in ((r10, 6), (r12, 3), (u16, 0)):
        with pytest.raises(ValueError, match="whole number of groups"):
            fmt.row_bytes(w)
    z8, z16 = torch.zeros((1, 3, 12), dtype=torch.uint8), torch.zeros((1, 3, 12), dtype=torch.uint16)
    assert S.frames(z8, r12, cpu)[1:] == (8, 12) and S.frames(z16, u16, cpu)[1:] == (12, 24)
    assert S.frames(z8, r12, cpu, stride=12, width=6)[1:] == (6, 12) and S.frames(z8, r10, cpu, stride=12, width=8)[1:] == (8, 12)
    for fmt, t, kw, word in ((r10, z8, {}, "give the width"),                                  # 12 bytes: no whole RAW10 groups
                             (r10, z8, dict(stride=12, width=12), "stride 12 is less than"),   # 12 pixels need 15 bytes
                             (r12, z8, dict(stride=12, width=10), "stride 12 is less than"),
                             (r10, z8, dict(stride=12, width=6), "whole number of groups"),
                             (r12, z8, dict(stride=12), "needs its width"),
                             (r12, z8, dict(stride=16, width=8), "the tensor's rows"),
                             (r12, z8, dict(width=6), "give the stride"),
                             (r12, z16, {}, "uint8"), (u16, z8, {}, "uint16"),
                             (u16, z16, dict(stride=24, width=13), "stride 24 is less than")):
        with pytest.raises(ValueError, match=word):
            S.frames(t, fmt, cpu, **kw)
    with pytest.raises(ValueError, match="HIP device"):
        S.unpack(None, z8, r12, want_q=False, want_spread=True)
    with pytest.raises(ValueError, match="q0 needs the net's input domain"):
        S.unpack(None, z8, r12)
    with pytest.raises(ValueError, match="does not fit"):
        S.pack(np.array([[1024, 0, 0, 0]], np.uint16), r10)
    with pytest.raises(ValueError, match="stride"):
        S.pack(np.zeros((1, 4), np.uint16), r10, stride=4)
    # files: the reference's naming, the size checked against rows x row_bytes
    S.pack(np.zeros((6, 8), np.uint16), r10).tofile(tmp_path / "shot_6_8.raw")
    assert S.load_raw(str(tmp_path / "shot_6_8.raw"), r10).shape == (6, 10)
    for fmt in (r12, u16):
        with pytest.raises(ValueError, match="bytes"):
            S.load_raw(str(tmp_path / "shot_6_8.raw"), fmt)
    np.zeros((5, 7), "<u2").tofile(tmp_path / "odd_5_7.raw")
    assert S.load_raw(str(tmp_path / "odd_5_7.raw"), S.Format(white=1023)).shape == (5, 7)
    with pytest.raises(ValueError, match="whole number of groups"):
        S.load_raw(str(tmp_path / "odd_5_7.raw"), r12)
    # the MFLAG 1 metric is the RGGB mosaic: every other CFA order is refused, before the engine is touched
    for cfa in CFAS[1:]:
        with pytest.raises(ValueError, match="^MFLAG 1"):
            quality.evaluate_raw(None, [], [], 1, fmt=S.Format(cfa=cfa))
    quality.check_mosaic_format(1, S.Format(black=64, white=1023))
    quality.check_mosaic_format(3, S.Format(cfa="bggr"))


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def test_cli_flag_errors_and_the_mflag_1_refusal(tmp_path):
    import sim
    import test as calib_cli
    params = os.path.join(GOLDEN, "nrdm_3_nat.params.npz")
    rawp = str(tmp_path / "f_4_8.raw")
    np.zeros((4, 8), "<u2").tofile(rawp)
    np.save(str(tmp_path / "gt16.npy"), np.zeros((1, 3, 4, 8), np.uint16))
    np.save(str(tmp_path / "x.npy"), np.zeros((1, 3, 4, 8), F32))
    base = ["--mflag", "3", "--params", params]
    for cli, inp in ((sim, ["--input", rawp]), (calib_cli, ["--input", rawp])):
        who = "sim.py" if cli is sim else "test.py"
        for flags, word in ((["--black", "4095"], "levels"), (["--white", "1024", "--packing", "raw10"], "above the range"),
                            (["--black", "-3"], "levels"), (["--white", "70000"], "levels")):
            with pytest.raises(SystemExit, match=who + ": .*" + word):
                cli.main(base + inp + flags)
        for flags in (["--cfa", "rgbg"], ["--packing", "raw14"], ["--black", "x"]):
            with pytest.raises(SystemExit):
                cli.main(base + inp + flags)
    with pytest.raises(SystemExit, match=r"sim.py: .*describe \*.raw inputs"):
        sim.main(base + ["--input", str(tmp_path / "x.npy"), "--cfa", "bggr"])
    with pytest.raises(SystemExit, match=r"test.py: .*describe \*.raw inputs"):
        calib_cli.main(base + ["--frames", str(tmp_path / "x.npy"), "--white", "1023"])
    for cfa in CFAS[1:]:
        with pytest.raises(SystemExit, match="^MFLAG 1"):
            sim.main(["--mflag", "1", "--params", params, "--input", rawp, "--gt", str(tmp_path / "gt16.npy"), "--cfa", cfa])


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(device())          # shared frames are read-only


def _launch(fmt, s0, z0, ed, rows, W, want_q=True, want_sp=True):
    """One sesrq_sensor_unpack of the device tensor `rows` (N, H, row) into fresh outputs filled with a pattern no result has."""
    import torch
    from sesrq import sensor as S
    N, H = rows.shape[0], rows.shape[1]
    q = torch.full((N, 3, H, W), 0x55, dtype=torch.int8, device=device()) if want_q else None
    sp = torch.full((N, 3, H, W), float("nan"), dtype=torch.float32, device=device()) if want_sp else None
    S.launch(device(), fmt, s0, z0, ed, rows, W, rows.shape[2] * rows.element_size(), q, sp, torch.cuda.current_stream(device()))
    return q, sp


def _check(what, fmt, s0, z0, ed, codes, rows, outs=((True, True), (True, False), (False, True))):
    """The unpack of `rows` (device) against the oracle on `codes` (host, (N, H, W)), for each output set of `outs`."""
    import torch
    t = SO.q_table(fmt.black, fmt.white, s0, z0, ed)
    want_q = SO.spread(codes, t, t[0], fmt.cfa, fmt.black, fmt.white)
    want_sp = SO.spread(codes, SO.levels(fmt.black, fmt.white), F32(0), fmt.cfa, fmt.black, fmt.white)
    for wq, ws in outs:
        q, sp = _launch(fmt, s0, z0, ed, rows, codes.shape[2], wq, ws)
        torch.cuda.synchronize()
        if wq:
            same(f"{what} q0 (q0={wq} spread={ws})", q, want_q)
        if ws:
            same(f"{what} spread (q0={wq} spread={ws})", sp, want_sp)
    return want_q, want_sp


@functools.lru_cache(maxsize=None)
def every_code_frame():
    """512 x 516 uint16: every code 0 .. 65535 at each of the four Bayer phases (a phase has 256 x 258 = 66048 sites)."""
    rng = np.random.default_rng(65536)
    f = np.empty((512, 516), np.uint16)
    for py in (0, 1):
        for px in (0, 1):
            v = np.concatenate([np.arange(65536), rng.integers(0, 65536, 66048 - 65536)]).astype(np.uint16)
            f[py::2, px::2] = rng.permutation(v).reshape(256, 258)
            assert set(f[py::2, px::2].ravel().tolist()) == set(range(65536))
    f.setflags(write=False)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("levels", DEEP_LEVELS, ids=lambda l: f"{l[0]}-{l[1]}")
@pytest.mark.parametrize("cfa", CFAS)
def test_every_code_at_every_phase(cfa, levels):
    codes = every_code_frame()[None]
    rows = _dev(codes)
    fmt = Format(cfa=cfa, black=levels[0], white=levels[1])
    for k, (s0, z0) in enumerate(DOMAINS):
        for ed in (0, 2):
            outs = ((True, True), (True, False), (False, True)) if (k, ed) == (0, 0) else ((True, True),)
            want_q, want_sp = _check(f"{cfa} {levels} z0={z0} exact_div={ed}", fmt, s0, z0, ed, codes, rows, outs)
            # the non-sites hold q0(0.0f) / 0.0f
            t0 = SO.q_table(*levels, s0, z0, ed)[0]
            assert t0 == O_quant0(s0, z0, ed)
            non = SO.sites(cfa, 512, 516)[None] != np.arange(3)[:, None, None]
            assert np.all(want_q[0][non] == t0) and np.all(want_sp[0][non].view(np.uint32) == 0)


def O_quant0(s0, z0, ed):
    from oracle import sesrq_oracle as O
    return O.quantize_input(np.zeros(1, F32), s0, z0, reciprocal=ed == 2)[0]


def _batch(f, n):
    """n frames of frame f's size: frame f itself first, then its codes shuffled (seeded), as tests/test_raw.py batches them."""
    raw = raw_frame(f)[0]
    rng = np.random.default_rng(7)
    return np.stack([raw] + [rng.permutation(raw.ravel()).reshape(raw.shape) for _ in range(n - 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("f", FRAMES)
def test_default_format_equals_libsesrq_raw_and_the_reference(f, N):
    import torch
    from sesrq import raw as R, sensor as S
    from sesrq.bundle import Bundle
    b = Bundle.load(os.path.join(RAW, "nrdm_3.npz"))
    _, meta = net_fixture()
    x = _dev(_batch(f, N))
    for wq, ws in ((True, True), (True, False), (False, True)):
        q, sp = S.unpack(b if wq else None, x if ws else x.unsqueeze(1), S.Format(), want_q=wq, want_spread=ws)
        q2, sp2 = R.unpack(b if wq else None, x, want_q=wq, want_spread=ws)
        torch.cuda.synchronize()
        if wq:
            assert sha256(q[:1].cpu().numpy()) == meta["sha"][f"input0_{f}"], f
            same("q0 against libsesrq_raw", q, q2)
        if ws:
            assert sha256(sp[:1].cpu().numpy()) == raw_frames_sha()[f"inp_{f}"], f
            same("spread against libsesrq_raw", sp, sp2)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["auto", "dot4"])
def test_forward_raw_default_format_equals_reference_outputs(engine):
    import torch
    from sesrq import _lib, sensor as S
    _, meta = net_fixture()
    e = _engine(engine=_lib.ENGINE_AUTO if engine == "auto" else _lib.ENGINE_DOT4)
    for f in FRAMES:
        q, y = e.forward_raw(_dev(raw_frame(f)[0])[None, None], fmt=S.Format())
        torch.cuda.synchronize()
        assert sha256(q.cpu().numpy()) == meta["sha"][f"out_q_{f}"], (engine, f)
        assert sha256(y.cpu().numpy()) == meta["sha"][f"out_{f}"], (engine, f)


@pytest.mark.gpu
def test_ties_that_need_no_oracle():
    import torch
    from sesrq import sensor as S
    from sesrq.bundle import Bundle
    b = Bundle.load(os.path.join(RAW, "nrdm_3.npz"))
    F = raw_frame("a")[0]                                  # every 12-bit code at every phase, and codes above 4095
    F = np.minimum(F, 60000)
    base = S.unpack(b, _dev(F), S.Format(), want_q=True, want_spread=True)
    # black level: a pedestal added to the codes and to both levels changes nothing
    for k in (64, 1000):
        got = S.unpack(b, _dev((F + k).astype(np.uint16)), S.Format(black=k, white=4095 + k), want_q=True, want_spread=True)
        torch.cuda.synchronize()
        same(f"black {k} q0", got[0], base[0])
        same(f"black {k} spread", got[1], base[1])
    # BGGR is RGGB with planes 0 and 2 swapped
    got = S.unpack(b, _dev(F), S.Format(cfa="bggr"), want_q=True, want_spread=True)
    torch.cuda.synchronize()
    for g, w, name in zip(got, base, ("q0", "spread")):
        same("bggr " + name, g, w[:, [2, 1, 0]].contiguous())
    # GRBG of F is RGGB of F moved one column: pixel (y, x) of the one is pixel (y, x + 1) of the other
    moved = np.ascontiguousarray(np.roll(F, 1, axis=1))
    got = S.unpack(b, _dev(F), S.Format(cfa="grbg"), want_q=True, want_spread=True)
    ref = S.unpack(b, _dev(moved), S.Format(), want_q=True, want_spread=True)
    torch.cuda.synchronize()
    for g, w, name in zip(got, ref, ("q0", "spread")):
        same("grbg " + name, g[..., :-1].contiguous(), w[..., 1:].contiguous())


PACKED_SHAPES = ((1, 1, 4), (2, 5, 8), (1, 3, 12), (3, 7, 40), (1, 6, 136), (1, 2, 1920))


@pytest.mark.gpu
@pytest.mark.parametrize("packing,levels", [("raw10", (64, 1023)), ("raw12", (256, 4095))])
def test_packed_equals_unpacked(packing, levels):
    import torch
    from sesrq import sensor as S
    fmt = S.Format(cfa="gbrg", black=levels[0], white=levels[1], packing=packing)
    plain = S.Format(cfa="gbrg", black=levels[0], white=levels[1])
    s0, z0 = DOMAINS[1]
    shapes = PACKED_SHAPES + (((1, 3, 2), (1, 3, 6), (1, 3, 10)) if packing == "raw12" else ())
    for i, (N, H, W) in enumerate(shapes):
        rng = np.random.default_rng(N * H * W)
        codes = rng.integers(0, levels[1] + 1, (N, H, W)).astype(np.uint16)
        codes[0, 0, :2], codes[-1, -1, -2:] = (0, levels[1]), (levels[0], levels[0] + 1)
        want = _launch(plain, s0, z0, 0, _dev(codes), W)
        nb = fmt.row_bytes(W)
        for stride, pads in ((nb, (0,)), (nb + 3, (0xFF, 0x00)), (-(-nb // 16) * 16, (0xA5,))):
            for pad in pads:
                rows = S.pack(codes, fmt, stride, pad)
                same("host round trip", S.unpack_host(rows, fmt, W), codes)
                for wq, ws in ((True, True), (True, False), (False, True)) if stride == nb else ((True, True),):
                    q, sp = _launch(fmt, s0, z0, 0, _dev(rows), W, wq, ws)
                    torch.cuda.synchronize()
                    what = f"{packing} {(N, H, W)} stride {stride} pad {pad:#x}"
                    if wq:
                        same(what + " q0", q, want[0])
                    if ws:
                        same(what + " spread", sp, want[1])
        # the entry point: unpadded rows give their width, padded rows are told it
        b = _bundle()
        q, _ = S.unpack(b, _dev(S.pack(codes, fmt)), fmt)
        q2, _ = S.unpack(b, _dev(S.pack(codes, fmt, nb + 3)), fmt, stride=nb + 3, width=W)
        q3, _ = S.unpack(b, _dev(codes), plain)
        torch.cuda.synchronize()
        same("unpack unpadded", q, q3)
        same("unpack padded", q2, q3)
    _check(f"{packing} against the oracle", fmt, s0, z0, 2, codes, _dev(S.pack(codes, fmt)), ((True, True),))


@pytest.mark.gpu
@pytest.mark.parametrize("packing", ["u16", "raw10"])
def test_the_loop_wraps(packing):
    """One launch of more segments than one grid round takes (include/sesrq_sensor.h: N H ceil(W / S) segments, S = 8 pixels of U16 and
    16 of RAW10, 256 per workgroup, 8 workgroups per compute unit): N = 3 (U16) and 5 (RAW10) frames of 1080 x 1920 on a 256-CU part."""
    import torch
    from sesrq import sensor as S
    H, W = 1080, 1920
    cus = torch.cuda.get_device_properties(device()).multi_processor_count
    round_items = cus * 8 * 256
    seg = 8 if packing == "u16" else 16
    N = round_items // (H * (W // seg)) + 1
    assert N * H * (W // seg) > round_items
    fmt = S.Format(cfa="grbg", black=1024, white=16383) if packing == "u16" else S.Format(cfa="grbg", black=64, white=1023, packing="raw10")
    rng = np.random.default_rng(N)
    codes = rng.integers(0, (1 << 14) + 100 if packing == "u16" else 1024, (N, H, W)).astype(np.uint16)
    rows = codes if packing == "u16" else S.pack(codes, fmt)
    _check(f"{packing} N={N}", fmt, *DOMAINS[0], 0, codes, _dev(rows), ((True, True),))


# ------------------------------------------------------------------------------------------------------------------------ routes
def _bundle(net="nrdm_3"):
    from sesrq.bundle import Bundle
    return Bundle.load(os.path.join(RAW, net + ".npz"))


@functools.lru_cache(maxsize=None)
def _engine(net="nrdm_3", **kw):
    import sesrq
    return sesrq.Engine(_bundle(net), device(), **kw)


def route_cases():
    from sesrq import sensor as S
    return (("10-bit bggr black 64", S.Format(cfa="bggr", black=64, white=1023), 1100),
            ("raw12 grbg black 256", S.Format(cfa="grbg", black=256, white=4095, packing="raw12"), 4096))


def _route_frame(fmt, top, shape, seed):
    from sesrq import sensor as S
    codes = np.random.default_rng(seed).integers(0, top, shape).astype(np.uint16)
    return codes, (codes if fmt.packing == "u16" else S.pack(codes, fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(1080, 1920), (80, 960)])
def test_forward_raw_with_a_format_equals_forward_on_the_spread(hw):
    import torch
    from sesrq import sensor as S
    e = _engine()
    for what, fmt, top in route_cases():
        codes, rows = _route_frame(fmt, top, (1,) + hw, hw[0])
        x = _dev(rows)
        q, y = e.forward_raw(x, fmt=fmt)
        _, sp = S.unpack(e, x, fmt, want_q=False, want_spread=True)
        q2, y2 = e.forward(sp)
        torch.cuda.synchronize()
        same(what + " spread", sp, SO.spread(codes, SO.levels(fmt.black, fmt.white), F32(0), fmt.cfa, fmt.black, fmt.white))
        same(what + " q", q, q2)
        same(what + " y", y, y2)
        q3, none = e.forward_raw(x, want_f=False, slot=1, fmt=fmt)
        torch.cuda.synchronize()
        assert none is None
        same(what + " q alone, slot 1", q3, q)


@pytest.mark.gpu
def test_narrow_engine_takes_the_fp32_route():
    import sesrq
    import torch
    from sesrq import sensor as S
    from sesrq.bundle import Bundle
    e = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "quan_bits", "nrdm_3.q4.crop.npz")), device())
    assert e.quan_bits == 4
    for what, fmt, top in route_cases():
        codes, rows = _route_frame(fmt, top, (2, 18, 32), 6)
        x = _dev(rows)
        before = S.instances()
        q, y = e.forward_raw(x, fmt=fmt)
        ran = [n for n, c in S.instances().items() if c != before[n]]
        assert len(ran) == 1 and ran[0].endswith(",spread>"), ran
        _, sp = S.unpack(None, x, fmt, want_q=False, want_spread=True)
        q2, y2 = e(sp)
        torch.cuda.synchronize()
        same(what + " q", q, q2)
        same(what + " y", y, y2)


@pytest.mark.gpu
def test_enqueue_raw_with_a_format_equals_enqueue_on_the_spread():
    import torch
    from calib_cases import calibrators
    from sesrq import sensor as S
    for what, fmt, top in route_cases():
        a, b, _ = calibrators("nrdm_3")
        for seed in (1, 2):
            codes, rows = _route_frame(fmt, top, (1, 20, 48), seed)
            x = _dev(rows)
            ya = a.enqueue_raw(x, fmt=fmt)
            _, sp = S.unpack(None, x, fmt, want_q=False, want_spread=True)
            same(what + " last_input", a.last_input, sp)
            yb = b.enqueue(sp)
            torch.cuda.synchronize()
            same(what + " output", ya, yb)
        a.sync(), b.sync()
        assert a._slots.cpu().numpy().tobytes() == b._slots.cpu().numpy().tobytes(), what
        assert a.run_min == b.run_min and a.run_max == b.run_max and a.last_scale == b.last_scale and a.last_zero == b.last_zero
        assert a.finalize() == b.finalize()


@pytest.mark.gpu
def test_evaluate_raw_with_a_format_equals_evaluate_on_the_spread():
    import torch
    from sesrq import quality, sensor as S
    e = _engine()
    for what, fmt, top in route_cases():
        pairs = []
        for seed in (3, 4):
            codes, rows = _route_frame(fmt, top, (64, 96), seed)
            gt16 = np.random.default_rng(seed + 10).integers(0, top, (3, 64, 96)).astype(np.uint16)
            pairs.append((codes, rows, gt16))
        got = quality.evaluate_raw(e, [p[1] for p in pairs], [p[2] for p in pairs], 3, fmt=fmt)
        lv = SO.levels(fmt.black, fmt.white)
        gts = [lv[np.clip(p[2].astype(np.int64), fmt.black, fmt.white) - fmt.black][None] for p in pairs]
        for p, g in zip(pairs, gts):
            same(what + " load_gt", S.load_gt(p[2], fmt, device()), g)
        sps = [SO.spread(p[0][None], lv, F32(0), fmt.cfa, fmt.black, fmt.white) for p in pairs]
        want = quality.evaluate(e, [torch.from_numpy(s) for s in sps], [torch.from_numpy(g) for g in gts], 3)
        assert got.shape == (2, 3) and got.tobytes() == want.tobytes(), (what, got, want)
    # MFLAG 1 scores the RGGB mosaic: an RGGB format at other levels is taken, every other order refused
    fmt = S.Format(black=64, white=1023)
    codes, rows = _route_frame(fmt, 1100, (64, 96), 5)
    one = quality.evaluate_raw(e, [rows], [pairs[0][2]], 1, fmt=fmt)
    assert one.shape == (1, 3) and np.isfinite(one[0, 0])
    with pytest.raises(ValueError, match="^MFLAG 1"):
        quality.evaluate_raw(e, [rows], [pairs[0][2]], 1, fmt=S.Format(cfa="bggr", black=64, white=1023))


@pytest.mark.gpu
def test_sim_sensor_flags_print_the_fp32_route_mean_line(capsys, tmp_path):
    import sim
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "nrdm_3_nat.params.npz")
    rng = np.random.default_rng(960)
    codes = rng.integers(0, 1100, (80, 960)).astype(np.uint16)
    gt16 = rng.integers(0, 1100, (1, 3, 80, 960)).astype(np.uint16)
    lv = SO.levels(64, 1023)
    rawp = str(tmp_path / "frame_80_960.raw")
    codes.astype("<u2").tofile(rawp)
    np.save(str(tmp_path / "gt16.npy"), gt16)
    np.save(str(tmp_path / "inp.npy"), SO.spread(codes[None], lv, F32(0), "bggr", 64, 1023))
    np.save(str(tmp_path / "gt.npy"), lv[np.clip(gt16.astype(np.int64), 64, 1023) - 64])
    STORE.clear()
    y_raw = sim.main(["--mflag", "3", "--params", params, "--input", rawp, "--gt", str(tmp_path / "gt16.npy"), "--cfa", "bggr",
                      "--black", "64", "--white", "1023"])
    out_raw = capsys.readouterr().out.strip().split("\n")
    STORE.clear()
    y_f32 = sim.main(["--mflag", "3", "--params", params, "--input", str(tmp_path / "inp.npy"), "--gt", str(tmp_path / "gt.npy")])
    out_f32 = capsys.readouterr().out.strip().split("\n")
    assert out_raw[-1].startswith("nrdm_small mean psnr is: ")
    assert out_raw[-1] == out_f32[-1] and out_raw[-2] == out_f32[-2]
    assert y_raw.cpu().numpy().tobytes() == y_f32.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_forward_raw_with_a_format_on_a_side_stream():
    import torch
    from sesrq import sensor as S
    e = _engine()
    fmt = S.Format(cfa="bggr", black=64, white=1023)
    dev = device()
    codes, _ = _route_frame(fmt, 1100, (1, 80, 960), 80)
    want, _ = e.forward_raw(_dev(codes), want_f=False, fmt=fmt)
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    side = torch.cuda.Stream(device=dev)
    src = torch.from_numpy(codes.astype(np.int32)).to(dev)
    for _ in range(3):
        x = (src * 1).to(torch.uint16)                 # produced on the current stream just before the call
        q, y = e.forward_raw(x, stream=side, fmt=fmt)
        side.synchronize()
        same("side stream q", q, want)
        del x


@pytest.mark.gpu
def test_forward_raw_refusals_with_a_format():
    import sesrq
    import torch
    from sesrq import sensor as S
    from sesrq.bundle import Bundle
    fmt = S.Format(cfa="bggr", black=64, white=1023)
    x = _dev(raw_frame("c")[0])[None]
    one = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "sesr_x4.crop.npz")), device())
    with pytest.raises(ValueError, match="3-channel"):
        one.forward_raw(x, fmt=fmt)
    nrdm = _bundle()
    chained = sesrq.Engine(nrdm, device(), upstream=nrdm)
    with pytest.raises(ValueError, match="upstream"):
        chained.forward_raw(x, fmt=fmt)
    anchored = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "sesr_x2_rand.crop.npz")), device(), anchor_add=True)
    with pytest.raises(ValueError, match="anchor_add"):
        anchored.forward_raw(x, fmt=fmt)
    e = _engine()
    with pytest.raises(ValueError, match="uint16"):
        e.forward_raw(x.to(dtype=torch.int32), fmt=fmt)
    with pytest.raises(ValueError, match="one channel"):
        e.forward_raw(x.unsqueeze(1).expand(1, 2, *x.shape[1:]).contiguous(), fmt=fmt)
    with pytest.raises(ValueError, match="uint8"):
        e.forward_raw(x, fmt=S.Format(packing="raw12"))
    with pytest.raises(ValueError, match="belong to a sensor format"):
        e.forward_raw(x, stride=2 * x.shape[2], width=x.shape[2])
    with pytest.raises(ValueError, match="sesrq.sensor.Format"):
        e.forward_raw(x, fmt="bggr")


@pytest.mark.gpu
def test_zz_every_sensor_instance_ran():
    """LAST in this file: every kernel instantiation libsesrq_sensor.so can launch was launched by a checked case above."""
    from sesrq import sensor as S
    k = S.instances()
    assert len(k) == 12, k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
