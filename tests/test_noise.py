"""GPU tests of libsesrq_noise.so (include/sesrq_noise.h) and of the `noise=` argument of the raw entry points.

The deviates are compared with the float64 oracle (tests/noise_oracle.py) at T_Z, the one tolerance here.  Everything else is exact: the
fused kernel's fp32 frame is noise_oracle.combine on the device's own deviates (sesrq_noise_deviates runs the device function the fused
kernel calls), bit for bit, and its q0 is the oracle's input quantiser of that frame, bit for bit.

T_Z.  The largest |z_dev - z_oracle| measured over the frames of SHAPES on an MI355X is 4.77e-07 (tools/noise_probe.py,
profiles/noise_probe.txt), against an estimate of 1.5e-6 from the 1 - 2 ulp of logf / sincospif at |z| = 5.8.  The test asserts four
times the measured value rounded up to a power of two, 2^-19 = 1.9e-6: the margin covers other seeds reaching other corners of the two
functions.  Those corners have since been looked at (tests/test_noise_limits.py, profiles/noise_limits.txt): over the 2.0e8 deviates
of 16 frames of 2048 x 2048, which hold every corner word of both functions, the largest error is 7.90e-07 (at |z| = 4.05), and
8.58e-07 (at |z| = 4.93) is the largest over the about 3.7e9 deviates that module compares; 4.77e-07 was the maximum of 1e4 samples, not of
the functions.  The bound stays 2^-19."""
import functools
import os

import numpy as np
import pytest

import noise_oracle as NO
import sensor_oracle as SO
from conftest import GOLDEN
from helpers import device, same

pytestmark = pytest.mark.gpu

F32 = np.float32
T_Z = 2.0 ** -19
SEED = 0x0123456789ABCDEF
DOMAINS = ((0.00392155787524055, -128), (0.003686274624630517, -136))
CFAS = ("rggb", "grbg", "gbrg", "bggr")
# (packing, (N, H, W), extra stride bytes): the smallest frames that reach every path
SHAPES = (("u16", (3, 5, 37), 0),          # per-pixel path, odd H, partial segment
          ("u16", (2, 4, 64), 0),          # wide path
          ("raw10", (3, 5, 40), 0),        # packed rows, a tail of half a segment
          ("raw10", (2, 3, 36), 7),        # padded rows
          ("raw12", (2, 7, 18), 0),        # packed rows
          ("raw12", (2, 4, 32), 0),        # packed rows, wide path
          ("raw10", (2, 2, 32), 0),        # packed rows, wide path
          ("u16", (1, 1, 70001), 0),       # counter word x above 2^16
          ("u16", (1, 70001, 2), 0))       # counter word y above 2^16
WHITE = {"u16": 4095, "raw10": 1023, "raw12": 4095}
FRAME_HI = 2 ** 32 - 1                     # a batch from here crosses into the high word of the frame number


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


def _fmt(cfa, packing, black=16):
    from sesrq import sensor as S
    return S.Format(cfa=cfa, black=black, white=WHITE[packing], packing=packing)


def _codes(packing, nhw, seed=0):
    top = {"u16": 65535, "raw10": 1023, "raw12": 4095}[packing]
    c = np.random.default_rng(seed + nhw[2]).integers(0, min(top, WHITE[packing] + 40) + 1, nhw).astype(np.uint16)
    c.flat[0], c.flat[-1] = WHITE[packing], 0
    return c


def _rows(codes, fmt, extra=0, pad=0xEE):
    from sesrq import sensor as S
    W = codes.shape[-1]
    return S.pack(codes, fmt, fmt.row_bytes(W) + extra, pad)


def _z_dev(nhw, seed, frame0):
    import torch
    from sesrq import noise
    z = noise.deviates(nhw, seed, frame0, device())
    torch.cuda.synchronize()
    return z.cpu().numpy()


def _unpack(fmt, s0, z0, ed, rows, W, levels, seed, frame0, want_q=True, want_sp=True, stream=None, q=None, sp=None):
    """One sesrq_noise_unpack of (N, H, stride) uint8 rows through the C ABI.  levels: (shot, read) or an (N, 2) array."""
    import torch
    from sesrq import noise
    N, H = rows.shape[:2]
    x = rows if hasattr(rows, "data_ptr") else _dev(rows)
    h = noise.context(device(), fmt, s0, z0, ed)
    if want_q and q is None:
        q = torch.full((N, 3, H, W), 99, dtype=torch.int8, device=device())
    if want_sp and sp is None:
        sp = torch.full((N, 3, H, W), float("nan"), dtype=torch.float32, device=device())
    lv = np.asarray(levels, F32)
    dlv = _dev(lv) if lv.ndim == 2 else None
    st = stream if stream is not None else torch.cuda.current_stream(device())
    rc = noise.lib().sesrq_noise_unpack(h, x.data_ptr(), x.shape[2], q.data_ptr() if want_q else None, sp.data_ptr() if want_sp else None,
                                        N, H, W, 0.0 if dlv is not None else float(lv[0]), 0.0 if dlv is not None else float(lv[1]),
                                        dlv.data_ptr() if dlv is not None else None, seed, frame0, st.cuda_stream)
    assert rc == 0, noise.last_error()
    st.synchronize()
    return (q if want_q else None), (sp if want_sp else None)


# ------------------------------------------------------------------------------------------------------------------- 6. deviates
@functools.lru_cache(maxsize=None)
def _z_oracle(nhw, seed, frame0):
    z = NO.deviates(seed, frame0, *nhw).astype(F32)
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("nhw,frame0", [(s[1], 3) for s in SHAPES] + [((3, 5, 37), FRAME_HI)])
def test_deviates_against_the_float64_oracle(nhw, frame0):
    z = _z_dev(nhw, SEED, frame0)
    want = _z_oracle(nhw, SEED, frame0)
    err = float(np.abs(z.astype(np.float64) - want).max())
    print(f"T_z {nhw} frame0 {frame0}: max |z_dev - z_oracle| = {err:.3e}, max |z| = {np.abs(z).max():.3f}")
    assert z.shape == (nhw[0], 3, nhw[1], nhw[2]) and np.abs(z).max() <= NO.Z_MAX
    assert err <= T_Z


def test_a_batch_of_deviates_is_its_frames():
    for frame0 in (0, FRAME_HI, 2 ** 64 - 2):
        z = _z_dev((3, 5, 37), SEED, frame0)
        for n in range(3):
            same(f"frame {frame0} + {n}", _z_dev((1, 5, 37), SEED, (frame0 + n) % 2 ** 64)[0], z[n])
    assert not np.array_equal(_z_dev((1, 5, 37), SEED, 0), _z_dev((1, 5, 37), SEED + 1, 0))
    assert not np.array_equal(_z_dev((1, 5, 37), SEED, 0), _z_dev((1, 5, 37), SEED + 2 ** 32, 0))      # the key's high word counts


# ------------------------------------------------------------------------------------------------------------------- 7. fused, exact
def _levels_cases(N):
    per_frame = np.array([[0.003 * (n + 1), 1e-5 * (n + 1)] for n in range(N)], F32)
    return ((0.01, 0.0005), (0.012, 0.0), (0.0, 1e-4), per_frame)


def _check(what, fmt, codes, rows, W, levels, s0, z0, ed, seed, frame0, outs=((True, True),)):
    z = _z_dev(codes.shape, seed, frame0)
    want_sp, _ = NO.frame(codes, fmt.cfa, fmt.black, fmt.white, levels, z, s0, z0, ed)
    x = _dev(rows)
    for wq, wsp in outs:
        q, sp = _unpack(fmt, s0, z0, ed, x, W, levels, seed, frame0, wq, wsp)
        if wsp:
            same(f"{what} spread (q0 {wq})", sp, want_sp)
        if wq:
            same(f"{what} q0 (spread {wsp})", q, NO.O.quantize_input(want_sp, s0, z0, reciprocal=ed == 2))
    return want_sp


@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("packing,nhw,extra", SHAPES, ids=[f"{s[0]}-{'x'.join(map(str, s[1]))}+{s[2]}" for s in SHAPES])
def test_fused_kernel_is_combine_on_the_device_deviates(cfa, packing, nhw, extra):
    fmt = _fmt(cfa, packing)
    codes = _codes(packing, nhw)
    rows = _rows(codes, fmt, extra)
    frame0 = FRAME_HI if nhw == (3, 5, 37) else 11
    k = 0
    for ed in (0, 2):
        for s0, z0 in DOMAINS:
            for lv in _levels_cases(nhw[0]):
                outs = ((True, True), (True, False), (False, True)) if k % 4 == 0 else ((True, True),)
                _check(f"{cfa} {packing} {nhw} ed {ed} z0 {z0} levels {np.asarray(lv).tolist()}", fmt, codes, rows, nhw[2], lv, s0, z0, ed,
                       SEED + k, frame0, outs)
                k += 1


@pytest.mark.parametrize("packing,nhw,extra", SHAPES[:7], ids=[f"{s[0]}-{'x'.join(map(str, s[1]))}+{s[2]}" for s in SHAPES[:7]])
def test_zero_levels_give_the_sensor_librarys_bytes(packing, nhw, extra):
    import torch
    from sesrq import sensor as S
    for cfa in CFAS:
        fmt = _fmt(cfa, packing)
        codes = _codes(packing, nhw, 5)
        x = _dev(_rows(codes, fmt, extra))
        for (s0, z0), ed in zip(DOMAINS, (0, 2)):
            q, sp = _unpack(fmt, s0, z0, ed, x, nhw[2], (0.0, 0.0), SEED, 1)
            q2 = torch.empty_like(q)
            sp2 = torch.empty_like(sp)
            S.launch(device(), fmt, s0, z0, ed, x, nhw[2], x.shape[2], q2, sp2, torch.cuda.current_stream(device()))
            torch.cuda.synchronize()
            same(f"{cfa} {packing} {nhw} q0", q, q2)
            same(f"{cfa} {packing} {nhw} spread", sp, sp2)
            t = SO.q_table(fmt.black, fmt.white, s0, z0, ed)
            same(f"{cfa} {packing} {nhw} q0 oracle", q, SO.spread(codes, t, t[0], cfa, fmt.black, fmt.white))
    # all-zero per-frame levels too
    q3, sp3 = _unpack(fmt, s0, z0, ed, x, nhw[2], np.zeros((nhw[0], 2), F32), SEED, 1)
    same("levels array of zeros q0", q3, q2)
    same("levels array of zeros spread", sp3, sp2)


def test_reference_format_context_is_rggb_4095():
    """fmt == NULL in the C ABI, fmt=None in Python: the reference's dataset format."""
    import ctypes as C
    from sesrq import noise, sensor as S
    codes = _codes("u16", (2, 4, 64), 9)
    h = C.c_void_p()
    assert noise.lib().sesrq_noise_create(None, 0.0039, -128, 0, C.byref(h)) == 0, noise.last_error()
    import torch
    x = _dev(codes)
    q = torch.empty((2, 3, 4, 64), dtype=torch.int8, device=device())
    assert noise.lib().sesrq_noise_unpack(h, x.data_ptr(), 128, q.data_ptr(), None, 2, 4, 64, 0.01, 1e-4, None, 3, 4,
                                          torch.cuda.current_stream(device()).cuda_stream) == 0, noise.last_error()
    torch.cuda.synchronize()
    noise.lib().sesrq_noise_destroy(h)
    q2, _ = _unpack(S.Format(), 0.0039, -128, 0, _rows(codes, S.Format()), 64, (0.01, 1e-4), 3, 4, True, False)
    same("fmt NULL", q, q2)


# ------------------------------------------------------------------------------------------------------------------- 8. invariance
def test_same_bytes_whatever_the_packing_padding_batch_alignment_and_stream():
    import torch
    from sesrq import sensor as S
    N, H, W = 3, 6, 64
    s0, z0 = DOMAINS[1]
    codes = np.random.default_rng(8).integers(0, 1024, (N, H, W)).astype(np.uint16)
    lv, seed, f0 = (0.006, 2e-4), 77, FRAME_HI - 1
    ref = None
    for packing in ("u16", "raw10", "raw12"):
        fmt = S.Format(cfa="gbrg", black=16, white=1023, packing=packing)
        for extra in (0, 16, 5):
            q, sp = _unpack(fmt, s0, z0, 0, _rows(codes, fmt, extra), W, lv, seed, f0)
            if ref is None:
                ref = (q.cpu().numpy(), sp.cpu().numpy())
                assert len(np.unique(ref[0])) > 50
            same(f"{packing} +{extra} q0", q, ref[0])
            same(f"{packing} +{extra} spread", sp, ref[1])
    fmt = S.Format(cfa="gbrg", black=16, white=1023)
    rows = _rows(codes, fmt)
    # one batch of 3 == three calls with frame0 + n (crossing 2^32); per-frame levels follow the frame
    plv = np.array([[0.001, 1e-5], [0.004, 1e-4], [0.012, 1e-3]], F32)
    qb, spb = _unpack(fmt, s0, z0, 0, rows, W, plv, seed, f0)
    for n in range(3):
        q1, sp1 = _unpack(fmt, s0, z0, 0, rows[n:n + 1], W, tuple(plv[n]), seed, f0 + n)
        same(f"frame {n} alone q0", q1[0], qb[n])
        same(f"frame {n} alone spread", sp1[0], spb[n])
    # outputs at addresses that force the per-pixel stores
    flat_q = torch.zeros(3 * N * H * W + 16, dtype=torch.int8, device=device())
    flat_sp = torch.zeros(3 * N * H * W + 4, dtype=torch.float32, device=device())
    for qo, so in ((1, 1), (3, 0), (0, 3), (8, 0)):
        q = flat_q[qo:qo + 3 * N * H * W].view(N, 3, H, W)
        sp = flat_sp[so:so + 3 * N * H * W].view(N, 3, H, W)
        _unpack(fmt, s0, z0, 0, rows, W, lv, seed, f0, q=q, sp=sp)
        same(f"q0 at +{qo}", q, ref[0])
        same(f"spread at +{so} floats", sp, ref[1])
    # raw at an address that forces the byte loads
    flat = torch.zeros(rows.size + 16, dtype=torch.uint8, device=device())
    for ro in (1, 2, 6):
        flat[ro:ro + rows.size] = _dev(rows).flatten()
        q, sp = _unpack(fmt, s0, z0, 0, flat[ro:ro + rows.size].view(rows.shape), W, lv, seed, f0)
        same(f"raw at +{ro} q0", q, ref[0])
        same(f"raw at +{ro} spread", sp, ref[1])
    # a non-default stream
    side = torch.cuda.Stream(device=device())
    torch.cuda.synchronize()
    q, sp = _unpack(fmt, s0, z0, 0, rows, W, lv, seed, f0, stream=side)
    same("side stream q0", q, ref[0])
    same("side stream spread", sp, ref[1])


# ------------------------------------------------------------------------------------------------------------------- 9. end to end
def _bundle():
    """The nrdm_3 net of tests/golden/nrdm_3.params.npz with the domains the reference calibrated on its raw frames."""
    from sesrq.bundle import Bundle
    return Bundle.load(os.path.join(GOLDEN, "raw", "nrdm_3.npz"))


PLANS = (("default", dict()), ("per-layer", dict(fuse_hidden=0)), ("dot4", dict(engine=1)))


@functools.lru_cache(maxsize=None)
def _engine(plan="default"):
    import sesrq
    return sesrq.Engine(_bundle(), device(), **dict(PLANS)[plan])


@pytest.mark.parametrize("plan", [p[0] for p in PLANS])
def test_forward_raw_with_noise_is_forward_on_the_noisy_frame(plan):
    import torch
    from sesrq import noise, sensor as S
    e = _engine(plan)
    codes = np.random.default_rng(21).integers(0, 4096, (2, 36, 80)).astype(np.uint16)
    for fmt, rows in ((None, codes), (S.Format(cfa="bggr", black=64, white=4095, packing="raw12"), None)):
        x = _dev(rows if rows is not None else S.pack(codes, fmt))
        for m in (noise.NoiseModel(0.003, 1e-5, seed=3, frame0=5), noise.NoiseModel(seed=4, frame0=FRAME_HI)):
            q, y = e.forward_raw(x, fmt=fmt, noise=m)
            _, sp = noise.apply(e, x, fmt, m, want_q=False, want_spread=True)
            q2, y2 = e.forward(sp)
            torch.cuda.synchronize()
            same(f"{plan} {fmt} {m} q", q, q2)
            same(f"{plan} {fmt} {m} y", y, y2)
            q0, _ = noise.apply(e, x, fmt, m)
            same(f"{plan} {fmt} {m} q0", q0, NO.O.quantize_input(sp.cpu().numpy(), e.bundle.scale[0], e.bundle.zero[0],
                                                                  reciprocal=e.exact_div == 2))
        # the clean frame differs, and a call without `noise` is what it was: sensor.unpack + forward
        qc, yc = e.forward_raw(x, fmt=fmt)
        _, spc = S.unpack(e, x, fmt, want_q=False, want_spread=True)
        q3, y3 = e.forward(spc)
        torch.cuda.synchronize()
        same(f"{plan} {fmt} clean q", qc, q3)
        same(f"{plan} {fmt} clean y", yc, y3)
        assert not np.array_equal(qc.cpu().numpy(), q.cpu().numpy())


def test_apply_python_levels_match_the_oracle():
    """noise.apply through the model: fixed levels and per-frame drawn levels (NoiseModel.levels) land in the kernel as the oracle
    takes them."""
    import torch
    from sesrq import noise, sensor as S
    e = _engine()
    fmt = S.Format(cfa="grbg", black=16, white=1023, packing="raw10")
    codes = _codes("raw10", (3, 5, 40), 2)
    x = _dev(S.pack(codes, fmt))
    for m in (noise.NoiseModel(0.01, 5e-4, seed=9, frame0=2), noise.NoiseModel(seed=9, frame0=2)):
        q, sp = noise.apply(e, x, fmt, m, want_spread=True)
        torch.cuda.synchronize()
        z = _z_dev(codes.shape, 9, 2)
        want_sp, want_q = NO.frame(codes, fmt.cfa, fmt.black, fmt.white, m.levels(3), z, e.bundle.scale[0], e.bundle.zero[0], e.exact_div)
        same(f"{m} spread", sp, want_sp)
        same(f"{m} q0", q, want_q)


def test_narrow_engine_takes_the_noisy_fp32_frame():
    import sesrq
    import torch
    from sesrq import noise
    from sesrq.bundle import Bundle
    e = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "quan_bits", "nrdm_3.q4.crop.npz")), device())
    assert e.quan_bits == 4
    x = _dev(np.random.default_rng(1).integers(0, 4096, (2, 18, 32)).astype(np.uint16))
    m = noise.NoiseModel(0.004, 1e-4, seed=1)
    before = noise.instances()
    q, y = e.forward_raw(x, noise=m)
    ran = [n for n, c in noise.instances().items() if c != before[n]]
    assert ran == ["noise_unpack<u16,spread>"], ran
    _, sp = noise.apply(None, x, None, m, want_q=False, want_spread=True)
    q2, y2 = e(sp)
    torch.cuda.synchronize()
    same("narrow q", q, q2)
    same("narrow y", y, y2)


def test_evaluate_raw_with_noise_does_not_depend_on_the_batch_split():
    from sesrq import noise, quality
    e = _engine()
    rng = np.random.default_rng(31)
    raws = rng.integers(0, 4096, (5, 1, 64, 96)).astype(np.uint16)
    gts = rng.integers(0, 4096, (5, 3, 64, 96)).astype(np.uint16)
    for m in (noise.NoiseModel(0.003, 1e-5, seed=3, frame0=FRAME_HI - 2), noise.NoiseModel(seed=8)):
        one = quality.evaluate_raw(e, [r for r in raws], [g for g in gts], 3, noise=m)
        five = quality.evaluate_raw(e, [raws], [gts], 3, noise=m)
        assert one.shape == (5, 3) and one.tobytes() == five.tobytes(), (one, five)
        again = quality.evaluate_raw(e, [raws[:2], raws[2:]], [gts[:2], gts[2:]], 3, noise=m)
        assert again.tobytes() == one.tobytes()
        clean = quality.evaluate_raw(e, [raws], [gts], 3)
        assert clean.tobytes() != one.tobytes()
        other = quality.evaluate_raw(e, [raws], [gts], 3, noise=m.advance(1))
        assert other.tobytes() != one.tobytes()          # other frame numbers, other noise
    with pytest.raises(ValueError, match="NoiseModel"):
        quality.evaluate_raw(e, [raws], [gts], 3, noise=0.003)


def test_enqueue_raw_with_noise_equals_enqueue_on_the_noisy_frame():
    import torch
    from calib_cases import calibrators
    from sesrq import noise
    a, b, _ = calibrators("nrdm_3")
    m = noise.NoiseModel(seed=12, frame0=40)
    for k in range(2):
        x = _dev(np.random.default_rng(k).integers(0, 4096, (1, 20, 48)).astype(np.uint16))
        ya = a.enqueue_raw(x, noise=m.advance(k))
        _, sp = noise.apply(None, x, None, m.advance(k), want_q=False, want_spread=True)
        same("last_input", a.last_input, sp)
        yb = b.enqueue(sp)
        torch.cuda.synchronize()
        same("output", ya, yb)
    a.sync(), b.sync()
    assert a._slots.cpu().numpy().tobytes() == b._slots.cpu().numpy().tobytes()
    assert a.run_min == b.run_min and a.run_max == b.run_max and a.finalize() == b.finalize()


def test_refusals_carry_over():
    import sesrq
    from sesrq import noise
    from sesrq.bundle import Bundle
    m = noise.NoiseModel(0.003, 1e-5)
    x = _dev(np.zeros((1, 8, 16), np.uint16))
    one = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "sesr_x4.crop.npz")), device())
    with pytest.raises(ValueError, match="3-channel"):
        one.forward_raw(x, noise=m)
    anchored = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "sesr_x2_rand.crop.npz")), device(), anchor_add=True)
    with pytest.raises(ValueError, match="anchor_add"):
        anchored.forward_raw(x, noise=m)
    e = _engine()
    with pytest.raises(ValueError, match="NoiseModel"):
        e.forward_raw(x, noise=(0.003, 1e-5))
    with pytest.raises(ValueError, match="belong to a sensor format"):
        e.forward_raw(x, stride=32, width=16, noise=m)
    with pytest.raises(ValueError, match="q0 needs"):
        noise.apply(None, x, None, m)
    with pytest.raises(ValueError, match="ask for"):
        noise.apply(e, x, None, m, want_q=False)


# ------------------------------------------------------------------------------------------------------------------- 11. CLI
def test_sim_and_test_py_add_noise(capsys, tmp_path, monkeypatch):
    """sim.py --add-noise runs, is reproducible between two invocations, differs from the run without it and from another seed, and
    define.TEST_RAW_ADD_NOISE = True does what the flag does; test.py --add-noise calibrates (other ranges than the clean pass)."""
    import define
    import sim
    from calib_cases import load_test_py
    test_py = load_test_py()
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "nrdm_3_nat.params.npz")
    rng = np.random.default_rng(96)
    codes = rng.integers(0, 4096, (80, 96)).astype(np.uint16)
    rawp = str(tmp_path / "frame_80_96.raw")
    codes.astype("<u2").tofile(rawp)
    np.save(str(tmp_path / "gt16.npy"), rng.integers(0, 4096, (1, 3, 80, 96)).astype(np.uint16))
    base = ["--mflag", "3", "--params", params, "--input", rawp, "--gt", str(tmp_path / "gt16.npy")]
    flags = ["--add-noise", "--shot", "0.003", "--read", "1e-5", "--noise-seed", "3"]

    def run(extra):
        STORE.clear()
        y = sim.main(base + extra).cpu().numpy()
        return y, capsys.readouterr().out.strip().split("\n")[-1]
    y1, l1 = run(flags)
    y2, l2 = run(flags)
    y0, l0 = run([])
    y3, l3 = run(flags[:-1] + ["4"])
    y4, _ = run(["--add-noise"])                    # levels drawn per frame
    assert l1.startswith("nrdm_small mean psnr is: ") and l1 == l2 and y1.tobytes() == y2.tobytes()
    assert y0.tobytes() != y1.tobytes() and l0 != l1 and y3.tobytes() != y1.tobytes() and y4.tobytes() != y0.tobytes()
    monkeypatch.setattr(define, "TEST_RAW_ADD_NOISE", True)
    y5, _ = run(flags[1:])
    y6, _ = run(["--no-add-noise"])
    assert y5.tobytes() == y1.tobytes() and y6.tobytes() == y0.tobytes()
    monkeypatch.setattr(define, "TEST_RAW_ADD_NOISE", False)
    with pytest.raises(SystemExit, match="belong to --add-noise"):
        sim.main(base + ["--shot", "0.003", "--read", "1e-5"])
    with pytest.raises(SystemExit, match="both shot and read"):
        sim.main(base + ["--add-noise", "--shot", "0.003"])
    # test.py: the calibration pass on the noisy frames
    cal = ["--mflag", "3", "--params", params, "--input", rawp, rawp]
    clean = test_py.main(cal)
    noisy = test_py.main(cal + ["--add-noise", "--shot", "0.012", "--read", "1e-3", "--noise-seed", "3"])
    again = test_py.main(cal + ["--add-noise", "--shot", "0.012", "--read", "1e-3", "--noise-seed", "3"])
    scored = test_py.main(cal + ["--gt", str(tmp_path / "gt16.npy"), str(tmp_path / "gt16.npy"), "--add-noise", "--shot", "0.012", "--read",
                                 "1e-3", "--noise-seed", "3"])
    capsys.readouterr()
    assert noisy == again and noisy != clean and scored == noisy


def test_zz_every_noise_instance_ran():
    """LAST in this file: every kernel instantiation libsesrq_noise.so can launch was launched by a checked case above."""
    from sesrq import noise
    k = noise.instances()
    assert sorted(k) == sorted([f"noise_unpack<{p},{o}>" for p in ("u16", "raw10", "raw12") for o in ("q0", "spread", "q0+spread")]
                               + ["noise_deviates"]), k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
