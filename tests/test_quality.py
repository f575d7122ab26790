"""PSNR / SSIM on the device (sesrq.quality, libsesrq_eval.so, sim.py --gt) against the reference's evaluation loop.

CPU: the float64 oracle (tests/quality_oracle.py) against the reference-run PSNR values of tests/golden/quality/quality.npz and an independent
SSIM built on scipy; the C ABI (symbols, argument checks without a device); the ISA hazard scan.  GPU: every form x pred dtype against
the fixture, int8 <-> fp32 identity on reference-made frames, bitwise reproducibility, 4K frames, evaluate(), sim.py --gt, and that
every kernel instantiation of the library ran."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_fixture, fixture_input
from helpers import device, score as _score
import quality_oracle as Q

CSRC = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "sesrq_eval.h")
HIPCC = "/opt/rocm/bin/hipcc"
EPS_PSNR_SAME = 10.0 * np.log10(255.0 ** 2 / 1e-8)


def quality_fixture():
    z = np.load(os.path.join(GOLDEN, "quality", "quality.npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_oracle_reproduces_reference_run_psnr():
    z, meta = quality_fixture()
    n = 0
    for name, c in meta["cases"].items():
        got = Q.metrics(z[name + ".pred"], z[name + ".gt"], c["mflag"])
        ref = z[name + ".psnr_ref"]
        if c["mflag"] in (5, 6):
            np.testing.assert_allclose(got[:, 1], ref, rtol=0, atol=1e-9, err_msg=name)
            n += len(ref)
        else:
            assert np.isnan(ref).all()
        np.testing.assert_array_equal(got[:, 1], z[name + ".psnr_restated"])
        np.testing.assert_array_equal(got[:, 2], z[name + ".ssim_restated"])
    assert n >= 10


def _ssim_scipy(x, y):
    """skimage's structural_similarity restated on scipy.ndimage.uniform_filter, the way skimage itself forms it."""
    from scipy.ndimage import uniform_filter
    x, y = x.astype(np.float64), y.astype(np.float64)
    f = lambda a: uniform_filter(a, size=7)
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    cn = 49.0 / 48.0
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return S[3:-3, 3:-3].mean(dtype=np.float64)


def test_oracle_ssim_matches_scipy_uniform_filter():
    pytest.importorskip("scipy")
    z, meta = quality_fixture()
    for name in meta["cases"]:
        p, g = np.clip(z[name + ".pred"].astype(np.float64), 0, 1), z[name + ".gt"]
        for n in range(p.shape[0]):
            want = np.mean([_ssim_scipy(g[n, c], p[n, c]) for c in range(p.shape[1])])
            got = np.mean([Q.ssim_channel(g[n, c], p[n, c]) for c in range(p.shape[1])])
            assert abs(got - want) <= 1e-9, (name, n, got, want)


def test_eval_library_exports_every_declared_symbol():
    from sesrq import quality
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_eval[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 6, names
    assert sorted(quality.SYMBOLS) == names, "python binding and header disagree"
    lib = quality.lib()
    for n in names:
        assert getattr(lib, n) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", quality.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sesrq_\w+)", nm))
    assert set(names) <= exported
    assert not any(e.startswith("sesrq_") and not e.startswith("sesrq_eval") for e in exported), "libsesrq_eval.so exports libsesrq symbols"


def test_eval_argument_checks_without_a_device():
    import ctypes as C
    from sesrq import quality
    lib = quality.lib()
    fake = C.c_void_p(4096)                       # never dereferenced: every check runs before any HIP call
    ws = lib.sesrq_eval_workspace_bytes(2, 3, 67, 101)
    assert ws > 0 and lib.sesrq_eval_workspace_bytes(2, 3, 6, 101) == 0 and lib.sesrq_eval_workspace_bytes(0, 3, 67, 101) == 0
    # the geometry depends on (C, H, W) only: one slab per frame
    assert lib.sesrq_eval_workspace_bytes(1, 3, 67, 101) * 2 == ws == 3 * lib.sesrq_eval_workspace_bytes(2, 1, 67, 101)

    def call(form=0, dtype=0, scale=0.5, zero=0, N=2, Ch=3, H=67, W=101, pred=fake, gt=fake, out=fake, work=fake, nbytes=ws, desc=True):
        d = quality.EvalDesc(form=form, pred_dtype=dtype, pred_scale=scale, pred_zero=zero)
        rc = lib.sesrq_eval(C.byref(d) if desc else None, pred, gt, N, Ch, H, W, out, work, nbytes, None)
        return rc, quality.last_error()

    cases = {
        "form / C": dict(form=quality.FORM_Y255, Ch=3),
        "form / C (x2)": dict(form=quality.FORM_X2, Ch=1),
        "H < 7": dict(H=6),
        "W < 7": dict(W=6),
        "N < 1": dict(N=0),
        "workspace too small": dict(nbytes=ws - 1),
        "NULL pred": dict(pred=None),
        "NULL gt": dict(gt=None),
        "NULL out": dict(out=None),
        "NULL workspace": dict(work=None),
        "NULL desc": dict(desc=False),
        "int8 x2": dict(form=quality.FORM_X2, dtype=quality.PRED_I8),
        "unknown form": dict(form=7),
        "unknown dtype": dict(dtype=5),
        "int8 scale": dict(dtype=quality.PRED_I8, scale=0.0),
    }
    for what, kw in cases.items():
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("sesrq_eval"), (what, rc, msg)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_eval_isa_clears_the_hazard_scan(tmp_path):
    asm = str(tmp_path / "sesrq_eval.s")
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-cxxflags"], check=True, capture_output=True, text=True).stdout.split()
    assert "-ffp-contract=off" in flags
    flags += ["-I" + CSRC, "--cuda-device-only", "-S"]
    subprocess.run([HIPCC] + flags + [os.path.join(CSRC, "sesrq_eval.hip"), "-o", asm], check=True, capture_output=True)
    text = open(asm).read()
    assert text.count(".amdhsa_kernel ") == 6
    assert "global_atomic" not in text and "scratch_" not in text       # fixed-order slab, no float atomics; no spills
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "store_hazard_scan.py"), asm], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_score_refuses_bad_arguments_on_the_host():
    torch = pytest.importorskip("torch")
    from sesrq import quality
    a = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError):
        quality.score(a, a, 2)                                      # no integer path
    with pytest.raises(ValueError):
        quality.score(a, torch.zeros(1, 1, 8, 9), 5)                # shape
    with pytest.raises(ValueError):
        quality.score(a, a, 3)                                      # channels
    with pytest.raises(ValueError):
        quality.score(torch.zeros(1, 1, 6, 8), torch.zeros(1, 1, 6, 8), 5)
    with pytest.raises(ValueError):
        quality.score(a, a, 5)                                      # not on a device


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _check(got, want_psnr, want_ssim, what):
    for n in range(len(want_psnr)):
        if np.isinf(want_psnr[n]):
            assert np.isinf(got[n, 1]) and got[n, 1] > 0, (what, n, got[n])
        else:
            assert abs(got[n, 1] - want_psnr[n]) <= 1e-5, (what, n, got[n, 1], want_psnr[n])
        assert abs(got[n, 2] - want_ssim[n]) <= 1e-6, (what, n, got[n, 2], want_ssim[n])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "i8"])
def test_every_form_against_the_fixture(dtype):
    z, meta = quality_fixture()
    ran = 0
    for name, c in meta["cases"].items():
        if dtype == "i8" and not c["int8"]:
            continue
        mflag = c["mflag"]
        pred = z[name + ".q"] if dtype == "i8" else z[name + ".pred"]
        kw = dict(scale=meta["scale"], zero=meta["zero"]) if dtype == "i8" else {}
        got = _score(pred, z[name + ".gt"], mflag, **kw)
        want_psnr = z[name + ".psnr_ref"] if mflag in (5, 6) else z[name + ".psnr_restated"]
        _check(got, want_psnr, z[name + ".ssim_restated"], name)
        if c["identical"]:
            assert (got[:, 2] == 1.0).all(), (name, got)
            assert (got[:, 0] == 0.0).all()
            if mflag in (3, 4):
                assert np.isinf(got[:, 1]).all()
            else:
                assert np.allclose(got[:, 1], EPS_PSNR_SAME, rtol=0, atol=1e-9), got
        ran += 1
    assert ran == (9 if dtype == "f32" else 6)


@pytest.mark.gpu
def test_int8_prediction_scores_as_its_float_output():
    """An Engine forward on reference-made frames writes out_q and out_f; scoring out_q in the net's output domain gives the bits of
    scoring out_f: the in-kernel dequantisation is the forward's own."""
    import torch
    import sesrq
    from sesrq import quality
    from sesrq.bundle import Bundle
    for case, mflag in (("sesr_x4_nat.crop", 5), ("nrdm_3_nat.crop", 3)):
        path = os.path.join(GOLDEN, case + ".npz")
        fx, meta = load_fixture(path)
        b = Bundle.load(path)
        e = sesrq.Engine(b, device())
        x = torch.from_numpy(fixture_input(fx, meta)).to(device())
        q, y = e.forward(x)
        np.testing.assert_array_equal(y.cpu().numpy(), fx["out"])          # the reference's output, for the record
        rng = np.random.default_rng(7)
        gt = torch.from_numpy((fx["out"] + rng.normal(0, 0.03, fx["out"].shape)).astype(np.float32)).to(device())
        L = b.L
        sq = quality.score(q, gt, mflag, scale=b.scale[L], zero=b.zero[L])
        sf = quality.score(y, gt, mflag)
        torch.cuda.synchronize()
        assert torch.equal(sq, sf), (case, sq, sf)
        want = Q.metrics(y.cpu().numpy(), gt.cpu().numpy(), mflag)
        _check(sf.cpu().numpy(), want[:, 1], want[:, 2], case)


@pytest.mark.gpu
def test_bitwise_reproducible():
    import torch
    from sesrq import quality
    z, _ = quality_fixture()
    for name, mflag in (("x2_67x101", 6), ("y255_67x101", 5), ("rgb_7x7", 3)):
        p3 = torch.from_numpy(np.concatenate([z[name + ".pred"]] * 2)[:3]).to(device())
        g3 = torch.from_numpy(np.concatenate([z[name + ".gt"]] * 2)[:3]).to(device())
        runs = [quality.score(p3, g3, mflag) for _ in range(3)]
        side = torch.cuda.Stream()
        runs.append(quality.score(p3, g3, mflag, stream=side))
        torch.cuda.synchronize()
        for r in runs[1:]:
            assert torch.equal(r, runs[0]), name
        for k in range(3):
            alone = quality.score(p3[k:k + 1], g3[k:k + 1], mflag)
            torch.cuda.synchronize()
            assert torch.equal(alone[0], runs[0][k]), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("mflag,C", [(6, 3), (5, 1)])
def test_4k_frames_against_the_oracle(mflag, C):
    sys.path.insert(0, GOLDEN)
    from natural import natural_frame
    gt = natural_frame(C, 2160, 3840, 11)
    rng = np.random.default_rng(3)
    pred = (gt + rng.normal(0, 0.02, gt.shape)).astype(np.float32)
    pred[0, :, :50, :50] = 1.2                                      # clipped
    got = _score(pred, gt, mflag)
    want = Q.metrics(pred, gt, mflag)
    _check(got, want[:, 1], want[:, 2], f"4K mflag {mflag}")


def _engine(case, **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(os.path.join(GOLDEN, case + ".npz")), device(), **kw)


@pytest.mark.gpu
def test_evaluate_matches_score_of_a_separate_forward():
    import torch
    from sesrq import quality
    rng = np.random.default_rng(5)
    # MFLAG 5: int8 output scored in the output domain
    e = _engine("sesr_x4_nat.crop")
    xs = [torch.from_numpy(rng.uniform(0, 1, (1, 1, 24, 40)).astype(np.float32)) for _ in range(3)]
    gts = [torch.from_numpy(rng.uniform(0, 1, (1, 1, 96, 160)).astype(np.float32)) for _ in range(3)]
    got = quality.evaluate(e, xs, gts, 5)
    for k in range(3):
        _, y = e.forward(xs[k].to(device()), want_q=False)
        want = quality.score(y, gts[k].to(device()), 5)
        torch.cuda.synchronize()
        assert np.array_equal(got[k], want[0].cpu().numpy()), k
    # MFLAG 6: the anchored float output, and only on an anchored engine
    ea = _engine("sesr_x2_rand.crop", anchor_add=True)
    xs = [torch.from_numpy(rng.uniform(0, 1, (1, 3, 24, 40)).astype(np.float32)) for _ in range(2)]
    gts = [torch.from_numpy(rng.uniform(0, 1, (1, 3, 48, 80)).astype(np.float32)) for _ in range(2)]
    got = quality.evaluate(ea, xs, gts, 6)
    plain = _engine("sesr_x2_rand.crop")
    for k in range(2):
        x = xs[k].to(device())
        _, y = plain.forward(x, want_q=False)
        y = y + x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)         # reference test.py:149-155
        want = quality.score(y, gts[k].to(device()), 6)
        torch.cuda.synchronize()
        assert np.array_equal(got[k], want[0].cpu().numpy()), k
    with pytest.raises(ValueError, match="anchor"):
        quality.evaluate(plain, xs, gts, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("mflag,params,inp", [(5, "sesr_x4", "rand_SR_Input_80x960.npy"), (6, "sesr_x2_rand", "rand_DM_Input_80x960.npy")])
def test_sim_gt_prints_the_reference_lines(mflag, params, inp, capsys, tmp_path):
    import sim
    from sesrq.store import STORE
    STORE.clear()
    x = np.load(os.path.join(GOLDEN, inp))
    r = 4 if mflag == 5 else 2
    rng = np.random.default_rng(9)
    gt = rng.uniform(0, 1, (x.shape[0], 1 if mflag == 5 else 3, x.shape[2] * r, x.shape[3] * r)).astype(np.float32)
    gpath = str(tmp_path / "gt.npy")
    np.save(gpath, gt)
    y = sim.main(["--mflag", str(mflag), "--params", os.path.join(GOLDEN, params + ".params.npz"),
                  "--input", os.path.join(GOLDEN, inp), "--gt", gpath])
    out = capsys.readouterr().out.strip().split("\n")
    pred = y.cpu().numpy()
    if mflag == 6:
        pred = pred + np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)
    want = Q.metrics(pred, gt, mflag)
    task = "srx4" if mflag == 5 else "srx2"
    m = re.fullmatch(task + r" mean psnr is:  (\S+)  ssim is:  (\S+)", out[-1])
    assert m, out[-3:]
    per_frame = [float(v) for v in out[-1 - len(want):-1]]
    assert len(per_frame) == len(want)
    assert np.allclose(per_frame, want[:, 1], rtol=0, atol=1e-5), (per_frame, want[:, 1])
    assert abs(float(m.group(1)) - want[:, 1].mean()) <= 1e-5 and abs(float(m.group(2)) - want[:, 2].mean()) <= 1e-6
    # without --gt nothing is scored
    STORE.clear()
    sim.main(["--mflag", str(mflag), "--params", os.path.join(GOLDEN, params + ".params.npz"), "--input", os.path.join(GOLDEN, inp)])
    assert "mean psnr" not in capsys.readouterr().out


@pytest.mark.gpu
def test_zz_every_eval_kernel_ran():
    """LAST in this file: every kernel instantiation libsesrq_eval.so can launch was launched by a checked case above."""
    from sesrq import quality
    k = quality.kernels()
    assert len(k) == 6, k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
