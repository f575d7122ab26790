"""The reference's nr (MFLAG 1, denoise) and dm (MFLAG 2, demosaic) tasks end to end: model mirrors, sim.py / test.py --mflag 1|2,
raw-frame evaluation, and the fixtures the reference made from its own nr_* / dm_* checkpoints (tests/golden/nr_dm/, made by
tests/golden/make_nr_dm_golden.py, whose docstring says what the integer path of these tasks is: the nrdm_3_sim graph with the task's
weights and calibrated domains).

Tolerances of the calibration pass are those of tests/test_calib_reference.py (the reference sums in fp32 in oneDNN's order, the device
pass exactly in integers): running ranges within 1e-4 of their span, zero points equal, scales within rtol 2e-4, mode-0 outputs within
4 steps of the output domain on the synthetic frame (a), 0.5 step on the natural frames (b), (c), 0.05 step in the mean."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_fixture
from helpers import device, raw_frame, ref_gt, ref_inp, same, sha256, to_device
from oracle import sesrq_oracle as O
import mosaic_oracle as M
import qat_calib_oracle as QO
import quality_oracle as Q
from test_calib_reference import OUT_MAX_STEPS, OUT_MAX_STEPS_NATURAL, OUT_MEAN_STEPS, PSNR_ATOL, SSIM_ATOL, _ranges_and_domains
from test_quality import _check

ND = os.path.join(GOLDEN, "nr_dm")
CASES = ["nr", "dm", "nr_qat", "dm_qat"]
MFLAG = {"nr": 1, "dm": 2, "nr_qat": 1, "dm_qat": 2}
FRAMES = ("a", "b", "c")
PLANS = {"default": dict(), "per-layer": dict(fuse_hidden=0), "dot4": dict(engine=1)}        # engine 1: sesrq._lib.ENGINE_DOT4


def crop(case):
    return load_fixture(os.path.join(ND, case + ".crop.npz"))


def record(case):
    return load_fixture(os.path.join(ND, case + ".calib.npz"))


def params(case):
    p, pm = load_fixture(os.path.join(ND, case + ".params.npz"))
    return [p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], pm


def skip_scale(case):
    add = record(case)[1]["qat_add"]
    return None if add is None else float(QO.skip_scale(*[add[k] for k in QO.OBSERVERS]))


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_fixtures_are_the_four_tasks():
    ref = load_fixture(os.path.join(GOLDEN, "nrdm_3.crop.npz"))[0]
    for case in CASES:
        fx, meta = crop(case)
        assert meta["task_mflag"] == MFLAG[case] and meta["mflag"] == 3 and meta["graph"] == "nrdm_3_sim"
        assert fx["x"].shape == ref["x"].shape == (1, 3, 24, 40) and fx["out"].shape == ref["out"].shape      # the crop size of nrdm_3.crop.npz
        assert [fx[f"Wq{k}"].shape for k in range(5)] == [ref[f"Wq{k}"].shape for k in range(5)]              # 3 -> 16 -> 16 -> 16 -> 16 -> 3
        x_b = ref_inp("b")
        r0, c0 = meta["crop_at"]
        assert r0 % 2 == 0 and c0 % 2 == 0 and np.array_equal(fx["x"], x_b[:, :, r0:r0 + 24, c0:c0 + 40])
        _, _, pm = params(case)
        _, rec = record(case)
        assert pm["scale"] == meta["scale"] == rec["scale"] and pm["zero"] == meta["zero"] == rec["zero"]
        assert rec["frames"] == list(FRAMES) and (rec["qat_add"] is not None) == case.endswith("_qat")
        assert ("mosaic_oracle" in rec["metrics"]) == (MFLAG[case] == 1)
        if rec["qat_add"] is not None:       # the scale the traced QuantAdd held is the one its observers give
            assert np.float32(rec["qat_add"]["traced_scale"]) == np.float32(skip_scale(case))
    assert len({sha256(crop(c)[0]["Wq0"]) for c in CASES}) == 4


@pytest.mark.parametrize("case", CASES)
def test_both_oracles_reproduce_the_reference_stage_by_stage(case):
    """The numpy oracle gives every tensor the reference dumped on the crop, bit for bit; the C oracle its int8 and fp32 outputs."""
    from oracle import c_oracle as CO
    fx, meta = crop(case)
    net = O.net_from_fixture(fx)
    st = O.forward(net, fx["x"], keep=True)
    for name, want_sha in meta["sha"].items():
        got = np.asarray(st["y" if name == "out" else name]).astype(fx[name].dtype)
        assert sha256(got) == want_sha, f"{case}: {name} differs from the reference"
        np.testing.assert_array_equal(got, fx[name], err_msg=name)
    r = CO.forward(net, fx["x"], threads=2, want_f=True)
    same(case + " C oracle q_out", r["q_out"], fx["input5"])
    same(case + " C oracle y", r["y"], fx["out"])


@pytest.mark.parametrize("case", CASES)
def test_calibration_oracle_reproduces_the_records(case):
    """oracle.calib_oracle (a QAT record: tests/qat_calib_oracle.py at the checkpoint's QuantAdd scale) over frames a, b, c gives the
    reference's running ranges, zero points and scales."""
    from oracle import calib_oracle as CO
    Wf, bf, _ = params(case)
    _, rec = record(case)
    frames = [ref_inp(f) for f in FRAMES]
    s = skip_scale(case)
    r = CO.forward(Wf, bf, 1, frames, 8) if s is None else QO.forward(Wf, bf, 1, frames, 8, s)
    for k in range(6):
        span = rec["max"][k] - rec["min"][k]
        assert abs(r.run_min[k] - rec["min"][k]) <= 1e-4 * span and abs(r.run_max[k] - rec["max"][k]) <= 1e-4 * span, (case, k)
    sz = [O.calib_scale_zero(0.0 if k == 5 else r.run_min[k], r.run_max[k], 8) for k in range(6)]
    assert [z for _, z in sz] == rec["zero"]
    np.testing.assert_allclose([s_ for s_, _ in sz], rec["scale"], rtol=2e-4)


def test_float_model_loads_nr_and_dm_checkpoints(tmp_path):
    """sim.float_model(1 | 2, ckpt=...) loads a checkpoint with the keys of nr_G.pth / dm_G.pth (the class body of nrdm_3) and its
    QAT layout; a 6-block checkpoint (nrdm_6) and a SESR checkpoint are refused."""
    torch = pytest.importorskip("torch")
    import sim
    from models import nr, dm, nrdm_3_sim, nrdm_6, sesr_sim
    assert sim.MODELS[1] is nr.nr and sim.MODELS[2] is dm.dm
    assert sorted(nr.nr().state_dict()) == sorted(dm.dm().state_dict()) == sorted(nrdm_3_sim.nr().state_dict())
    for mflag in (1, 2):
        torch.manual_seed(mflag)
        src = sim.MODELS[mflag]()
        ckpt = str(tmp_path / f"m{mflag}_G.pth")
        torch.save(src.state_dict(), ckpt)
        m = sim.float_model(mflag, ckpt=ckpt)
        src.collapse()
        for a, b in zip([m.conv_first] + list(m.residual_block) + [m.conv_last], [src.conv_first] + list(src.residual_block) + [src.conv_last]):
            assert torch.equal(a.conv_expand.weight, b.conv_expand.weight) and torch.equal(a.conv_expand.bias, b.conv_expand.bias)
        assert m.__dict__["sesrq_skip_quant_scale"] is None
        add = record("nr_qat" if mflag == 1 else "dm_qat")[1]["qat_add"]
        qckpt = str(tmp_path / f"m{mflag}_qat_G.pth")
        torch.save(QO.qat_state_dict(mflag, add), qckpt)
        mq = sim.float_model(mflag, ckpt=qckpt)
        assert np.float32(mq.__dict__["sesrq_skip_quant_scale"]) == np.float32(add["traced_scale"])
        for other, cls in (("nrdm_6", nrdm_6.nr), ("sesr", sesr_sim.sesr)):
            bad = str(tmp_path / f"{other}_{mflag}.pth")
            torch.save(cls().state_dict(), bad)
            with pytest.raises(ValueError, match=f"MFLAG {mflag}"):
                sim.float_model(mflag, ckpt=bad)
    with pytest.raises(ValueError, match="MFLAG 7"):
        sim.float_model(7)


def test_float_model_takes_the_fixture_params():
    """--params: the collapsed convs of the fixture and its calibrated domains (STORE)."""
    pytest.importorskip("torch")
    import sim
    from sesrq.store import STORE
    for case in CASES:
        STORE.clear()
        Wf, bf, pm = params(case)
        m = sim.float_model(MFLAG[case], params=os.path.join(ND, case + ".params.npz"))
        convs = [m.conv_first.conv_expand] + [b.conv_expand for b in m.residual_block] + [m.conv_last.conv_expand]
        for k, c in enumerate(convs):
            assert np.array_equal(c.weight.detach().numpy(), Wf[k]) and np.array_equal(c.bias.detach().numpy(), bf[k])
    STORE.clear()


def test_scored_calibration_refuses_mflag_1_and_takes_mflag_2():
    """The scored calibration loop has no mosaic form: MFLAG 1 is refused with a message that begins "MFLAG 1" ("Not
    covered"); the pass alone (scored=False: test.py --mflag 1 without --gt) is not.  MFLAG 2 is scored in the RGB form."""
    import types
    from sesrq import quality
    stub = types.SimpleNamespace(in_channels=3, method="minmax")
    for kind in ("f32", "raw"):
        with pytest.raises(ValueError, match="^MFLAG 1"):
            quality.check_calibration_input(stub, 1, kind)
        quality.check_calibration_input(stub, 1, kind, scored=False)
        quality.check_calibration_input(stub, 2, kind)
    with pytest.raises(ValueError, match="^MFLAG 1"):
        quality.evaluate_calibration(stub, [], [], 1)
    with pytest.raises(ValueError, match="MFLAG 2"):
        quality.check_calibration_input(stub, 2, "image")
    with pytest.raises(ValueError, match="MFLAG 5"):
        quality.evaluate_raw(None, [], [], 5)


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _engine(case, **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(os.path.join(ND, case + ".crop.npz")), device(), **kw)


def _calibrator(case):
    from sesrq.calibrate import Calibrator
    Wf, bf, _ = params(case)
    return Calibrator(Wf, bf, 1, device(), quan_bits=8, skip_quant_scale=skip_scale(case))


@pytest.mark.gpu
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("case", CASES)
def test_crop_fixtures_on_every_plan(case, plan):
    """The reference-made crop on the default plan (fused trio), one launch per layer, and the dot4 kernels, from the fp32 frame and
    from the int8 q0: the int8 and fp32 outputs are the reference's bytes."""
    import torch
    fx, meta = crop(case)
    e = _engine(case, **PLANS[plan])
    names = e.layer_engines()
    if plan == "dot4":
        assert not any(n.startswith("mfma") for n in names), names
    else:
        assert all(n.startswith("mfma") for n in names) and (plan == "default" or not any("trio" in n for n in names)), names
    for what, x in (("fp32 input", fx["x"]), ("int8 input", fx["input0"])):
        q, y = e.forward(to_device(x))
        torch.cuda.synchronize()
        same(f"{case} {plan} {what} q_out", q, fx["input5"])
        same(f"{case} {plan} {what} y", y, fx["out"])
        assert sha256(y.cpu().numpy()) == meta["sha"]["out"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_device_calibration_reproduces_the_records(case):
    """Calibrator.enqueue_raw over the raw dataset frames a, b, c (a QAT record: at its checkpoint's QuantAdd scale): the mode-0 outputs
    against the reference's crops (plain checkpoints), then the running ranges and the final domains against the record."""
    fx, rec = record(case)
    cal = _calibrator(case)
    step = rec["scale"][5]
    h, w = rec["crop"]
    for f in FRAMES:
        y = cal.enqueue_raw(to_device(raw_frame(f)[0]))
        assert list(y.shape) == rec["per_frame"][f]["out_shape"]
        if f"out_{f}" in fx.files:
            d = np.abs(y[:, :, :h, :w].cpu().numpy().astype(np.float64) - fx[f"out_{f}"]) / step
            print(case, f, "max steps", d.max(), "mean steps", d.mean())
            assert d.max() <= (OUT_MAX_STEPS if f == "a" else OUT_MAX_STEPS_NATURAL) and d.mean() <= OUT_MEAN_STEPS, (f, d.max(), d.mean())
    assert ("out_a" in fx.files) == (rec["qat_add"] is None)
    _ranges_and_domains(cal, rec)
    assert list(cal.bundle().zero) == rec["zero"]


@pytest.mark.gpu
def test_evaluate_calibration_mflag_2_and_the_mflag_1_refusal():
    """evaluate_calibration(..., 2, kind="raw") over frames a, b, c against the reference's mode-0 outputs scored by the RGB restatement;
    at MFLAG 1 it raises before any device work."""
    from sesrq import quality
    _, rec = record("dm")
    cal = _calibrator("dm")
    pairs = [raw_frame(f) for f in FRAMES]
    res = quality.evaluate_calibration(cal, [p[0] for p in pairs], [p[1] for p in pairs], 2, kind="raw")
    want = np.array([[rec["per_frame"][f][k] for k in ("mse", "psnr", "ssim")] for f in FRAMES])
    print("dm", res.tolist(), want.tolist())
    np.testing.assert_allclose(res[:, 1], want[:, 1], rtol=0, atol=PSNR_ATOL)
    np.testing.assert_allclose(res[:, 2], want[:, 2], rtol=0, atol=SSIM_ATOL)
    _ranges_and_domains(cal, rec)
    cal1 = _calibrator("nr")
    with pytest.raises(ValueError, match="^MFLAG 1"):
        quality.evaluate_calibration(cal1, [p[0] for p in pairs], [p[1] for p in pairs], 1, kind="raw")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nr", "nr_qat"])
def test_evaluate_raw_mflag_1_equals_the_mosaic_oracle(case):
    """evaluate_raw(engine, raws, gts, 1): the int8 output scored on the Bayer mosaic.  Against tests/mosaic_oracle.py on the numpy
    oracle's output frame; the int8 score has the bits of the fp32 output's score."""
    import torch
    from sesrq import quality
    fx, _ = crop(case)
    net = O.net_from_fixture(fx)
    e = _engine(case)
    pairs = [raw_frame(f) for f in ("b", "c")]
    got = quality.evaluate_raw(e, [p[0] for p in pairs], [p[1] for p in pairs], 1)
    assert got.shape == (2, 3)
    for k, f in enumerate(("b", "c")):
        y = O.forward(net, ref_inp(f))["y"]
        gt = ref_gt(f)
        want = M.metrics(y, gt)
        print(case, f, got[k].tolist(), want[0].tolist())
        _check(got[k:k + 1], want[:, 1], want[:, 2], (case, f))
        _, yf = e.forward_raw(to_device(raw_frame(f)[0]), want_q=False, want_f=True)
        same(f"{case} {f} fp32 output", yf, y)
        sf = quality.score(yf, to_device(gt), 1)
        torch.cuda.synchronize()
        assert sf.cpu().numpy().tobytes() == got[k:k + 1].tobytes(), (case, f, sf, got[k])
    # the same frames from the fp32 route
    via = quality.evaluate(e, [torch.from_numpy(ref_inp(f)) for f in ("b", "c")], [torch.from_numpy(ref_gt(f)) for f in ("b", "c")], 1)
    assert via.tobytes() == got.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["dm", "dm_qat"])
def test_evaluate_raw_mflag_2_equals_the_rgb_oracle(case):
    from sesrq import quality
    fx, _ = crop(case)
    net = O.net_from_fixture(fx)
    e = _engine(case)
    pairs = [raw_frame(f) for f in ("b", "c")]
    got = quality.evaluate_raw(e, [p[0] for p in pairs], [p[1] for p in pairs], 2)
    for k, f in enumerate(("b", "c")):
        want = Q.metrics(O.forward(net, ref_inp(f))["y"], ref_gt(f), 3)
        _check(got[k:k + 1], want[:, 1], want[:, 2], (case, f))
    assert got.tobytes() == quality.evaluate_raw(e, [p[0] for p in pairs], [p[1] for p in pairs], 3).tobytes()      # one form


@pytest.mark.gpu
@pytest.mark.parametrize("mflag,case,task", [(1, "nr", "nr"), (2, "dm", "dm")])
def test_sim_main_runs_end_to_end(mflag, case, task, capsys, tmp_path):
    """sim.py --mflag 1|2 --params --input *.raw --gt --save-png: the output is the oracle's frame, the mean line has the reference's
    format and the oracle's values."""
    import sim
    from sesrq.store import STORE
    from sesrq import image
    fx, _ = crop(case)
    raw, gt16 = raw_frame("c")
    rawp = str(tmp_path / f"framec_{raw.shape[0]}_{raw.shape[1]}.raw")
    raw.astype("<u2").tofile(rawp)
    np.save(str(tmp_path / "gt16.npy"), gt16)
    png = str(tmp_path / "out.png")
    STORE.clear()
    y = sim.main(["--mflag", str(mflag), "--params", os.path.join(ND, case + ".params.npz"), "--input", rawp,
                  "--gt", str(tmp_path / "gt16.npy"), "--save-png", png])
    out = capsys.readouterr().out.strip().split("\n")
    STORE.clear()
    want_y = O.forward(O.net_from_fixture(fx), ref_inp("c"))["y"]
    same("sim output", y, want_y)
    want = M.metrics(want_y, ref_gt("c")) if mflag == 1 else Q.metrics(want_y, ref_gt("c"), 3)
    line = [l for l in out if "mean psnr is" in l]
    assert len(line) == 1
    m = re.fullmatch(task + r" mean psnr is:  (\S+)  ssim is:  (\S+)", line[0])
    assert m, line
    assert abs(float(m.group(1)) - want[0, 1]) <= 1e-5 and abs(float(m.group(2)) - want[0, 2]) <= 1e-6, (line, want)
    assert abs(float(out[out.index(line[0]) - 1]) - want[0, 1]) <= 1e-5
    u8 = image.load_image(png)
    assert u8.shape == (raw.shape[0], raw.shape[1], 3)
    assert np.array_equal(u8.transpose(2, 0, 1), (np.clip(want_y[0], 0, 1) * np.float32(255)).astype(np.uint8))


@pytest.mark.gpu
def test_test_py_calibrates_mflag_1_and_2(tmp_path, capsys):
    """test.py --mflag 1 --params --input *.raw (no --gt) gives the record's domains; with --gt it stops with "MFLAG 1"; --mflag 2
    --gt scores and calibrates."""
    from calib_cases import load_test_py
    mod = load_test_py()
    paths, gts = [], []
    for f in FRAMES:
        raw, gt16 = raw_frame(f)
        p = str(tmp_path / f"frame{f}_{raw.shape[0]}_{raw.shape[1]}.raw")
        raw.astype("<u2").tofile(p)
        np.save(str(tmp_path / f"gt_{f}.npy"), gt16)
        paths.append(p)
        gts.append(str(tmp_path / f"gt_{f}.npy"))
    _, rec = record("nr")
    scale, zero = mod.main(["--mflag", "1", "--params", os.path.join(ND, "nr.params.npz"), "--input"] + paths)
    out = capsys.readouterr().out
    assert "mean psnr" not in out and list(zero) == rec["zero"]
    np.testing.assert_allclose(scale, rec["scale"], rtol=2e-4)
    with pytest.raises(SystemExit, match="MFLAG 1"):
        mod.main(["--mflag", "1", "--params", os.path.join(ND, "nr.params.npz"), "--input"] + paths + ["--gt"] + gts)
    capsys.readouterr()
    _, rec = record("dm")
    scale, zero = mod.main(["--mflag", "2", "--params", os.path.join(ND, "dm.params.npz"), "--input"] + paths + ["--gt"] + gts)
    out = capsys.readouterr().out
    m = re.search(r"dm mean psnr is:  (\S+)  ssim is:  (\S+)", out)
    want = np.array([[rec["per_frame"][f][k] for k in ("psnr", "ssim")] for f in FRAMES]).mean(axis=0)
    assert m and abs(float(m.group(1)) - want[0]) <= PSNR_ATOL and abs(float(m.group(2)) - want[1]) <= SSIM_ATOL, (out[-400:], want)
    assert list(zero) == rec["zero"]
    np.testing.assert_allclose(scale, rec["scale"], rtol=2e-4)
