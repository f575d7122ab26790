"""The device-resident calibration pass (Calibrator.enqueue / enqueue_raw / enqueue_image, sesrq_calib_observe_slot / _conv_slot /
_fakequant_slot), its scores (quality.evaluate_calibration, sesrq_eval_anchored) and test.py --input / --gt.

GPU: bit identity with the host-driven pass (Calibrator.observe) on the committed frames -- per-frame mode-0 outputs, running min/max,
per-batch (scale, zero), finalize() and bundle() -- at b = 8 for nrdm_3, SESR-x4 and SESR-x2 and at b = 4, 2 for nrdm_3; no host wait
while frames are enqueued; the anchored x2 score against scoring a pre-added frame; the CLI's lines.  CPU: the refusals, raised before
any device work."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import GOLDEN, load_fixture
from calib_cases import calibrators, image_frames, load_test_py, raw_dataset_frames
from helpers import device, full_input

CASES = {"nrdm_3": 3, "sesr_x4": 5, "sesr_x2_rand": 6}


def f32_frames(mflag):
    """Three fp32 frames from the reference's random 80 x 960 frame: itself, a flipped half-scale copy, a crop."""
    x = full_input(dict(mflag=mflag))
    return [x, np.ascontiguousarray(x[:, :, ::-1, :] * np.float32(0.5)), np.ascontiguousarray(x[:, :, 8:45, 100:421])]


# ----------------------------------------------------------------------------------------------------------------- CPU
def stub(cin, method="minmax"):
    return types.SimpleNamespace(in_channels=cin, method=method)


def test_refusals_before_device_work():
    from sesrq import quality
    with pytest.raises(ValueError, match="3-channel"):
        quality.check_calibration_input(stub(1), 3, "raw")           # raw frames for a 1-channel net
    with pytest.raises(ValueError, match="MFLAG 5"):
        quality.check_calibration_input(stub(1), 5, "raw")           # raw frames feed MFLAG 3 / 4 only
    with pytest.raises(ValueError, match="MFLAG 3"):
        quality.check_calibration_input(stub(3), 3, "image")         # images feed MFLAG 5 / 6 only
    with pytest.raises(ValueError, match="channel"):
        quality.check_calibration_input(stub(3), 5, "image")         # MFLAG 5 images are the 1-channel luma
    with pytest.raises(ValueError, match="entropy"):
        quality.check_calibration_input(stub(3, "entropy"), 3, "f32")
    with pytest.raises(ValueError, match="kind"):
        quality.check_calibration_input(stub(3), 3, "u8")
    with pytest.raises(ValueError, match="MFLAG 1"):
        quality.check_calibration_input(stub(3), 1, "f32")
    quality.check_calibration_input(stub(3), 3, "raw")
    quality.check_calibration_input(stub(1), 5, "image")
    quality.check_calibration_input(stub(3), 6, "image")
    # evaluate_calibration refuses through the same checks, before it touches the calibrator's device
    with pytest.raises(ValueError, match="entropy"):
        quality.evaluate_calibration(stub(3, "entropy"), [], [], 3)


def test_cli_refusals_before_device_work(tmp_path):
    mod = load_test_py()
    nr = os.path.join(GOLDEN, "nrdm_3.params.npz")
    x4 = os.path.join(GOLDEN, "sesr_x4.params.npz")
    img = str(tmp_path / "lr.npy")
    np.save(img, np.zeros((8, 8, 3), np.uint8))
    raw = str(tmp_path / "f_8_8.raw")
    np.zeros((8, 8), "<u2").tofile(raw)
    frames = os.path.join(GOLDEN, "rand_DM_Input_80x960.npy")
    with pytest.raises(SystemExit, match="MFLAG 3"):
        mod.main(["--mflag", "3", "--params", nr, "--input", img, "--image"])           # images for MFLAG 3
    with pytest.raises(SystemExit, match="MFLAG 5"):
        mod.main(["--mflag", "5", "--params", x4, "--input", raw])                      # raw frames for the 1-channel SESR-x4
    with pytest.raises(SystemExit, match="entropy"):
        mod.main(["--mflag", "3", "--params", nr, "--input", raw, "--method", "entropy"])
    with pytest.raises(SystemExit, match="one of them"):
        mod.main(["--mflag", "3", "--params", nr, "--input", raw, "--frames", frames])
    with pytest.raises(SystemExit, match="one of them"):
        mod.main(["--mflag", "3", "--params", nr])


def test_slot_layout_matches_the_library():
    from sesrq import _lib
    assert C.sizeof(_lib.CalibSlot) == _lib.lib().sesrq_calib_slot_bytes() == 136
    s = (_lib.CalibSlot * 2)()
    assert _lib.lib().sesrq_calib_slots_init(s, 2) == 0
    assert s[1].ord[0] == 0xffffffff and s[1].ord[1] == 0 and s[1].batches == 0 and s[1].degenerate == 0
    assert s[1].run_min == float("inf") and s[1].run_max == float("-inf")


def test_anchored_entry_checks_without_a_device():
    from sesrq import quality
    lib = quality.anchored_lib()
    fake = C.c_void_p(4096)                       # never dereferenced: every check runs before any HIP call
    ws = C.c_size_t(1 << 20)
    d = quality.EvalDesc(form=quality.FORM_RGB, pred_dtype=quality.PRED_F32, pred_scale=0.0, pred_zero=0)
    assert lib.sesrq_eval_anchored(C.byref(d), fake, fake, fake, 1, 3, 16, 16, fake, fake, ws, None) != 0
    assert "x2 form" in quality.last_error()
    d.form = quality.FORM_X2
    assert lib.sesrq_eval_anchored(C.byref(d), fake, fake, fake, 1, 3, 15, 16, fake, fake, ws, None) != 0
    assert "twice" in quality.last_error()
    assert lib.sesrq_eval_anchored(C.byref(d), fake, None, fake, 1, 3, 16, 16, fake, fake, ws, None) != 0
    assert "lr" in quality.last_error()


# ----------------------------------------------------------------------------------------------------------------- GPU
def _host_input(kind, frame, mflag):
    """The fp32 frame the host pass observes: the reference's input, decoded as the device pass decodes it."""
    import torch
    from sesrq import image, raw
    t = torch.from_numpy(np.ascontiguousarray(frame)).to(device())
    if kind == "raw":
        return raw.unpack(None, t, want_q=False, want_spread=True)[1]
    if kind == "image":
        return image.decode(None, t, image.form_of(mflag), want_q=False, want_f=True)[1]
    return t


def _enqueue(cal, kind, frame):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(frame)).to(device())
    return cal.enqueue_raw(t) if kind == "raw" else cal.enqueue_image(t) if kind == "image" else cal.enqueue(t)


def _assert_same_calibration(dev_cal, host_cal):
    s_d, z_d = dev_cal.finalize()
    s_h, z_h = host_cal.finalize()
    assert dev_cal.run_min == host_cal.run_min and dev_cal.run_max == host_cal.run_max
    assert dev_cal.last_scale == host_cal.last_scale and dev_cal.last_zero == host_cal.last_zero
    assert s_d == s_h and z_d == z_h
    bd, bh = dev_cal.bundle(), host_cal.bundle()
    assert bd.scale == bh.scale and bd.zero == bh.zero and (bd.M_res, bd.n_res) == (bh.M_res, bh.n_res)
    for ld, lh in zip(bd.layers, bh.layers):
        np.testing.assert_array_equal(ld.wq, lh.wq)
        np.testing.assert_array_equal(ld.add_const, lh.add_const)
        assert (ld.M, ld.n, ld.relu) == (lh.M, lh.n, lh.relu)


def _frames(case, kind):
    mflag = CASES[case]
    if kind == "raw":
        return [r for r, _ in raw_dataset_frames()]
    if kind == "image":
        return [lr for lr, _ in image_frames(mflag)]
    return f32_frames(mflag)


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind,bits", [("nrdm_3", "f32", 8), ("sesr_x4", "f32", 8), ("sesr_x2_rand", "f32", 8),
                                            ("nrdm_3", "raw", 8), ("sesr_x4", "image", 8), ("sesr_x2_rand", "image", 8),
                                            ("nrdm_3", "raw", 4), ("nrdm_3", "f32", 2)])
def test_device_pass_equals_host_pass(case, kind, bits):
    """Frame by frame: the mode-0 output and the per-batch (scale, zero) of enqueue* equal observe()'s on the same decoded frame;
    after the frames, running min/max, finalize() and bundle() are identical."""
    import torch
    dev_cal, host_cal, mflag = calibrators(case, bits)
    for fr in _frames(case, kind):
        y_d = _enqueue(dev_cal, kind, fr)
        y_h = host_cal.observe(_host_input(kind, fr, mflag))
        torch.cuda.synchronize()
        assert y_d.shape == y_h.shape and torch.equal(y_d, y_h)
        dev_cal.sync()
        assert dev_cal.last_scale == host_cal.last_scale and dev_cal.last_zero == host_cal.last_zero
    _assert_same_calibration(dev_cal, host_cal)


@pytest.mark.gpu
def test_device_pass_batches_and_reset():
    """A batch of N frames is one batch on both passes; reset() forgets the slots; mixing the passes is refused."""
    import torch
    dev_cal, host_cal, _ = calibrators("sesr_x2_rand")
    x = torch.from_numpy(np.concatenate(f32_frames(6)[:2])).to(device())
    assert torch.equal(dev_cal.enqueue(x), host_cal.observe(x))
    with pytest.raises(RuntimeError, match="reset"):
        dev_cal.observe(x)
    with pytest.raises(RuntimeError, match="reset"):
        host_cal.enqueue(x)
    _assert_same_calibration(dev_cal, host_cal)
    dev_cal.reset()
    host_cal.reset()
    y = x[:1].contiguous()
    y_h = host_cal.observe(y)
    out = torch.empty_like(y_h)
    assert dev_cal.enqueue(y, out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out, y_h)
    _assert_same_calibration(dev_cal, host_cal)


@pytest.mark.gpu
def test_device_pass_refuses_entropy_and_flags_a_constant_input():
    import torch
    from sesrq.calibrate import Calibrator
    p, _ = load_fixture(os.path.join(GOLDEN, "nrdm_3.params.npz"))
    cal = Calibrator([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], 1, device(), method="entropy")
    with pytest.raises(ValueError, match="entropy"):
        cal.enqueue(torch.zeros((1, 3, 16, 16), device=device()))
    cal = Calibrator([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], 1, device())
    with pytest.raises(ValueError, match="3-channel|channels"):
        cal.enqueue(torch.zeros((1, 1, 16, 16), device=device()))
    cal.enqueue(torch.full((1, 3, 16, 16), 0.5, device=device()))        # max == min: observe() asserts, finalize() raises
    with pytest.raises(RuntimeError, match="all equal,0"):
        cal.finalize()


@pytest.mark.gpu
def test_enqueue_does_not_wait_on_the_host(monkeypatch):
    """K frames of each kind enqueue with no host synchronisation: under torch's sync debug mode "error", and with every host
    readback of torch made to fail."""
    import torch
    cases = [("nrdm_3", "f32"), ("nrdm_3", "raw"), ("sesr_x4", "image"), ("sesr_x2_rand", "image")]
    prepared = []
    for case, kind in cases:
        cal, _, _ = calibrators(case)
        frames = [torch.from_numpy(np.ascontiguousarray(f)).to(device()) for f in _frames(case, kind)]
        # first use of a shape / decoder context outside the checked region: buffers are kept per (N, H, W)
        for f in frames:
            cal.enqueue_raw(f) if kind == "raw" else cal.enqueue_image(f) if kind == "image" else cal.enqueue(f)
        prepared.append((cal, kind, frames))
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("host synchronisation while enqueueing")
    outs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        with monkeypatch.context() as m:
            for name in ("cpu", "item", "tolist", "numpy"):
                m.setattr(torch.Tensor, name, refuse)
            m.setattr(torch.cuda, "synchronize", refuse)
            for cal, kind, frames in prepared:
                for _ in range(2):
                    for f in frames:
                        outs.append(cal.enqueue_raw(f) if kind == "raw" else cal.enqueue_image(f) if kind == "image" else cal.enqueue(f))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert len(outs) == 2 * sum(len(f) for _, _, f in prepared)
    for cal, _, _ in prepared:
        cal.finalize()


@pytest.mark.gpu
def test_anchored_score_equals_scoring_the_added_frame():
    """sesrq_eval_anchored on the SESR-x2 image fixture: the bits of quality.score(pred + up2(x), gt, 6)."""
    import torch
    from sesrq import image, quality
    cal, _, _ = calibrators("sesr_x2_rand")
    for lr, hr in image_frames(6):
        y = cal.enqueue_image(torch.from_numpy(lr).to(device()))
        x = cal.last_input.clone()
        gt = image.load_gt(hr, 6, device())
        got = quality.score_anchored(y, x, gt)
        want = quality.score(y + x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), gt, 6)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", [("nrdm_3", "raw"), ("sesr_x4", "image"), ("sesr_x2_rand", "image"), ("nrdm_3", "f32")])
def test_evaluate_calibration_equals_host_pass_then_score(case, kind):
    """evaluate_calibration: per-frame scores equal scoring observe()'s outputs one by one (MFLAG 6 anchored), and the
    calibration it accumulated equals the host pass's."""
    import torch
    from sesrq import image, quality, raw
    dev_cal, host_cal, mflag = calibrators(case)
    if kind == "raw":
        pairs = raw_dataset_frames()
    elif kind == "image":
        pairs = image_frames(mflag)
    else:
        xs = f32_frames(mflag)[:2]
        pairs = [(x, np.clip(x[:, :, :, :] * np.float32(0.9), 0, 1)) for x in xs]
    got = quality.evaluate_calibration(dev_cal, [p[0] for p in pairs], [p[1] for p in pairs], mflag, kind=kind)
    want = []
    for fr, g in pairs:
        x = _host_input(kind, fr, mflag)
        y = host_cal.observe(x)
        gt = raw.load_gt(g, device()) if kind == "raw" else image.load_gt(g, mflag, device()) if kind == "image" else \
            torch.from_numpy(g).to(device())
        if mflag == 6:
            y = y + x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        want.append(quality.score(y, gt, mflag).cpu().numpy())
    np.testing.assert_array_equal(got, np.concatenate(want))
    _assert_same_calibration(dev_cal, host_cal)


def _lines(out):
    return [l for l in out.splitlines() if l.strip()]


def _check_reference_order(lines, K, task, bits):
    """each frame's PSNR, the mean line, calibrate start, (scale, zero) x 6, calibrate end, bit: b -- the reference's order."""
    i = next(i for i, l in enumerate(lines) if re.fullmatch(r"-?[0-9.]+(e[-+]?[0-9]+)?|inf", l))
    for l in lines[i:i + K]:
        float(l)
    assert re.fullmatch(re.escape(task) + r" mean psnr is:  \S+  ssim is:  \S+", lines[i + K]), lines[i + K]
    assert lines[i + K + 1] == "calibrate start"
    sz = lines[i + K + 2:i + K + 14]
    assert [l.split(":")[0] for l in sz] == ["scale", "zero"] * 6
    assert lines[i + K + 14] == "calibrate end" and lines[i + K + 15] == f"bit: {bits}"
    return [float(l.split()[1]) for l in sz[0::2]], [int(l.split()[1]) for l in sz[1::2]]


@pytest.mark.gpu
def test_cli_raw_frames_with_gt(tmp_path, capsys, monkeypatch):
    """test.py --mflag 3 --input <raw frames> --gt <npy>: the reference's lines in its order; the domains equal the --frames run
    (host pass) on the spread fp32 frames."""
    import torch
    import define
    from sesrq import raw
    from sesrq.store import STORE
    monkeypatch.setattr(define, "QUAN_BIT", 8)
    frames = raw_dataset_frames()
    paths, gts = [], []
    for i, (r, g) in enumerate(frames):
        p = tmp_path / f"frame{i}_{r.shape[0]}_{r.shape[1]}.raw"
        r.astype("<u2").tofile(p)
        paths.append(str(p))
        gp = tmp_path / f"gt{i}.npy"
        np.save(gp, g)
        gts.append(str(gp))
    params = os.path.join(GOLDEN, "nrdm_3.params.npz")
    mod = load_test_py()
    STORE.clear()
    scale, zero = mod.main(["--mflag", "3", "--params", params, "--input", *paths, "--gt", *gts])
    s2, z2 = _check_reference_order(_lines(capsys.readouterr().out), len(frames), "nrdm_small", 8)
    assert z2 == list(zero) and s2 == [float(str(v)) for v in scale]
    # the same frames, spread to fp32 on the device, through the host-driven pass of the spliced mode-0 model (what --frames runs)
    import sim
    STORE.clear()
    model = mod.splice_calibration(sim.float_model(3, None, params))
    for r, _ in frames:
        model(raw.unpack(None, torch.from_numpy(r).to(device()), want_q=False, want_spread=True)[1])
    s_h, z_h = mod.finish_calibration(STORE, 5)
    assert list(scale) == list(s_h) and list(zero) == list(z_h)


@pytest.mark.gpu
def test_cli_pngs_with_gt_and_without(tmp_path, capsys, monkeypatch):
    """test.py --mflag 5 --input LR.png ... --gt HR.png ...: the reference's lines; the domains equal the --frames run on the decoded
    luma frames; without --gt no score is printed and the domains are the same."""
    import torch
    import define
    from sesrq import image
    from sesrq.store import STORE
    monkeypatch.setattr(define, "QUAN_BIT", 8)
    pairs = image_frames(5)
    lrs, hrs = [], []
    for i, (lr, hr) in enumerate(pairs):
        image.save_png(str(tmp_path / f"lr{i}.png"), lr)
        image.save_png(str(tmp_path / f"hr{i}.png"), hr)
        lrs.append(str(tmp_path / f"lr{i}.png"))
        hrs.append(str(tmp_path / f"hr{i}.png"))
    params = os.path.join(GOLDEN, "sesr_x4.params.npz")
    mod = load_test_py()
    STORE.clear()
    scale, zero = mod.main(["--mflag", "5", "--params", params, "--input", *lrs, "--gt", *hrs])
    _check_reference_order(_lines(capsys.readouterr().out), len(pairs), "srx4", 8)
    import sim
    STORE.clear()
    model = mod.splice_calibration(sim.float_model(5, None, params))
    for lr, _ in pairs:
        model(image.decode(None, torch.from_numpy(lr).to(device()), "y", want_q=False, want_f=True)[1])
    s_h, z_h = mod.finish_calibration(STORE, 5)
    assert list(scale) == list(s_h) and list(zero) == list(z_h)
    STORE.clear()
    s3, z3 = mod.main(["--mflag", "5", "--params", params, "--input", *lrs, "--save-bundle", str(tmp_path / "b.npz")])
    out = capsys.readouterr().out
    assert "mean psnr" not in out and "calibrate start" in out
    assert list(s3) == list(scale) and list(z3) == list(zero)
    from sesrq.bundle import Bundle
    assert Bundle.load(str(tmp_path / "b.npz")).zero == list(zero)
