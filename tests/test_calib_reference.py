"""The device-resident calibration pass against the reference's own calibration loop over the dataset frames
(tests/golden/calib/*.npz, made by tests/golden/make_calib_golden.py from the reference's mode-0 graph).

Frames (a), (b), (c) of the raw fixture (nrdm_3, MFLAG 3) and of the image fixture (SESR-x4, MFLAG 5; SESR-x2, MFLAG 6) go through
Calibrator.enqueue_raw / enqueue_image and quality.evaluate_calibration.  The reference forms its sums in fp32 in oneDNN's order, this
path exactly in integers (csrc/sesrq_calib.hip), so the bar is a tolerance: the running ranges within 1e-4 of their span, zeros equal,
scales within rtol 2e-4 (test_gpu_parity.py:test_calibration_pass_matches_reference_ranges), and the mode-0 outputs and their scores
close to the reference's (bounds below)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_fixture
from calib_cases import calibrators, image_frames, raw_dataset_frames

CASES = ["nrdm_3", "sesr_x4", "sesr_x2_rand"]
# Output deviation in steps of the output domain (scale[5]).  Where an upstream fake-quantiser input lies at a rounding tie the two
# summation orders break it differently and the pixel moves by a step or two: on frame (a), a synthetic sweep of every code at every
# phase, 0.2 % (x2) to 2.7 % (x4) of the cropped pixels do, by at most 2.2 steps (mean 0.03 step); on the natural frames (b), (c) no pixel
# moves by more than 0.33 step (measured on the MI355X).
OUT_MAX_STEPS = 4.0                 # any frame
OUT_MEAN_STEPS = 0.05               # any frame, mean over the crop
OUT_MAX_STEPS_NATURAL = 0.5         # frames (b), (c)
PSNR_ATOL, SSIM_ATOL = 1e-2, 1e-4


def fixture(case):
    return load_fixture(os.path.join(GOLDEN, "calib", f"{case}.npz"))


def pairs(case, mflag):
    return raw_dataset_frames() if case == "nrdm_3" else image_frames(mflag)


def test_fixtures_hold_the_dataset_frames():
    """CPU: each fixture covers frames a, b, c of its dataset, with a crop of every frame's output and the metrics of every frame."""
    for case in CASES:
        fx, meta = fixture(case)
        assert meta["frames"] == ["a", "b", "c"] and len(meta["min"]) == len(meta["zero"]) == 6
        for f in meta["frames"]:
            assert fx[f"out_{f}"].dtype == np.float32 and fx[f"out_{f}"].ndim == 4
            assert set(meta["per_frame"][f]) >= {"mse", "psnr", "ssim", "out_shape"}
        assert "quality_oracle" in meta["metrics"]


def _ranges_and_domains(cal, meta):
    scale, zero = cal.finalize()
    for k in range(6):
        span = meta["max"][k] - meta["min"][k]
        assert abs(cal.run_min[k] - meta["min"][k]) <= 1e-4 * span, (k, cal.run_min[k], meta["min"][k])
        assert abs(cal.run_max[k] - meta["max"][k]) <= 1e-4 * span, (k, cal.run_max[k], meta["max"][k])
    assert list(zero) == meta["zero"]
    np.testing.assert_allclose(scale, meta["scale"], rtol=2e-4)
    return scale, zero


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_enqueue_matches_the_reference_loop(case):
    """enqueue_raw / enqueue_image over frames a, b, c: each frame's mode-0 output against the reference's crop, then the running
    ranges and the final domains against the reference's."""
    import torch
    fx, meta = fixture(case)
    cal, _, mflag = calibrators(case)
    assert mflag == meta["mflag"]
    step = meta["scale"][5]
    h, w = meta["crop"]
    for f, (x, _) in zip(meta["frames"], pairs(case, mflag)):
        t = torch.from_numpy(np.ascontiguousarray(x)).to(cal.device)
        y = cal.enqueue_raw(t) if meta["kind"] == "raw" else cal.enqueue_image(t)
        assert list(y.shape) == meta["per_frame"][f]["out_shape"]
        got = y[:, :, :h, :w].cpu().numpy()
        want = fx[f"out_{f}"]
        d = np.abs(got.astype(np.float64) - want) / step
        assert d.max() <= (OUT_MAX_STEPS if f == "a" else OUT_MAX_STEPS_NATURAL) and d.mean() <= OUT_MEAN_STEPS, (f, d.max(), d.mean())
    _ranges_and_domains(cal, meta)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_evaluate_calibration_matches_the_reference_scores(case):
    """evaluate_calibration over frames a, b, c: per-frame PSNR / SSIM of the mode-0 output (MFLAG 6 anchored) against the reference's
    outputs scored by the metric restatement, the mean line's values, and the domains it accumulated."""
    fx, meta = fixture(case)
    cal, _, mflag = calibrators(case)
    ps = pairs(case, mflag)
    res = quality_eval(cal, ps, mflag, meta["kind"])
    want = np.array([[meta["per_frame"][f][k] for k in ("mse", "psnr", "ssim")] for f in meta["frames"]])
    np.testing.assert_allclose(res[:, 1], want[:, 1], rtol=0, atol=PSNR_ATOL, err_msg=json.dumps(res[:, 1].tolist()))
    np.testing.assert_allclose(res[:, 2], want[:, 2], rtol=0, atol=SSIM_ATOL, err_msg=json.dumps(res[:, 2].tolist()))
    assert abs(res[:, 1].mean() - want[:, 1].mean()) <= PSNR_ATOL and abs(res[:, 2].mean() - want[:, 2].mean()) <= SSIM_ATOL
    _ranges_and_domains(cal, meta)


def quality_eval(cal, ps, mflag, kind):
    from sesrq import quality
    return quality.evaluate_calibration(cal, [p[0] for p in ps], [p[1] for p in ps], mflag, kind=kind)
