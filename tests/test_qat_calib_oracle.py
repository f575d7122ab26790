"""tests/qat_calib_oracle.py -- the calibration pass of a QAT net, long skip merged through the QuantAdd -- against every calibration
the reference recorded for its QAT checkpoints (CPU), and the loader helper that forms the QuantAdd's scale.

Records: the four one-frame records tests/golden/<case>.params.npz (random and natural 80 x 960 frames) and the two three-frame loops
tests/golden/calib/<case>.npz (make_qat_calib_golden.py).  Bars, the project's own: running min / max within 1e-4 of the span, zero
points equal, scales within rtol 2e-4 -- over all six domains, the last domain's min included.  The three-frame loops settle that the
scale is a constant of the traced graph: with live moving-average observers frames b and c would be merged at other scales."""
import os

import numpy as np
import pytest
import torch

import qat_calib_oracle as QO
from calib_cases import (ADD, BAR, LOOPS, MEASURED, ONE_FRAME, assert_record, dataset_frames, frame_of, load_test_py,
                         scale_of)
from conftest import GOLDEN, load_fixture
from helpers import PIXEL_SHUFFLE
from oracle import calib_oracle as CO

# (record, domain) -> bar between the float64 and the fp32-faithful forms where float64 resolves a tie of the QuantAdd or of an
# upstream quantiser the other way (as EXACT_SLACK of test_calib_oracle.py): measured 1.687e-4 and 3.203e-4 of the span, both in the
# last domain's max; the fp32 form is the one that matches the record there (within 1.2e-7).
EXACT_SLACK = {("nrdm_3_qat_nat", 5): 3.4e-4, ("loop nrdm_3_qat", 5): 6.5e-4}


_RUNS = {}


def run(record, frames_of=None, exact=False):
    """The oracle's pass for a record (computed once per record and form), and the record."""
    key = (record, frames_of, exact)
    p, pm = load_fixture(os.path.join(GOLDEN, f"{record}.params.npz"))
    if frames_of is None:
        rec = pm
    else:
        _, rec = load_fixture(os.path.join(GOLDEN, "calib", f"{record}.npz"))
    if key not in _RUNS:
        frames = [frame_of(pm)] if frames_of is None else dataset_frames(frames_of, pm["mflag"])
        _RUNS[key] = QO.forward([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], PIXEL_SHUFFLE[pm["mflag"]], frames, 8,
                                scale_of(record), exact=exact, keep_outputs=False, keep_inputs=frames_of is None and not exact)
    return _RUNS[key], rec


@pytest.mark.parametrize("record", ONE_FRAME)
def test_oracle_reproduces_the_qat_records(record):
    r, rec = run(record)
    assert_record(record, r, rec)


@pytest.mark.parametrize("record", sorted(LOOPS))
def test_oracle_reproduces_the_three_frame_loops(record):
    """The reference's test.py loop over dataset frames a, b, c on the QAT-prepared model: one constant scale for all three."""
    r, rec = run(record, LOOPS[record])
    assert rec["frames"] == ["a", "b", "c"]
    assert_record("loop " + record, r, rec)


def test_only_sesr_x4_qat_is_excepted():
    assert {r for r, _ in MEASURED} == {"sesr_x4_qat"} and all(2 * m <= 1e-3 for m in MEASURED.values())


@pytest.mark.parametrize("record,frames_of", [(r, None) for r in ONE_FRAME] + sorted(LOOPS.items()))
def test_float64_and_fp32_forms_agree(record, frames_of):
    r32, rec = run(record, frames_of)
    r64, _ = run(record, frames_of, exact=True)
    name = record if frames_of is None else "loop " + record
    for k in range(6):
        bar, span = EXACT_SLACK.get((name, k), BAR), rec["max"][k] - rec["min"][k]
        assert abs(r64.run_max[k] - r32.run_max[k]) <= bar * span, (name, k, r64.run_max[k], r32.run_max[k])
        assert abs(r64.run_min[k] - r32.run_min[k]) <= bar * span, (name, k, r64.run_min[k], r32.run_min[k])


def test_the_plain_pass_misses_what_the_quantised_merge_reproduces():
    """The float add (oracle.calib_oracle.forward) on the three-frame loops: upstream of the merge the same ranges, bit for bit; from
    the residual sum on, off by more than 1e-3 of the span."""
    for record, frames_of in LOOPS.items():
        r, rec = run(record, frames_of)
        p, pm = load_fixture(os.path.join(GOLDEN, f"{record}.params.npz"))
        plain = CO.forward([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], PIXEL_SHUFFLE[pm["mflag"]],
                           dataset_frames(frames_of, pm["mflag"]), 8, keep_outputs=False)
        assert plain.run_max[:4] == r.run_max[:4] and plain.run_min[:4] == r.run_min[:4]
        assert any(abs(plain.run_max[k] - rec["max"][k]) > 1e-3 * (rec["max"][k] - rec["min"][k]) for k in (4, 5)), record


def test_sesr_x4_qat_deviates_by_one_upstream_tie():
    """The cause of MEASURED, named: quantiser input 1 of sesr_x4_qat holds one value (two adjacent floats), at 42 pixels, whose pre-round value is exactly
    -85.5 with the oracle's scale_1; the reference's domain 1 max is 3 ulp below the oracle's.  Upstream of that the ranges agree
    exactly, and the QuantAdd has no part in it: domains 0..3 are those of the plain oracle bit for bit."""
    r, rec = run("sesr_x4_qat")
    x, d = r.inputs[0][1], r.domains[0][1]
    t = (x / d.scale32).astype(np.float32) + d.zero32
    tie = t == np.float32(-85.5)
    assert int(tie.sum()) == 42 and np.all(np.abs(x[tie] - np.float32(0.13814925)) <= np.float32(2e-8))
    ulp = float(np.spacing(np.float32(rec["max"][1])))
    assert r.run_max[0] == rec["max"][0] and 0 < r.run_max[1] - rec["max"][1] <= 3 * ulp
    p, pm = load_fixture(os.path.join(GOLDEN, "sesr_x4_qat.params.npz"))
    plain = CO.forward([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], 4, [frame_of(pm)], 8, keep_outputs=False)
    assert plain.run_max[:4] == r.run_max[:4] and plain.run_min[:4] == r.run_min[:4]
    span = rec["max"][2] - rec["min"][2]
    assert abs(abs(r.run_max[2] - rec["max"][2]) / span - MEASURED[("sesr_x4_qat", 2)]) < 1e-6
    assert r.run_max[4] == rec["max"][4] and r.run_min[4] == rec["min"][4]          # the QuantAdd's grid: exact


# ------------------------------------------------------------------------------------------------------------- the QuantAdd itself
def test_skip_fakequant_rounds_half_away_and_clamps():
    s = np.float32(0.25)
    t = np.array([0.0, 0.124, 0.125, 0.126, -0.125, -0.126, 0.375, -0.375, 31.75, 31.9, 40.0, -32.0, -32.2, -40.0, np.inf, -np.inf], np.float32)
    want = np.array([0, 0, 1, 1, -1, -1, 2, -2, 127, 127, 127, -128, -128, -128, 127, -128], np.float32) * s
    np.testing.assert_array_equal(QO.skip_fakequant(t, s), want)
    np.testing.assert_array_equal(QO.skip_fakequant(t, s, exact=True), want.astype(np.float64))
    assert QO.skip_fakequant(np.array([np.nan], np.float32), s)[0] == -128 * s      # fmaxf(NaN, lo) = lo, as the kernel


# ------------------------------------------------------------------------------------------------------------- the loader helper
@pytest.mark.parametrize("record,mflag", [("nrdm_3_qat", 3), ("sesr_x4_qat", 5)])
def test_loader_helper_gives_the_traced_scale(record, mflag, tmp_path):
    """quantize.skip_quant_scale on a synthetic QAT state_dict with the checkpoint's observer extrema: the scale the reference's traced
    graph holds (qat_add.json traced_scale), not the one the checkpoint stores; load_checkpoint hands it on and float_model keeps it."""
    import sim
    from models import quantize_utils_pt as quantize
    add = ADD[record]
    sd = QO.qat_state_dict(mflag, add)
    s = quantize.skip_quant_scale(sd)
    assert isinstance(s, float) and np.float32(s) == np.float32(add["traced_scale"]) == scale_of(record)
    assert np.float32(s) != np.float32(add["stored_scale"])
    p = tmp_path / "fake_qat_G.pth"
    torch.save(sd, p)
    assert sim.load_checkpoint(quantize_target(mflag), str(p), mflag) == s
    assert sim.float_model(mflag, ckpt=str(p)).__dict__["sesrq_skip_quant_scale"] == s
    plain = tmp_path / "plain_G.pth"
    torch.save({k: v for k, v in sd.items() if "quantizer" not in k and not k.startswith("add_")}, plain)
    assert sim.float_model(mflag, ckpt=str(plain)).__dict__["sesrq_skip_quant_scale"] is None


def quantize_target(mflag):
    import sim
    m = sim.MODELS[mflag]()
    m.train()
    return m


def test_loader_helper_refusals_and_edges():
    from models import quantize_utils_pt as quantize
    import sim
    sd = QO.qat_state_dict(3, ADD["nrdm_3_qat"])
    assert quantize.skip_quant_scale(sim.MODELS[3]().state_dict()) is None              # not a QAT checkpoint
    assert quantize.skip_quant_scale({k: v for k, v in sd.items() if not k.startswith("add_residual.")}) is None
    for k in QO.OBSERVERS:                                                               # some of the four, not all
        with pytest.raises(ValueError, match="incomplete"):
            quantize.skip_quant_scale({n: v for n, v in sd.items() if n != "add_residual." + k})
    zero = dict(sd)
    for k in QO.OBSERVERS:
        zero["add_residual." + k] = torch.zeros(1)
    assert quantize.skip_quant_scale(zero) == float(np.finfo(np.float32).eps) == float(QO.skip_scale(0, 0, 0, 0))
    neg = dict(sd)                                                                       # the larger magnitude is the lower end
    neg["add_residual.observer_shortcut.min_val"] = torch.tensor([-2.0])
    assert np.float32(quantize.skip_quant_scale(neg)) == np.float32(2.0) / np.float32(127.5) == QO.skip_scale(0.0, 0.6, -2.0, 0.5)


def test_incomplete_state_stops_calibration_not_the_integer_path(tmp_path):
    """A QAT checkpoint with some of the four observer extrema: sim.float_model (the integer path never evaluates the QuantAdd) loads
    it as before; test.py refuses it, before any device work, unless told how to add the skip."""
    import sim
    sd = QO.qat_state_dict(3, ADD["nrdm_3_qat"])
    del sd["add_residual.observer_shortcut.max_val"]
    p = str(tmp_path / "partial_qat_G.pth")
    torch.save(sd, p)
    assert isinstance(sim.float_model(3, ckpt=p).__dict__["sesrq_skip_quant_scale"], ValueError)
    frames = os.path.join(GOLDEN, "rand_DM_Input_80x960.npy")
    with pytest.raises(SystemExit, match="incomplete.*--float-skip"):
        load_test_py().main(["--mflag", "3", "--ckpt", p, "--frames", frames])
