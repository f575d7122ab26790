"""oracle/calib_oracle.py, the calibration pass's definition, against every calibration the reference recorded (CPU).

The reference ran its mode-0 graph in fp32 in oneDNN's order; the oracle forms the integer PE sums exactly and scales them once
(fp32-faithful form: what csrc/sesrq_calib.hip computes bit for bit, tests/test_calib_kernels.py) or evaluates the reference's
arithmetic in float64 (exact=True).  Bars as for the device pass (test_gpu_parity.py, test_calib_reference.py): running min / max
within 1e-4 of the span, zero points equal, scales within rtol 2e-4; the two forms within 1e-4 of the span of each other."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_fixture
from calib_cases import dataset_frames, finalize, frame_of
from helpers import PIXEL_SHUFFLE
from oracle import calib_oracle as CO

QAT = ("nrdm_3_qat", "sesr_x4_qat", "nrdm_3_qat_nat", "sesr_x4_qat_nat")
QB = os.path.join(GOLDEN, "quan_bits")


def _id(p):
    return os.path.basename(p)[:-len(".params.npz")]


RECORDS = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.params.npz")) if _id(p) not in QAT) + \
    sorted(p for p in glob.glob(os.path.join(QB, "*.params.npz")) if os.path.basename(p) != "sesr_x4.q3.params.npz")
# (record, domain) -> bar between the float64 and the fp32-faithful forms, in units of the span, where float64 resolves a tie of an
# upstream quantiser the other way: measured 2.9e-4, 4.6e-4 and 1.9e-3 of the span, all in the last domain; the fp32 form is the one
# that matches the reference's record there (within 2e-7 of the span, test_oracle_reproduces_the_reference_calibration)
EXACT_SLACK = {("sesr_x2_rand.params.npz", 5): 3e-4, ("nrdm_3.q6.params.npz", 5): 5e-4, ("sesr_x2_rand.q4.params.npz", 5): 2e-3}


def run(path, exact=False, frames=None):
    p, pm = load_fixture(path)
    b = pm.get("quan_bits", 8)
    frames = [frame_of(pm)] if frames is None else frames
    return CO.forward([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], PIXEL_SHUFFLE[pm["mflag"]], frames, b, exact=exact,
                      keep_outputs=False), pm, b


def assert_ranges(what, r, mins, maxs, check_last_min=False, bar=1e-4):
    for k in range(len(maxs)):
        span = maxs[k] - mins[k]
        if k < len(maxs) - 1 or check_last_min:
            assert abs(r.run_min[k] - mins[k]) <= bar * span, (what, k, r.run_min[k], mins[k])
        assert abs(r.run_max[k] - maxs[k]) <= bar * span, (what, k, r.run_max[k], maxs[k])


def test_records_are_all_covered():
    """Every calibration record is under one of the tests below: the range test, the QAT note or the sesr_x4.q3 finding."""
    every = {os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "*.params.npz")) + glob.glob(os.path.join(QB, "*.params.npz"))}
    covered = {os.path.basename(p) for p in RECORDS} | {f"{c}.params.npz" for c in QAT} | {"sesr_x4.q3.params.npz"}
    assert every == covered and len(RECORDS) == 19


@pytest.mark.parametrize("path", RECORDS, ids=_id)
def test_oracle_reproduces_the_reference_calibration(path):
    """fp32-faithful form: running ranges, zero points and scales of the reference's record (b = 8: random and natural frames;
    b = 2..7: the quan_bits cases)."""
    r, pm, b = run(path)
    assert_ranges(_id(path), r, pm["min"], pm["max"])
    scale, zero = finalize(r, b)
    assert zero == pm["zero"]
    np.testing.assert_allclose(scale, pm["scale"], rtol=2e-4)


@pytest.mark.parametrize("path", RECORDS, ids=_id)
def test_float64_and_fp32_forms_agree(path):
    r32, pm, _ = run(path)
    r64, _, _ = run(path, exact=True)
    for k in range(6):
        bar = EXACT_SLACK.get((os.path.basename(path), k), 1e-4)
        span = pm["max"][k] - pm["min"][k]
        assert abs(r64.run_max[k] - r32.run_max[k]) <= bar * span, (k, r64.run_max[k], r32.run_max[k])
        assert abs(r64.run_min[k] - r32.run_min[k]) <= bar * span, (k, r64.run_min[k], r32.run_min[k])


@pytest.mark.parametrize("case", QAT)
def test_qat_records_hold_the_graph_of_their_training(case):
    """The QAT records come from the reference's QAT-prepared model: models/quantize_utils_pt.prepare replaces the long skip's AddOp
    by a fake-quantised QuantAdd, which neither this pass nor the Calibrator models.  Upstream of it (domains 0 and 1) the ranges are
    the oracle's to the usual bar; from the residual sum (domain 4) on they are not, by design."""
    r, pm, _ = run(os.path.join(GOLDEN, f"{case}.params.npz"))
    for k in (0, 1):
        span = pm["max"][k] - pm["min"][k]
        assert abs(r.run_min[k] - pm["min"][k]) <= 1e-4 * span and abs(r.run_max[k] - pm["max"][k]) <= 1e-4 * span, k
    assert any(abs(r.run_max[k] - pm["max"][k]) > 1e-3 * (pm["max"][k] - pm["min"][k]) for k in (4, 5))


# ------------------------------------------------------------------------------------------------------------- dataset loops
@pytest.mark.parametrize("case", ["nrdm_3", "sesr_x4", "sesr_x2_rand"])
def test_oracle_reproduces_the_dataset_loops(case):
    """tests/golden/calib/<case>.npz: running ranges over frames a, b, c (every domain's min included), zero points, scales; both
    forms."""
    fx, meta = load_fixture(os.path.join(GOLDEN, "calib", f"{case}.npz"))
    frames = dataset_frames(case, meta["mflag"])
    for exact in (False, True):
        r, _, b = run(os.path.join(GOLDEN, f"{case}.params.npz"), exact=exact, frames=frames)
        assert_ranges(f"{case} exact={exact}", r, meta["min"], meta["max"], check_last_min=True)
        scale, zero = finalize(r, b)
        assert zero == meta["zero"]
        np.testing.assert_allclose(scale, meta["scale"], rtol=2e-4)


# ------------------------------------------------------------------------------------------------------------- domain
def test_domain_follows_the_host_pass_and_the_clamp():
    """calib_oracle.domain against the host pass's arithmetic written out (sesrq/calibrate.py observe), and the +-2^30 zero clamp."""
    from sesrq.calibrate import ZERO_LIMIT
    assert ZERO_LIMIT == CO.ZERO_CLAMP
    bias = np.array([0.3, -2.0, 1e4, -1e4, 0.0], np.float32)
    for mn, mx, b, sw in ((0.0, 2.0, 8, 0.01), (-0.3, 0.2, 3, 0.07), (0.7, 0.705, 8, 0.004), (1e6, 1e6 + 0.0625, 8, 0.01)):
        mn, mx = float(np.float32(mn)), float(np.float32(mx))          # the extrema of an fp32 tensor
        d = CO.domain(mn, mx, b, sw, bias)
        scale = (mx - mn) / ((1 << b) - 1)
        zero = min(max(-(1 << (b - 1)) - round(mn / scale), -(1 << 30)), 1 << 30)
        assert d.scale == scale and d.zero == zero
        f = np.float32
        assert d.ss == f(scale * sw) and d.acc_lo == f((-(1 << 17) - zero) * scale * sw) and d.add_hi == f(((1 << 19) - 1 - zero) * scale * sw)
        bq = np.clip(np.rint(bias / f(scale * sw)), -32768, 32767).astype(f)
        np.testing.assert_array_equal(d.qbias, bq * f(scale * sw))
    assert CO.domain(1e6, 1e6 + 0.0625, 8).zero == -(1 << 30)
    d = CO.domain(0.5, 0.5, 8, 0.1, bias)
    assert d.degenerate and d.zero == 0 and np.all(d.qbias == 0)


def test_minmax_skips_nan():
    x = np.array([np.nan, 1.0, -2.0, np.nan, np.inf], np.float32)
    assert CO.minmax(x) == (np.float32(-2.0), np.float32(np.inf))
    assert CO.minmax(np.array([np.nan], np.float32)) == (np.float32(np.inf), np.float32(-np.inf))


# ------------------------------------------------------------------------------------------------------------- sesr_x4.q3
def test_sesr_x4_q3_differs_by_one_tie_of_the_reference():
    """SESR-x4 at b = 3: the oracle (and the device pass, which equals it bit for bit) gives 8.6454 / 2.1507 for the maxima of domains
    4 / 5 where the reference recorded 9.4313 / 2.3463.  tests/golden/quan_bits/sesr_x4.q3.trace.npz (make_quan_bits_golden.py
    --trace) holds the reference's own run: its codes first differ from the oracle's at quantiser input 2, at pixels whose value sits
    on the rounding boundary between codes -1 and 0 (x = 3.5 x scale_2, within a few ulp on both sides); the reference's fp32
    summation order put domain 2's max 2 ulp higher, hence a slightly larger scale_2, and its copies of that value round up where the
    oracle's round down.  With those codes taken as the reference has them, the oracle reproduces every range of the record."""
    fx, meta = load_fixture(os.path.join(QB, "sesr_x4.q3.trace.npz"))
    path = os.path.join(QB, "sesr_x4.q3.params.npz")
    p, pm = load_fixture(path)
    Wf, bf, b, k = [p[f"Wf{i}"] for i in range(5)], [p[f"bf{i}"] for i in range(5)], 3, meta["layer"]
    frames = [frame_of(pm)]
    r = CO.forward(Wf, bf, 4, frames, b, keep_outputs=False, keep_inputs=True)
    assert k == 2 and abs(r.run_max[4] - 8.6454) < 1e-4 and abs(pm["max"][4] - 9.4313) < 1e-4
    assert abs(r.run_max[5] - 2.1507) < 1e-4 and abs(pm["max"][5] - 2.3463) < 1e-4
    for i in range(k):                                   # upstream of the tie the ranges agree to the bar ...
        assert abs(r.run_max[i] - pm["max"][i]) <= 1e-4 * (pm["max"][i] - pm["min"][i])
    d = r.domains[0][k]
    ulp = float(np.spacing(np.float32(pm["max"][k])))
    assert 0 < pm["max"][k] - r.run_max[k] <= 2 * ulp            # ... and domain 2's max is the reference's 2 ulp higher
    idx = tuple(fx["pos"].astype(np.int64).T)
    x = r.inputs[0][k][idx]
    np.testing.assert_array_equal(x, fx["oracle_x"])
    np.testing.assert_array_equal(CO.codes(x, d, b), fx["oracle_code"])
    assert np.all(np.abs(fx["ref_code"] - fx["oracle_code"]) == 1)
    t = (x / d.scale32).astype(np.float32) + d.zero32                # the pre-round value: on the boundary between two codes
    off = np.abs(t - (np.floor(t) + np.float32(0.5)))
    assert np.all(off <= 16 * np.spacing(np.abs(t))), off.max()
    assert np.all(np.abs(fx["ref_x"].view(np.int32) - x.view(np.int32)) <= 8)          # the same values, a few ulp apart
    assert len(set(x.tolist())) <= 8                                 # a handful of values, each repeated at many pixels
    fixed = CO.forward(Wf, bf, 4, frames, b, keep_outputs=False, override={k: (idx, fx["ref_code"].astype(np.int64))})
    assert_ranges("sesr_x4.q3 with the reference's codes", fixed, pm["min"], pm["max"], check_last_min=True)
    scale, zero = finalize(fixed, b)
    assert zero == pm["zero"]
    np.testing.assert_allclose(scale, pm["scale"], rtol=2e-4)
