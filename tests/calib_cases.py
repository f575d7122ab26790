"""Calibration cases shared by the calibration test modules -- TEST INFRASTRUCTURE (not collected): the frames the reference calibrated
on, the dataset frames a, b, c, test.py loaded as a module, the QAT records and their bars, and the seeded inputs of the calibration
kernels.  tests/test_calib_*.py and tests/test_qat_calib_*.py run these; none of them imports another."""
import importlib.util
import json
import os
import sys

import numpy as np

import image_oracle
import qat_calib_oracle as QO
from conftest import GOLDEN, ROOT, load_fixture
from helpers import calib_params, device, full_input, ref_inp
from oracle import calib_oracle as CO

F32 = np.float32
PKG = os.path.join(ROOT, "sesr-pytorch-quantize_amd")
NAT_SEED = {"sesr_x4_nat": 2024, "nrdm_3_nat": 2025, "sesr_x2_rand_nat": 2026, "sesr_x4_qat_nat": 2027,
            "nrdm_3_qat_nat": 2028}                                              # tests/golden/make_golden.py CASES


# ---------------------------------------------------------------------------------------------------------------------- frames
def frame_of(meta):
    """The frame the reference calibrated on: its random 80 x 960 input, or the natural frame of the case."""
    if meta["case"] in NAT_SEED:
        sys.path.insert(0, GOLDEN)
        from natural import natural_frame
        return natural_frame(1 if meta["mflag"] == 5 else 3, 80, 960, NAT_SEED[meta["case"]])
    return full_input(meta)


def load_test_py():
    spec = importlib.util.spec_from_file_location("sesrq_test_entry_calib", os.path.join(PKG, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def raw_dataset_frames():
    """Frames (a), (b), (c) of the raw fixture: (raw (H, W) uint16, gt (1, 3, H, W) uint16)."""
    F = np.load(os.path.join(GOLDEN, "raw", "frames.npz"), allow_pickle=False)
    sys.path.insert(0, GOLDEN)
    from make_raw_golden import natural_raw
    out = [(F["raw_a"], F["gt16_a"])]
    for f in ("b", "c"):
        raw, gt16 = natural_raw(f)
        out.append((raw, gt16[None]))
    return out


def image_frames(mflag):
    """Frames (a), (b), (c) of the image fixture: (LR (H, W, 3), HR (uH, uW, 3)) uint8 RGB."""
    F = np.load(os.path.join(GOLDEN, "image", "frames.npz"), allow_pickle=False)
    sys.path.insert(0, GOLDEN)
    from make_image_golden import natural_image
    return [(F["lr_a"], F[f"hr{mflag}_a"])] + [natural_image(f, mflag) for f in ("b", "c")]


def dataset_frames(case, mflag):
    """fp32 frames a, b, c of the reference's dataset loop (tests/golden/make_calib_golden.py), decoded on the CPU."""
    if case == "nrdm_3":
        return [ref_inp(f) for f in ("a", "b", "c")]
    return [image_oracle.decode(lr, "y" if mflag == 5 else "rgb") for lr, _ in image_frames(mflag)]


def finalize(r, b):
    """test.py:185-217: the output domain's min := 0."""
    from oracle.sesrq_oracle import calib_scale_zero
    sz = [calib_scale_zero(0.0 if k == len(r.run_min) - 1 else r.run_min[k], r.run_max[k], b) for k in range(len(r.run_min))]
    return [s for s, _ in sz], [z for _, z in sz]


def calibrators(case, quan_bits=8):
    """Two Calibrators of a golden net on the device (one per pass under comparison) and the net's mflag."""
    from sesrq.calibrate import Calibrator
    Wf, bf, ps = calib_params(case)
    mflag = load_fixture(os.path.join(GOLDEN, f"{case}.params.npz"))[1]["mflag"]
    mk = lambda: Calibrator(Wf, bf, ps, device(), quan_bits=quan_bits)
    return mk(), mk(), mflag


# ---------------------------------------------------------------------------------------------------------------------- QAT records
ADD = json.load(open(os.path.join(GOLDEN, "calib", "qat_add.json")))
ONE_FRAME = ("nrdm_3_qat", "sesr_x4_qat", "nrdm_3_qat_nat", "sesr_x4_qat_nat")
LOOPS = {"nrdm_3_qat": "nrdm_3", "sesr_x4_qat": "sesr_x4"}           # record -> the plain case whose dataset frames a, b, c it ran on
BAR, SCALE_RTOL = 1e-4, 2e-4

# (record, domain) -> deviation of the fp32-faithful form from the reference's record, in units of the span, where it misses the
# bar (measured; the test allows twice that and never more than 1e-3).  One cause, upstream of the QuantAdd -- the plain oracle has
# it too -- and pinned in test_sesr_x4_qat_deviates_by_one_upstream_tie: 42 pixels of quantiser input 1 hold 0.13814925 (two adjacent floats), which sits
# exactly on the rounding boundary between codes -86 and -85 with the oracle's scale_1; the reference's fp32 summation order put
# domain 1's max 3 ulp lower, hence a smaller scale_1, and its copies of that value round the other way.  Domain 2's max moves by
# five weight codes (1.21e-4 of its span), domain 3's by 6.9e-5 (inside the bar), domain 4 is exact (the QuantAdd's grid), and
# domain 5 inherits 2.1e-4 (min) / 4.1e-4 (max).  nrdm_3_qat, both natural-frame records and both loops need none (at most 3e-7).
MEASURED = {("sesr_x4_qat", 2): 1.210e-4, ("sesr_x4_qat", 5): 4.106e-4}


def bar_of(record, k):
    m = MEASURED.get((record, k))
    if m is None:
        return BAR
    assert BAR < 2 * m <= 1e-3
    return 2 * m


def scale_of(record):
    return QO.skip_scale(*[ADD[record.replace("_nat", "")][k] for k in QO.OBSERVERS])


def assert_record(record, r, rec):
    """Running min and max of all six domains, the zero points and the scales of a record."""
    scale, zero = finalize(r, 8)
    for k in range(6):
        span, bar = rec["max"][k] - rec["min"][k], bar_of(record, k)
        dmin, dmax = abs(r.run_min[k] - rec["min"][k]) / span, abs(r.run_max[k] - rec["max"][k]) / span
        print(f"{record} domain {k}: min off {dmin:.3e}, max off {dmax:.3e} of the span (bar {bar:.1e}); zero {zero[k]} / "
              f"{rec['zero'][k]}; scale off {abs(scale[k] / rec['scale'][k] - 1):.3e}")
        assert dmin <= bar and dmax <= bar, (record, k, r.run_min[k], rec["min"][k], r.run_max[k], rec["max"][k])
        # scale_k = (max_k - min_k) / 255 (min_5 := 0): an excepted domain's scale moves by what its ends may move
        used = rec["max"][k] - (0.0 if k == 5 else rec["min"][k])
        rtol = SCALE_RTOL if bar == BAR else max(SCALE_RTOL, (1 if k == 5 else 2) * bar * span / used)
        assert abs(scale[k] - rec["scale"][k]) <= rtol * abs(rec["scale"][k]), (record, k, scale[k], rec["scale"][k])
    assert zero == rec["zero"], (record, zero, rec["zero"])       # no zero point differs: no tie to account for


# ---------------------------------------------------------------------------------------------------------------------- kernel inputs
def zero_domain(kind, b, span=1.5):
    """(mn, mx) whose zero point is of the kind: 'low' = -2^(b-1), 'below' far below it, 'far' (min / span = 200) further still,
    'positive', or a float min / span."""
    if kind == "low":
        return 0.0, span
    if kind == "below":
        return 2.0 * span, 3.0 * span
    if kind == "far":
        return 200.0 * span, 201.0 * span
    if kind == "positive":
        return -0.9 * span, 0.1 * span
    r = float(kind) * (1.0 if b == 8 else 255.0 / 7.0)
    mn = F32(0.7)
    return float(mn), float(F32(mn * (1.0 + 1.0 / r)))


def frame(rng, shape, d: CO.Domain, b):
    """fp32 values of the domain: uniform inside it, on the quantiser's ties and one ulp either side, beyond both clamps."""
    n = int(np.prod(shape))
    span = d.mx - d.mn
    x = (d.mn + rng.random(n) * span).astype(F32)
    k = np.arange(-(1 << (b - 1)) - 1, (1 << (b - 1)) + 1, dtype=np.float64)
    ties = ((k + 0.5 - float(d.zero32)) * float(d.scale32)).astype(F32)
    row = np.concatenate([ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf)),
                          np.array([d.mn - span, d.mx + span, d.mn, d.mx], F32)])
    pos = rng.permutation(n)[:min(n, row.size)]
    x[pos] = row[rng.permutation(row.size)[:pos.size]]
    return x.reshape(shape)


def weights(rng, oc, ic, K, b, sat=False):
    lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
    if sat:                        # one sign per output channel: the PE sums run to the accumulator's bounds
        s = np.where(np.arange(oc) % 2 == 0, hi, lo)[:, None, None, None]
        return np.broadcast_to(s, (oc, ic, K, K)).astype(np.int32).copy()
    return rng.integers(lo, hi + 1, size=(oc, ic, K, K)).astype(np.int32)


def bias(rng, oc, ss, big=False):
    b = (rng.standard_normal(oc) * 200.0 * float(ss)).astype(F32)
    if big:                        # beyond the 16-bit bias code on both sides
        b[::2] = F32(50000.0 * float(ss))
        b[1::2] = F32(-50000.0 * float(ss))
    return b


def slot_bytes(d: CO.Domain, batches=1):
    from sesrq import _lib
    s = _lib.CalibSlot()
    s.ord[0], s.ord[1] = 0xffffffff, 0
    s.min = s.run_min = d.mn
    s.max = s.run_max = d.mx
    s.scale, s.zero, s.degenerate, s.batches = d.scale, d.zero, int(d.degenerate), batches
    s.scale32, s.zero32, s.ss = float(d.scale32), float(d.zero32), float(d.ss)
    s.acc_lo, s.acc_hi, s.add_lo, s.add_hi = float(d.acc_lo), float(d.acc_hi), float(d.add_lo), float(d.add_hi)
    for i, v in enumerate(d.qbias):
        s.qbias[i] = float(v)
    import torch
    return torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).to(device())
