"""The calibration pass kernels (csrc/sesrq_calib.hip) bit for bit against their definition, oracle/calib_oracle.py.

calib_conv_kernel (both instances, through sesrq_calib_conv_q and sesrq_calib_conv_slot) on ragged shapes around the 32 x 8 tile and
its halo, empty and partial PEs, every width, inputs on quantiser ties and beyond both clamps, clamps of the PE accumulator, the adder
and the bias that fire, zero points at -2^(b-1), far below it, positive, and offset domains (min / span up to 1e5) whose codes need
more than 16 bits and whose PE sums need more than 32; sesrq_calib_minmax and sesrq_calib_observe_slot against numpy and
calib_oracle.domain; the whole pass (Calibrator.observe and enqueue) against calib_oracle.forward, and a near-flat frame end to end."""
import ctypes as C
import zlib

import numpy as np
import pytest

from calib_cases import F32, bias, frame, slot_bytes, weights, zero_domain
from helpers import calib_params, device, pass_equals, same, stream_ptr, to_device
from oracle import calib_oracle as CO

NETS = ("nrdm_3", "sesr_x4", "sesr_x2_rand")
SHAPES = [(1, 1), (1, 33), (8, 32), (9, 33), (37, 70), (80, 960)]
OFFSETS = (100, 127, 129, 1e3, 1e5)               # min / span at b = 8; at b = 3 the same zero points: x 255 / 7


# ---------------------------------------------------------------------------------------------------------------------- inputs
# ---------------------------------------------------------------------------------------------------------------------- launchers


def run_conv(entry, x, wq, d: CO.Domain, b, relu, skip):
    """sesrq_calib_conv_q ('q', the domain in the descriptor) or sesrq_calib_conv_slot ('slot', the domain in a device slot)."""
    import torch
    from sesrq import _lib
    lib = _lib.lib()
    N, ic, H, W = x.shape
    oc, _, K, _ = wq.shape
    xt, wt, qb = to_device(x), to_device(wq), to_device(d.qbias.astype(F32))
    st = to_device(skip) if skip is not None else None
    out = torch.full((N, oc, H, W), float("nan"), dtype=torch.float32, device=device())
    desc = _lib.CalibConvDesc(k=K, ic=ic, oc=oc, w=wt.data_ptr(), qbias=qb.data_ptr(), in_scale=float(d.scale32), in_zero=d.zero,
                              ss=float(d.ss), acc_lo=float(d.acc_lo), acc_hi=float(d.acc_hi), add_lo=float(d.add_lo),
                              add_hi=float(d.add_hi), relu=int(relu))
    sp = st.data_ptr() if st is not None else None
    if entry == "q":
        _lib.check(lib.sesrq_calib_conv_q(C.byref(desc), xt.data_ptr(), sp, out.data_ptr(), N, H, W, b, stream_ptr()))
    else:
        desc.qbias, desc.in_scale, desc.in_zero = None, 0.0, 0          # the slot's are used
        slot = slot_bytes(d)
        _lib.check(lib.sesrq_calib_conv_slot(C.byref(desc), slot.data_ptr(), xt.data_ptr(), sp, out.data_ptr(), N, H, W, b, stream_ptr()))
    torch.cuda.synchronize()
    return out


def conv_cases():
    """(id, K, ic, oc, N, (H, W), relu, skip, b, zero kind, saturating weights and bias)."""
    ics, ocs, kinds = (1, 2, 3, 4, 5, 16), (1, 3, 16), ("low", "below", "positive")
    out = []
    i = 0
    for K in (3, 5):
        for hw in SHAPES:
            ic, oc = ics[i % 6], ocs[i % 3]
            if hw == (80, 960):
                ic, oc = 16, 16
            c = (K, ic, oc, 1 + i % 2, hw, i % 2 == 0, (i // 2) % 2 == 0, (2, 3, 8)[i % 3], kinds[(i // 3) % 3], False)
            out.append(c)
            i += 1
    for b in range(2, 9):                                         # every width on one shape
        out.append((3, 5, 3, 2, (9, 33), True, b % 2 == 0, b, ("low", "below", "positive")[b % 3], False))
    for b in (8, 3):
        for r in OFFSETS:                                         # offset domains: codes beyond 16 bits, PE sums beyond 32
            out.append((5, 16, 16, 1, (9, 33), True, r == 129, b, r, False))
        for kind in (("low", "positive") if b == 8 else ("far",)):   # the PE, adder and bias clamps fire (at b = 3 only with
            out.append((3, 16, 16, 2, (9, 33), False, False, b, kind, True))     # codes of more than 8 bits)
    return out


def _cid(c):
    K, ic, oc, N, (H, W), relu, skip, b, kind, sat = c
    return f"k{K}-ic{ic}-oc{oc}-n{N}-{H}x{W}-{'relu' if relu else 'lin'}{'-skip' if skip else ''}-b{b}-z{kind}{'-sat' if sat else ''}"


CONV_CASES = conv_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["q", "slot"])
def test_calib_conv_bit_exact_with_the_oracle(entry):
    """Both calib_conv_kernel instances, through both entry points, equal calib_oracle.conv on every case; the saturating cases fire
    the 18-bit PE clamp, the 20-bit adder clamp and the 16-bit bias clamp (asserted in the oracle)."""
    for n, c in enumerate(CONV_CASES):
        K, ic, oc, N, (H, W), relu, skip, b, kind, sat = c
        rng = np.random.default_rng(1000 + n)
        mn, mx = zero_domain(kind, b)
        sw = 0.0113
        d0 = CO.domain(mn, mx, b, sw, np.zeros(oc, F32))
        d = CO.domain(mn, mx, b, sw, bias(rng, oc, d0.ss, big=sat))
        if sat:
            x = np.full((N, ic, H, W), d.mx, F32)               # every code at the top: all PE sums at their bounds
            x[..., ::3, ::2] = d.mn
        else:
            x = frame(rng, (N, ic, H, W), d, b)
        wq = weights(rng, oc, ic, K, b, sat)
        sk = (rng.standard_normal((N, oc, H, W)) * 3.0).astype(F32) if skip else None
        fired = CO.Fired()
        want = CO.conv(x, wq, d, b, relu, sk, fired=fired)
        if sat:
            assert fired.pe and fired.add and fired.bias, (_cid(c), fired)
        if not isinstance(kind, str):                              # offset domains: from min / span 129 on, codes beyond 16 bits
            q = CO.codes(x, d, b) - d.zero
            assert (np.abs(q).max() > 32767) == (kind >= 129), (_cid(c), np.abs(q).max())
        same(f"{entry} {_cid(c)}", run_conv(entry, x, wq, d, b, relu, sk), want, values=True, cast=F32)


# ---------------------------------------------------------------------------------------------------------------------- minmax
def _minmax(x):
    import torch
    from sesrq import _lib
    xt = to_device(x)
    mm = torch.empty(2, dtype=torch.float32, device=device())
    scratch = torch.empty(2, dtype=torch.int32, device=device())
    _lib.check(_lib.lib().sesrq_calib_minmax(xt.data_ptr(), xt.numel(), mm.data_ptr(), scratch.data_ptr(), stream_ptr()))
    return mm.cpu().numpy()


@pytest.mark.gpu
def test_calib_minmax_equals_numpy():
    """n not a multiple of 256 and above 2048 x 256 (the grid-stride loop), +-0, +-inf, denormals, all-negative input: equal to
    numpy's min / max.  NaN is skipped (calib_oracle.minmax; torch.max would propagate it)."""
    rng = np.random.default_rng(7)
    for n in (1, 255, 257, 1000, 2048 * 256 + 777, 3 * 2048 * 256 + 5):
        x = (rng.standard_normal(n) * 3.0).astype(F32)
        got = _minmax(x)
        assert got[0] == x.min() and got[1] == x.max(), (n, got, x.min(), x.max())
        neg = -np.abs(x) - F32(1.0)                                  # all negative
        got = _minmax(neg)
        assert got[0] == neg.min() and got[1] == neg.max(), n
    tiny = np.array([1e-45, 3e-39, -2e-40, 1e-44], F32)              # denormals only
    got = _minmax(tiny)
    assert got[0] == tiny.min() and got[1] == tiny.max(), got
    z = np.array([0.0, -0.0, 0.0], F32)
    got = _minmax(z)
    assert got[0] == 0.0 and got[1] == 0.0
    inf = np.concatenate([x[:1000], np.array([np.inf, -np.inf], F32)])
    got = _minmax(inf)
    assert got[0] == -np.inf and got[1] == np.inf
    nan = x[:5000].copy()
    nan[::7] = np.nan
    got = _minmax(nan)
    want = CO.minmax(nan)
    assert got[0] == want[0] and got[1] == want[1] and not np.isnan(got).any(), (got, want)
    assert want[0] == np.nanmin(nan) and want[1] == np.nanmax(nan)


# ---------------------------------------------------------------------------------------------------------------------- observe_slot
def _read_slot(t):
    from sesrq import _lib
    return _lib.CalibSlot.from_buffer_copy(bytes(t.cpu().numpy().tobytes()))


def _slot_equals_domain(what, s, d: CO.Domain, oc):
    assert s.scale == d.scale and s.zero == d.zero, (what, s.scale, d.scale, s.zero, d.zero)
    for f in ("scale32", "zero32", "ss", "acc_lo", "acc_hi", "add_lo", "add_hi"):
        assert F32(getattr(s, f)) == F32(getattr(d, f)), (what, f, getattr(s, f), getattr(d, f))
    assert np.array_equal(np.array(s.qbias[:oc], F32), d.qbias), what


@pytest.mark.gpu
@pytest.mark.parametrize("b", [2, 3, 8])
def test_observe_slot_equals_the_domain(b):
    """sesrq_calib_observe_slot over several batches on one slot: the batch's extrema, the running fold, every domain field equal to
    calib_oracle.domain (zero points low, far below, positive, offset up to the +-2^30 clamp; the bias clamp), the keys reset between
    batches, and the degenerate flag raised by a constant batch and kept."""
    import torch
    from sesrq import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(70 + b)
    oc, sw = 16, 0.0071
    bt = (rng.standard_normal(oc) * 2.0).astype(F32)
    bt[0] = F32(1e4)                                             # beyond the 16-bit code at every domain here
    btd = to_device(bt)
    desc = _lib.CalibDomainDesc(quan_bits=b, oc=oc, bias=btd.data_ptr(), sw=sw, acc_bits=18, add_bits=20, bias_bits=16)
    init = _lib.CalibSlot()
    _lib.check(lib.sesrq_calib_slots_init(C.byref(init), 1))
    slot = torch.frombuffer(bytearray(bytes(init)), dtype=torch.uint8).to(device())
    run_mn, run_mx = None, None
    batches = [("low", 1.0), ("positive", 2.0), ("below", 0.5), (129, 1.0), (1e5, 1.0), ("huge", 1.0), ("low", 7.0)]
    for i, (kind, span) in enumerate(batches):
        if kind == "huge":                                      # zero beyond 2^30: clamped
            mn, mx = 1.0e6, float(np.nextafter(F32(1.0e6), F32(np.inf)))
        else:
            mn, mx = zero_domain(kind, b, span)
        x = (mn + rng.random(3 * 256 + 11) * (mx - mn)).astype(F32)
        x[:2] = (F32(mn), F32(mx))
        _lib.check(lib.sesrq_calib_observe_slot(to_device(x).data_ptr(), x.size, slot.data_ptr(), C.byref(desc), stream_ptr()))
        s = _read_slot(slot)
        bmn, bmx = CO.minmax(x)
        assert (s.min, s.max) == (bmn, bmx), (i, s.min, s.max)
        run_mn = bmn if run_mn is None or run_mn > bmn else run_mn
        run_mx = bmx if run_mx is None or run_mx < bmx else run_mx
        assert (s.run_min, s.run_max, s.batches) == (run_mn, run_mx, i + 1), i
        assert (s.ord[0], s.ord[1]) == (0xffffffff, 0), i                  # the keys are back at their initial value
        d = CO.domain(bmn, bmx, b, sw, bt)
        if kind == "huge" and b == 8:                           # min / span = 2^24 x 255: the clamp (out of reach at b <= 6)
            assert abs(d.zero) == CO.ZERO_CLAMP
        assert d.bias_raw[0] > 32767
        _slot_equals_domain((b, i, kind), s, d, oc)
        assert not s.degenerate
    x = np.full(300, 0.25, F32)                                 # constant: degenerate, and it stays raised
    _lib.check(lib.sesrq_calib_observe_slot(to_device(x).data_ptr(), x.size, slot.data_ptr(), C.byref(desc), stream_ptr()))
    s = _read_slot(slot)
    assert s.degenerate and s.scale == 0.0 and s.zero == 0 and s.batches == len(batches) + 1
    x = (rng.random(300)).astype(F32)
    _lib.check(lib.sesrq_calib_observe_slot(to_device(x).data_ptr(), x.size, slot.data_ptr(), C.byref(desc), stream_ptr()))
    s = _read_slot(slot)
    assert s.degenerate
    _slot_equals_domain((b, "after"), s, CO.domain(*CO.minmax(x), b, sw, bt), oc)


# ---------------------------------------------------------------------------------------------------------------------- whole pass
@pytest.mark.gpu
@pytest.mark.parametrize("b", [8, 3])
@pytest.mark.parametrize("case", NETS)
def test_whole_pass_equals_the_oracle(case, b):
    """Calibrator.observe and Calibrator.enqueue over two batches of N = 2, 37 x 70 random frames: running extrema, the last batch's
    (scale, zero) and each batch's returned output equal calib_oracle.forward."""
    import torch
    from sesrq.calibrate import Calibrator
    Wf, bf, ps = calib_params(case)
    cin = Wf[0].shape[1]
    rng = np.random.default_rng(zlib.crc32(f"{case}.{b}".encode()))
    frames = [rng.random((2, cin, 37, 70)).astype(F32), (rng.random((2, cin, 37, 70)) * 1.3 - 0.1).astype(F32)]
    want = CO.forward(Wf, bf, ps, frames, b)
    host = Calibrator(Wf, bf, ps, device(), quan_bits=b)
    dev = Calibrator(Wf, bf, ps, device(), quan_bits=b)
    for i, x in enumerate(frames):
        same(f"{case} b={b} observe {i}", host.observe(to_device(x)), want.outputs[i], values=True, cast=F32)
        y = dev.enqueue(to_device(x))
        torch.cuda.synchronize()
        same(f"{case} b={b} enqueue {i}", y, want.outputs[i], values=True, cast=F32)
    dev.sync()
    pass_equals(f"{case} b={b} observe", host, want)
    pass_equals(f"{case} b={b} enqueue", dev, want)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nrdm_3", "sesr_x4"])
def test_near_flat_frame_end_to_end(case):
    """A frame in [0.700, 0.705]: zero_0 near -35800 at b = 8 (codes far beyond 16 bits).  The device ranges equal the oracle's and
    cal.bundle() equals the bundle derived from the oracle's ranges."""
    import torch
    from sesrq.bundle import calib_scale_zero, derive_bundle_from_quantized
    from sesrq.calibrate import Calibrator
    Wf, bf, ps = calib_params(case)
    cin = Wf[0].shape[1]
    rng = np.random.default_rng(5)
    x = (F32(0.700) + rng.random((1, cin, 40, 96)) * F32(0.005)).astype(F32)
    x[0, 0, 0, 0], x[0, 0, 0, 1] = F32(0.700), F32(0.705)
    want = CO.forward(Wf, bf, ps, [x], 8)
    assert want.last_zero[0] < -35000
    for form in ("observe", "enqueue"):
        cal = Calibrator(Wf, bf, ps, device(), quan_bits=8)
        y = cal.observe(to_device(x)) if form == "observe" else cal.enqueue(to_device(x))
        torch.cuda.synchronize()
        same(f"{case} {form}", y, want.outputs[0], values=True, cast=F32)
        got = cal.bundle()
        pass_equals(f"{case} {form}", cal, want)
        sz = [calib_scale_zero(0.0 if k == 5 else want.run_min[k], want.run_max[k], 8) for k in range(6)]
        qw = CO.quantize(Wf, 8)
        ref = derive_bundle_from_quantized([w for w, _ in qw], [s for _, s in qw], bf, [s for s, _ in sz], [z for _, z in sz], ps)
        assert got.scale == ref.scale and got.zero == ref.zero
        for k in range(5):
            for f in ("wq", "add_const", "M", "n"):
                np.testing.assert_array_equal(getattr(got.layers[k], f), getattr(ref.layers[k], f), err_msg=f"{case} {form} {k} {f}")


@pytest.mark.gpu
def test_zero_clamp_agrees_on_host_and_device():
    """A frame one ulp wide at 1e6: min / span = 2^24 x 255, beyond the +-2^30 zero clamp.  observe (host-derived domains) and
    enqueue (device-derived) clamp alike and equal calib_oracle.forward."""
    import torch
    from sesrq.calibrate import Calibrator
    Wf, bf, ps = calib_params("nrdm_3")
    rng = np.random.default_rng(11)
    x = np.where(rng.random((1, 3, 9, 40)) < 0.5, F32(1.0e6), np.nextafter(F32(1.0e6), F32(np.inf))).astype(F32)
    want = CO.forward(Wf, bf, ps, [x], 8)
    assert want.last_zero[0] == -CO.ZERO_CLAMP
    for form in ("observe", "enqueue"):
        cal = Calibrator(Wf, bf, ps, device(), quan_bits=8)
        y = cal.observe(to_device(x)) if form == "observe" else cal.enqueue(to_device(x))
        torch.cuda.synchronize()
        cal.sync()
        same(f"clamp {form}", y, want.outputs[0], values=True, cast=F32)
        pass_equals(f"clamp {form}", cal, want)
