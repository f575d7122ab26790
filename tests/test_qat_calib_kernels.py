"""The quantised long-skip merge of the calibration pass (csrc/sesrq_calib.hip calib_conv_qadd_kernel, sesrq_calib_conv_qadd /
_slot_qadd, Calibrator(skip_quant_scale=...), test.py) bit for bit against its definition, tests/qat_calib_oracle.py, and -- to the
bars of tests/test_qat_calib_oracle.py -- against the calibrations the reference recorded for its QAT checkpoints.

Shapes are ragged against the 32 x 8 tile (9 x 35, 17 x 33, one and two frames); the QuantAdd's scale is chosen so that both of its
clamps fire and its inputs sit on the rounding ties (k + 1/2) s."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

import qat_calib_oracle as QO
import calib_cases as K
from conftest import GOLDEN, load_fixture
from helpers import PIXEL_SHUFFLE, calib_params, device, pass_equals, same, stream_ptr, to_device
from oracle import calib_oracle as CO

F32 = np.float32
NETS = {"nrdm_3": 3, "sesr_x4": 5, "sesr_x2_rand": 6}       # 3-channel ps 1; 1-channel ps 4; 3-channel ps 2
HIT = set()


def _track(before):
    from sesrq import _lib
    HIT.update(k for k, v in _lib.qadd_instances().items() if v > before.get(k, 0))


# ---------------------------------------------------------------------------------------------------------------------- one conv
def run_qadd(entry, x, wq, d, b, relu, skip, s):
    """sesrq_calib_conv_qadd ('q') or sesrq_calib_conv_slot_qadd ('slot')."""
    import torch
    from sesrq import _lib
    lib = _lib.lib()
    N, ic, H, W = x.shape
    oc, _, k, _ = wq.shape
    xt, wt, qb, st = to_device(x), to_device(wq), to_device(d.qbias.astype(F32)), to_device(skip)
    out = torch.full((N, oc, H, W), float("nan"), dtype=torch.float32, device=device())
    desc = _lib.CalibConvDesc(k=k, ic=ic, oc=oc, w=wt.data_ptr(), qbias=qb.data_ptr(), in_scale=float(d.scale32), in_zero=d.zero,
                              ss=float(d.ss), acc_lo=float(d.acc_lo), acc_hi=float(d.acc_hi), add_lo=float(d.add_lo),
                              add_hi=float(d.add_hi), relu=int(relu))
    before = _lib.qadd_instances()
    if entry == "q":
        _lib.check(lib.sesrq_calib_conv_qadd(C.byref(desc), xt.data_ptr(), st.data_ptr(), out.data_ptr(), N, H, W, b, float(s), stream_ptr()))
    else:
        desc.qbias, desc.in_scale, desc.in_zero = None, 0.0, 0
        slot = K.slot_bytes(d)
        _lib.check(lib.sesrq_calib_conv_slot_qadd(C.byref(desc), slot.data_ptr(), xt.data_ptr(), st.data_ptr(), out.data_ptr(), N, H, W,
                                                  b, float(s), stream_ptr()))
    torch.cuda.synchronize()
    _track(before)
    return out


def skip_tensor(rng, shape, s):
    """fp32 values around the QuantAdd's grid: uniform inside it, on every tie (k + 1/2) s and one ulp either side, beyond both clamps."""
    n = int(np.prod(shape))
    x = ((rng.random(n) * 300.0 - 150.0) * float(s)).astype(F32)
    k = np.arange(-130, 131, dtype=np.float64)
    ties = ((k + 0.5) * float(s)).astype(F32)
    row = np.concatenate([ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf)),
                          np.array([-200.0 * s, 200.0 * s, 0.0, -0.0, -128.0 * s, 127.0 * s, 127.5 * s, -128.5 * s], F32)])
    pos = rng.permutation(n)[:min(n, row.size)]
    x[pos] = row[rng.permutation(row.size)[:pos.size]]
    return x.reshape(shape)


# (K, ic, oc, N, (H, W), relu, b, zero kind): the merging conv of the nets is 3 x 3, 16 -> 16, ReLU; the others keep the kernel honest
QADD_CASES = [(3, 16, 16, 1, (9, 35), True, 8, "low"), (3, 16, 16, 2, (17, 33), True, 4, "below"), (3, 16, 16, 1, (9, 35), True, 2, "low"),
              (5, 3, 5, 2, (17, 33), False, 8, "positive"), (5, 1, 16, 1, (9, 35), True, 4, "low"), (3, 5, 3, 2, (17, 33), False, 2, "positive"),
              (3, 16, 16, 1, (1, 1), True, 8, "low"), (5, 16, 16, 1, (8, 32), True, 8, "low")]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["q", "slot"])
def test_qadd_conv_bit_exact_with_the_oracle(entry):
    """Both calib_conv_qadd_kernel instances through both entry points: the conv output after the quantised merge equals
    merge(calib_oracle.conv(skip=None), skip) on every case; the scale is a power of two in half of them (exact ties in t / s) and
    an odd float in the others; both clamps fire on both operands and ties occur."""
    for n, (k, ic, oc, N, (H, W), relu, b, kind) in enumerate(QADD_CASES):
        rng = np.random.default_rng(4000 + n)
        mn, mx = K.zero_domain(kind, b)
        d0 = CO.domain(mn, mx, b, 0.0113, np.zeros(oc, F32))
        d = CO.domain(mn, mx, b, 0.0113, K.bias(rng, oc, d0.ss))
        x = K.frame(rng, (N, ic, H, W), d, b)
        wq = K.weights(rng, oc, ic, k, b)
        v = CO.conv(x, wq, d, b, relu, None)
        top = float(np.abs(v).max())
        s = F32(2.0 ** np.floor(np.log2(top / 150.0))) if n % 2 == 0 else F32(top / 150.0)     # |v| reaches beyond 128 s
        skip = skip_tensor(rng, v.shape, s)
        u = (skip / s).astype(F32)
        if H * W * N * oc > 1000:
            assert np.any(np.abs(v) > F32(128.5) * s) and np.any(u > 128) and np.any(u < -129), "the clamps must fire"
            assert np.any(np.abs(u) - np.floor(np.abs(u)) == F32(0.5)), "ties must occur"
        want = QO.merge(v, skip, s)
        what = f"{entry} k{k}-ic{ic}-oc{oc}-n{N}-{H}x{W}-b{b}-z{kind}-s{float(s)!r}"
        same(what, run_qadd(entry, x, wq, d, b, relu, skip, s), want, values=True, cast=np.float32)


# ---------------------------------------------------------------------------------------------------------------------- whole pass
def _frames(rng, cin, dataset=False):
    """A 1 x C x 9 x 35 and a 2 x C x 17 x 33 batch of noise.  dataset: crops of the raw dataset frames a, b, c instead -- noise leaves
    the 2-bit nrdm_3's last output constant (with the float add as well), which the pass refuses as the reference does."""
    if dataset:
        a, b, c = K.dataset_frames("nrdm_3", 3)
        return [np.ascontiguousarray(a[:, :, :9, :35]), np.ascontiguousarray(np.concatenate([b[:, :, :17, :33], c[:, :, :17, :33]]))]
    return [rng.random((1, cin, 9, 35)).astype(F32), (rng.random((2, cin, 17, 33)) * 1.3 - 0.1).astype(F32)]


def _scale_for(Wf, bf, ps, frames, b):
    """A scale at which the shortcut reaches beyond the QuantAdd's clamp in every batch: its smallest per-batch max / 150."""
    plain = CO.forward(Wf, bf, ps, frames, b, keep_outputs=False, keep_inputs=True)
    a0 = min(float(bi[1].max()) for bi in plain.inputs)                 # a_0 (quantiser input 1) of the batch that reaches least far
    return F32(a0 / 150.0)


def _same_bundle(what, got, ref):
    assert got.scale == ref.scale and got.zero == ref.zero, what
    for k in range(len(ref.layers)):
        for f in ("wq", "add_const", "M", "n"):
            np.testing.assert_array_equal(getattr(got.layers[k], f), getattr(ref.layers[k], f), err_msg=f"{what} {k} {f}")


def _domains_equal(what, cal, doms):
    """The last batch's per-quantiser domain (scale, zero) as the oracle derives it."""
    assert cal.last_scale == [d.scale for d in doms] and cal.last_zero == [d.zero for d in doms], what


@pytest.mark.gpu
@pytest.mark.parametrize("b", [8, 4, 2])
@pytest.mark.parametrize("case", sorted(NETS))
def test_whole_pass_with_the_quantised_merge_equals_the_oracle(case, b):
    """Calibrator.observe (host pass) and .enqueue (device pass) with skip_quant_scale set, over a 1 x C x 9 x 35 and a 2 x C x 17 x 33
    batch: every batch's mode-0 output, the per-batch domains, the running extrema and the bundle equal the oracle's; the two passes
    give the same bundle."""
    import torch
    from sesrq.calibrate import Calibrator
    Wf, bf, ps = calib_params(case)
    cin = Wf[0].shape[1]
    rng = np.random.default_rng(zlib.crc32(f"qat.{case}.{b}".encode()))
    frames = _frames(rng, cin, dataset=(case, b) == ("nrdm_3", 2))
    s = _scale_for(Wf, bf, ps, frames, b)
    want = QO.forward(Wf, bf, ps, frames, b, s, keep_inputs=True)
    assert not any(d.degenerate for bd in want.domains for d in bd)
    for bi in want.inputs:          # the merge's upper clamp fires on the shortcut (behind ReLUs the lower one cannot: the conv test has it)
        assert float(bi[1].max()) > 128.5 * float(s)
    assert float(F32(127.0) * s) <= want.run_max[4] <= float(F32(F32(127.0) * s) + F32(F32(127.0) * s))
    host = Calibrator(Wf, bf, ps, device(), quan_bits=b, skip_quant_scale=float(s))
    dev = Calibrator(Wf, bf, ps, device(), quan_bits=b, skip_quant_scale=float(s))
    from sesrq import _lib
    before = _lib.qadd_instances()
    for i, x in enumerate(frames):
        same(f"{case} b={b} observe {i}", host.observe(to_device(x)), want.outputs[i], values=True, cast=np.float32)
        _domains_equal(f"{case} b={b} observe {i}", host, want.domains[i])
        y = dev.enqueue(to_device(x))
        dev.sync()
        same(f"{case} b={b} enqueue {i}", y, want.outputs[i], values=True, cast=np.float32)
        _domains_equal(f"{case} b={b} enqueue {i}", dev, want.domains[i])
    _track(before)
    pass_equals(f"{case} b={b} observe", host, want)
    pass_equals(f"{case} b={b} enqueue", dev, want)
    _same_bundle(f"{case} b={b}", dev.bundle(), host.bundle())
    plain = CO.forward(Wf, bf, ps, frames, b, keep_outputs=False)
    assert plain.run_max[4] != want.run_max[4]                  # and it is not the float add


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nrdm_3", "sesr_x4", "sesr_x2_rand"])
def test_four_entry_points_agree(case):
    """observe, enqueue and -- on the frame they decode -- enqueue_raw (3-channel nrdm_3) / enqueue_image (SESR) with skip_quant_scale
    set: the same output, ranges and bundle, bit for bit, and those of the oracle on the decoded frame; the entropy method runs on the
    host pass with it."""
    import torch
    from sesrq.calibrate import Calibrator
    Wf, bf, ps = calib_params(case)
    cin = Wf[0].shape[1]
    rng = np.random.default_rng(zlib.crc32(f"four.{case}".encode()))
    s = 0.0031
    mk = lambda **kw: Calibrator(Wf, bf, ps, device(), quan_bits=8, skip_quant_scale=s, **kw)
    front = mk()
    if case == "nrdm_3":
        outs = [front.enqueue_raw(torch.from_numpy(rng.integers(0, 4096, size=(2, 18, 34)).astype(np.uint16)).to(device())).clone()]
    else:
        outs = [front.enqueue_image(torch.from_numpy(rng.integers(0, 256, size=(2, 17, 33, 3)).astype(np.uint8)).to(device())).clone()]
    x = front.last_input.clone()
    front.sync()
    assert x.shape[1] == cin
    want = QO.forward(Wf, bf, ps, [x.cpu().numpy()], 8, F32(s))
    host, dev = mk(), mk()
    outs += [host.observe(x), dev.enqueue(x)]
    dev.sync()
    for name, y, cal in zip(("front", "observe", "enqueue"), outs, (front, host, dev)):
        same(f"{case} {name}", y, want.outputs[0], values=True, cast=np.float32)
        pass_equals(f"{case} {name}", cal, want)
        _same_bundle(f"{case} {name}", cal.bundle(), host.bundle())
    ent = mk(method="entropy")
    same(f"{case} entropy pass 1", ent.observe(x), want.outputs[0], values=True, cast=np.float32)
    ent.begin_histogram_pass()
    ent.observe(x)
    scale, zero = ent.finalize()
    assert len(scale) == 6 and ent.run_max == want.run_max


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(NETS))
def test_none_is_the_float_add(case):
    """skip_quant_scale=None: the plain pass, bit for bit oracle.calib_oracle.forward -- outputs, per-batch domains, running extrema --
    on both passes, and no launch of a quantised-merge kernel."""
    from sesrq import _lib
    from sesrq.calibrate import Calibrator
    Wf, bf, ps = calib_params(case)
    rng = np.random.default_rng(zlib.crc32(f"none.{case}".encode()))
    frames = _frames(rng, Wf[0].shape[1])
    want = CO.forward(Wf, bf, ps, frames, 8)
    before = _lib.qadd_instances()
    host = Calibrator(Wf, bf, ps, device(), quan_bits=8, skip_quant_scale=None)
    dev = Calibrator(Wf, bf, ps, device(), quan_bits=8)
    assert host.skip_quant_scale is None and dev.skip_quant_scale is None
    for i, x in enumerate(frames):
        same(f"{case} observe {i}", host.observe(to_device(x)), want.outputs[i], values=True, cast=np.float32)
        _domains_equal(f"{case} observe {i}", host, want.domains[i])
        y = dev.enqueue(to_device(x))
        dev.sync()
        same(f"{case} enqueue {i}", y, want.outputs[i], values=True, cast=np.float32)
        _domains_equal(f"{case} enqueue {i}", dev, want.domains[i])
    pass_equals(f"{case} observe", host, want)
    pass_equals(f"{case} enqueue", dev, want)
    assert _lib.qadd_instances() == before


# ---------------------------------------------------------------------------------------------------------------------- the reference
class _Ranges:
    def __init__(self, cal):
        self.run_min, self.run_max = list(cal.run_min), list(cal.run_max)


@pytest.mark.gpu
@pytest.mark.parametrize("record,frames_of", [(r, None) for r in K.ONE_FRAME] + sorted(K.LOOPS.items()))
def test_calibrator_reproduces_the_reference_records(record, frames_of):
    """Calibrator with the checkpoint's scale (qat_add.json) on the committed 80 x 960 frames and on the three-frame loops: the
    reference's running ranges, zero points and scales to the bars of test_qat_calib_oracle.py; the bundle carries the record's zero
    points.  The device pass; the host pass gives the same bits (above)."""
    from sesrq.calibrate import Calibrator
    p, pm = load_fixture(os.path.join(GOLDEN, f"{record}.params.npz"))
    rec = pm if frames_of is None else load_fixture(os.path.join(GOLDEN, "calib", f"{record}.npz"))[1]
    frames = [K.frame_of(pm)] if frames_of is None else K.dataset_frames(frames_of, pm["mflag"])
    cal = Calibrator([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], PIXEL_SHUFFLE[pm["mflag"]], device(), quan_bits=8,
                     skip_quant_scale=float(K.scale_of(record)))
    for x in frames:
        cal.enqueue(to_device(x))
    b = cal.bundle()
    K.assert_record(record if frames_of is None else "loop " + record, _Ranges(cal), rec)
    assert list(b.zero) == rec["zero"]


# ---------------------------------------------------------------------------------------------------------------------- test.py
@pytest.mark.gpu
def test_cli_on_a_synthetic_qat_checkpoint(tmp_path, capsys):
    """test.py --ckpt <synthetic QAT checkpoint>: prints the scale, gives the domains of a Calibrator built by hand with it; with
    --float-skip the parent's domains (oracle.calib_oracle.forward); --skip-quant-scale gives a --params net the same treatment."""
    import torch
    import sim
    from sesrq.calibrate import Calibrator
    add = K.ADD["nrdm_3_qat"]
    ckpt = str(tmp_path / "fake_qat_G.pth")
    torch.save(QO.qat_state_dict(3, add), ckpt)
    s = float(K.scale_of("nrdm_3_qat"))
    rng = np.random.default_rng(9)
    frames = rng.random((2, 3, 17, 33)).astype(F32)
    fpath = str(tmp_path / "frames.npy")
    np.save(fpath, frames)
    m = sim.float_model(3, ckpt=ckpt)
    convs = [m.conv_first.conv_expand] + [blk.conv_expand for blk in m.residual_block] + [m.conv_last.conv_expand]
    Wf, bf = [c.weight.detach().numpy() for c in convs], [c.bias.detach().numpy() for c in convs]
    mod = K.load_test_py()

    def by_hand(skip_s):
        cal = Calibrator(Wf, bf, 1, device(), quan_bits=8, skip_quant_scale=skip_s)
        for i in range(2):
            cal.observe(to_device(frames[i:i + 1]))
        return cal.finalize()

    capsys.readouterr()
    got = mod.main(["--mflag", "3", "--ckpt", ckpt, "--frames", fpath])
    out = capsys.readouterr().out
    assert f"skip_quant_scale: {s!r}" in out, out
    assert (list(got[0]), list(got[1])) == tuple(map(list, by_hand(s)))
    got_dev = mod.main(["--mflag", "3", "--ckpt", ckpt, "--input", fpath])              # the device-resident pass
    assert (list(got_dev[0]), list(got_dev[1])) == (list(got[0]), list(got[1]))
    capsys.readouterr()
    plain = mod.main(["--mflag", "3", "--ckpt", ckpt, "--frames", fpath, "--float-skip"])
    assert "skip_quant_scale: none" in capsys.readouterr().out
    want = CO.forward(Wf, bf, 1, [frames[0:1], frames[1:2]], 8, keep_outputs=False)
    assert (list(plain[0]), list(plain[1])) == tuple(map(list, K.finalize(want, 8)))
    assert list(plain[0]) != list(got[0])
    params = str(tmp_path / "net.params.npz")
    np.savez(params, meta=np.array(json.dumps({"case": "synthetic", "mflag": 3})), **{f"Wf{k}": Wf[k] for k in range(5)},
             **{f"bf{k}": bf[k] for k in range(5)})
    capsys.readouterr()
    byp = mod.main(["--mflag", "3", "--params", params, "--frames", fpath, "--skip-quant-scale", repr(s)])
    assert f"skip_quant_scale: {s!r}" in capsys.readouterr().out
    assert (list(byp[0]), list(byp[1])) == (list(got[0]), list(got[1]))
    with pytest.raises(SystemExit, match="positive"):
        mod.main(["--mflag", "3", "--params", params, "--frames", fpath, "--skip-quant-scale", "0"])
    with pytest.raises(SystemExit, match="exclude"):
        mod.main(["--mflag", "3", "--params", params, "--frames", fpath, "--skip-quant-scale", "0.1", "--float-skip"])


# ---------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_bad_scale_is_refused_before_any_launch():
    """s <= 0, NaN, inf (and a missing skip tensor) return the error code at the ABI; Calibrator raises ValueError; nothing is launched."""
    import torch
    from sesrq import _lib
    from sesrq.calibrate import Calibrator
    lib = _lib.lib()
    rng = np.random.default_rng(3)
    d = CO.domain(0.0, 1.5, 8, 0.0113, np.zeros(16, F32))
    x, wq = to_device(rng.random((1, 16, 9, 35)).astype(F32)), to_device(K.weights(rng, 16, 16, 3, 8))
    qb, skip = to_device(d.qbias), to_device(rng.random((1, 16, 9, 35)).astype(F32))
    out = torch.zeros((1, 16, 9, 35), dtype=torch.float32, device=device())
    desc = _lib.CalibConvDesc(k=3, ic=16, oc=16, w=wq.data_ptr(), qbias=qb.data_ptr(), in_scale=float(d.scale32), in_zero=d.zero,
                              ss=float(d.ss), acc_lo=float(d.acc_lo), acc_hi=float(d.acc_hi), add_lo=float(d.add_lo),
                              add_hi=float(d.add_hi), relu=1)
    slot = K.slot_bytes(d)
    torch.cuda.synchronize()
    launches = sum(_lib.instances().values()) + sum(_lib.qadd_instances().values())
    for s in (0.0, -0.004, float("nan"), float("inf"), -float("inf")):
        assert lib.sesrq_calib_conv_qadd(C.byref(desc), x.data_ptr(), skip.data_ptr(), out.data_ptr(), 1, 9, 35, 8, s, stream_ptr()) == 1
        assert "skip_scale" in _lib.last_error()
        assert lib.sesrq_calib_conv_slot_qadd(C.byref(desc), slot.data_ptr(), x.data_ptr(), skip.data_ptr(), out.data_ptr(), 1, 9, 35, 8, s,
                                              stream_ptr()) == 1
        assert "skip_scale" in _lib.last_error()
        with pytest.raises(ValueError, match="skip_quant_scale"):
            Calibrator(*calib_params("nrdm_3"), device(), skip_quant_scale=s)
    assert lib.sesrq_calib_conv_qadd(C.byref(desc), x.data_ptr(), None, out.data_ptr(), 1, 9, 35, 8, 0.01, stream_ptr()) == 1
    assert lib.sesrq_calib_conv_slot_qadd(C.byref(desc), slot.data_ptr(), x.data_ptr(), None, out.data_ptr(), 1, 9, 35, 8, 0.01, stream_ptr()) == 1
    assert lib.sesrq_calib_conv_qadd(C.byref(desc), x.data_ptr(), skip.data_ptr(), out.data_ptr(), 1, 9, 35, 9, 0.01, stream_ptr()) == 1
    with pytest.raises(ValueError, match="skip_quant_scale"):
        Calibrator(*calib_params("nrdm_3"), device(), skip_quant_scale="0.1")
    torch.cuda.synchronize()
    assert sum(_lib.instances().values()) + sum(_lib.qadd_instances().values()) == launches, "a refused call launched a kernel"
    assert not out.any()


def test_qadd_kernels_are_listed_apart():
    """The two quantised-merge kernels are in a list of their own; the main list holds the plain calibration kernels as before."""
    from sesrq import _lib
    assert sorted(_lib.qadd_instances()) == ["calib_conv_qadd_kernel<3>", "calib_conv_qadd_kernel<5>"]
    main = _lib.instances()
    assert "calib_conv_kernel<3>" in main and "calib_conv_kernel<5>" in main and not any("qadd" in n for n in main)


@pytest.mark.gpu
def test_zz_every_qadd_instance_ran():
    """LAST in this file: both instantiations were launched by a checked case above."""
    from sesrq import _lib
    inst = _lib.qadd_instances()
    missing = sorted(n for n, v in inst.items() if v == 0 or n not in HIT)
    assert inst and not missing, missing
