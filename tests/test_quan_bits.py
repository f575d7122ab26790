"""define.py QUAN_BIT = b < 8: the integer path at a narrow width of weights and activations, bit for bit with the reference.

Fixtures: tests/golden/quan_bits/ (make_quan_bits_golden.py runs the reference's own functions with define.QUAN_BIT = b and calibrates
on its random inputs at that width).  A net with b < 8 runs every layer on the dot4 kernels (sesrq_create_q)."""
import dataclasses
import glob
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_fixture
from helpers import PIXEL_SHUFFLE, calib_params, device, full_input, same, sha256

QB = os.path.join(GOLDEN, "quan_bits")
CROPS = sorted(glob.glob(os.path.join(QB, "*.crop.npz")))
STAGE_FILES = CROPS + sorted(glob.glob(os.path.join(QB, "*.zeros.npz")))


def _id(p):
    return os.path.basename(p)[:-4]


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_fixture_matrix():
    """b in {3, 4, 6, 7} for SESR-x4, nrdm_3 and SESR-x2, b = 2 and 5 for nrdm_3, each with its stage crop, zero-point variant and
    params."""
    got = {(json.loads(str(np.load(p)["meta"]))["case"], json.loads(str(np.load(p)["meta"]))["quan_bits"]) for p in CROPS}
    want = {(c, b) for c in ("sesr_x4", "nrdm_3", "sesr_x2_rand") for b in (3, 4, 6, 7)} | {("nrdm_3", 2), ("nrdm_3", 5)}
    assert got == want
    for c, b in want:
        for kind in ("crop", "zeros", "params"):
            assert os.path.isfile(os.path.join(QB, f"{c}.q{b}.{kind}.npz"))


def test_define_check_accepts_2_to_8_and_refuses_1_and_9(monkeypatch):
    import define
    for b in range(2, 9):
        monkeypatch.setattr(define, "QUAN_BIT", b)
        define.check()
    for b in (1, 9, 0, 16):
        monkeypatch.setattr(define, "QUAN_BIT", b)
        with pytest.raises(ValueError, match="QUAN_BIT"):
            define.check()


def test_bundle_round_trip_keeps_the_width(tmp_path):
    from sesrq.bundle import Bundle
    b = Bundle.load(os.path.join(QB, "sesr_x4.q4.crop.npz"))
    assert b.quan_bits == 4
    b.save(str(tmp_path / "b.npz"))
    b2 = Bundle.load(str(tmp_path / "b.npz"))
    assert b2.quan_bits == 4 and b2.zero == b.zero and b2.scale == b.scale
    for l1, l2 in zip(b.layers, b2.layers):
        np.testing.assert_array_equal(l1.wq, l2.wq)
    # a bundle written before the width existed (no key) is 8-bit
    old = Bundle.load(os.path.join(GOLDEN, "sesr_x4.crop.npz"))
    assert old.quan_bits == 8
    z = dict(np.load(str(tmp_path / "b.npz")))
    m = json.loads(str(z["meta"]))
    del m["quan_bits"]
    z["meta"] = np.array(json.dumps(m))
    np.savez(str(tmp_path / "old.npz"), **z)
    assert Bundle.load(str(tmp_path / "old.npz")).quan_bits == 8


@pytest.mark.parametrize("path", CROPS, ids=_id)
def test_derive_bundle_reproduces_the_reference(path):
    """Float convs + the reference's calibration at width b -> the reference's b-bit weights, (M, n), add constants and zeros."""
    from sesrq.bundle import derive_bundle
    fx, meta = load_fixture(path)
    b = meta["quan_bits"]
    p, pm = load_fixture(path.replace(".crop.npz", ".params.npz"))
    assert pm["quan_bits"] == b and pm["zero"] == meta["zero"]
    bun = derive_bundle([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], pm["scale"], pm["zero"], PIXEL_SHUFFLE[meta["mflag"]],
                        quan_bit=b)
    assert bun.quan_bits == b and bun.zero == meta["zero"]
    assert (bun.M_res, bun.n_res) == (meta["M_res"], meta["n_res"])
    for k, l in enumerate(bun.layers):
        np.testing.assert_array_equal(l.wq, fx[f"Wq{k}"])
        assert l.wq.min() >= -(1 << (b - 1)) and l.wq.max() <= (1 << (b - 1)) - 1
        assert (l.M, l.n) == (meta["M"][k], meta["n"][k]), k
        np.testing.assert_array_equal(l.add_const, fx[f"add_const{k}"])
    # an 8-bit derivation of the same convs is a different net: the width is live
    b8 = derive_bundle([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], pm["scale"], pm["zero"], PIXEL_SHUFFLE[meta["mflag"]])
    assert b8.quan_bits == 8 and not np.array_equal(b8.layers[0].wq, bun.layers[0].wq)


def test_derive_bundle_refuses_weights_wider_than_the_width():
    from sesrq.bundle import derive_bundle_from_quantized
    fx, meta = load_fixture(os.path.join(GOLDEN, "sesr_x4.crop.npz"))
    with pytest.raises(ValueError, match="4-bit"):
        derive_bundle_from_quantized([fx[f"Wq{k}"] for k in range(5)], meta["wscale"], [np.zeros(fx[f"Wq{k}"].shape[0], np.float32)
                                     for k in range(5)], meta["scale"], meta["zero"], 4, quan_bit=4)


@pytest.mark.parametrize("path", [p for p in CROPS if ".q4." in p], ids=_id)
def test_weight_txt_equals_the_reference_bytes(path):
    """output_txt/weight/conv.weight.K.txt at QUAN_BIT = 4 (quan_func.py:86-110: float_to_hex(w, QUAN_BIT), two digits minimum)."""
    from sesrq import stimulus as S
    fx, meta = load_fixture(path)
    for k in range(5):
        assert S.weight_txt(fx[f"Wq{k}"], 4).encode() == fx[f"wtxt{k}"].tobytes(), k


# ------------------------------------------------------------------------------------- CPU: the width-aware oracles pinned to the fixtures

def _oracle_net(path):
    from oracle import sesrq_oracle as O
    fx, meta = load_fixture(path)
    net = O.net_from_fixture(fx)
    assert net.quan_bits == meta["quan_bits"] and (net.qlo, net.qhi) == (-(1 << (meta["quan_bits"] - 1)), (1 << (meta["quan_bits"] - 1)) - 1)
    return fx, meta, net


def test_every_width_has_fixtures():
    assert sorted({load_fixture(p)[1]["quan_bits"] for p in STAGE_FILES}) == [2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("path", STAGE_FILES, ids=_id)
def test_numpy_oracle_reproduces_every_stage_at_the_width(path):
    """oracle.sesrq_oracle.forward at net.quan_bits = b: every array the reference dumped (input.0..5, input.4.spcial, shortcut,
    pe_out, pe_add, out, the shuffled int8 output), bit for bit -- as test_oracle_golden does at b = 8."""
    from oracle import sesrq_oracle as O
    fx, meta, net = _oracle_net(path)
    st = O.forward(net, fx["x"], keep=True)
    inv = {"out": "y"}
    names = [n for n in fx.files if n not in ("meta", "x") and not n.startswith(("Wq", "add_const", "wtxt"))]
    assert len(names) == 20
    for name in names:
        np.testing.assert_array_equal(np.asarray(st[inv.get(name, name)]).astype(fx[name].dtype), fx[name], err_msg=name)
    assert list(st["y"].shape) == meta["out_shape"]


@pytest.mark.parametrize("path", STAGE_FILES, ids=_id)
def test_c_oracle_reproduces_the_crop_and_the_full_frame_at_the_width(path):
    """oracle/sesrq_oracle.c (orc_forward_q) at b: the crop's stages and outputs, and the SHA-256 of the reference's 80 x 960 frame."""
    from oracle import c_oracle as CO
    fx, meta, net = _oracle_net(path)
    r = CO.forward(net, fx["x"], threads=4, keep=True)
    for k in range(5):
        for name in (f"input{k}", f"pe_out{k}"):
            np.testing.assert_array_equal(r[name].reshape(fx[name].shape), fx[name], err_msg=name)
        np.testing.assert_array_equal(r[f"pe_add{k}"], fx[f"pe_add{k}"], err_msg=f"pe_add{k}")
    np.testing.assert_array_equal(r["q_out"], fx["q_out"])
    np.testing.assert_array_equal(r["y"], fx["out"])
    if meta["tag"] == "crop":
        x = full_input(meta)
        assert sha256(x) == meta["full"]["x_sha256"]
        f = CO.forward(net, x, threads=8)
        assert list(f["y"].shape) == meta["full"]["shape"]
        assert sha256(f["q_out"]) == meta["full"]["q_out"] and sha256(f["y"]) == meta["full"]["y"]


@pytest.mark.parametrize("path", CROPS, ids=_id)
def test_oracle_derivation_at_the_width(path):
    """oracle.sesrq_oracle.derive_net(quan_bit=b) and calib_scale_zero(width=b) on the float convs and the reference's ranges: the
    reference's b-bit weights, (M, n), add constants and domains."""
    from oracle import sesrq_oracle as O
    fx, meta, _ = _oracle_net(path)
    b = meta["quan_bits"]
    p, pm = load_fixture(path.replace(".crop.npz", ".params.npz"))
    sz = [O.calib_scale_zero(0.0 if i == 5 else pm["min"][i], pm["max"][i], b) for i in range(6)]
    assert [s_ for s_, _ in sz] == pm["scale"] == meta["scale"] and [z for _, z in sz] == pm["zero"] == meta["zero"]
    net = O.derive_net([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], pm["scale"], pm["zero"], PIXEL_SHUFFLE[meta["mflag"]],
                       quan_bit=b)
    assert net.quan_bits == b
    for k in range(5):
        np.testing.assert_array_equal(net.layers[k].wq, fx[f"Wq{k}"], err_msg=f"Wq{k}")
        np.testing.assert_array_equal(net.layers[k].add_const, fx[f"add_const{k}"], err_msg=f"add_const{k}")
        assert (net.layers[k].M, net.layers[k].n) == (meta["M"][k], meta["n"][k])
    assert (net.M_res, net.n_res) == (meta["M_res"], meta["n_res"])


# sha256 (first 16 hex digits) of synth_net's 8-bit draws as they were before the width existed: the tests built on them keep their data
SYNTH8 = {("sesr_x4", False, 0): "3a7e7b0961340639", ("sesr_x4", False, 1): "72cd01668015273c", ("sesr_x4", True, 0): "8c230c442cd05f33",
          ("sesr_x4", True, 1): "19ff8cfd056da585", ("sesr_x2", False, 0): "420daa154266da6b", ("sesr_x2", False, 1): "a939679c3ad2c802",
          ("sesr_x2", True, 0): "1c7a08fb2924d310", ("sesr_x2", True, 1): "1f9cfe70a734f1dc", ("nrdm", False, 0): "7ba590d868a6471f",
          ("nrdm", False, 1): "d21fcdf63179fc07", ("nrdm", True, 0): "be659c81db43fe65", ("nrdm", True, 1): "fcb64b42f7487c2d"}


def _net_sha(net):
    h = hashlib.sha256()
    for l in net.layers:
        for a in (np.ascontiguousarray(l.wq), np.ascontiguousarray(l.add_const, np.int32), np.array([l.M, l.n], np.int64)):
            h.update(a.tobytes())
    for a in (np.array(net.zero, np.int64), np.array(net.scale, np.float64), np.array([net.M_res, net.n_res, net.pixel_shuffle], np.int64)):
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def test_synth_net_draws_at_8_bits_are_unchanged_and_narrow_ones_stay_in_range():
    from oracle import sesrq_oracle as O
    for (kind, hard, seed), want in SYNTH8.items():
        assert _net_sha(O.synth_net(kind, seed, hard=hard)) == want, (kind, hard, seed)
        assert _net_sha(O.synth_net(kind, seed, hard=hard, quan_bits=8)) == want
    for b in range(2, 8):
        lo, hi = -(1 << (b - 1)), (1 << (b - 1)) - 1
        for hard in (False, True):
            net = O.synth_net("sesr_x2", 0, hard=hard, quan_bits=b)
            assert net.quan_bits == b and all(lo <= l.wq.min() and l.wq.max() <= hi for l in net.layers)
            assert all(z <= hi for z in net.zero) and (min(net.zero) < -128) == hard


def test_c_oracle_equals_numpy_oracle_at_every_width():
    from oracle import c_oracle as CO
    from oracle import sesrq_oracle as O
    rng = np.random.default_rng(9)
    for b in range(2, 8):
        for kind, hard in (("sesr_x4", True), ("sesr_x2", False), ("nrdm", True)):
            net = O.synth_net(kind, b, hard=hard, quan_bits=b)
            x = rng.random((2, net.layers[0].wq.shape[1], 11, 37), dtype=np.float32)
            a, c = O.forward(net, x), CO.forward(net, x, threads=2)
            np.testing.assert_array_equal(a["q_out"], c["q_out"])
            np.testing.assert_array_equal(a["y"], c["y"])
            assert a["q_out"].min() >= net.qlo and a["q_out"].max() <= net.qhi


# ---------------------------------------------------------------------------------------------------------------------------- GPU

def _engine(path, **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(path), device(), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("force_general", [False, True], ids=["merged", "general"])
@pytest.mark.parametrize("path", STAGE_FILES, ids=_id)
def test_every_stage_matches_the_reference(path, force_general):
    import torch
    fx, meta = load_fixture(path)
    e = _engine(path, force_general=force_general)
    b = meta["quan_bits"]
    assert e.quan_bits == b
    r = e.forward_debug(torch.from_numpy(fx["x"]).to(device()), pe=True, acts=True, special=True)
    torch.cuda.synchronize()
    for k in range(5):
        same(f"input{k}", r[f"input{k}"], fx[f"input{k}"])
        same(f"pe_out{k}", r[f"pe_out{k}"], fx[f"pe_out{k}"], reshape=True)      # stored without the batch axis
        same(f"pe_add{k}", r[f"pe_add{k}"], fx[f"pe_add{k}"])
    same("shortcut", r["shortcut"], fx["shortcut"])
    same("input4_special", r["input4_special"], fx["input4_special"])
    same("q_out", r["q_out"], fx["q_out"])
    same("y", r["y"], fx["out"])
    q = r["q_out"].cpu().numpy()
    assert q.min() >= -(1 << (b - 1)) and q.max() <= (1 << (b - 1)) - 1
    # the production forward (no taps) gives the same bits
    q2, y2 = e.forward(torch.from_numpy(fx["x"]).to(device()))
    same("q_out (forward)", q2, fx["q_out"])
    same("y (forward)", y2, fx["out"])


@pytest.mark.gpu
def test_both_residual_layouts_are_covered():
    """zero[1] == -2^(b-1): layer 0's output is the residual operand (3 workspace tensors); else a separate one (4)."""
    for path in CROPS:
        meta = load_fixture(path)[1]
        zm = load_fixture(path.replace(".crop.", ".zeros."))[1]
        lo = -(1 << (meta["quan_bits"] - 1))
        assert meta["zero"][1] == lo and zm["zero"][1] != lo
        e, ez = _engine(path), _engine(path.replace(".crop.", ".zeros."))
        assert ez.workspace(1, 8, 8).numel() > e.workspace(1, 8, 8).numel()


@pytest.mark.gpu
@pytest.mark.parametrize("path", CROPS, ids=_id)
def test_full_frame_hashes_to_the_reference(path):
    import torch
    fx, meta = load_fixture(path)
    x = torch.from_numpy(full_input(meta)).to(device())
    assert sha256(full_input(meta)) == meta["full"]["x_sha256"]
    q, y = _engine(path)(x)
    torch.cuda.synchronize()
    assert list(y.shape) == meta["full"]["shape"]
    assert sha256(q.cpu().numpy()) == meta["full"]["q_out"]
    assert sha256(y.cpu().numpy()) == meta["full"]["y"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", [os.path.join(QB, f) for f in ("nrdm_3.q2.crop.npz", "nrdm_3.q4.zeros.npz", "sesr_x2_rand.q6.crop.npz")],
                         ids=_id)
def test_frame_shapes_and_batches_agree_with_single_frames(path):
    import torch
    fx, meta = load_fixture(path)
    x = fx["x"]
    for fg in (False, True):
        e = _engine(path, force_general=fg)
        q, y = e(torch.from_numpy(np.ascontiguousarray(x[:, :, 5:6, 7:8])).to(device()))      # a 1 x 1 frame
        r = PIXEL_SHUFFLE[meta["mflag"]]
        assert tuple(q.shape) == tuple(e.out_shape(1, 1, 1)) and tuple(q.shape[2:]) == (r, r)
        b = meta["quan_bits"]
        assert int(q.min()) >= -(1 << (b - 1)) and int(q.max()) <= (1 << (b - 1)) - 1
        crops = [np.ascontiguousarray(x[:, :, 2:11, 3:36]), np.ascontiguousarray(x[:, :, 13:22, 6:39])]
        qb, yb = e(torch.from_numpy(np.concatenate(crops)).to(device()))
        for i, c in enumerate(crops):
            q1, y1 = e(torch.from_numpy(c).to(device()))
            same(f"q frame {i}", qb[i:i + 1], q1.cpu().numpy())
            same(f"y frame {i}", yb[i:i + 1], y1.cpu().numpy())
        torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("path", [os.path.join(QB, f) for f in ("sesr_x4.q4.crop.npz", "nrdm_3.q6.crop.npz", "nrdm_3.q2.zeros.npz")],
                         ids=_id)
def test_int8_q0_input_equals_the_fp32_route(path):
    """An SESRQ_I8 input is q0 (input.0.pt); staged values beyond the width are clamped to it (a no-op at b = 8)."""
    import torch
    fx, meta = load_fixture(path)
    b = meta["quan_bits"]
    e = _engine(path)
    q0 = torch.from_numpy(fx["input0"]).to(device())
    q, y = e(q0)
    same("q from q0", q, fx["q_out"])
    same("y from q0", y, fx["out"])
    # out-of-range codes: the same bits as the clipped q0
    rng = np.random.default_rng(b)
    wild = rng.integers(-128, 128, size=fx["input0"].shape).astype(np.int8)
    qa, ya = e(torch.from_numpy(wild).to(device()))
    qc, yc = e(torch.from_numpy(np.clip(wild, -(1 << (b - 1)), (1 << (b - 1)) - 1).astype(np.int8)).to(device()))
    same("wild q", qa, qc.cpu().numpy())
    same("wild y", ya, yc.cpu().numpy())


@pytest.mark.gpu
def test_engine_names_carry_the_width_and_every_engine_option_lands_on_dot4():
    import torch
    from sesrq import _lib
    for path in CROPS:
        b = load_fixture(path)[1]["quan_bits"]
        for eng in (_lib.ENGINE_AUTO, _lib.ENGINE_DOT4, _lib.ENGINE_MFMA):
            e = _engine(path, engine=eng)
            names = e.layer_engines()
            assert all(n.startswith("dot4-") and n.endswith(f"-q{b}") for n in names), names
            assert e.launch_plan() == [(k, 1) for k in range(5)]          # no fused trio
            assert e.one_fma_layers() == [0] * 5                          # the reduced forms are proven for 8-bit clamps only
            assert _lib.lib().sesrq_net_quan_bits(e._h) == b
    # grouping (several frames as one launch sequence) needs the MFMA kernels: refused
    e = _engine(os.path.join(QB, "sesr_x4.q4.crop.npz"))
    fr = [torch.zeros((1, 1, 8, 8), device=device()) for _ in range(2)]
    outs = [torch.empty(e.out_shape(1, 8, 8), dtype=torch.int8, device=device()) for _ in range(2)]
    with pytest.raises(RuntimeError, match="MFMA first- and last-layer"):
        e.submission(fr, outs, [torch.cuda.current_stream()], group=2).enqueue(2)
        torch.cuda.synchronize()


@pytest.mark.gpu
def test_create_refuses_what_the_width_cannot_hold():
    import sesrq
    from sesrq.bundle import Bundle
    b = Bundle.load(os.path.join(QB, "sesr_x4.q4.crop.npz"))
    for qb in (1, 9):
        with pytest.raises(ValueError, match="quan_bits"):
            sesrq.Engine(dataclasses.replace(b, quan_bits=qb), device())
    wide = dataclasses.replace(b, quan_bits=4, layers=[dataclasses.replace(b.layers[0], wq=b.layers[0].wq * 2)] + b.layers[1:])
    with pytest.raises(ValueError, match="4-bit range"):
        sesrq.Engine(wide, device())
    with pytest.raises(ValueError, match="zero point"):
        sesrq.Engine(dataclasses.replace(b, zero=b.zero[:3] + [8] + b.zero[4:]), device())
    with pytest.raises(ValueError, match="upstream"):
        sesrq.Engine(b, device(), upstream=Bundle.load(os.path.join(GOLDEN, "sesr_x4.crop.npz")))


@pytest.mark.gpu
def test_an_8bit_engine_of_the_same_weights_differs():
    import sesrq
    import torch
    from sesrq.bundle import Bundle
    path = os.path.join(QB, "sesr_x4.q4.crop.npz")
    fx, _ = load_fixture(path)
    b = Bundle.load(path)
    x = torch.from_numpy(fx["x"]).to(device())
    q4, _ = sesrq.Engine(b, device())(x)
    e8 = sesrq.Engine(dataclasses.replace(b, quan_bits=8), device())
    q8, _ = e8(x)
    assert not any(n.endswith("-q8") for n in e8.layer_engines())
    assert not torch.equal(q4, q8)
    same("q4", q4, fx["q_out"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", CROPS, ids=_id)
def test_calibrator_matches_the_reference_ranges_at_the_width(path):
    """The device pass's ranges, zero points and scales against the reference's record.  SESR-x4 at b = 3 (sesr_x4.q3): where the
    reference's own fp32 run rounded one quantiser input at a tie to the other code (test_calib_oracle.py::
    test_sesr_x4_q3_differs_by_one_tie_of_the_reference, which names the element), domains 4 and 5 are held bit for bit to the
    oracle's ranges instead; its zeros and scales follow from them."""
    import torch
    from oracle import calib_oracle as CO
    from sesrq.calibrate import Calibrator
    fx, meta = load_fixture(path)
    b = meta["quan_bits"]
    p, pm = load_fixture(path.replace(".crop.npz", ".params.npz"))
    Wf, bf, ps = calib_params(path.replace(".crop.npz", ".params.npz"))
    cal = Calibrator(Wf, bf, ps, device(), quan_bits=b)
    cal.observe(torch.from_numpy(full_input(meta)).to(device()))
    want_min, want_max = list(pm["min"]), list(pm["max"])
    tie = os.path.basename(path) == "sesr_x4.q3.crop.npz"
    if tie:
        orc = CO.forward(Wf, bf, ps, [full_input(meta)], b, keep_outputs=False)
        for k in (4, 5):
            assert cal.run_min[k] == orc.run_min[k] and cal.run_max[k] == orc.run_max[k], k
            want_min[k], want_max[k] = orc.run_min[k], orc.run_max[k]
    for k in range(6):
        span = pm["max"][k] - pm["min"][k]
        # the output domain's min is observed but never used: the finaliser sets it to 0 (test.py:203-206)
        if k < 5:
            assert abs(cal.run_min[k] - want_min[k]) <= 1e-4 * span, (k, cal.run_min[k], want_min[k])
        assert abs(cal.run_max[k] - want_max[k]) <= 1e-4 * span, (k, cal.run_max[k], want_max[k])
    scale, zero = cal.finalize()
    if tie:
        from oracle.sesrq_oracle import calib_scale_zero
        want = [calib_scale_zero(0.0 if k == 5 else want_min[k], want_max[k], b) for k in range(6)]
        assert zero == [z for _, z in want] and zero[:4] == pm["zero"][:4]
        np.testing.assert_allclose(scale, [s for s, _ in want], rtol=2e-4)
        np.testing.assert_allclose(scale[:4], pm["scale"][:4], rtol=2e-4)
    else:
        assert zero == pm["zero"]
        np.testing.assert_allclose(scale, pm["scale"], rtol=2e-4)
    bun = cal.bundle()
    assert bun.quan_bits == b
    for k in range(5):
        np.testing.assert_array_equal(bun.layers[k].wq, fx[f"Wq{k}"])
    # the entropy variant runs at the width (2^b levels; parity unpinned)
    cal2 = Calibrator(Wf, bf, ps, device(), quan_bits=b, method="entropy")
    xt = torch.from_numpy(full_input(meta)).to(device())
    cal2.observe(xt)
    cal2.begin_histogram_pass()
    cal2.observe(xt)
    s2, z2 = cal2.finalize()
    assert all(-(1 << 20) < z <= (1 << (b - 1)) - 1 for z in z2) and all(s > 0 for s in s2)


@pytest.mark.gpu
def test_test_py_calibrates_at_the_width(monkeypatch, capsys):
    import define
    monkeypatch.setattr(define, "QUAN_BIT", 8)          # restored after the test: test.py sets it from --quan-bit
    spec = importlib.util.spec_from_file_location("sesrq_test_entry", os.path.join(ROOT, "sesr-pytorch-quantize_amd", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    params = os.path.join(QB, "sesr_x4.q4.params.npz")
    _, pm = load_fixture(params)
    scale, zero = mod.main(["--quan-bit", "4", "--mflag", "5", "--params", params, "--frames", os.path.join(GOLDEN, "rand_SR_Input_80x960.npy")])
    out = capsys.readouterr().out
    assert "QUAN_BIT: 4" in out and "bit: 4" in out
    assert list(zero) == pm["zero"]
    np.testing.assert_allclose(scale, pm["scale"], rtol=2e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sesr_x4.q4", "nrdm_3.q6"])
def test_sim_py_at_the_width_hashes_to_the_reference(case, monkeypatch, capsys):
    """sim.py --quan-bit B --params <case>.q<b>.params.npz on the reference's 80 x 960 frame: the spliced model lowers to a b-bit engine
    whose int8 and fp32 outputs hash to what the reference produced."""
    import define
    import sim
    import torch
    monkeypatch.setattr(define, "QUAN_BIT", 8)
    fx, meta = load_fixture(os.path.join(QB, f"{case}.crop.npz"))
    b = meta["quan_bits"]
    inp = os.path.join(GOLDEN, "rand_SR_Input_80x960.npy" if meta["mflag"] == 5 else "rand_DM_Input_80x960.npy")
    y = sim.main(["--quan-bit", str(b), "--mflag", str(meta["mflag"]), "--params", os.path.join(QB, f"{case}.params.npz"), "--input", inp])
    torch.cuda.synchronize()
    out = capsys.readouterr().out
    assert f"QUAN_BIT: {b}" in out and f"-q{b}" in out
    assert sha256(y.cpu().numpy()) == meta["full"]["y"]
    # the int8 frame behind it: the spliced model's engine, same input
    model = sim.splice(sim.float_model(meta["mflag"], None, os.path.join(QB, f"{case}.params.npz")))
    x = torch.from_numpy(np.load(inp)).cuda()
    assert sha256(model(x).cpu().numpy()) == meta["full"]["y"]
    eng = model._sesrq_engine(x.device)
    assert eng.quan_bits == b
    q, _ = eng(x)
    assert sha256(q.cpu().numpy()) == meta["full"]["q_out"]


@pytest.mark.gpu
@pytest.mark.parametrize("case,form", [("sesr_x4.q4", "y"), ("sesr_x2_rand.q4", "rgb")])
def test_forward_image_equals_forward_on_the_decoded_frame(case, form):
    import torch
    from sesrq import image
    e = _engine(os.path.join(QB, f"{case}.crop.npz"))
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(2, 17, 29, 3), dtype=np.uint8)).to(device())
    q, y = e.forward_image(img, form=form)
    _, x = image.decode(None, img, form, want_q=False, want_f=True)
    q2, y2 = e(x)
    torch.cuda.synchronize()
    same("q", q, q2.cpu().numpy())
    same("y", y, y2.cpu().numpy())


@pytest.mark.gpu
def test_forward_raw_equals_forward_on_the_unpacked_frame():
    import torch
    from sesrq import raw
    e = _engine(os.path.join(QB, "nrdm_3.q4.crop.npz"))
    fr = torch.from_numpy(np.random.default_rng(6).integers(0, 4096, size=(2, 18, 30)).astype(np.uint16)).to(device())
    q, y = e.forward_raw(fr)
    _, x = raw.unpack(None, fr, want_q=False, want_spread=True)
    q2, y2 = e(x)
    torch.cuda.synchronize()
    same("q", q, q2.cpu().numpy())
    same("y", y, y2.cpu().numpy())


@pytest.mark.gpu
def test_quality_score_of_the_int8_output_equals_scoring_y():
    import torch
    from sesrq import quality
    path = os.path.join(QB, "sesr_x4.q4.crop.npz")
    fx, meta = load_fixture(path)
    e = _engine(path)
    q, y = e(torch.from_numpy(fx["x"]).to(device()))
    gt = torch.from_numpy(np.random.default_rng(7).random(tuple(y.shape), dtype=np.float32)).to(device())
    a = quality.score(q, gt, 5, scale=float(np.float32(meta["scale"][5])), zero=meta["zero"][5])
    b = quality.score(y, gt, 5)
    torch.cuda.synchronize()
    same("scores", a, b, values=True)
