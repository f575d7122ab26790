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

QB = os.path.join(GOLDEN, "quan_bits")
CROPS = sorted(glob.glob(os.path.join(QB, "*.crop.npz")))
STAGE_FILES = CROPS + sorted(glob.glob(os.path.join(QB, "*.zeros.npz")))
PS = {5: 4, 6: 2, 3: 1}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _id(p):
    return os.path.basename(p)[:-4]


def full_input(meta):
    return np.load(os.path.join(GOLDEN, "rand_SR_Input_80x960.npy" if meta["mflag"] == 5 else "rand_DM_Input_80x960.npy"))


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_fixture_matrix():
    """b in {4, 6} for SESR-x4, nrdm_3 and SESR-x2, b = 2 for nrdm_3, each with its stage crop, zero-point variant and params."""
    got = {(json.loads(str(np.load(p)["meta"]))["case"], json.loads(str(np.load(p)["meta"]))["quan_bits"]) for p in CROPS}
    want = {(c, b) for c in ("sesr_x4", "nrdm_3", "sesr_x2_rand") for b in (4, 6)} | {("nrdm_3", 2)}
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
    bun = derive_bundle([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], pm["scale"], pm["zero"], PS[meta["mflag"]],
                        quan_bit=b)
    assert bun.quan_bits == b and bun.zero == meta["zero"]
    assert (bun.M_res, bun.n_res) == (meta["M_res"], meta["n_res"])
    for k, l in enumerate(bun.layers):
        np.testing.assert_array_equal(l.wq, fx[f"Wq{k}"])
        assert l.wq.min() >= -(1 << (b - 1)) and l.wq.max() <= (1 << (b - 1)) - 1
        assert (l.M, l.n) == (meta["M"][k], meta["n"][k]), k
        np.testing.assert_array_equal(l.add_const, fx[f"add_const{k}"])
    # an 8-bit derivation of the same convs is a different net: the width is live
    b8 = derive_bundle([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], pm["scale"], pm["zero"], PS[meta["mflag"]])
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


# ---------------------------------------------------------------------------------------------------------------------------- GPU

def _dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _engine(path, **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(path), _dev(), **kw)


def _eq(name, got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = np.asarray(want)
    assert got.size == want.size, (name, got.shape, want.shape)
    got = got.reshape(want.shape)
    bad = np.flatnonzero(got.astype(np.float64).ravel() != want.astype(np.float64).ravel())
    assert bad.size == 0, f"{name}: {bad.size} mismatches, first at {bad[0]}: got {got.ravel()[bad[0]]} want {want.ravel()[bad[0]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("force_general", [False, True], ids=["merged", "general"])
@pytest.mark.parametrize("path", STAGE_FILES, ids=_id)
def test_every_stage_matches_the_reference(path, force_general):
    import torch
    fx, meta = load_fixture(path)
    e = _engine(path, force_general=force_general)
    b = meta["quan_bits"]
    assert e.quan_bits == b
    r = e.forward_debug(torch.from_numpy(fx["x"]).to(_dev()), pe=True, acts=True, special=True)
    torch.cuda.synchronize()
    for k in range(5):
        _eq(f"input{k}", r[f"input{k}"], fx[f"input{k}"])
        _eq(f"pe_out{k}", r[f"pe_out{k}"], fx[f"pe_out{k}"])
        _eq(f"pe_add{k}", r[f"pe_add{k}"], fx[f"pe_add{k}"])
    _eq("shortcut", r["shortcut"], fx["shortcut"])
    _eq("input4_special", r["input4_special"], fx["input4_special"])
    _eq("q_out", r["q_out"], fx["q_out"])
    _eq("y", r["y"], fx["out"])
    q = r["q_out"].cpu().numpy()
    assert q.min() >= -(1 << (b - 1)) and q.max() <= (1 << (b - 1)) - 1
    # the production forward (no taps) gives the same bits
    q2, y2 = e.forward(torch.from_numpy(fx["x"]).to(_dev()))
    _eq("q_out (forward)", q2, fx["q_out"])
    _eq("y (forward)", y2, fx["out"])


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
    x = torch.from_numpy(full_input(meta)).to(_dev())
    assert sha(full_input(meta)) == meta["full"]["x_sha256"]
    q, y = _engine(path)(x)
    torch.cuda.synchronize()
    assert list(y.shape) == meta["full"]["shape"]
    assert sha(q.cpu().numpy()) == meta["full"]["q_out"]
    assert sha(y.cpu().numpy()) == meta["full"]["y"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", [os.path.join(QB, f) for f in ("nrdm_3.q2.crop.npz", "nrdm_3.q4.zeros.npz", "sesr_x2_rand.q6.crop.npz")],
                         ids=_id)
def test_frame_shapes_and_batches_agree_with_single_frames(path):
    import torch
    fx, meta = load_fixture(path)
    x = fx["x"]
    for fg in (False, True):
        e = _engine(path, force_general=fg)
        q, y = e(torch.from_numpy(np.ascontiguousarray(x[:, :, 5:6, 7:8])).to(_dev()))      # a 1 x 1 frame
        r = PS[meta["mflag"]]
        assert tuple(q.shape) == tuple(e.out_shape(1, 1, 1)) and tuple(q.shape[2:]) == (r, r)
        b = meta["quan_bits"]
        assert int(q.min()) >= -(1 << (b - 1)) and int(q.max()) <= (1 << (b - 1)) - 1
        crops = [np.ascontiguousarray(x[:, :, 2:11, 3:36]), np.ascontiguousarray(x[:, :, 13:22, 6:39])]
        qb, yb = e(torch.from_numpy(np.concatenate(crops)).to(_dev()))
        for i, c in enumerate(crops):
            q1, y1 = e(torch.from_numpy(c).to(_dev()))
            _eq(f"q frame {i}", qb[i:i + 1], q1.cpu().numpy())
            _eq(f"y frame {i}", yb[i:i + 1], y1.cpu().numpy())
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
    q0 = torch.from_numpy(fx["input0"]).to(_dev())
    q, y = e(q0)
    _eq("q from q0", q, fx["q_out"])
    _eq("y from q0", y, fx["out"])
    # out-of-range codes: the same bits as the clipped q0
    rng = np.random.default_rng(b)
    wild = rng.integers(-128, 128, size=fx["input0"].shape).astype(np.int8)
    qa, ya = e(torch.from_numpy(wild).to(_dev()))
    qc, yc = e(torch.from_numpy(np.clip(wild, -(1 << (b - 1)), (1 << (b - 1)) - 1).astype(np.int8)).to(_dev()))
    _eq("wild q", qa, qc.cpu().numpy())
    _eq("wild y", ya, yc.cpu().numpy())


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
    fr = [torch.zeros((1, 1, 8, 8), device=_dev()) for _ in range(2)]
    outs = [torch.empty(e.out_shape(1, 8, 8), dtype=torch.int8, device=_dev()) for _ in range(2)]
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
            sesrq.Engine(dataclasses.replace(b, quan_bits=qb), _dev())
    wide = dataclasses.replace(b, quan_bits=4, layers=[dataclasses.replace(b.layers[0], wq=b.layers[0].wq * 2)] + b.layers[1:])
    with pytest.raises(ValueError, match="4-bit range"):
        sesrq.Engine(wide, _dev())
    with pytest.raises(ValueError, match="zero point"):
        sesrq.Engine(dataclasses.replace(b, zero=b.zero[:3] + [8] + b.zero[4:]), _dev())
    with pytest.raises(ValueError, match="upstream"):
        sesrq.Engine(b, _dev(), upstream=Bundle.load(os.path.join(GOLDEN, "sesr_x4.crop.npz")))


@pytest.mark.gpu
def test_an_8bit_engine_of_the_same_weights_differs():
    import sesrq
    import torch
    from sesrq.bundle import Bundle
    path = os.path.join(QB, "sesr_x4.q4.crop.npz")
    fx, _ = load_fixture(path)
    b = Bundle.load(path)
    x = torch.from_numpy(fx["x"]).to(_dev())
    q4, _ = sesrq.Engine(b, _dev())(x)
    e8 = sesrq.Engine(dataclasses.replace(b, quan_bits=8), _dev())
    q8, _ = e8(x)
    assert not any(n.endswith("-q8") for n in e8.layer_engines())
    assert not torch.equal(q4, q8)
    _eq("q4", q4, fx["q_out"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", CROPS, ids=_id)
def test_calibrator_matches_the_reference_ranges_at_the_width(path):
    import torch
    from sesrq.calibrate import Calibrator
    fx, meta = load_fixture(path)
    b = meta["quan_bits"]
    p, pm = load_fixture(path.replace(".crop.npz", ".params.npz"))
    cal = Calibrator([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], PS[pm["mflag"]], _dev(), quan_bits=b)
    cal.observe(torch.from_numpy(full_input(meta)).to(_dev()))
    for k in range(6):
        span = pm["max"][k] - pm["min"][k]
        # the output domain's min is observed but never used: the finaliser sets it to 0 (test.py:203-206)
        if k < 5:
            assert abs(cal.run_min[k] - pm["min"][k]) <= 1e-4 * span, (k, cal.run_min[k], pm["min"][k])
        assert abs(cal.run_max[k] - pm["max"][k]) <= 1e-4 * span, (k, cal.run_max[k], pm["max"][k])
    scale, zero = cal.finalize()
    assert zero == pm["zero"]
    np.testing.assert_allclose(scale, pm["scale"], rtol=2e-4)
    bun = cal.bundle()
    assert bun.quan_bits == b
    for k in range(5):
        np.testing.assert_array_equal(bun.layers[k].wq, fx[f"Wq{k}"])
    # the entropy variant runs at the width (2^b levels; parity unpinned)
    cal2 = Calibrator([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], PS[pm["mflag"]], _dev(), quan_bits=b,
                      method="entropy")
    xt = torch.from_numpy(full_input(meta)).to(_dev())
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
    assert sha(y.cpu().numpy()) == meta["full"]["y"]
    # the int8 frame behind it: the spliced model's engine, same input
    model = sim.splice(sim.float_model(meta["mflag"], None, os.path.join(QB, f"{case}.params.npz")))
    x = torch.from_numpy(np.load(inp)).cuda()
    assert sha(model(x).cpu().numpy()) == meta["full"]["y"]
    eng = model._sesrq_engine(x.device)
    assert eng.quan_bits == b
    q, _ = eng(x)
    assert sha(q.cpu().numpy()) == meta["full"]["q_out"]


@pytest.mark.gpu
@pytest.mark.parametrize("case,form", [("sesr_x4.q4", "y"), ("sesr_x2_rand.q4", "rgb")])
def test_forward_image_equals_forward_on_the_decoded_frame(case, form):
    import torch
    from sesrq import image
    e = _engine(os.path.join(QB, f"{case}.crop.npz"))
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(2, 17, 29, 3), dtype=np.uint8)).to(_dev())
    q, y = e.forward_image(img, form=form)
    _, x = image.decode(None, img, form, want_q=False, want_f=True)
    q2, y2 = e(x)
    torch.cuda.synchronize()
    _eq("q", q, q2.cpu().numpy())
    _eq("y", y, y2.cpu().numpy())


@pytest.mark.gpu
def test_forward_raw_equals_forward_on_the_unpacked_frame():
    import torch
    from sesrq import raw
    e = _engine(os.path.join(QB, "nrdm_3.q4.crop.npz"))
    fr = torch.from_numpy(np.random.default_rng(6).integers(0, 4096, size=(2, 18, 30)).astype(np.uint16)).to(_dev())
    q, y = e.forward_raw(fr)
    _, x = raw.unpack(None, fr, want_q=False, want_spread=True)
    q2, y2 = e(x)
    torch.cuda.synchronize()
    _eq("q", q, q2.cpu().numpy())
    _eq("y", y, y2.cpu().numpy())


@pytest.mark.gpu
def test_quality_score_of_the_int8_output_equals_scoring_y():
    import torch
    from sesrq import quality
    path = os.path.join(QB, "sesr_x4.q4.crop.npz")
    fx, meta = load_fixture(path)
    e = _engine(path)
    q, y = e(torch.from_numpy(fx["x"]).to(_dev()))
    gt = torch.from_numpy(np.random.default_rng(7).random(tuple(y.shape), dtype=np.float32)).to(_dev())
    a = quality.score(q, gt, 5, scale=float(np.float32(meta["scale"][5])), zero=meta["zero"][5])
    b = quality.score(y, gt, 5)
    torch.cuda.synchronize()
    _eq("scores", a, b.cpu().numpy())
