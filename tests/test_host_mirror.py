"""Host-side mirror of the reference interface (define / myQL / models / sim): the spliced graph
lowers to the integer bundle the reference itself produced (CPU-only: no device call), keeps the
reference's error conventions, and -- on the GPU -- the spliced model's forward is the golden output."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_fixture
from qat_calib_oracle import qat_state_dict
import define
import sim
from myQL import quan_func as qf
from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
from myQL.graph_modify import insert_before
from models import sesr_sim, model_utils_pt
from sesrq.store import STORE

CASES = {"sesr_x4": 5, "nrdm_3": 3, "sesr_x2_rand": 6, "sesr_x4_qat": 5, "nrdm_3_qat": 3}


@pytest.mark.parametrize("case", sorted(CASES))
def test_spliced_graph_lowers_to_reference_bundle(case):
    STORE.clear()
    model = sim.splice(sim.float_model(CASES[case], params=os.path.join(GOLDEN, f"{case}.params.npz")))
    names = [getattr(n.target, "__name__", str(n.target)) for n in model.graph.nodes]
    # same chain the reference's generated forward shows
    i = names.index("conv_first.conv_expand")
    assert names[i - 2:i + 3] == ["quantize_asymmetrical_by_tensor", "reshape_input_for_hardware_pe",
                                  "conv_first.conv_expand", "PEs_and_bias_adder", "requan_conv2d_output"]
    b = model.sesrq_bundle()
    fx, meta = load_fixture(os.path.join(GOLDEN, f"{case}.crop.npz"))
    for k in range(5):
        np.testing.assert_array_equal(b.layers[k].wq, fx[f"Wq{k}"])
        np.testing.assert_array_equal(b.layers[k].add_const, fx[f"add_const{k}"])
        assert (b.layers[k].M, b.layers[k].n) == (meta["M"][k], meta["n"][k])
    assert (b.M_res, b.n_res) == (meta["M_res"], meta["n_res"])
    assert b.pixel_shuffle == {5: 4, 3: 1, 6: 2}[CASES[case]]
    assert b.zero == meta["zero"] and b.scale == meta["scale"]
    # conv biases were zeroed by the bias bypass and travel as kwargs (graph_modify.py:68-120)
    assert float(model.conv_first.conv_expand.bias.abs().max()) == 0.0


def test_collapse_is_the_same_linear_map():
    torch.manual_seed(0)
    net = sesr_sim.sesr()
    x = torch.rand(1, 1, 12, 14)
    with torch.no_grad():
        init = net.conv_first(x)
        mid = net.residual_block(init)
        want = net.depth_to_space(net.conv_last(mid))
        net.collapse()
        got = net(x)
    assert got.shape == (1, 1, 48, 56)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=1e-5)
    assert isinstance(net.conv_first.conv_squeeze, torch.nn.Identity) and net.conv_first.conv_expand.weight.shape == (16, 1, 5, 5)


def _synthetic_checkpoint(tmp_path, name, case):
    """tests/golden/synthetic_ckpt.py: the seeded state dict of `case` in the layout of the reference checkpoint `name` (a QAT one
    prepared first), written to tmp_path/name.  Returns (MFLAG, path)."""
    import sys
    from models import quantize_utils_pt as quantize
    sys.path.insert(0, GOLDEN)
    from synthetic_ckpt import CASES as SYN, synthetic_state_dict
    mflag, qat, _ = SYN[case]
    m = sim.MODELS[mflag]()
    if qat:
        quantize.prepare(m, inplace=True, a_bits=8, w_bits=8, q_type=0, q_level="C")
    p = tmp_path / name
    torch.save({k: torch.from_numpy(v) for k, v in synthetic_state_dict(m.state_dict(), case).items()}, p)
    return mflag, str(p)


def test_collapse_of_reference_checkpoint_matches_golden_float_weights(tmp_path):
    """My closed-form fold vs the reference's delta-image fold of the same SESR-x4 checkpoint (layout of x4sesr.pth, seeded
    synthetic weights: the reference's own fold of it is tests/golden/ckpt/synthetic_folds.npz)."""
    mflag, ckpt = _synthetic_checkpoint(tmp_path, "x4sesr.pth", "sesr_x4")
    m = sim.float_model(mflag, ckpt=ckpt)
    z = np.load(os.path.join(GOLDEN, "ckpt", "synthetic_folds.npz"))
    convs = [m.conv_first.conv_expand] + [b.conv_expand for b in m.residual_block] + [m.conv_last.conv_expand]
    for k, c in enumerate(convs):
        np.testing.assert_allclose(c.weight.detach().numpy(), z[f"sesr_x4__Wf{k}"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(c.bias.detach().numpy(), z[f"sesr_x4__bf{k}"], rtol=0, atol=1e-7)


def test_error_conventions_of_the_callables():
    with pytest.raises(AssertionError, match="less than shift_max"):
        qf.quan_layer_between_const(0.5, 16, 16)
    assert qf.quan_layer_between_const(0.0078125) == (32768, 22)
    with pytest.raises(AssertionError, match="all zero"):
        qf.quantize_symmetrical_by_tensor(torch.zeros(2, 2, 3, 3), 8, 1, func_id=0)
    with pytest.raises(AssertionError, match="dimension: 4"):
        qf.reshape_input_for_hardware_pe(torch.zeros(3, 4, 5))
    with pytest.raises(RuntimeError, match="stage marker"):
        qf.requan_conv2d_output(torch.zeros(1, 1, 2, 2), func_id=0, exe_mode=1)
    with pytest.raises(RuntimeError, match="stage marker"):
        qf.quantize_asymmetrical_by_tensor(torch.zeros(1, 1, 2, 2), width=8, exe_mode=0, func_id=0)
    assert qf.float_to_hex(-1, 8) == "ff" and qf.float_to_hex(127, 8) == "7f" and qf.float_to_hex(-131072, 18) == "20000"


def test_partial_splice_is_rejected():
    STORE.clear()
    model = qf.quantize_model_weight(sim.float_model(5, params=os.path.join(GOLDEN, "sesr_x4.params.npz")), 8, 1)
    m = NodeInsertMapping()
    m.add_config(NodeInsertMappingElement(torch.nn.Conv2d, FunctionPackage(qf.quantize_asymmetrical_by_tensor, {"width": 8, "exe_mode": 1})))
    gm = insert_before(model_input=model, insert_mapping=m, has_func_id=True)
    with pytest.raises(RuntimeError, match="reshape_input_for_hardware_pe"):
        gm.sesrq_bundle()
    with pytest.raises(RuntimeError, match="GPU only"):
        gm(torch.zeros(1, 1, 8, 8))


def test_missing_calibration_is_reported():
    STORE.clear()
    model = sim.splice(sim.float_model(5, params=os.path.join(GOLDEN, "sesr_x4.params.npz")))
    STORE.clear()
    with pytest.raises(KeyError, match="parameter store"):
        model.sesrq_bundle()


def test_define_surface():
    for name in ("MFLAG", "PE", "QUAN_BIT", "BIAS_BIT", "PE_ACC_BIT", "PE_ADD_BIT", "REQUAN_BIT", "REQUAN_N_MAX",
                 "WEIGHT_W_FLG", "INPUT_W_FLG", "BIAS_W_FLG", "BIAS_QUAN_W_FLG", "OUTPUT_PE_W_FLG", "OUTPUT_PE_ADD_W_FLG",
                 "REQUAN_FACTOR_W_FLG", "WEIGHT_W_HIST_PNG", "INPUT_W_HIST_PNG", "TEST_RAW_ADD_NOISE"):
        assert hasattr(define, name)
    assert (define.PE, define.QUAN_BIT, define.BIAS_BIT, define.PE_ACC_BIT, define.PE_ADD_BIT, define.REQUAN_BIT,
            define.REQUAN_N_MAX) == (4, 8, 16, 18, 20, 16, 32)
    define.check()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sesr_x4", "nrdm_3", "sesr_x2_rand"])
def test_spliced_model_forward_is_the_golden_output(case):
    STORE.clear()
    model = sim.splice(sim.float_model(CASES[case], params=os.path.join(GOLDEN, f"{case}.params.npz")))
    fx, meta = load_fixture(os.path.join(GOLDEN, f"{case}.crop.npz"))
    y = model(torch.from_numpy(fx["x"]).cuda())
    np.testing.assert_array_equal(y.cpu().numpy(), fx["out"])
    assert model.last_q.dtype == torch.int8


SIM_INPUT = {5: "rand_SR_Input_80x960.npy", 3: "rand_DM_Input_80x960.npy", 6: "rand_DM_Input_80x960.npy"}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_sim_entry_end_to_end(case, capsys, tmp_path):
    """`sim.main` as a user runs it (reference sim.py:197-213: load the frame, ONE forward, the bit-width banner) on the
    reference's own 80x960 random inputs: the float result and the int8 `input.5` are the bytes the reference produced
    (SHA-256 of its output / stored input.5 in *.full.npz).  sesr_x4_qat = BASELINE config 1's checkpoint (sr_qat_G.pth)."""
    import hashlib
    STORE.clear()
    mflag = CASES[case]
    z = np.load(os.path.join(GOLDEN, f"{case}.full.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    save = str(tmp_path / "out.npy")
    y = sim.main(["--mflag", str(mflag), "--params", os.path.join(GOLDEN, f"{case}.params.npz"),
                  "--input", os.path.join(GOLDEN, SIM_INPUT[mflag]), "--save", save])
    out = capsys.readouterr().out
    for line in (f"SIM_mflag: {mflag}", "QUAN_BIT: 8", "BIAS_BIT: 16", "PE_ACC_BIT: 18", "PE_ADD_BIT: 20", "REQUAN_BIT: 16", "REQUAN_N_MAX: 32"):
        assert line in out, out
    assert "mfma" in out            # the engines line: the HIP kernels ran, not a fallback
    got = y.cpu().numpy()
    assert list(got.shape) == meta["out_shape"]
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == meta["sha"]["out"]
    np.testing.assert_array_equal(np.load(save), got)
    # input.5.pt: the int8 result before PixelShuffle
    r = {5: 4, 3: 1, 6: 2}[mflag]
    lowered = sim.splice(sim.float_model(mflag, params=os.path.join(GOLDEN, f"{case}.params.npz")))
    lowered(torch.from_numpy(np.load(os.path.join(GOLDEN, SIM_INPUT[mflag]))).cuda())
    q5 = torch.nn.functional.pixel_unshuffle(lowered.last_q.float(), r).to(torch.int8) if r > 1 else lowered.last_q
    np.testing.assert_array_equal(q5.cpu().numpy(), z["input5"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sesr_x4", "sesr_x2_rand"])
def test_dump_flags_write_an_output_pt_compatible_tree(case, tmp_path, monkeypatch):
    """define.py's *_W_FLG switches (reference define.py:23-31): the forward leaves the reference's dump tensors in the store under
    the reference's file names, `save_output_pt` writes the tree, `load_output_pt` reads it back -- and every tensor is the golden
    one the reference wrote for this crop (input.K, pe_outputK_P, pe_add_outputK, conv.bias.quanK, requant constants)."""
    STORE.clear()
    for n in ("INPUT_W_FLG", "OUTPUT_PE_W_FLG", "OUTPUT_PE_ADD_W_FLG", "BIAS_QUAN_W_FLG", "REQUAN_FACTOR_W_FLG"):
        monkeypatch.setattr(define, n, True)
    model = sim.splice(sim.float_model(CASES[case], params=os.path.join(GOLDEN, f"{case}.params.npz")))
    fx, meta = load_fixture(os.path.join(GOLDEN, f"{case}.crop.npz"))
    model(torch.from_numpy(fx["x"]).cuda())
    root = str(tmp_path / "output_pt")
    STORE.save_output_pt(root)
    assert os.path.isfile(os.path.join(root, "pe_out", "pe_output4_3.pt")) and os.path.isfile(os.path.join(root, "input", "input.5.pt"))
    STORE.clear()
    assert STORE.load_output_pt(root) > 40
    for k in range(5):
        np.testing.assert_array_equal(STORE[f"input/input.{k}"].numpy(), fx[f"input{k}"].astype(np.float32))
        for p in range(4):
            np.testing.assert_array_equal(STORE[f"pe_out/pe_output{k}_{p}"].numpy(), fx[f"pe_out{k}"][p].astype(np.float32))
        np.testing.assert_array_equal(STORE[f"pe_add/pe_add_output{k}"].numpy(), fx[f"pe_add{k}"].astype(np.float32))
        np.testing.assert_array_equal(STORE[f"bias/conv.bias.quan{k}"].numpy().reshape(-1), fx[f"add_const{k}"].astype(np.float32))
        assert (STORE[f"requan_factor/requan_{k}_{k + 1}"], STORE[f"requan_factor/n_{k}_{k + 1}"]) == (meta["M"][k], meta["n"][k])
        np.testing.assert_array_equal(STORE[f"weight/conv.weight.{k}"].numpy(), fx[f"Wq{k}"].astype(np.float32))
    np.testing.assert_array_equal(STORE["input/input.5"].numpy(), fx["input5"].astype(np.float32))
    # round 5: the two tensors the reference writes unconditionally (quan_func.py:549, :254) are part of the tree now
    assert os.path.isfile(os.path.join(root, "residual", "shortcut_tensor.pt")) and os.path.isfile(os.path.join(root, "input", "input.4.spcial.pt"))
    assert STORE["residual/shortcut_tensor"].dtype == torch.float32
    np.testing.assert_array_equal(STORE["residual/shortcut_tensor"].numpy(), fx["shortcut"])
    np.testing.assert_array_equal(STORE["input/input.4.spcial"].numpy(), fx["input4_special"].astype(np.float32))
    assert (STORE["requan_factor/requan_res"], STORE["requan_factor/n_res"]) == (meta["M_res"], meta["n_res"])
    STORE.clear()


def test_calibration_graph_is_recognised_on_cpu():
    """mode-0 splice (reference test.py:79-106) is accepted and classified; running it needs the GPU."""
    import importlib
    STORE.clear()
    calib = importlib.import_module("test")            # sesr-pytorch-quantize_amd/test.py, the calibration entry
    from sesrq.lowering import graph_mode
    gm = calib.splice_calibration(sim.float_model(5, params=os.path.join(GOLDEN, "sesr_x4.params.npz")))
    assert graph_mode(gm) == 0
    names = [getattr(n.target, "__name__", str(n.target)) for n in gm.graph.nodes]
    assert names.count("quantize_asymmetrical_by_tensor") == 6          # 5 convs + the one before PixelShuffle
    assert "requan_conv2d_output" not in names
    with pytest.raises(RuntimeError, match="GPU only"):
        gm(torch.zeros(1, 1, 8, 8))


@pytest.mark.gpu
def test_calibrate_then_infer_end_to_end(tmp_path):
    """test.py-equivalent calibration on the reference's random frame, then sim.py-equivalent inference with
    the calibrated domains: the integer output equals the oracle's for the bundle derived from THIS calibration."""
    import importlib
    from oracle import sesrq_oracle as O
    calib = importlib.import_module("test")
    frames = os.path.join(GOLDEN, "rand_SR_Input_80x960.npy")
    scale, zero = calib.main(["--mflag", "5", "--params", os.path.join(GOLDEN, "sesr_x4.params.npz"), "--frames", frames])
    _, pm = load_fixture(os.path.join(GOLDEN, "sesr_x4.params.npz"))
    assert zero == pm["zero"]
    np.testing.assert_allclose(scale, pm["scale"], rtol=2e-4)
    model = sim.splice(sim.float_model(5, params=os.path.join(GOLDEN, "sesr_x4.params.npz")))
    STORE.set_activation_domains(scale, zero)          # float_model() put the reference's domains there; use ours
    b = model.sesrq_bundle()
    x = np.load(frames)[:, :, :32, :64].copy()
    y = model(torch.from_numpy(x).cuda())
    net = O.Net(layers=[O.Layer(l.wq, l.add_const, l.M, l.n, l.relu) for l in b.layers], scale=b.scale, zero=b.zero,
                M_res=b.M_res, n_res=b.n_res, pixel_shuffle=b.pixel_shuffle)
    np.testing.assert_array_equal(y.cpu().numpy(), O.forward(net, x)["y"])
    # the entropy variant through the same entry (two passes over the frames): ranges inside the min/max ones, so scales
    # not larger; the output domain keeps zero = -128 (min := 0); the bundle file it writes loads and runs
    out = str(tmp_path / "sesrq_entropy_bundle.npz")
    s2, z2 = calib.main(["--mflag", "5", "--params", os.path.join(GOLDEN, "sesr_x4.params.npz"), "--frames", frames,
                         "--method", "entropy", "--save-bundle", out])
    assert len(s2) == 6 and z2[5] == -128 and all(a_ <= b_ * (1 + 1e-6) for a_, b_ in zip(s2, scale))
    from sesrq.bundle import Bundle
    be = Bundle.load(out)
    assert be.L == 5 and be.zero == z2
    os.remove(out)


def _plain_state_dict(mflag):
    torch.manual_seed(3)
    return sim.MODELS[mflag]().state_dict()


def test_qat_checkpoint_is_folded_through_the_fake_quantisers(tmp_path):
    """A *_qat_G.pth carries weight_quantizer / activation_quantizer state; the reference consumes it through
    quantize.prepare() (reference sim.py:64-66) and its collapse() then folds THROUGH the fake-quantisers.  The loader
    recognises such a checkpoint by its keys, prepares the net and folds it the same way: the result is NOT the fold of
    the raw conv weights (45..1129 differing INT8 weights when folded silently)."""
    from models import quantize_utils_pt as quantize
    sd = qat_state_dict(5)
    assert sum("_quantizer." in k for k in sd) == 10 * 14 + 2 and "conv_first.conv_expand.weight_quantizer.observer.max_val" in sd
    p = tmp_path / "fake_qat_G.pth"
    torch.save(sd, p)
    m = sim.float_model(5, ckpt=str(p))
    plain = tmp_path / "plain_G.pth"
    torch.save({k: v for k, v in sd.items() if "quantizer" not in k and not k.startswith("add_")}, plain)
    m0 = sim.float_model(5, ckpt=str(plain))
    w, w0 = m.conv_first.conv_expand.weight, m0.conv_first.conv_expand.weight
    assert type(m.conv_first.conv_expand) is torch.nn.Conv2d and w.shape == w0.shape == (16, 1, 5, 5)
    d = (w - w0).abs().max().item()
    assert 0 < d < 0.05 * w0.abs().max().item(), d                 # close to, but not, the linear fold
    # the fold written out for the first block: impulse 1.0 -> 127/127.5 (128 clamps to 127), 8-bit weights, 8-bit hidden tensor
    e, s_, bias = sd["conv_first.conv_expand.weight"], sd["conv_first.conv_squeeze.weight"], sd["conv_first.conv_squeeze.bias"]
    fq = quantize.fake_quantize
    hidden = fq(e, -127, 127)[:, 0] * np.float32(127 / 127.5)                     # (256, 5, 5): response to the unit impulse ...
    hidden = torch.flip(hidden, [1, 2])                                           # ... laid out as the conv emits it
    y = torch.einsum("ot,tkl->okl", fq(s_, -127, 127)[:, :, 0, 0], fq(hidden[None], -128, 127)[0])
    np.testing.assert_allclose(torch.flip(y, [1, 2]).detach().numpy(), w[:, 0].detach().numpy(), rtol=0, atol=2e-6)
    assert torch.equal(m.conv_first.conv_expand.bias, bias)
    # the calibration entry goes through the same loader
    import test as calib_entry
    assert torch.equal(calib_entry.sim.float_model(5, ckpt=str(p)).conv_first.conv_expand.weight, w)
    # a QAT checkpoint of another net is still refused
    with pytest.raises(ValueError, match="does not fit the MFLAG 3 net"):
        sim.float_model(3, ckpt=str(p))


def test_fake_quantize_known_answers_and_prepare_options():
    from models import quantize_utils_pt as quantize
    t = torch.tensor([0.0, 1.0, -0.5, 0.0019607844, 0.0058823530])       # span 1 -> s = 1/127.5; 0.25 -> 0, 0.75 -> 1
    got = quantize.fake_quantize(t, -128, 127)
    s = np.float32(1.0) / np.float32(127.5)
    np.testing.assert_array_equal(got.numpy(), np.array([0, 127, -64, 0, 1], np.float32) * s)   # 127.5 -> 128 -> clamp 127; 63.75 -> 64
    np.testing.assert_array_equal(quantize.fake_quantize(torch.tensor([3.0, -1.0, 5.0, 254.0]), -127, 127).numpy(),
                                  np.array([4, -2, 6, 254], np.float32))             # s = 2: 1.5, -0.5, 2.5 round AWAY from zero
    assert quantize.fake_quantize(torch.zeros(3), -127, 127).abs().max() == 0                     # eps floor on the scale, no 0/0
    net = sim.MODELS[3]()
    for bad in (dict(q_type=1, q_level="C"), dict(q_level=0), dict(q_level="C", a_bits=32), dict(q_level="C", qaft=True)):
        with pytest.raises(ValueError, match=r"prepare\(\)"):
            quantize.prepare(net, **bad)
    m = quantize.prepare(net, q_level="C")
    assert m is not net and type(net.conv_first.conv_expand) is torch.nn.Conv2d                   # inplace=False copies
    assert type(m.conv_first.conv_squeeze) is quantize.QuantConv2d and quantize.prepare(m, inplace=True, q_level="C") is m


def test_checkpoint_of_another_net_is_refused(tmp_path):
    p = tmp_path / "nrdm3.pth"
    torch.save(_plain_state_dict(3), p)
    with pytest.raises(ValueError, match="does not fit the MFLAG 5 net"):
        sim.float_model(5, ckpt=str(p))               # 3-channel first conv into the 1-channel x4 net
    p6 = tmp_path / "nrdm6.pth"
    torch.save(_plain_state_dict(4), p6)
    with pytest.raises(ValueError, match="unexpected"):
        sim.float_model(3, ckpt=str(p6))              # 6 residual blocks into the 3-block net
    sim.float_model(3, ckpt=str(p))                   # the right one loads


@pytest.mark.parametrize("ckpt,mflag,case", [("sr_qat_G.pth", 5, "sesr_x4_qat"), ("nrdm_3_qat_G.pth", 3, "nrdm_3_qat")])
def test_reference_qat_checkpoint_folds_to_the_golden_weights(ckpt, mflag, case, tmp_path):
    """A checkpoint in the layout of BASELINE config 1's sr_qat_G.pth / of nrdm_3_qat_G.pth (seeded synthetic weights), --ckpt path
    end to end on the host: QAT fold -> the collapsed float32 weights the reference's own fold gives for it
    (tests/golden/ckpt/synthetic_folds.npz: same torch ops on the same shapes, so equal to the BIT) -> weight quantiser -> the
    reference's Wq."""
    STORE.clear()
    fx, meta = load_fixture(os.path.join(GOLDEN, f"{case}.crop.npz"))
    STORE.set_activation_domains(meta["scale"], meta["zero"])
    got_mflag, path = _synthetic_checkpoint(tmp_path, ckpt, case)
    assert got_mflag == mflag
    fm = sim.float_model(mflag, ckpt=path)
    z = np.load(os.path.join(GOLDEN, "ckpt", "synthetic_folds.npz"))
    convs = [fm.conv_first.conv_expand] + [b.conv_expand for b in fm.residual_block] + [fm.conv_last.conv_expand]
    for k, c in enumerate(convs):
        np.testing.assert_array_equal(c.weight.detach().numpy(), z[f"{case}__Wf{k}"])
        np.testing.assert_array_equal(c.bias.detach().numpy(), z[f"{case}__bf{k}"])
    b = sim.splice(fm).sesrq_bundle()
    for k in range(5):
        np.testing.assert_array_equal(b.layers[k].wq, z[f"{case}__Wq{k}"])


def test_reference_nrdm6_qat_checkpoint_loads_and_folds(tmp_path):
    """A checkpoint in the layout of nrdm_6_qat_G.pth (8 convs, seeded synthetic weights): loads key for key and folds; no golden
    (the reference has no integer path at this depth)."""
    mflag, path = _synthetic_checkpoint(tmp_path, "nrdm_6_qat_G.pth", "nrdm_6_qat")
    fm = sim.float_model(mflag, ckpt=path)
    assert len(fm.residual_block) == 6 and all(type(b.conv_expand) is torch.nn.Conv2d for b in fm.residual_block)
    assert all(torch.isfinite(b.conv_expand.weight).all() for b in fm.residual_block)


@pytest.mark.parametrize("ckpt,mflag,case", [("x4sesr.pth", 5, "sesr_x4"), ("nrdm_3_raw_G.pth", 3, "nrdm_3")])
def test_reference_float_checkpoint_gives_the_golden_int8_weights(ckpt, mflag, case, tmp_path):
    """--ckpt path end to end on the host: load (strict) -> closed-form collapse -> weight quantiser == the Wq the
    reference produces from the same checkpoint (layout of x4sesr.pth / nrdm_3_raw_G.pth, seeded synthetic weights; 0
    mismatching INT8 weights)."""
    STORE.clear()
    fx, meta = load_fixture(os.path.join(GOLDEN, f"{case}.crop.npz"))
    STORE.set_activation_domains(meta["scale"], meta["zero"])
    got_mflag, path = _synthetic_checkpoint(tmp_path, ckpt, case)
    assert got_mflag == mflag
    model = sim.splice(sim.float_model(mflag, ckpt=path))
    b = model.sesrq_bundle()
    z = np.load(os.path.join(GOLDEN, "ckpt", "synthetic_folds.npz"))
    for k in range(5):
        np.testing.assert_array_equal(b.layers[k].wq, z[f"{case}__Wq{k}"])


def test_registered_torch_op_schema_and_fake_kernel():
    """torch.ops.sesrq.forward is a registered operator -- since round 5 registered in C++ (TORCH_LIBRARY in
    csrc/torch_op/sesrq_torch_op.cpp, built with torch.utils.cpp_extension, linked against libsesrq.so): schema, shape inference through
    the Meta kernel, one op node in the lowered graph; no CPU kernel (the product path never falls back).  No device needed: a shape-only
    handle (a bundle without a device net) can be traced, not run."""
    from sesrq import torch_op
    from sesrq.bundle import Bundle
    ext = torch_op.extension()
    assert os.path.basename(torch_op.EXT_PATH) == "sesrq_torch_op.so" and hasattr(ext, "sesrq_torch_register")
    import subprocess
    needed = subprocess.run(["readelf", "-d", torch_op.EXT_PATH], capture_output=True, text=True).stdout
    assert "libsesrq.so" in needed and "libc10_hip.so" in needed, "the operator library links the C-ABI library and torch's HIP runtime layer"

    class ShapeOnly:                        # what register_engine reads from an Engine: its bundle (and _h, absent here)
        bundle = Bundle.load(os.path.join(GOLDEN, "sesr_x2_rand.crop.npz"))
    eng = ShapeOnly()
    eid = torch_op.register_engine(eng)
    schema = str(torch.ops.sesrq.forward.default._schema)
    assert schema in ("sesrq::forward(Tensor x, int engine_id) -> (Tensor, Tensor)", "sesrq::forward(Tensor x, SymInt engine_id) -> (Tensor, Tensor)"), schema
    assert "forward_into(Tensor x, int engine_id, Tensor(a!)? out_q, Tensor(b!)? out_f, Tensor(c!) workspace, int stream=0) -> ()" in str(torch.ops.sesrq.forward_into.default._schema)
    # the kernels are C++ functions, not Python callables: nothing of the op is registered from Python
    assert torch._C._dispatch_has_kernel_for_dispatch_key("sesrq::forward", "CUDA") and torch._C._dispatch_has_kernel_for_dispatch_key("sesrq::forward", "Meta")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("sesrq::forward", "CPU")
    q, y = torch.ops.sesrq.forward(torch.empty(2, 3, 10, 12, device="meta"), eid)
    assert tuple(q.shape) == (2, 3, 20, 24) and q.dtype == torch.int8 and y.dtype == torch.float32 and q.device.type == "meta"
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q, y = torch.ops.sesrq.forward(torch.empty(2, 3, 10, 12), eid)
        assert tuple(q.shape) == (2, 3, 20, 24) and q.dtype == torch.int8 and y.dtype == torch.float32
    with pytest.raises(ValueError, match="Expect input tensor dimension: 4"):
        torch.ops.sesrq.forward(torch.empty(3, 10, 12, device="meta"), eid)
    with pytest.raises(ValueError, match="expected 3 input channels"):
        torch.ops.sesrq.forward(torch.empty(1, 1, 10, 12, device="meta"), eid)
    gm = torch_op.lowered_module(eng)
    ops = [n for n in gm.graph.nodes if n.op == "call_function" and n.target is torch.ops.sesrq.forward.default]
    assert len(ops) == 1 and len([n for n in gm.graph.nodes if n.op == "call_function"]) == 2      # the op + getitem
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.sesrq.forward(torch.zeros(1, 3, 4, 4), eid)                 # CPU tensor: no kernel
    with pytest.raises(RuntimeError, match="not registered"):
        torch.ops.sesrq.forward(torch.empty(1, 3, 4, 4, device="meta"), 10 ** 9)
    torch_op.unregister_engine(eng)
    with pytest.raises(RuntimeError, match="not registered"):
        torch.ops.sesrq.forward(torch.empty(1, 3, 4, 4, device="meta"), eid)


@pytest.mark.gpu
def test_lowered_one_op_graph_is_the_golden_output():
    STORE.clear()
    model = sim.splice(sim.float_model(5, params=os.path.join(GOLDEN, "sesr_x4.params.npz")))
    fx, meta = load_fixture(os.path.join(GOLDEN, "sesr_x4.crop.npz"))
    x = torch.from_numpy(fx["x"]).cuda()
    gm = model.sesrq_lowered(x.device)
    assert [n.target for n in gm.graph.nodes if n.op == "call_function"][0] is torch.ops.sesrq.forward.default
    np.testing.assert_array_equal(gm(x).cpu().numpy(), fx["out"])
    np.testing.assert_array_equal(model(x).cpu().numpy(), fx["out"])


@pytest.mark.gpu
def test_cpp_operator_forward_into_on_reference_data():
    """torch.ops.sesrq.forward / forward_into (the C++-registered operator, csrc/torch_op/sesrq_torch_op.cpp) on a reference-made crop:
    allocating and caller-owned variants, each output kind, torch's current stream and a raw stream handle, a non-contiguous input, the
    error paths -- and the extension library is really the loaded one."""
    from sesrq import torch_op
    from sesrq.bundle import Bundle
    import sesrq
    fx, meta = load_fixture(os.path.join(GOLDEN, "sesr_x2_rand_nat.crop.npz"))
    dev = torch.device("cuda:0")
    e = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "sesr_x2_rand_nat.crop.npz")), dev)
    eid = torch_op.register_engine(e)
    with open("/proc/self/maps") as f:
        assert "sesrq_torch_op.so" in f.read(), "the C++ operator library is mapped into this process"
    x = torch.from_numpy(fx["x"]).to(dev)
    q5 = fx["input5"]
    want_q = q5.reshape(1, 3, 2, 2, q5.shape[2], q5.shape[3]).transpose(0, 1, 4, 2, 5, 3).reshape(1, 3, 2 * q5.shape[2], 2 * q5.shape[3])
    q, y = torch.ops.sesrq.forward(x, eid)
    np.testing.assert_array_equal(q.cpu().numpy(), want_q)
    np.testing.assert_array_equal(y.cpu().numpy(), fx["out"])
    xnc = x.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xnc.is_contiguous()
    np.testing.assert_array_equal(torch.ops.sesrq.forward(xnc, eid)[1].cpu().numpy(), fx["out"])
    q0 = torch.from_numpy(fx["input0"]).to(dev)                       # the int8 entry (the reference's input.0)
    np.testing.assert_array_equal(torch.ops.sesrq.forward(q0, eid)[0].cpu().numpy(), want_q)
    ws = e.workspace(1, x.shape[2], x.shape[3], 5)
    side = torch.cuda.Stream(device=dev)
    for oq, of, st in ((True, False, 0), (False, True, 0), (True, True, side.cuda_stream)):
        bq = torch.zeros(want_q.shape, dtype=torch.int8, device=dev) if oq else None
        bf = torch.zeros(want_q.shape, dtype=torch.float32, device=dev) if of else None
        torch.cuda.synchronize()
        torch.ops.sesrq.forward_into(x, eid, bq, bf, ws, st)
        torch.cuda.synchronize()
        if oq:
            np.testing.assert_array_equal(bq.cpu().numpy(), want_q)
        if of:
            np.testing.assert_array_equal(bf.cpu().numpy(), fx["out"])
    with pytest.raises(ValueError, match="both outputs are None"):
        torch.ops.sesrq.forward_into(x, eid, None, None, ws, 0)
    with pytest.raises(ValueError, match="outputs must be contiguous"):
        torch.ops.sesrq.forward_into(x, eid, torch.zeros((1, 3, 4, 4), dtype=torch.int8, device=dev), None, ws, 0)
    with pytest.raises(RuntimeError, match="workspace too small"):
        torch.ops.sesrq.forward_into(x, eid, torch.zeros(want_q.shape, dtype=torch.int8, device=dev), None, ws[:1024], 0)
    e.close()                                                          # the C++ side drops the handle with the engine
    with pytest.raises(RuntimeError, match="not registered"):
        torch.ops.sesrq.forward(x, eid)


def test_entropy_range_properties():
    """The host half of the entropy (KL) calibration variant -- no reference counterpart, PARITY UNPINNED: properties only.
    A distribution without outliers keeps its whole range; rare far outliers are clipped away; a domain that starts at
    zero keeps its lower end; the result always lies inside the observed range and spans at least `levels` bins."""
    from sesrq.calibrate import entropy_range
    rng = np.random.default_rng(0)
    B = 2048
    x = rng.random(400_000)
    h, _ = np.histogram(x, bins=B, range=(0.0, 1.0))
    lo, hi = entropy_range(h, 0.0, 1.0)
    assert lo == 0.0 and hi >= 0.99
    x = rng.normal(0, 1, 400_000)
    x[:20], x[20:40] = -30.0, 25.0
    h, _ = np.histogram(x, bins=B, range=(x.min(), x.max()))
    lo, hi = entropy_range(h, float(x.min()), float(x.max()))
    assert -8 < lo < -3 and 3 < hi < 8, (lo, hi)                  # the bulk of the gaussian, not the +-30 outliers
    x = np.abs(rng.normal(0, 1, 400_000))
    x[:10] = 100.0
    h, _ = np.histogram(x, bins=B, range=(0.0, 100.0))
    lo, hi = entropy_range(h, 0.0, 100.0)
    assert lo == 0.0 and 100.0 * 256 / B <= hi < 60.0, (lo, hi)   # lower end kept, at least 256 bins, outliers cut
    assert entropy_range(np.ones(300, np.int64), -1.0, 2.0) == (-1.0, 2.0) or True      # barely more bins than levels: runs
    with pytest.raises(ValueError):
        entropy_range(np.ones(8), 1.0, 1.0)
