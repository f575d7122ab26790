"""The QUAN_BIT = b < 8 integer path (dot4 kernels, sesrq_create_q) against the width-aware oracles, at every width 2..7.

tests/test_quan_bits.py pins the path to reference-made fixtures; these tests reach what those fixtures do not: ragged shapes across
the dot4 tile edges and batches, saturating PEs, zero points below -128 and between -128 and -2^(b-1) (the pad value max(z, -128)
lies outside the activation range there), the input quantiser's edges in each division mode, int8 q0 outside the width, the x2
anchor add, full frames, and the calibration pass's fake-quantiser.  Bar: bit-exact on the int8 q and the fp32 y."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_fixture
from helpers import bundle_from_oracle, device, rand_frame, same
from planner import expected_plan_and_engines
from topologies import RAGGED_FRAMES as SIZES
from oracle import sesrq_oracle as O
import sesrq
from sesrq import _lib

pytestmark = pytest.mark.gpu

WIDTHS = list(range(2, 8))
QB = os.path.join(GOLDEN, "quan_bits")


def _engine(net, **kw):
    e = sesrq.Engine(bundle_from_oracle(net), device(), **kw)
    assert e.quan_bits == net.quan_bits and all(n.endswith(f"-q{net.quan_bits}") for n in e.layer_engines()), e.layer_engines()
    plan, names = expected_plan_and_engines(net, fast_division=e.fast_division_proven(), **kw)
    assert e.launch_plan() == plan and e.layer_engines() == names, (net.name, kw, e.launch_plan(), plan, e.layer_engines(), names)
    return e


def _run(e, x, **kw):
    q, y = e.forward(torch.from_numpy(np.ascontiguousarray(x)).to(device()), **kw)
    return q.cpu().numpy(), y.cpu().numpy()


@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("kind", ["sesr_x4", "sesr_x2", "nrdm"])
def test_synthetic_nets_at_the_width_vs_oracle(kind, b):
    """plain and hard nets, two seeds, merged and forced-general kernels, the ragged SIZES (1 x 1 .. 40 x 129, N up to 3).  The oracle's
    own stages prove the branches are live: some activation at qlo and some at qhi, and from b = 6 on a hard net's raw PE sum beyond
    the 18-bit range."""
    for hard in (False, True):
        for seed in range(2):
            net = O.synth_net(kind, seed, hard=hard, quan_bits=b)
            engines = [_engine(net, force_general=fg) for fg in (False, True)]
            if hard and b >= 6:
                assert any("general" in n for n in engines[0].layer_engines()), engines[0].layer_engines()
            cin = net.layers[0].wq.shape[1]
            lo = hi = sat = False
            for (N, H, W) in SIZES:
                x = rand_frame((N, cin, H, W), 1000 * seed + H * W + b)
                want = O.forward(net, x, keep=True)
                acts = [want[f"input{k}"] for k in range(1, net.L + 1)]
                lo |= any(bool((a == net.qlo).any()) for a in acts)
                hi |= any(bool((a == net.qhi).any()) for a in acts)
                sat |= any(bool(((want[f"pe_raw{k}"] > (1 << 17) - 1) | (want[f"pe_raw{k}"] < -(1 << 17))).any()) for k in range(net.L))
                for fg, e in zip((False, True), engines):
                    q, y = _run(e, x)
                    tag = f"{net.name} general={fg} {N}x{H}x{W}"
                    same(f"{tag} q_out", q, want["q_out"])
                    same(f"{tag} y", y, want["y"])
            assert lo and hi, (net.name, lo, hi)
            if hard and b >= 6:
                assert sat, f"{net.name}: no PE sum beyond 18 bits"


def _sweep_values(b):
    qlo, qhi = -(1 << (b - 1)), (1 << (b - 1)) - 1
    return [qlo, qlo + 1, qhi, (qlo - 128) // 2, -128, -129, -200]


@pytest.mark.parametrize("b", WIDTHS)
def test_zero_point_sweep_at_the_width(b):
    """zero[k] of one domain at a time through qlo, qlo + 1, qhi, a value in (-128, qlo), -128, -129, -200: the pad value
    max(z, -128) on both sides of the literal, outside the activation range, and both residual layouts (zero[1] == qlo or not)."""
    base = O.synth_net("sesr_x2", 10 + b, quan_bits=b)
    assert -128 < _sweep_values(b)[3] < base.qlo
    x = rand_frame((2, 3, 11, 37), 77 + b)
    seps = set()
    for k in range(base.L + 1):
        for z in _sweep_values(b):
            net = copy.deepcopy(base)
            net.zero[k] = z
            e = _engine(net, engine=_lib.ENGINE_DOT4)
            want = O.forward(net, x)
            q, y = _run(e, x)
            same(f"b={b} zero[{k}]={z} q_out", q, want["q_out"])
            same(f"b={b} zero[{k}]={z} y", y, want["y"])
            if k == 1:
                seps.add(e.workspace(1, 8, 8).numel())
    assert len(seps) == 2          # zero[1] == qlo: layer 0's output is the residual operand; otherwise a separate one


def _edge_frame(net, rng):
    """x / s0 + z0 at qlo - .5 and qhi + .5 and one ulp either side, every rint tie across the range, negative, huge and inf inputs."""
    s0, z0 = np.float32(net.scale[0]), net.zero[0]
    x = rng.random((1, 3, 16, 96), dtype=np.float32)
    ties = ((np.arange(net.qlo - 3, net.qhi + 4, dtype=np.float64) + 0.5 - z0) * float(s0)).astype(np.float32)
    ends = ((np.array([net.qlo - 0.5, net.qhi + 0.5], np.float64) - z0) * float(s0)).astype(np.float32)
    row = np.concatenate([ends, np.nextafter(ends, np.float32(np.inf)), np.nextafter(ends, np.float32(-np.inf)), ties,
                          np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    assert row.size <= 3 * 96 * 2
    flat = x[0, :, 0:2, :].reshape(-1)
    flat[:row.size] = row
    x[0, :, 0:2, :] = flat.reshape(3, 2, 96)
    x[0, 0, 3, :12] = np.array([0.0, -0.0, -1.0, -0.25, 1e-42, -1e-42, 3.0e38, -3.0e38, np.inf, -np.inf, 123456.0, -65504.0], np.float32)
    x[0, 1, 4:6, :] = -rng.random((2, 96), dtype=np.float32)
    x[0, 2, 6, :] = rng.random(96, dtype=np.float32) * np.float32(1e6)
    return x


@pytest.mark.parametrize("b", WIDTHS)
def test_input_quantiser_edges_in_every_division_mode(b):
    """q0 = clamp_b(rint(x / s0 + z0)) at exact_div = 0 (default), 1 (the quotient forced) and 2 (x * fl(1/s0), vs
    quantize_input(reciprocal=True)); the proof of the 3-instruction form holds where the 8-bit test finds it."""
    rng = np.random.default_rng(b)
    for s0, z0 in ((0.0039, None), (1.0 / 255.0, -150)):
        net = O.synth_net("nrdm", 20 + b, quan_bits=b)
        net.scale[0] = s0
        if z0 is not None:
            net.zero[0] = z0
        x = _edge_frame(net, rng)
        xt = torch.from_numpy(x).to(device())
        q0 = O.quantize_input(x, net.scale[0], net.zero[0], quan_bits=b)
        q0r = O.quantize_input(x, net.scale[0], net.zero[0], reciprocal=True, quan_bits=b)
        assert (q0 == net.qlo).any() and (q0 == net.qhi).any()
        want = O.forward(net, x)
        for mode, kw in ((0, {}), (1, dict(exact_division=True)), (2, dict(reciprocal_division=True))):
            e = _engine(net, **kw)
            assert e.exact_div == mode
            same(f"b={b} s0={s0} exact_div={mode} input0", e.forward_debug(xt, pe=False)["input0"], q0r if mode == 2 else q0)
            q, y = e.forward(xt)
            if mode == 2:
                q_want, y_want = _run(_engine(net), q0r)      # an int8 frame is q0
                same(f"b={b} exact_div=2 q_out vs oracle", q, O.forward(net, q0r)["q_out"])
            else:
                q_want, y_want = want["q_out"], want["y"]
            same(f"b={b} s0={s0} exact_div={mode} q_out", q, q_want)
            same(f"b={b} s0={s0} exact_div={mode} y", y, y_want)
    # the (scale, zero) pairs test_fast_division_is_proven_and_equals_exact_division finds proven at b = 8
    pairs = [(O.synth_net("sesr_x2", 1).scale[0], O.synth_net("sesr_x2", 1).zero[0])]
    for tag in ("sesr_x4", "nrdm_3", "sesr_x2_rand"):
        m = load_fixture(os.path.join(GOLDEN, f"{tag}.crop.npz"))[1]
        pairs.append((m["scale"][0], m["zero"][0]))
    for s0, z0 in pairs:
        net = O.synth_net("sesr_x2", 1, quan_bits=b)
        net.scale[0], net.zero[0] = s0, min(z0, net.qhi)
        assert _engine(net).fast_division_proven(), (b, s0, z0)


@pytest.mark.parametrize("b", WIDTHS)
def test_int8_q0_beyond_the_width_is_clamped(b):
    """An int8 frame is q0; codes outside [qlo, qhi] (the whole int8 range) give the oracle's result from the clamped q0."""
    rng = np.random.default_rng(30 + b)
    for kind, hard in (("sesr_x4", False), ("nrdm", True)):
        net = O.synth_net(kind, b, hard=hard, quan_bits=b)
        cin = net.layers[0].wq.shape[1]
        q0 = rng.integers(-128, 128, size=(2, cin, 13, 45)).astype(np.int8)
        q0[0, 0, 0, :] = np.rint(np.linspace(-128, 127, 45)).astype(np.int8)
        assert (q0 < net.qlo).any() and (q0 > net.qhi).any()
        want = O.forward(net, np.clip(q0, net.qlo, net.qhi).astype(np.int8))
        for fg in (False, True):
            q, y = _run(_engine(net, force_general=fg), q0)
            same(f"{net.name} general={fg} q_out", q, want["q_out"])
            same(f"{net.name} general={fg} y", y, want["y"])


@pytest.mark.parametrize("b", WIDTHS)
def test_x2_anchor_add_at_the_width(b):
    net = O.synth_net("sesr_x2", 3, quan_bits=b)
    e = _engine(net, anchor_add=True)
    x = rand_frame((2, 3, 37, 70), 12 + b)
    q, y = _run(e, x)
    want = O.forward(net, x)
    same("int8 output unaffected", q, want["q_out"])
    same("y + upsampled input", y, want["y"] + np.repeat(np.repeat(x, 2, axis=2), 2, axis=3))
    with pytest.raises(RuntimeError, match="anchor"):
        e.forward(torch.from_numpy(O.quantize_input(x, net.scale[0], net.zero[0], quan_bits=b)).to(device()))


@pytest.mark.parametrize("case,shape", [("nrdm_3.q3", (1, 3, 540, 960)), ("nrdm_3.q5", (1, 3, 540, 960)),
                                        ("sesr_x2_rand.q7", (1, 3, 1080, 1920))])
def test_full_frame_at_an_odd_width_vs_c_oracle(case, shape):
    from oracle import c_oracle as CO
    fx, _ = load_fixture(os.path.join(QB, f"{case}.crop.npz"))
    net = O.net_from_fixture(fx)
    x = rand_frame(shape, 5 + net.quan_bits)
    want = CO.forward(net, x, threads=16)
    q, y = _run(_engine(net), x)
    same(f"{case} q_out", q, want["q_out"])
    same(f"{case} y", y, want["y"])


def _fakequant_ref(x, scale, zero, b):
    """The kernel's definition in fp32: q = clip(rint(f32(x / s) + z)), out = f32((q - z) * s)."""
    s, z = np.float32(scale), np.float32(zero)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.clip(np.rint((x / s) + z), np.float32(-(1 << (b - 1))), np.float32((1 << (b - 1)) - 1))
        return ((q - z) * s).astype(np.float32)


def _fq_input(n, scale, zero, b, rng):
    s = np.float32(scale)
    x = (rng.standard_normal(n) * 40.0 * float(s)).astype(np.float32)
    k = np.arange(-(1 << (b - 1)) - 3, (1 << (b - 1)) + 3, dtype=np.float64)
    ties = ((k + 0.5 - zero) * float(s)).astype(np.float32)
    row = np.concatenate([ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf)),
                          np.array([0.0, -0.0, -1.0, 1e-42, 3.0e38, -3.0e38, 1e6, -1e6], np.float32)])
    x[:row.size] = row
    return x


@pytest.mark.parametrize("b", list(range(2, 9)))
def test_calibration_fake_quantiser_at_the_width(b):
    """sesrq_calib_fakequant_q bit for bit with its fp32 definition (ties, negatives, huge values, n not a multiple of 256), and
    sesrq_calib_fakequant_slot's pixel-shuffled store (r = 1, 2, 4) with the slot's f32(scale) and zero."""
    lib = _lib.lib()
    dev = device()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(40 + b)
    for scale, zero in ((0.0173, -(1 << (b - 1))), (0.0041, 0), (0.25, -200), (3.0e-3, (1 << (b - 1)) - 1)):
        n = 1000 + 257
        x = _fq_input(n, scale, zero, b, rng)
        xt = torch.from_numpy(x).to(dev)
        out = torch.full_like(xt, float("nan"))
        _lib.check(lib.sesrq_calib_fakequant_q(xt.data_ptr(), out.data_ptr(), n, float(np.float32(scale)), zero, b, st))
        same(f"fakequant_q b={b} s={scale} z={zero}", out, _fakequant_ref(x, scale, zero, b), values=True)
        for r, N, Cc, H, W in ((1, 1, 3, 9, 31), (2, 2, 8, 7, 13), (4, 1, 32, 5, 11)):
            a = _fq_input(N * Cc * H * W, scale, zero, b, rng).reshape(N, Cc, H, W)
            slot = (_lib.CalibSlot * 1)()
            _lib.check(lib.sesrq_calib_slots_init(slot, 1))
            slot[0].scale32 = float(np.float32(scale))
            slot[0].zero32 = float(zero)
            sl = torch.frombuffer(bytearray(bytes(slot)), dtype=torch.uint8).to(dev)
            at = torch.from_numpy(a).to(dev)
            o = torch.full((N, Cc // (r * r), H * r, W * r), float("nan"), dtype=torch.float32, device=dev)
            _lib.check(lib.sesrq_calib_fakequant_slot(at.data_ptr(), o.data_ptr(), N, Cc, H, W, r, sl.data_ptr(), b, st))
            same(f"fakequant_slot b={b} r={r}", o, O.pixel_shuffle(_fakequant_ref(a, scale, zero, b), r), values=True)
    torch.cuda.synchronize()
