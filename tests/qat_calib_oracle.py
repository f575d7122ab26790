"""CPU ORACLE (numpy) of the calibration pass of a QAT net -- TEST INFRASTRUCTURE ONLY, never on the product path.

quantize.prepare() replaces the long skip's AddOp of a QAT net by a fake-quantising QuantAdd (reference
models/quantize_utils_pt.py:654-711), so the reference's mode-0 pass adds two quantised tensors between conv L-2 and quantiser L-1.
test.py traces the prepared model while it is in training mode and buffers are not proxied: the union of the two observers' ranges
and update_qparams run at trace time, on the observer state the checkpoint holds, and the scale is a constant of the graph.

    lo = min(observer_res.min_val, observer_shortcut.min_val);  hi = max(observer_res.max_val, observer_shortcut.max_val)
    s  = max(f32(max(|lo|, |hi|)) / f32(127.5), eps_f32)                       a_bits = 8 (test.py:62), whatever QUAN_BIT is
    fq(t) = clamp(sign(t / s) * floor(|t / s| + 0.5), -128, 127) * s           round half away from zero (Round, :150-166)
    x_{L-1} = fq(relu(conv_{L-2} output)) + fq(conv_0 output)

The pass is oracle.calib_oracle.forward with that merge in place of the float add, built from that module's public functions
(minmax, domain, conv with skip=None, fakequant).  Two forms, as there:
  * fp32-faithful (`exact=False`): what csrc/sesrq_calib.hip's calib_conv_qadd_kernel computes, bit for bit -- every step a single fp32
    operation in the order written above; fmaxf / fminf clamps (a NaN takes the lower clamp);
  * float64 (`exact=True`): the same arithmetic in float64 at the fp32 scale s.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from oracle import calib_oracle as CO
from oracle import sesrq_oracle as O

F32 = np.float32
EPS = F32(np.finfo(np.float32).eps)
OBSERVERS = ("observer_res.min_val", "observer_res.max_val", "observer_shortcut.min_val", "observer_shortcut.max_val")


def skip_scale(res_min, res_max, shortcut_min, shortcut_max) -> np.float32:
    """The QuantAdd's constant scale from the four observer extrema (fp32, as the reference forms it)."""
    lo = min(F32(res_min), F32(shortcut_min))
    hi = max(F32(res_max), F32(shortcut_max))
    return max(F32(F32(max(abs(lo), abs(hi))) / F32(127.5)), EPS)


def skip_fakequant(t: np.ndarray, s, exact: bool = False) -> np.ndarray:
    """fq(t) at scale s (fp32): 8-bit symmetric, round half away from zero."""
    s = F32(s)
    if exact:
        u = np.asarray(t, np.float64) / np.float64(s)
        r = np.floor(np.abs(u) + 0.5)
        return np.clip(np.where(u < 0, -r, r), -128.0, 127.0) * np.float64(s)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (np.asarray(t, F32) / s).astype(F32)
        r = np.floor((np.abs(u) + F32(0.5)).astype(F32))
        q = np.fmin(np.fmax(np.where(u < 0, -r, r).astype(F32), F32(-128)), F32(127))
        return (q * s).astype(F32)


def merge(res: np.ndarray, shortcut: np.ndarray, s, exact: bool = False) -> np.ndarray:
    """The QuantAdd: fq(res) + fq(shortcut)."""
    a, b = skip_fakequant(res, s, exact), skip_fakequant(shortcut, s, exact)
    return a + b if exact else (a + b).astype(F32)


def forward(weights, biases, ps: int, frames: Sequence[np.ndarray], b: int, skip_s, exact: bool = False, quantized=None,
            acc_bits: int = 18, add_bits: int = 20, bias_bits: int = 16, keep_outputs: bool = True,
            keep_inputs: bool = False) -> CO.Pass:
    """oracle.calib_oracle.forward with the long skip merged through the QuantAdd at scale skip_s: per batch each quantiser input's
    domain from the batch's extrema, the running extrema folded across batches, x_{L-1} = fq(a_{L-2}) + fq(a_0)."""
    qw = quantized if quantized is not None else CO.quantize(weights, b)
    L = len(qw)
    run_min: List[Optional[float]] = [None] * (L + 1)
    run_max: List[Optional[float]] = [None] * (L + 1)
    last_scale, last_zero = [None] * (L + 1), [None] * (L + 1)
    doms, outs, ins = [], [], []

    def observe(k, t):
        if exact:
            a = np.asarray(t, np.float64)
            mn, mx = float(a.min()), float(a.max())
        else:
            mn, mx = (float(v) for v in CO.minmax(t))
        if run_max[k] is None or run_max[k] < mx:
            run_max[k] = mx
        if run_min[k] is None or run_min[k] > mn:
            run_min[k] = mn
        return mn, mx

    for x in frames:
        a = np.asarray(x, F32)
        first = None
        bd, bi = [], []
        for k in range(L):
            wq, sw = qw[k]
            mn, mx = observe(k, a)
            bi.append(a)
            d = CO.domain(mn, mx, b, sw, biases[k], acc_bits, add_bits, bias_bits)
            bd.append(d)
            last_scale[k], last_zero[k] = d.scale, d.zero
            a = CO.conv(a, wq, d, b, relu=k != L - 1, skip=None, exact=exact)
            if k == L - 2:
                a = merge(a, first, skip_s, exact)
            if k == 0:
                first = a
        mn, mx = observe(L, a)
        bi.append(a)
        d = CO.domain(mn, mx, b, 1.0, None, acc_bits, add_bits, bias_bits)
        bd.append(d)
        last_scale[L], last_zero[L] = d.scale, d.zero
        doms.append(bd)
        if keep_inputs:
            ins.append(bi)
        if keep_outputs:
            outs.append(O.pixel_shuffle(CO.fakequant(a, d, b, exact), ps) if ps > 1 else a)
    return CO.Pass(run_min, run_max, last_scale, last_zero, doms, outs, ins)


def qat_state_dict(mflag, add=None):
    """A synthetic state_dict shaped like the reference's *_qat_G.pth (seeded): conv weights + the buffers of both quantisers of every
    conv + the QuantAdd state of the long-skip adds.  add: the add_residual.* observer extrema and stored scale of a checkpoint record
    (tests/golden/qat_add.json); None leaves both adds with a unit scale."""
    import sim
    import torch
    from models import quantize_utils_pt as quantize
    torch.manual_seed(4)
    sd = dict(quantize.prepare(sim.MODELS[mflag](), a_bits=8, w_bits=8, q_type=0, q_level="C").state_dict())
    for name in ("add_residual", "add_upsampled_input"):
        sd[f"{name}.activation_quantizer.scale"] = torch.ones(1)
        sd[f"{name}.observer_res.min_val"] = torch.zeros(1)
    if add is not None:
        for k in OBSERVERS:
            sd["add_residual." + k] = torch.tensor([add[k]], dtype=torch.float32)
        sd["add_residual.activation_quantizer.scale"] = torch.tensor([add["stored_scale"]], dtype=torch.float32)
        sd["add_residual.activation_quantizer.observer.max_val"] = torch.tensor([add["observer_res.max_val"]], dtype=torch.float32)
    return sd
