"""CPU ORACLE (numpy) of the calibration pass -- TEST INFRASTRUCTURE ONLY, never on the product path.

An independent restatement of the reference's exe_mode 0 (test.py:79-113,141-217): the float net run with fake-quantised weights
and activations while the running min/max of every conv input is observed.  The shipped package never imports this file.

Two forms of the same arithmetic:

* fp32-faithful (`exact=False`): the definition csrc/sesrq_calib.hip implements, bit for bit.
    r      = clamp_b(rint(f32(f32(x / scale32) + zero32)))     fmaxf / fminf: a NaN input takes the lower clamp
    q      = r - zero                                         exact integer; 0 outside the frame
    acc_p  = sum_{ic = p mod 4, taps} Wq * q                  exact integer (PE p = 0..3, an empty PE sums to 0)
    v_p    = clamp(f32(acc_p) * ss, acc_lo, acc_hi)           fp32
    v      = clamp(((v_0 + v_1) + v_2) + v_3, add_lo, add_hi) + qbias[o], then ReLU, then + skip   fp32, in that order
* float64 (`exact=True`): the reference's mode-0 arithmetic evaluated in float64 -- fake-quantised activations (r - zero) * scale,
  weights Wq * sw, the PE sums, both clamps and the bias in float64 (myQL/quan_func.py:160-215 quantiser, :298-333 PE split and
  accumulator clamp, :395-460 bias and adder clamp).  The reference itself runs that in fp32 in oneDNN's order; float64 is the
  diagnosis yardstick between the two.

The domain of a batch (`domain`) follows the device's derive_domain (csrc/sesrq_calib.hip) and the host pass
(sesrq/calibrate.py, Calibrator._observe / observe); where the two could differ this module says which it follows:
  * zero is clamped to +-2^30 on both (the int the slot and the conv descriptor hold);
  * a constant batch (max == min) is the device's degenerate slot; the host pass asserts instead.
NaN in a quantiser input: the min/max reduction skips it (fminf / fmaxf; `minmax`), where torch.max would propagate it.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import sesrq_oracle as O

F32 = np.float32
ZERO_CLAMP = 1 << 30             # derive_domain: |zero| <= 2^30 (the int the slot holds)
PE = 4


# --------------------------------------------------------------------------- observer
def minmax(x: np.ndarray):
    """(min, max) of a quantiser input as fp32, NaN skipped (calib_minmax_kernel: fminf / fmaxf, INFINITY / -INFINITY start).
    An all-NaN tensor gives (inf, -inf).  The sign of a zero extremum is not pinned (compare with ==)."""
    a = np.asarray(x, F32).reshape(-1)
    a = a[~np.isnan(a)]
    if a.size == 0:
        return F32(np.inf), F32(-np.inf)
    return F32(a.min()), F32(a.max())


@dataclass
class Domain:
    """One quantiser input's domain for one batch: the fields of sesrq_calib_slot (csrc/sesrq_calib.hip derive_domain) and the
    constants the host pass passes in sesrq_calib_conv_desc (sesrq/calibrate.py observe)."""
    mn: float
    mx: float
    degenerate: bool
    scale: float                # fp64
    zero: int                   # clamped to +-2^30
    scale32: np.float32
    zero32: np.float32
    ss: np.float32              # f32(scale * sw)
    acc_lo: np.float32
    acc_hi: np.float32
    add_lo: np.float32
    add_hi: np.float32
    qbias: np.ndarray           # [oc] f32: clip(rint(f32 bias / ss)) * ss
    sw: float = 1.0
    bias: np.ndarray = field(default_factory=lambda: np.zeros(0, F32))     # [oc] the float bias
    bias_raw: np.ndarray = field(default_factory=lambda: np.zeros(0, F32))  # [oc] rint(f32 bias / ss) before the bias clamp
    acc_bits: int = 18
    add_bits: int = 20
    bias_bits: int = 16


def zero_point(mn: float, scale: float, b: int) -> int:
    """-2^(b-1) - round(min / scale) (test.py:189-215; Python's round is half to even), clamped to +-2^30 (derive_domain)."""
    z = -(1 << (b - 1)) - round(float(mn) / scale)
    return int(min(max(z, -ZERO_CLAMP), ZERO_CLAMP))


def domain(mn, mx, b: int, sw: float = 1.0, bias: Optional[np.ndarray] = None, acc_bits: int = 18, add_bits: int = 20,
           bias_bits: int = 16) -> Domain:
    """The domain of a batch whose quantiser input spans [mn, mx] (fp32 values), at width b, for a conv of weight scale sw."""
    mn, mx = float(F32(mn)), float(F32(mx))
    bias = np.zeros(0, F32) if bias is None else np.asarray(bias, F32)
    if not mx != mn:
        inf = F32(np.inf)
        return Domain(mn, mx, True, 0.0, 0, F32(1), F32(0), F32(1), -inf, inf, -inf, inf, np.zeros(len(bias), F32), sw, bias,
                      np.zeros(len(bias), F32), acc_bits, add_bits, bias_bits)
    scale = (mx - mn) / float((1 << b) - 1)                                      # quan_func.py:198
    zero = zero_point(mn, scale, b)                                              # quan_func.py:199
    ssd = scale * sw
    ss = F32(ssd)
    lo_a, hi_a = -(1 << (acc_bits - 1)), (1 << (acc_bits - 1)) - 1               # quan_func.py:326-333
    lo_s, hi_s = -(1 << (add_bits - 1)), (1 << (add_bits - 1)) - 1               # quan_func.py:431-434
    bound = lambda v: F32(((v - zero) * scale) * sw)                             # python float, left to right
    lo16, hi16 = F32(-(1 << (bias_bits - 1))), F32((1 << (bias_bits - 1)) - 1)  # quan_func.py:402-404
    raw = np.rint(bias / ss).astype(F32)
    bq = np.clip(raw, lo16, hi16).astype(F32)
    return Domain(mn, mx, False, scale, zero, F32(scale), F32(zero), ss, bound(lo_a), bound(hi_a), bound(lo_s), bound(hi_s),
                  (bq * ss).astype(F32), sw, bias, raw, acc_bits, add_bits, bias_bits)


# --------------------------------------------------------------------------- one conv
def codes(x: np.ndarray, d: Domain, b: int) -> np.ndarray:
    """clamp_b(rint(f32(x / scale32) + zero32)) as int64 (NaN -> the lower clamp, as fmaxf(NaN, lo) = lo)."""
    qlo, qhi = F32(-(1 << (b - 1))), F32((1 << (b - 1)) - 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = np.rint((np.asarray(x, F32) / d.scale32).astype(F32) + d.zero32)
    return np.fmin(np.fmax(t, qlo), qhi).astype(np.int64)


def _pe_sums(q: np.ndarray, wq: np.ndarray) -> np.ndarray:
    """Exact per-PE sums (PE, N, OC, H, W) as float64 integers of q (N, IC, H, W) int64 (0 = outside the frame: padded here) and
    wq (OC, IC, K, K).  float64 products and sums are exact while every partial sum stays below 2^53: |q| <= 2^30 + 2^7, |Wq| <= 2^7
    and at most 4 x 25 taps per PE keep them below 2^45."""
    N, IC, H, W = q.shape
    OC, _, K, _ = wq.shape
    R = K // 2
    qp = np.zeros((N, IC, H + 2 * R, W + 2 * R), np.float64)
    qp[:, :, R:R + H, R:R + W] = q
    w = wq.astype(np.float64)
    acc = np.zeros((PE, N, OC, H, W), np.float64)
    for p in range(PE):
        cs = list(range(p, IC, PE))
        if not cs:
            continue
        for ky in range(K):
            for kx in range(K):
                acc[p] += np.einsum("oc,nchw->nohw", w[:, cs, ky, kx], qp[:, cs, ky:ky + H, kx:kx + W], optimize=True)
    assert np.abs(acc).max(initial=0) < 2.0 ** 53
    return acc


@dataclass
class Fired:
    """Which clamps fired in one conv (for tests that must exercise them)."""
    pe: bool = False
    add: bool = False
    bias: bool = False


def conv(x: np.ndarray, wq: np.ndarray, d: Domain, b: int, relu: bool, skip: Optional[np.ndarray] = None, exact: bool = False,
         fired: Optional[Fired] = None, override=None) -> np.ndarray:
    """One calibration conv: x (N, IC, H, W) fp32 in the domain d -> (N, OC, H, W) (fp32; float64 with exact=True).
    override: (index, codes) -- these input codes r taken as given instead of computed (diagnosis of a reference run)."""
    wq = np.asarray(wq)
    if exact:
        return _conv_exact(x, wq, d, b, relu, skip)
    r = codes(x, d, b)
    if override is not None:
        r[override[0]] = override[1]
    q = r - d.zero
    acc = _pe_sums(q, wq)
    with np.errstate(over="ignore", invalid="ignore"):
        v = [np.fmin(np.fmax(acc[p].astype(F32) * d.ss, d.acc_lo), d.acc_hi) for p in range(PE)]
        s = v[0]
        for p in range(1, PE):
            s = (s + v[p]).astype(F32)
        pre = s
        s = np.fmin(np.fmax(s, d.add_lo), d.add_hi)
        out = (s + d.qbias[None, :, None, None]).astype(F32)
        if relu:
            out = np.fmax(out, F32(0))
        if skip is not None:
            out = (out + np.asarray(skip, F32)).astype(F32)
    if fired is not None:
        fired.pe |= any(bool(np.any((acc[p].astype(F32) * d.ss < d.acc_lo) | (acc[p].astype(F32) * d.ss > d.acc_hi)))
                        for p in range(PE))
        fired.add |= bool(np.any((pre < d.add_lo) | (pre > d.add_hi)))
        lo16, hi16 = -(1 << (d.bias_bits - 1)), (1 << (d.bias_bits - 1)) - 1
        fired.bias |= bool(np.any((d.bias_raw < lo16) | (d.bias_raw > hi16)))
    return out


def _conv_exact(x, wq, d: Domain, b: int, relu: bool, skip):
    """The reference's mode-0 conv in float64 (see the module docstring)."""
    qlo, qhi = -(1 << (b - 1)), (1 << (b - 1)) - 1
    r = np.clip(np.rint(np.asarray(x, np.float64) / d.scale + d.zero), qlo, qhi)
    xf = (r - d.zero) * d.scale                                                  # quan_func.py:215
    N, IC, H, W = xf.shape
    OC, _, K, _ = wq.shape
    R = K // 2
    xp = np.zeros((N, IC, H + 2 * R, W + 2 * R), np.float64)
    xp[:, :, R:R + H, R:R + W] = xf
    w = wq.astype(np.float64) * d.sw
    scale, sw = d.scale, d.sw
    lo_a, hi_a = bounds64(d, d.acc_bits)
    lo_s, hi_s = bounds64(d, d.add_bits)
    s = np.zeros((N, OC, H, W))
    for p in range(PE):
        acc = np.zeros((N, OC, H, W))
        cs = list(range(p, IC, PE))
        for ky in range(K):
            for kx in range(K):
                if cs:
                    acc += np.einsum("oc,nchw->nohw", w[:, cs, ky, kx], xp[:, cs, ky:ky + H, kx:kx + W], optimize=True)
        s += np.clip(acc, lo_a, hi_a)
    s = np.clip(s, lo_s, hi_s)
    bs = scale * sw
    lo16, hi16 = -(1 << (d.bias_bits - 1)), (1 << (d.bias_bits - 1)) - 1
    bq = np.clip(np.rint(np.asarray(d.bias, np.float64) / bs), lo16, hi16)
    out = s + (bq * bs)[None, :, None, None]
    if relu:
        out = np.maximum(out, 0.0)
    if skip is not None:
        out = out + skip
    return out


def bounds64(d: Domain, bits: int):
    """The float64 clamp bounds of a bits-wide accumulator in the domain d, before the fp32 rounding (quan_func.py:326-333)."""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return ((lo - d.zero) * d.scale) * d.sw, ((hi - d.zero) * d.scale) * d.sw


# --------------------------------------------------------------------------- the whole pass
@dataclass
class Pass:
    """The state Calibrator leaves after a run over `frames`: running extrema, the last batch's (scale, zero), the per-batch domains
    and outputs (the mode-0 return value, pixel-shuffled when ps > 1)."""
    run_min: List[float]
    run_max: List[float]
    last_scale: List[float]
    last_zero: List[int]
    domains: List[List[Domain]]      # [batch][quantiser]
    outputs: List[np.ndarray]        # [batch]
    inputs: List[List[np.ndarray]] = field(default_factory=list)    # [batch][quantiser] with keep_inputs


def quantize(weights: Sequence[np.ndarray], b: int):
    """[(Wq, sw)] of float convs at width b (oracle.sesrq_oracle.quantize_weight, quan_func.py:58-71)."""
    return [O.quantize_weight(w, b) for w in weights]


def forward(weights, biases, ps: int, frames: Sequence[np.ndarray], b: int, exact: bool = False, quantized=None,
            acc_bits: int = 18, add_bits: int = 20, bias_bits: int = 16, keep_outputs: bool = True, keep_inputs: bool = False,
            override=None) -> Pass:
    """The calibration pass over `frames` (each (N, C, H, W) fp32, one batch each), as Calibrator.observe / enqueue run it:
    per batch, each quantiser input's domain from this batch's extrema; the running extrema folded across batches (a strictly larger
    max / smaller min replaces); the long skip a_{L-2} += a_0; the last quantiser (in front of PixelShuffle when ps > 1, else the
    last conv's output) observed, and for ps > 1 the fake-quantised output pixel-shuffled.
    override: {k: (index, codes)} -- codes of quantiser input k (k < L) taken as given in every batch (fp32 form only)."""
    qw = quantized if quantized is not None else quantize(weights, b)
    L = len(qw)
    run_min: List[Optional[float]] = [None] * (L + 1)
    run_max: List[Optional[float]] = [None] * (L + 1)
    last_scale, last_zero = [None] * (L + 1), [None] * (L + 1)
    doms, outs, ins = [], [], []

    def observe(k, t):
        if exact:                  # float64 extrema; domain() takes them as the fp32 values .item() of an fp32 tensor would give
            a = np.asarray(t, np.float64)
            mn, mx = float(a.min()), float(a.max())
        else:
            mn, mx = (float(v) for v in minmax(t))
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
            d = domain(mn, mx, b, sw, biases[k], acc_bits, add_bits, bias_bits)
            bd.append(d)
            last_scale[k], last_zero[k] = d.scale, d.zero
            skip = first if k == L - 2 else None
            a = conv(a, wq, d, b, relu=k != L - 1, skip=skip, exact=exact, override=(override or {}).get(k))
            if k == 0:
                first = a
        mn, mx = observe(L, a)
        bi.append(a)
        d = domain(mn, mx, b, 1.0, None, acc_bits, add_bits, bias_bits)
        bd.append(d)
        last_scale[L], last_zero[L] = d.scale, d.zero
        doms.append(bd)
        if keep_inputs:
            ins.append(bi)
        if keep_outputs:
            if ps > 1:
                outs.append(O.pixel_shuffle(fakequant(a, d, b, exact), ps))
            else:
                outs.append(a)
    return Pass(run_min, run_max, last_scale, last_zero, doms, outs, ins)


def fakequant(a: np.ndarray, d: Domain, b: int, exact: bool = False) -> np.ndarray:
    """The quantiser in front of PixelShuffle: (r - zero32) * scale32 in fp32 (calib_fakequant_kernel); float64 with exact=True."""
    if exact:
        qlo, qhi = -(1 << (b - 1)), (1 << (b - 1)) - 1
        return (np.clip(np.rint(np.asarray(a, np.float64) / d.scale + d.zero), qlo, qhi) - d.zero) * d.scale
    r = codes(a, d, b).astype(F32)
    return ((r - d.zero32).astype(F32) * d.scale32).astype(F32)
