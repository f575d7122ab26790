"""Parameter bundle: the in-memory replacement of the reference's CWD-relative ``output_pt/``
tree.  Pure data + the load-time derivation, which calls the host-scalar
entry points of libsesrq.so (sesrq_quantize_weight / sesrq_add_const / sesrq_requant_const /
sesrq_calib_scale_zero) so that Python never re-implements the arithmetic."""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib


@dataclass
class LayerParams:
    wq: np.ndarray          # (OC, IC, k, k) int8   conv.weight.K.pt
    add_const: np.ndarray   # (OC,) int32           conv.bias.quanK.pt
    M: int                  # requan_K_K+1.pt
    n: int                  # n_K_K+1.pt
    relu: bool = True
    w_scale: float = 0.0    # conv.weight.K.scale.pt (informational once M/n are derived)
    # per-OUTPUT-CHANNEL requant constants (sesrq_layer_desc.M_oc / n_oc) or None = the reference's per-tensor (M, n).  No reference counterpart
    # (its weight quantiser is per tensor): parity unpinned; such a layer runs on the dot4 kernels
    M_oc: Optional[np.ndarray] = None
    n_oc: Optional[np.ndarray] = None


@dataclass
class Bundle:
    layers: List[LayerParams]
    scale: List[float]      # input.K.scale.pt, K = 0..L
    zero: List[int]         # input.K.zero.pt,  K = 0..L
    M_res: int
    n_res: int
    pixel_shuffle: int = 1
    pe_num: int = 4
    pe_acc_bits: int = 18
    pe_add_bits: int = 20
    name: str = ""
    quan_bits: int = 8      # define.py QUAN_BIT: width of weights and activations (sesrq_create_q)

    @property
    def L(self) -> int:
        return len(self.layers)

    @property
    def in_channels(self) -> int:
        return int(self.layers[0].wq.shape[1])

    @property
    def out_channels(self) -> int:
        return int(self.layers[-1].wq.shape[0]) // (self.pixel_shuffle ** 2)

    # ---- (de)serialisation: one .npz instead of ~40 output_pt files
    def save(self, path: str) -> None:
        meta = dict(scale=self.scale, zero=self.zero, M=[l.M for l in self.layers], n=[l.n for l in self.layers],
                    relu=[bool(l.relu) for l in self.layers], w_scale=[l.w_scale for l in self.layers],
                    M_res=self.M_res, n_res=self.n_res, pixel_shuffle=self.pixel_shuffle, pe_num=self.pe_num,
                    pe_acc_bits=self.pe_acc_bits, pe_add_bits=self.pe_add_bits, name=self.name, quan_bits=self.quan_bits)
        arrs = {f"Wq{k}": l.wq for k, l in enumerate(self.layers)}
        arrs.update({f"add_const{k}": l.add_const for k, l in enumerate(self.layers)})
        for k, l in enumerate(self.layers):
            if l.M_oc is not None:
                arrs[f"M_oc{k}"], arrs[f"n_oc{k}"] = np.asarray(l.M_oc, np.uint32), np.asarray(l.n_oc, np.uint32)
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrs)

    @staticmethod
    def load(path: str) -> "Bundle":
        z = np.load(path, allow_pickle=False)
        m = json.loads(str(z["meta"]))
        L = len(m["M"])
        relu = m.get("relu", [True] * (L - 1) + [False])
        wsc = m.get("w_scale", m.get("wscale", [0.0] * L))
        ps = m.get("pixel_shuffle")
        if ps is None:                       # golden fixtures carry the reference's MFLAG instead
            ps = {5: 4, 6: 2, 3: 1}[m["mflag"]]
        layers = [LayerParams(wq=z[f"Wq{k}"].astype(np.int8), add_const=z[f"add_const{k}"].astype(np.int32),
                              M=int(m["M"][k]), n=int(m["n"][k]), relu=bool(relu[k]), w_scale=float(wsc[k]),
                              M_oc=z[f"M_oc{k}"].astype(np.uint32) if f"M_oc{k}" in z.files else None,
                              n_oc=z[f"n_oc{k}"].astype(np.uint32) if f"n_oc{k}" in z.files else None)
                  for k in range(L)]
        return Bundle(layers=layers, scale=[float(s) for s in m["scale"]], zero=[int(v) for v in m["zero"]],
                      M_res=int(m["M_res"]), n_res=int(m["n_res"]), pixel_shuffle=int(ps),
                      pe_num=int(m.get("pe_num", 4)), pe_acc_bits=int(m.get("pe_acc_bits", 18)),
                      pe_add_bits=int(m.get("pe_add_bits", 20)), name=m.get("name", m.get("case", "")),
                      quan_bits=int(m.get("quan_bits", 8)))        # bundles written before the width existed are 8-bit


# ---- load-time derivation through the library's host-scalar entry points -----------------
def requant_form(M: int, n: int, output_layer: bool = False) -> int:
    """Which reduced form of the requant into a -128 domain is bit-identical for (M, n) (sesrq_requant_form, a host-side
    proof over every accumulator value): 1 = one fma, 2 = one fma that also subtracts the 128 + the add back (output layer
    only), 0 = neither (the kernels keep the two-step form)."""
    return int(_lib.lib().sesrq_requant_form(int(M), int(n), 1 if output_layer else 0))


def saturation_verdict(wq: np.ndarray, add_const=None, zero: int = -128, acc_bits: int = 18, add_bits: int = 20) -> dict:
    """The load-time saturation analysis of one layer (sesrq_saturation_verdict, a host function: what sesrq_create decides from it).
    wq (OC, IC, k, k) int8, add_const (OC,) or None, zero = the zero point of the layer's input domain.  Returns saturation_free,
    biased_ok, risky_mask (bit p = PE p's clamp can fire), worst_pe, worst_sum and reach = the largest |adder output + add constant|."""
    w = np.ascontiguousarray(wq, dtype=np.int8)
    if w.ndim != 4 or w.shape[2] != w.shape[3]:
        raise ValueError("saturation_verdict: weights must be (OC, IC, k, k)")
    ac = None if add_const is None else np.ascontiguousarray(add_const, dtype=np.int32)
    if ac is not None and ac.shape != (w.shape[0],):
        raise ValueError("saturation_verdict: one add constant per output channel")
    mask, wp, ws, reach = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
    rc = _lib.lib().sesrq_saturation_verdict(w.ctypes.data_as(C.POINTER(C.c_int8)), w.shape[2], w.shape[1], w.shape[0],
                                             None if ac is None else ac.ctypes.data_as(C.POINTER(C.c_int32)), int(zero), int(acc_bits),
                                             int(add_bits), C.byref(mask), C.byref(wp), C.byref(ws), C.byref(reach))
    if rc < 0:
        raise ValueError("sesrq: " + _lib.last_error())
    return dict(saturation_free=bool(rc & _lib.VERDICT_SATURATION_FREE), biased_ok=bool(rc & _lib.VERDICT_BIASED_OK),
                risky_mask=int(mask.value), worst_pe=int(wp.value), worst_sum=int(ws.value), reach=int(reach.value))


def requant_const(r: float, data_bit: int = 16, shift_max: int = 32):
    M, n = C.c_uint32(), C.c_uint32()
    _lib.check(_lib.lib().sesrq_requant_const(float(r), data_bit, shift_max, C.byref(M), C.byref(n)), ValueError)
    return int(M.value), int(n.value)


def quantize_weight(w: np.ndarray, width: int = 8):
    w = np.ascontiguousarray(w, dtype=np.float32)
    q = np.empty(w.shape, np.int8)
    s = C.c_double()
    _lib.check(_lib.lib().sesrq_quantize_weight(w.ctypes.data_as(C.POINTER(C.c_float)), w.size, width,
                                                q.ctypes.data_as(C.POINTER(C.c_int8)), C.byref(s)), ValueError)
    return q, float(s.value)


def quantize_weight_per_channel(w: np.ndarray, width: int = 8):
    """(OC, ...) float weights -> (int8 weights, [OC] scales), one symmetric scale per OUTPUT channel (sesrq_quantize_weight_per_channel;
    no reference counterpart: its quantiser is per tensor, quan_func.py:58-71)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    q = np.empty(w.shape, np.int8)
    oc = w.shape[0]
    s = (C.c_double * oc)()
    _lib.check(_lib.lib().sesrq_quantize_weight_per_channel(w.ctypes.data_as(C.POINTER(C.c_float)), oc, w.size // oc, width,
                                                            q.ctypes.data_as(C.POINTER(C.c_int8)), s), ValueError)
    return q, np.array(list(s), dtype=np.float64)


def add_const(bias: np.ndarray, wq: np.ndarray, s_in: float, z_in: int, s_w: float, bias_width: int = 16):
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    wq = np.ascontiguousarray(wq, dtype=np.int8)
    oc = wq.shape[0]
    out = np.empty(oc, np.int32)
    _lib.check(_lib.lib().sesrq_add_const(bias.ctypes.data_as(C.POINTER(C.c_float)), wq.ctypes.data_as(C.POINTER(C.c_int8)),
                                          oc, wq.size // oc, float(s_in), int(z_in), float(s_w), bias_width,
                                          out.ctypes.data_as(C.POINTER(C.c_int32))), ValueError)
    return out


def calib_scale_zero(min_val: float, max_val: float, width: int = 8):
    s, z = C.c_double(), C.c_int()
    _lib.check(_lib.lib().sesrq_calib_scale_zero(float(min_val), float(max_val), width, C.byref(s), C.byref(z)), ValueError)
    return float(s.value), int(z.value)


def derive_bundle(weights: Sequence[np.ndarray], biases: Sequence[np.ndarray], scale: Sequence[float],
                  zero: Sequence[int], pixel_shuffle: int, name: str = "", quan_bit: int = 8, bias_bit: int = 16,
                  requan_bit: int = 16, requan_n_max: int = 32, pe_num: int = 4, pe_acc_bits: int = 18,
                  pe_add_bits: int = 20, per_channel: bool = False) -> Bundle:
    """Float collapsed convs + calibrated (scale, zero) -> integer bundle.
    per_channel: one weight scale per OUTPUT channel instead of the reference's one per tensor (parity unpinned).

    Layer roles by position, as in myQL/quan_func.py:523-609: layers 0 and L-2 requantise into
    domain 1, layer L-1 into domain L, the rest into k+1; residual multiplier s_1/s_{L-1}.
    quan_bit: define.py QUAN_BIT, the width of the weights (quantised here) and of the activations (recorded in the bundle)."""
    quantised = [(quantize_weight_per_channel if per_channel else quantize_weight)(w, quan_bit) for w in weights]
    return derive_bundle_from_quantized([q for q, _ in quantised], [s for _, s in quantised], biases, scale, zero,
                                        pixel_shuffle, name=name, bias_bit=bias_bit, requan_bit=requan_bit,
                                        requan_n_max=requan_n_max, pe_num=pe_num, pe_acc_bits=pe_acc_bits,
                                        pe_add_bits=pe_add_bits, quan_bit=quan_bit)


def derive_bundle_from_quantized(wqs: Sequence[np.ndarray], w_scales: Sequence[float], biases: Sequence[np.ndarray],
                                 scale: Sequence[float], zero: Sequence[int], pixel_shuffle: int, name: str = "",
                                 bias_bit: int = 16, requan_bit: int = 16, requan_n_max: int = 32, pe_num: int = 4,
                                 pe_acc_bits: int = 18, pe_add_bits: int = 20, quan_bit: int = 8) -> Bundle:
    """Same as derive_bundle for weights that quantize_model_weight already turned into integers."""
    L = len(wqs)
    if len(scale) != L + 1 or len(zero) != L + 1:
        raise ValueError("derive_bundle: need L+1 scales and zeros")
    if not 2 <= int(quan_bit) <= 8:
        raise ValueError("derive_bundle: quan_bit must be 2..8")
    lo, hi = -(1 << (quan_bit - 1)), (1 << (quan_bit - 1)) - 1
    for k, w in enumerate(wqs):
        if np.min(w) < lo or np.max(w) > hi:
            raise ValueError(f"derive_bundle: conv {k} weights are not {quan_bit}-bit integers")
    layers = []
    for k in range(L):
        wq = np.ascontiguousarray(wqs[k], dtype=np.int8)
        nxt = 1 if k in (0, L - 2) else k + 1
        if np.ndim(w_scales[k]) == 1:      # one weight scale per output channel (no reference counterpart): per-channel requant constants
            sws = np.asarray(w_scales[k], np.float64)
            Mn = [requant_const(scale[k] / scale[nxt] * float(s), requan_bit, requan_n_max) for s in sws]
            ac = np.concatenate([add_const(np.asarray(biases[k], np.float32)[o:o + 1], wq[o:o + 1], scale[k], zero[k], float(sws[o]), bias_bit)
                                 for o in range(wq.shape[0])])
            layers.append(LayerParams(wq=wq, add_const=ac, M=Mn[0][0], n=Mn[0][1], relu=(k != L - 1), w_scale=float(sws.max()),
                                      M_oc=np.array([m for m, _ in Mn], np.uint32), n_oc=np.array([n for _, n in Mn], np.uint32)))
            continue
        sw = float(w_scales[k])
        M, n = requant_const(scale[k] / scale[nxt] * sw, requan_bit, requan_n_max)
        layers.append(LayerParams(wq=wq, add_const=add_const(biases[k], wq, scale[k], zero[k], sw, bias_bit),
                                  M=M, n=n, relu=(k != L - 1), w_scale=sw))
    M_res, n_res = requant_const(scale[1] / scale[L - 1], requan_bit, requan_n_max)
    return Bundle(layers=layers, scale=[float(s) for s in scale], zero=[int(z) for z in zero], M_res=M_res, n_res=n_res,
                  pixel_shuffle=pixel_shuffle, pe_num=pe_num, pe_acc_bits=pe_acc_bits, pe_add_bits=pe_add_bits, name=name,
                  quan_bits=int(quan_bit))
