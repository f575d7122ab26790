"""Calibration pass on the GPU: the reference's exe_mode 0 (test.py:79-113,141-217).

The float net -- collapsed convs with fake-quantised weights, the float long skip, a fake-quantiser in
front of every conv (and of PixelShuffle) -- is run on calibration frames while the running min/max of
every quantiser input is observed; `finalize()` turns them into the activation domains (scale, zero) the
integer path consumes, with the reference's rule for the output domain (min := 0, so zero_L = -128).
The per-conv arithmetic lives in libsesrq (sesrq_calib_conv / _minmax / _fakequant); this module is the
host-side bookkeeping (python float arithmetic exactly as the reference's scripts do it).
Pinned to the reference within a tolerance (fp32 summation order differs), not bit for bit.

Entropy variant (`method="entropy"`; BASELINE's north star names KL-entropy activation ranges, the reference itself only
has min/max -- no oracle, PARITY UNPINNED): after the min/max pass a second pass over the same frames accumulates a
histogram of every quantiser input over its observed range (sesrq_calib_histogram), and `finalize()` replaces (min, max)
by the clipping range that minimises the KL divergence between the observed distribution and its 256-level quantisation
(`entropy_range`).  The output domain keeps the reference's rule (min := 0).

Device-resident pass (`enqueue`, `enqueue_raw`, `enqueue_image`, `enqueue_hr`): the same forward with no host round trip.  `observe` reads each
quantiser's min/max back to the host to form the next conv's (scale, zero); here one device slot per quantiser input holds the batch's
extrema, the running extrema and the domain derived from them (sesrq_calib_observe_slot), and the conv / fake-quantiser read it there
(sesrq_calib_conv_slot / _fakequant_slot).  Nothing waits on the host until `finalize()` (or `sync()`) reads the slots back.  Bit for
bit the results of `observe` on the same frames: per-batch (scale, zero), mode-0 output, running min/max, domains, bundle.  Frames
come as fp32 (N, C, H, W), 12-bit RGGB raw frames (decoded on the device into the reference's fp32 input, sesrq.raw) or 8-bit images
(sesrq.image).  min/max only: the entropy variant keeps the host pass.

QAT nets (`skip_quant_scale`): quantize.prepare() replaces the long skip's AddOp of a QAT net by a fake-quantising QuantAdd (reference
models/quantize_utils_pt.py:654-711), so the reference's mode-0 pass adds two quantised tensors: x_{L-1} = fq(a_{L-2}) + fq(a_0), fq
the 8-bit symmetric quantiser at the constant scale the checkpoint's observer state gives (models/quantize_utils_pt.skip_quant_scale).
With the scale set, the conv in front of the merge runs sesrq_calib_conv_qadd / _slot_qadd, which fuse it into their epilogue, on
both passes and for every kind of frame."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .bundle import Bundle, derive_bundle, quantize_weight

ZERO_LIMIT = 1 << 30        # |zero| of a batch's domain (csrc/sesrq_calib.hip derive_domain), for a domain far from 0


def _smooth(d: np.ndarray, eps: float = 1e-4) -> np.ndarray:
    """Move a little mass onto the empty bins of a normalised histogram so that KL(p || q) stays finite where the folded
    outliers of p meet an empty bin of q (the usual smoothing of entropy calibrators)."""
    zero = d == 0
    nz = int(zero.sum())
    if nz == 0 or nz == d.size:
        return d
    take = eps * nz / (d.size - nz)
    out = np.where(zero, eps, d - take)
    return np.maximum(out, eps * 1e-3)          # a non-empty bin lighter than its share of the smoothing stays positive


def _kl_upper_cut(hist: np.ndarray, levels: int, stride: int) -> int:
    """Number of leading bins to keep (levels..len(hist)): the cut i minimising KL(P_i || Q_i), P_i = hist[:i] with the
    mass beyond folded into its last bin, Q_i = hist[:i] merged into `levels` equal buckets and spread back evenly over the
    non-empty bins of each bucket (the usual entropy-calibration construction)."""
    B = len(hist)
    h = hist.astype(np.float64)
    total = h.sum()
    if total <= 0 or B <= levels:
        return B
    tail = np.concatenate([np.cumsum(h[::-1])[::-1][1:], [0.0]])          # tail[i-1] = mass of bins i..B-1
    best_i, best_kl = B, np.inf
    for i in list(range(levels, B, stride)) + [B]:
        p = h[:i].copy()
        p[i - 1] += tail[i - 1]
        bucket = (np.arange(i) * levels) // i
        mass = np.bincount(bucket, weights=h[:i], minlength=levels)
        nonzero = np.bincount(bucket, weights=(h[:i] > 0).astype(np.float64), minlength=levels)
        q = np.where(h[:i] > 0, mass[bucket] / np.maximum(nonzero[bucket], 1.0), 0.0)
        qs = q.sum()
        if qs <= 0:
            continue
        p, q = _smooth(p / p.sum()), _smooth(q / qs)
        kl = float(np.sum(p * np.log(p / q)))
        if kl < best_kl - 1e-12:
            best_kl, best_i = kl, i
    return best_i


def entropy_range(hist: np.ndarray, lo: float, hi: float, levels: int = 256, stride: int = 8):
    """Clipping range (min, max) inside [lo, hi] for a histogram of equal bins over [lo, hi): the upper cut by KL search,
    then -- for domains that reach below zero -- the lower cut by the same search on the mirrored histogram of what is
    left.  A domain that starts at or above zero (everything behind a ReLU, image inputs) keeps its lower end."""
    hist = np.asarray(hist)
    B = len(hist)
    if B < 2 or not hi > lo:
        raise ValueError("entropy_range: need at least two bins and lo < hi")
    w = (hi - lo) / B
    up = _kl_upper_cut(hist, levels, stride)
    kept = hist[:up].astype(np.float64).copy()
    kept[up - 1] += float(hist[up:].sum())
    down = 0
    if lo < 0 and up > levels:
        down = up - _kl_upper_cut(kept[::-1], levels, stride)
    return lo + down * w, lo + up * w


class Calibrator:
    def __init__(self, weights: Sequence[np.ndarray], biases: Sequence[np.ndarray], pixel_shuffle: int = 1,
                 device: Optional[torch.device] = None, pe_acc_bits: int = 18, pe_add_bits: int = 20, bias_bits: int = 16,
                 quantized=None, method: str = "minmax", bins: int = 2048, quan_bits: int = 8,
                 skip_quant_scale: Optional[float] = None):
        """weights: float collapsed convs (quantised here), or None with `quantized` = [(Wq int8, weight scale)]
        when quantize_model_weight already did it.  quan_bits: define.py QUAN_BIT, the width b of weights and activations
        (scale = range / (2^b - 1), zero = -2^(b-1) - round(min / scale), clamps to [-2^(b-1), 2^(b-1) - 1]; test.py:189-215).
        skip_quant_scale: None = the float long skip x_{L-1} = a_{L-2} + a_0; a positive finite float s (taken as fp32) = the QuantAdd
        of a QAT net, x_{L-1} = fq(a_{L-2}) + fq(a_0) with fq(t) = clamp(round_half_away(t / s), -128, 127) * s, in observe, enqueue,
        enqueue_raw and enqueue_image alike.  The QuantAdd stays 8-bit at every quan_bits, as the reference's does (its test.py:62
        prepares the model with a_bits=8 whatever QUAN_BIT is); no reference record of a QAT net exists below b = 8, so there this
        is pinned to the oracle alone."""
        if skip_quant_scale is not None:
            s32 = float(np.float32(skip_quant_scale)) if isinstance(skip_quant_scale, (int, float, np.floating)) else float("nan")
            if not (np.isfinite(s32) and s32 > 0.0):
                raise ValueError("Calibrator: skip_quant_scale must be None or a positive finite float (in fp32)")
            skip_quant_scale = s32
        self.skip_quant_scale = skip_quant_scale
        if not torch.cuda.is_available():
            raise RuntimeError("sesrq.Calibrator needs a HIP device (no CPU fallback)")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if not 2 <= int(quan_bits) <= 8:
            raise ValueError("Calibrator: quan_bits must be 2..8")
        self.quan_bits = int(quan_bits)
        self.L = len(biases)
        self.pixel_shuffle = int(pixel_shuffle)
        self.acc_bits, self.add_bits, self.bias_bits = pe_acc_bits, pe_add_bits, bias_bits
        self.weights_f = [np.asarray(w, np.float32) for w in weights] if weights is not None else None
        self.biases_f = [np.asarray(b, np.float32) for b in biases]
        self.wq, self.sw, self._wdev = [], [], []
        if quantized is None:
            quantized = [quantize_weight(w, self.quan_bits) for w in self.weights_f]
        for q, s in quantized:
            q = np.ascontiguousarray(q, dtype=np.int8)
            self.wq.append(q)
            self.sw.append(float(s))
            self._wdev.append(torch.from_numpy(q.astype(np.int32)).to(self.device).contiguous())
        self.run_min: List[Optional[float]] = [None] * (self.L + 1)
        self.run_max: List[Optional[float]] = [None] * (self.L + 1)
        self.last_scale: List[Optional[float]] = [None] * (self.L + 1)   # per-batch values, like input.K.scale.pt during test.py
        self.last_zero: List[Optional[int]] = [None] * (self.L + 1)
        self._mm = torch.empty(2, dtype=torch.float32, device=self.device)
        self._scratch = torch.empty(2, dtype=torch.int32, device=self.device)
        self.hist: List[Optional[torch.Tensor]] = [None] * (self.L + 1)     # entropy variant: second-pass histograms
        self._hist_pass = False
        self.set_method(method, bins)
        self.in_channels = int(self.wq[0].shape[1])
        # device-resident pass: float biases, descriptors, one slot per quantiser input (uploaded here and by reset(): enqueueing never
        # waits on the host), kept activation buffers per (N, H, W)
        self._bias_dev = [torch.from_numpy(b).to(self.device) for b in self.biases_f]
        self._conv_desc, self._dom_desc = [], []
        for k in range(self.L):
            oc, ic, ks, _ = self.wq[k].shape
            self._conv_desc.append(_lib.CalibConvDesc(k=ks, ic=ic, oc=oc, w=self._wdev[k].data_ptr(), relu=int(k != self.L - 1)))
            self._dom_desc.append(_lib.CalibDomainDesc(quan_bits=self.quan_bits, oc=oc, bias=self._bias_dev[k].data_ptr(), sw=self.sw[k],
                                                       acc_bits=self.acc_bits, add_bits=self.add_bits, bias_bits=self.bias_bits))
        self._dom_desc.append(_lib.CalibDomainDesc(quan_bits=self.quan_bits, oc=0, bias=None, sw=1.0, acc_bits=self.acc_bits,
                                                   add_bits=self.add_bits, bias_bits=self.bias_bits))
        self._slot_bytes = C.sizeof(_lib.CalibSlot)
        self._slots = torch.empty((self.L + 1) * self._slot_bytes, dtype=torch.uint8, device=self.device)
        self._buffers = {}
        self.last_input: Optional[torch.Tensor] = None
        self._reset_slots()

    def set_method(self, method: str, bins: int = 2048):
        """'minmax' = the reference's rule; 'entropy' = KL-minimising clipping ranges from a second (histogram) pass."""
        if method not in ("minmax", "entropy"):
            raise ValueError("Calibrator: method must be 'minmax' (the reference's) or 'entropy'")
        if not 256 < bins <= 4096:
            raise ValueError("Calibrator: bins must be in 257..4096")
        if self._hist_pass:
            raise RuntimeError("Calibrator.set_method: a histogram pass is in progress (reset() first)")
        self.method, self.bins = method, int(bins)

    # ---- observers -----------------------------------------------------------------------
    def reset(self):
        """test.py:108-113: forget earlier ranges before a calibration run."""
        self.run_min = [None] * (self.L + 1)
        self.run_max = [None] * (self.L + 1)
        self.hist = [None] * (self.L + 1)
        self._hist_pass = False
        self._reset_slots()

    def _reset_slots(self):
        init = (_lib.CalibSlot * (self.L + 1))()
        _lib.check(_lib.lib().sesrq_calib_slots_init(init, self.L + 1))
        self._slots.copy_(torch.frombuffer(bytearray(bytes(init)), dtype=torch.uint8))
        self._dev_pass = False

    def begin_histogram_pass(self):
        """Entropy variant: call after the min/max pass; the following observe() calls (the same frames again) accumulate
        the histograms over the ranges found so far instead of widening them."""
        if self.method != "entropy":
            raise RuntimeError("begin_histogram_pass: the calibrator was built with method='minmax'")
        if any(v is None for v in self.run_min):
            raise RuntimeError("begin_histogram_pass: run the min/max pass (observe) first")
        self.hist = [torch.zeros(self.bins, dtype=torch.int32, device=self.device) for _ in range(self.L + 1)]
        self._hist_pass = True

    def _observe(self, k: int, t: torch.Tensor):
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.lib().sesrq_calib_minmax(t.data_ptr(), t.numel(), self._mm.data_ptr(), self._scratch.data_ptr(), st))
        mn, mx = (float(v) for v in self._mm.cpu().numpy())
        if self._hist_pass:
            _lib.check(_lib.lib().sesrq_calib_histogram(t.data_ptr(), t.numel(), float(np.float32(self.run_min[k])),
                                                        float(np.float32(self.run_max[k])), self.bins, self.hist[k].data_ptr(), st))
        else:
            if self.run_max[k] is None or self.run_max[k] < mx:
                self.run_max[k] = mx
            if self.run_min[k] is None or self.run_min[k] > mn:
                self.run_min[k] = mn
        assert mx != mn, "Input tensor is all equal,{}".format(k)
        scale = (mx - mn) / ((1 << self.quan_bits) - 1)
        zero = -(1 << (self.quan_bits - 1)) - round(mn / scale)
        zero = min(max(zero, -ZERO_LIMIT), ZERO_LIMIT)      # as the device pass clamps it (derive_domain): the int the conv reads
        self.last_scale[k], self.last_zero[k] = scale, int(zero)
        return scale, int(zero)

    # ---- one calibration forward -----------------------------------------------------------
    def observe(self, x: torch.Tensor) -> torch.Tensor:
        """x: (N, Cin, H, W) fp32 on the device.  Returns what the reference's mode-0 model returns (the
        fake-quantised float output, pixel-shuffled)."""
        if x.dim() != 4 or x.dtype != torch.float32 or x.device != self.device:
            raise ValueError("Calibrator.observe: need a (N,C,H,W) float32 tensor on " + str(self.device))
        if self._dev_pass:
            raise RuntimeError("Calibrator.observe: this calibrator holds a device-resident pass (enqueue*); reset() first")
        lib = _lib.lib()
        st = torch.cuda.current_stream(self.device).cuda_stream
        N, _, H, W = x.shape
        a = x.contiguous()
        first = None
        L = self.L
        for k in range(L):
            scale, zero = self._observe(k, a)
            sw = self.sw[k]
            oc, ic, ks, _ = self.wq[k].shape
            bias_scale = scale * sw
            lo16, hi16 = -(2 ** (self.bias_bits - 1)), 2 ** (self.bias_bits - 1) - 1
            bq = np.clip(np.rint(self.biases_f[k] / np.float32(bias_scale)), lo16, hi16).astype(np.float32)
            qb = torch.from_numpy((bq * np.float32(bias_scale)).astype(np.float32)).to(self.device)
            hi_a, lo_a = 2 ** (self.acc_bits - 1) - 1, -(2 ** (self.acc_bits - 1))
            hi_s, lo_s = 2 ** (self.add_bits - 1) - 1, -(2 ** (self.add_bits - 1))
            desc = _lib.CalibConvDesc(k=ks, ic=ic, oc=oc, w=self._wdev[k].data_ptr(), qbias=qb.data_ptr(),
                                      in_scale=float(np.float32(scale)), in_zero=zero, ss=float(np.float32(scale * sw)),
                                      acc_lo=float(np.float32((lo_a - zero) * scale * sw)), acc_hi=float(np.float32((hi_a - zero) * scale * sw)),
                                      add_lo=float(np.float32((lo_s - zero) * scale * sw)), add_hi=float(np.float32((hi_s - zero) * scale * sw)),
                                      relu=int(k != L - 1))
            out = torch.empty((N, oc, H, W), dtype=torch.float32, device=self.device)
            skip = first if k == L - 2 else None          # long skip: x_{L-1} = a_{L-2} + a_0 (float AddOp, or the QuantAdd)
            if skip is not None and self.skip_quant_scale is not None:
                _lib.check(lib.sesrq_calib_conv_qadd(C.byref(desc), a.data_ptr(), skip.data_ptr(), out.data_ptr(), N, H, W,
                                                     self.quan_bits, self.skip_quant_scale, st))
            else:
                _lib.check(lib.sesrq_calib_conv_q(C.byref(desc), a.data_ptr(), skip.data_ptr() if skip is not None else None,
                                                  out.data_ptr(), N, H, W, self.quan_bits, st))
            if k == 0:
                first = out
            a = out
        if self.pixel_shuffle > 1:
            scale, zero = self._observe(L, a)                 # quantiser in front of PixelShuffle (test.py:90-91)
            fq = torch.empty_like(a)
            _lib.check(lib.sesrq_calib_fakequant_q(a.data_ptr(), fq.data_ptr(), a.numel(), float(np.float32(scale)), zero,
                                                   self.quan_bits, st))
            return torch.nn.functional.pixel_shuffle(fq, self.pixel_shuffle)
        self._observe(L, a)                                   # nets without PixelShuffle: range of the last conv's output (quan_func.py:460-479)
        return a


    # ---- device-resident pass ----------------------------------------------------------------
    def _check_device_pass(self, who: str):
        if self.method != "minmax":
            raise ValueError(f"Calibrator.{who}: the device-resident pass computes the reference's min/max ranges only; "
                             "method='entropy' runs on the host pass (observe, begin_histogram_pass)")
        if not self._dev_pass and any(v is not None for v in self.run_min):
            raise RuntimeError(f"Calibrator.{who}: frames were observed on the host pass (observe); reset() first")

    def _slot(self, k: int) -> int:
        return self._slots.data_ptr() + k * self._slot_bytes

    def _acts(self, N: int, H: int, W: int):
        """The kept activation buffers of one (N, H, W): conv outputs 0 .. L-2, the last conv's output of a PixelShuffle net, and the
        decoded input frame of raw / image input.  Only the most recent frame size is kept (a dataset of many sizes does not pile up
        buffer sets); the caching allocator recycles the previous set only behind the work already queued on this stream."""
        key = (N, H, W)
        b = self._buffers.get(key)
        if b is None:
            shapes = [(N, self.wq[k].shape[0], H, W) for k in range(self.L - 1 if self.pixel_shuffle == 1 else self.L)]
            b = {"acts": [torch.empty(sh, dtype=torch.float32, device=self.device) for sh in shapes],
                 "input": torch.empty((N, self.in_channels, H, W), dtype=torch.float32, device=self.device)}
            self._buffers = {key: b}
        return b

    def _forward_device(self, x: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
        lib = _lib.lib()
        st = torch.cuda.current_stream(self.device).cuda_stream
        N, _, H, W = x.shape
        acts, L, r, qb = self._acts(N, H, W)["acts"], self.L, self.pixel_shuffle, self.quan_bits
        oc = self.wq[L - 1].shape[0]
        shape = (N, oc // (r * r), H * r, W * r)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"Calibrator: out must be a contiguous float32 {shape} tensor on {self.device}")
        last = out if r == 1 else acts[L - 1]
        a = x
        self._dev_pass = True
        for k in range(L):
            _lib.check(lib.sesrq_calib_observe_slot(a.data_ptr(), a.numel(), self._slot(k), C.byref(self._dom_desc[k]), st))
            dst = acts[k] if k < L - 1 else last
            skip = acts[0] if k == L - 2 else None          # long skip: x_{L-1} = a_{L-2} + a_0 (float AddOp, or the QuantAdd)
            if skip is not None and self.skip_quant_scale is not None:
                _lib.check(lib.sesrq_calib_conv_slot_qadd(C.byref(self._conv_desc[k]), self._slot(k), a.data_ptr(), skip.data_ptr(),
                                                          dst.data_ptr(), N, H, W, qb, self.skip_quant_scale, st))
            else:
                _lib.check(lib.sesrq_calib_conv_slot(C.byref(self._conv_desc[k]), self._slot(k), a.data_ptr(),
                                                     skip.data_ptr() if skip is not None else None, dst.data_ptr(), N, H, W, qb, st))
            a = dst
        _lib.check(lib.sesrq_calib_observe_slot(a.data_ptr(), a.numel(), self._slot(L), C.byref(self._dom_desc[L]), st))
        if r > 1:      # the quantiser in front of PixelShuffle, written shuffled (test.py:90-91)
            _lib.check(lib.sesrq_calib_fakequant_slot(a.data_ptr(), out.data_ptr(), N, oc, H, W, r, self._slot(L), qb, st))
        return out

    def enqueue(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """observe() without a host round trip: x (N, Cin, H, W) float32 on the device -> the mode-0 output (a new tensor, or `out`),
        enqueued on the current stream and not synchronised.  The ranges are read back by finalize() / sync().

        One stream per calibrator: the slots and the kept activation buffers are shared by every frame and ordered only by the stream
        the frames are enqueued on, so enqueue all of a pass's frames on one stream.  last_input is the fp32 frame the pass read
        (for enqueue_raw / enqueue_image a kept buffer): valid until the next enqueue*."""
        self._check_device_pass("enqueue")
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.float32 or x.device != self.device:
            raise ValueError("Calibrator.enqueue: need a (N,C,H,W) float32 tensor on " + str(self.device))
        if x.shape[1] != self.in_channels or min(x.shape) < 1:
            raise ValueError(f"Calibrator.enqueue: expected {self.in_channels} input channels and a non-empty frame, got {tuple(x.shape)}")
        x = x.contiguous()
        self.last_input = x
        return self._forward_device(x, out)

    def enqueue_raw(self, raw_u16: torch.Tensor, out: Optional[torch.Tensor] = None, fmt=None, stride=None, width=None,
                    noise=None) -> torch.Tensor:
        """12-bit RGGB raw frames (N, 1, H, W) / (N, H, W) / (H, W) torch.uint16 on the device, unpacked on the device into the
        reference's fp32 input (sesrq.raw, the spread frame: self_dataset.py TestDataset's inp) and calibrated as enqueue() does.
        fmt: a sesrq.sensor.Format -- frames in that sensor format (`stride`, `width` as sesrq.sensor.frames takes them), unpacked by
        libsesrq_sensor.so; without it nothing changes.  noise: a sesrq.noise.NoiseModel -- libsesrq_noise.so unpacks the frames and
        adds the model's shot and read noise (the reference's TEST_RAW_ADD_NOISE; frame n is the model's frame0 + n); without it
        nothing changes."""
        from . import sensor
        self._check_device_pass("enqueue_raw")
        if self.in_channels != 3:
            raise ValueError(f"Calibrator.enqueue_raw: a raw RGGB frame feeds 3-channel nets; this one takes {self.in_channels}")
        st = torch.cuda.current_stream(self.device)
        raw, W, S = sensor.frames(raw_u16, fmt, self.device, stride, width, "Calibrator.enqueue_raw: ")
        raw = raw.contiguous()
        x = self._acts(raw.shape[0], raw.shape[1], W)["input"]
        if noise is None:
            sensor.launch(self.device, fmt, 1.0, 0, 0, raw, W, S, None, x, st)
        else:
            from . import noise as noisemod
            noisemod.launch(self.device, fmt, 1.0, 0, 0, raw, W, S, None, x, st, noise)
        self.last_input = x
        return self._forward_device(x, out)

    def enqueue_image(self, img_u8: torch.Tensor, order: str = "rgb", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """8-bit images (N, H, W, 3) / (H, W, 3) torch.uint8 on the device, in `order`, decoded on the device into the reference's fp32
        input (sesrq.image: the float64 luma for a 1-channel net (MFLAG 5), RGB / 255 for a 3-channel one (MFLAG 6)) and calibrated
        as enqueue() does."""
        from . import image as imgmod
        self._check_device_pass("enqueue_image")
        form = imgmod.Y if self.in_channels == 1 else imgmod.RGB if self.in_channels == 3 else None
        if form is None:
            raise ValueError(f"Calibrator.enqueue_image: an 8-bit image feeds 1- or 3-channel nets; this one takes {self.in_channels}")
        imgmod._order(order)
        img = imgmod._images(img_u8, self.device).contiguous()
        N, H, W, _ = img.shape
        x = self._acts(N, H, W)["input"]
        imgmod.launch(self.device, 1.0, 0, 0, img, form, order, None, x, torch.cuda.current_stream(self.device))
        self.last_input = x
        return self._forward_device(x, out)

    def enqueue_hr(self, hr_u8: torch.Tensor, order: str = "rgb", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """8-bit HR images (N, H, W, 3) / (H, W, 3) torch.uint8 on the device, in `order`, sizes multiples of the net's PixelShuffle
        factor r: downscaled bicubically by r and decoded in one kernel (sesrq.downscale) into the fp32 input enqueue_image forms
        from the LR file, and calibrated as enqueue() does."""
        from . import downscale as ds
        self._check_device_pass("enqueue_hr")
        form = ds.Y if self.in_channels == 1 else ds.RGB if self.in_channels == 3 else None
        if form is None:
            raise ValueError(f"Calibrator.enqueue_hr: an 8-bit image feeds 1- or 3-channel nets; this one takes {self.in_channels}")
        r = self.pixel_shuffle
        if r not in ds.FACTORS:
            raise ValueError(f"Calibrator.enqueue_hr: the HR image is downscaled by the net's PixelShuffle factor, 2 or 4; this net's is {r}")
        ds._order(order)
        img = ds.hr_images(hr_u8, r, who="Calibrator.enqueue_hr")
        ds._on_device(img, self.device, "Calibrator.enqueue_hr")
        img = img.contiguous()
        N, H, W, _ = img.shape
        x = self._acts(N, H // r, W // r)["input"]
        ds.launch(self.device, 1.0, 0, 0, img, order, r, form, None, None, x, torch.cuda.current_stream(self.device))
        self.last_input = x
        return self._forward_device(x, out)

    def sync(self):
        """Wait for the enqueued frames and read the slots back: run_min / run_max, last_scale / last_zero as observe() leaves them.
        A batch whose quantiser input was constant (max == min, which observe() asserts against) raises here."""
        if not self._dev_pass:
            return
        raw = bytes(self._slots.cpu().numpy().tobytes())
        slots = (_lib.CalibSlot * (self.L + 1)).from_buffer_copy(raw)
        for k, s in enumerate(slots):
            if s.degenerate:
                raise RuntimeError("Input tensor is all equal,{}".format(k))
            if s.batches:
                self.run_min[k], self.run_max[k] = float(s.run_min), float(s.run_max)
                self.last_scale[k], self.last_zero[k] = float(s.scale), int(s.zero)

    # ---- results ------------------------------------------------------------------------------
    def finalize(self):
        """running (min, max) -> (scale[0..L], zero[0..L]) as test.py:185-217 (output domain: min := 0)."""
        from .bundle import calib_scale_zero
        self.sync()
        if self.method == "entropy" and not self._hist_pass:
            raise RuntimeError("Calibrator.finalize: method='entropy' needs the histogram pass (begin_histogram_pass, observe again)")
        scale, zero = [], []
        self.ranges = []
        for k in range(self.L + 1):
            if self.run_min[k] is None:
                raise RuntimeError("Calibrator.finalize: no frames observed")
            mn, mx = self.run_min[k], self.run_max[k]
            if self.method == "entropy":
                lo32, hi32 = float(np.float32(mn)), float(np.float32(mx))       # the edges the histogram kernel used
                mn, mx = entropy_range(self.hist[k].cpu().numpy().astype(np.int64), lo32, hi32, levels=1 << self.quan_bits)
            self.ranges.append((mn, mx))
            s, z = calib_scale_zero(0.0 if k == self.L else mn, mx, self.quan_bits)
            scale.append(s)
            zero.append(z)
        return scale, zero

    def bundle(self, name: str = "") -> Bundle:
        from .bundle import derive_bundle_from_quantized
        scale, zero = self.finalize()
        return derive_bundle_from_quantized(self.wq, self.sw, self.biases_f, scale, zero, self.pixel_shuffle, name=name,
                                            pe_acc_bits=self.acc_bits, pe_add_bits=self.add_bits, bias_bit=self.bias_bits,
                                            quan_bit=self.quan_bits)


def finish_calibration(store, L: int, quan_bits: Optional[int] = None):
    """The tail of the reference's test.py (:185-217): running input.K.{min,max}_val -> final
    input.K.{scale,zero} for K = 0..L, output domain with min := 0, at width quan_bits (None: define.QUAN_BIT)."""
    from .bundle import calib_scale_zero
    if quan_bits is None:
        import define
        quan_bits = int(define.QUAN_BIT)
    scale, zero = [], []
    for k in range(L + 1):
        mn = 0.0 if k == L else float(store[f"input/input.{k}.min_val"])
        s, z = calib_scale_zero(mn, float(store[f"input/input.{k}.max_val"]), quan_bits)
        scale.append(s)
        zero.append(z)
    store.set_activation_domains(scale, zero)
    return scale, zero
