"""Shot and read noise on raw frames, added on the device while they are unpacked: the reference's TEST_RAW_ADD_NOISE.

With define.TEST_RAW_ADD_NOISE the reference's TestDataset draws a noise level per frame (self_dataset.py random_noise_levels) and adds
signal-dependent Gaussian noise to the sparse 3-channel frame before the clamp (add_noise: variance = x * shot + read).  Here the clean
raw frame goes to the device as the sensor wrote it and libsesrq_noise.so (C ABI include/sesrq_noise.h, which states the per-pixel
arithmetic) turns it into the NOISY frame's q0 -- the int8 input of sesrq_forward -- and, when asked, into the noisy fp32 frame.  The
deviates are a counter-based stream (Philox4x32-10, Box-Muller): a sample is a function of (seed, frame number, y, x, channel) alone,
so a dataset pass is reproducible from its seed whatever the batch split.  The reference draws from torch's CPU generator, so its
individual samples cannot be reproduced; its arithmetic and its distribution are what is pinned (tests/noise_oracle.py).  There is no
CPU path.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
from typing import Optional

import numpy as np

from . import _lib, sensor

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_noise.so"))

SHOT_MIN, SHOT_MAX = 0.0001, 0.012          # random_noise_levels: ln shot ~ U(ln 1e-4, ln 0.012)
LINE_SLOPE, LINE_OFFSET, LINE_SIGMA = 2.18, 1.20, 0.26      # ln read = 2.18 ln shot + 1.20 + N(0, 0.26)

_FMT = C.POINTER(sensor.CFormat)
# every symbol include/sesrq_noise.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_noise_create": (C.c_int, [_FMT, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_noise_destroy": (None, [C.c_void_p]),
    "sesrq_noise_unpack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                     C.c_float, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "sesrq_noise_deviates": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]),
    "sesrq_noise_instance_count": (C.c_int, []),
    "sesrq_noise_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_noise_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_noise_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.noise", "sesrq_noise")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances

_U64 = (1 << 64) - 1


def levels_from(log_shot, g):
    """(shot, read) of the reference's random_noise_levels from its two draws, in its float32 steps: shot = exp(log_shot),
    read = exp(fl(fl(fl(2.18 * log_shot) + 1.20) + g)).  Scalars or arrays; float32 out."""
    ls, g = np.asarray(log_shot, np.float32), np.asarray(g, np.float32)
    line = (np.float32(LINE_SLOPE) * ls).astype(np.float32) + np.float32(LINE_OFFSET)
    return np.exp(ls).astype(np.float32), np.exp((line + g).astype(np.float32)).astype(np.float32)


def random_levels(rng: np.random.Generator, n: int) -> np.ndarray:
    """(n, 2) float32 (shot, read) pairs, one per frame, drawn as random_noise_levels draws them: ln shot ~ U(ln 1e-4, ln 0.012),
    ln read = 2.18 ln shot + 1.20 + N(0, 0.26).  shot stays inside [1e-4, 0.012]."""
    if not isinstance(rng, np.random.Generator):
        raise ValueError("random_levels: rng must be a numpy.random.Generator")
    lo, hi = math.log(SHOT_MIN), math.log(SHOT_MAX)
    ls = rng.uniform(lo, hi, int(n)).astype(np.float32)
    g = (rng.standard_normal(int(n)) * LINE_SIGMA).astype(np.float32)
    shot, read = levels_from(ls, g)
    shot = np.clip(shot, np.float32(SHOT_MIN), np.float32(SHOT_MAX))       # the float32 roundings of ln and exp at the two ends
    return np.stack([shot, read], 1).astype(np.float32)


@dataclasses.dataclass(frozen=True)
class NoiseModel:
    """The noise of a pass over raw frames.  shot, read: fixed levels (both given), or both None for per-frame levels drawn as the
    reference draws them -- frame f's pair comes from numpy's default_rng((seed, f)), so it depends on (seed, f) alone.  seed selects
    the deviates' stream; frame0 is the global number of the first frame of a call that takes this model, whose frame n is frame
    frame0 + n.  A model is a value: a loop over batches passes model.advance(frames so far), so consecutive frames get consecutive
    numbers whatever the batch split (quality.evaluate_raw does)."""
    shot: Optional[float] = None
    read: Optional[float] = None
    seed: int = 0
    frame0: int = 0

    def __post_init__(self):
        if (self.shot is None) != (self.read is None):
            raise ValueError("NoiseModel: give both shot and read, or neither (levels drawn per frame)")
        for name in ("shot", "read"):
            v = getattr(self, name)
            if v is not None and not (math.isfinite(float(v)) and float(v) >= 0):
                raise ValueError(f"NoiseModel: {name} = {v!r} must be finite and not negative")
        for name in ("seed", "frame0"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= _U64:
                raise ValueError(f"NoiseModel: {name} = {v!r} is not an unsigned 64-bit integer")

    @property
    def fixed(self) -> bool:
        return self.shot is not None

    def levels(self, n: int) -> np.ndarray:
        """(n, 2) float32 (shot, read) of frames frame0 .. frame0 + n - 1."""
        if self.fixed:
            return np.tile(np.array([self.shot, self.read], np.float32), (int(n), 1))
        return np.concatenate([random_levels(np.random.default_rng((int(self.seed), (int(self.frame0) + k) & _U64)), 1)
                               for k in range(int(n))])

    def advance(self, n: int) -> "NoiseModel":
        """The model of the frames behind the next n: frame0 + n (wrapping at 2^64)."""
        return dataclasses.replace(self, frame0=(int(self.frame0) + int(n)) & _U64)

    def plan(self, n: int):
        """(shot, read, host levels | None, seed, frame0) of a call over n frames."""
        lv = None if self.fixed else self.levels(n)
        return (float(self.shot) if self.fixed else 0.0), (float(self.read) if self.fixed else 0.0), lv, int(self.seed), int(self.frame0)


def _model(model) -> NoiseModel:
    if not isinstance(model, NoiseModel):
        raise ValueError(f"noise must be a sesrq.noise.NoiseModel, got {type(model).__name__}")
    return model


_ctx = {}          # (device index, f32 scale bits, zero, exact_div, format | None) -> context handle; lives as long as the process


def context(device, fmt, scale_in, zero_in, exact_div):
    """The device context (sesrq_noise_create) of one (device, input domain, format), created once.  fmt None: the reference's."""
    import torch
    fmt, _ = sensor.route(fmt)
    key = (device.index, np.float32(scale_in).tobytes(), int(zero_in), int(exact_div), fmt)
    h = _ctx.get(key)
    if h is None:
        h, cf = C.c_void_p(), fmt.c()
        with torch.cuda.device(device):
            if lib().sesrq_noise_create(C.byref(cf), float(np.float32(scale_in)), int(zero_in), int(exact_div), C.byref(h)) != 0:
                raise ValueError(last_error())
        _ctx[key] = h
    return h


def launch(device, fmt, scale_in, zero_in, exact_div, raw, W, S, q0, spread, stream, model: NoiseModel):
    """Enqueue one noisy unpack of the contiguous (N, H, S bytes) `raw` of W pixels a row into caller-owned q0 / spread (either may be
    None) on `stream`.  Per-frame levels are uploaded on `stream` ahead of the kernel."""
    import torch
    N, H = raw.shape[0], raw.shape[1]
    h = context(device, fmt, scale_in, zero_in, exact_div)
    shot, read, lv, seed, f0 = _model(model).plan(N)
    dlv = None
    if lv is not None:
        with torch.cuda.stream(stream):
            dlv = torch.from_numpy(lv).to(device)
    rc = lib().sesrq_noise_unpack(h, raw.data_ptr(), S, q0.data_ptr() if q0 is not None else None,
                                  spread.data_ptr() if spread is not None else None, N, H, W, shot, read,
                                  dlv.data_ptr() if dlv is not None else None, seed, f0, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def deviates(shape, seed: int = 0, frame0: int = 0, device=None, stream=None):
    """(N, 3, H, W) fp32 standard normal deviates on `device`: z[n, c, y, x] of the stream (seed, frame0 + n), the values the noisy
    unpack scales -- a reproducible device normal source.  shape: (N, H, W) or (N, 3, H, W)."""
    import torch
    shape = tuple(int(v) for v in shape)
    if len(shape) == 4 and shape[1] == 3:
        shape = (shape[0], shape[2], shape[3])
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"deviates: shape is (N, H, W) or (N, 3, H, W), got {shape}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError("deviates: a HIP device is needed")
    N, H, W = shape
    with torch.cuda.device(dev):
        z = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
        st = _lib.enter_stream(dev, stream, z)
        if lib().sesrq_noise_deviates(z.data_ptr(), N, H, W, int(seed) & _U64, int(frame0) & _U64, st.cuda_stream) != 0:
            raise ValueError(last_error())
    return z


def apply(engine_or_bundle, raw, fmt=None, model: NoiseModel = None, want_q: bool = True, want_spread: bool = False, stride: int = None,
          width: int = None, stream=None):
    """sesrq.sensor.unpack with the model's noise added: raw in `fmt` on a HIP device (see sensor.frames; None: the reference's 12-bit
    RGGB uint16) -> (q0 int8 (N, 3, H, W) | None, spread fp32 (N, 3, H, W) | None) of the noisy frame; frame n is the model's frame0 + n.
    Enqueued on `stream` (default: current), not synchronised."""
    import torch
    _model(model)
    if not (want_q or want_spread):
        raise ValueError("apply: ask for q0, spread or both")
    b, scale_in, zero_in, exact_div, dev = _lib.input_domain(engine_or_bundle, want_q, "apply")
    if b is not None and b.in_channels != 3:
        raise ValueError(f"a raw Bayer frame feeds 3-channel nets; this one takes {b.in_channels}")
    if dev is None:
        dev = raw.device if isinstance(raw, torch.Tensor) else None
    raw, W, S = sensor.frames(raw, fmt, dev, stride, width)
    if dev is None or dev.type != "cuda":
        raise ValueError("the raw frame must be on a HIP device")
    N, H = raw.shape[0], raw.shape[1]
    with torch.cuda.device(dev):
        raw = raw.contiguous()
        q0 = torch.empty((N, 3, H, W), dtype=torch.int8, device=dev) if want_q else None
        sp = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev) if want_spread else None
        launch(dev, fmt, scale_in, zero_in, exact_div, raw, W, S, q0, sp, _lib.enter_stream(dev, stream, raw, q0, sp), model)
    return q0, sp
