"""A classical denoiser of a Bayer frame on the device: the baseline the denoising raw nets are measured against.

The demosaic nets have their classical yardstick in sesrq.demosaic; this is the one of the denoise half (MFLAG 1, and MFLAG 3 / 4 on
noisy frames, where the honest classical row is denoise, then demosaic): non-local means in the Bayer domain, its sample differences
scaled by the variance of the shot / read noise model of sesrq.noise, as one kernel of libsesrq_denoise.so (C ABI
include/sesrq_denoise.h, which states the per-pixel arithmetic; tests/denoise_oracle.py restates it in numpy).  The input is the packed
sensor frame as sesrq.sensor takes it, or the fp32 spread frame the sensor, noise and unprocess routes write.  The output is a spread
frame (N, 3, H, W) fp32: quality.score(., ., 1), demosaic.run_spread and the nets' fp32 input take it as it is.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
from typing import Optional

from . import _lib, sensor

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_denoise.so"))

# every symbol include/sesrq_denoise.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_denoise_raw": (C.c_int, [C.POINTER(sensor.CFormat), C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_void_p, C.c_float,
                                    C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_denoise_spread": (C.c_int, [C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p]),
    "sesrq_denoise_instance_count": (C.c_int, []),
    "sesrq_denoise_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_denoise_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_denoise_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.denoise", "sesrq_denoise")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


@dataclasses.dataclass(frozen=True)
class Params:
    """shot, read: the noise levels of every frame (both given), or both None where the caller brings per-frame levels -- a device
    (N, 2) fp32 `levels` tensor, or the sesrq.noise.NoiseModel of Engine.forward_raw(noise=...).  h: the strength (1.0: weights reach
    zero where the mean squared difference of two patches, in units of the model's variance, exceeds 1 + h)."""
    shot: Optional[float] = None
    read: Optional[float] = None
    h: float = 1.0

    def __post_init__(self):
        if (self.shot is None) != (self.read is None):
            raise ValueError("denoise.Params: give both shot and read, or neither (per-frame levels)")
        for name in ("shot", "read"):
            v = getattr(self, name)
            if v is not None and not (math.isfinite(float(v)) and float(v) >= 0):
                raise ValueError(f"denoise.Params: {name} = {v!r} must be finite and not negative")
        if not (math.isfinite(float(self.h)) and float(self.h) > 0):
            raise ValueError(f"denoise.Params: h = {self.h!r} must be finite and positive")

    @property
    def fixed(self) -> bool:
        return self.shot is not None


def params_of(denoise) -> Params:
    """The Params of a `denoise=` argument: a Params, or True for Params()."""
    if denoise is True:
        return Params()
    if isinstance(denoise, Params):
        return denoise
    raise ValueError(f"denoise must be a sesrq.denoise.Params or True, got {denoise!r}")


def model_levels(params: Params, model, N: int, device, stream):
    """The device (N, 2) `levels` of a call over N frames whose Params carry none: the per-frame levels of the NoiseModel `model`
    (its frame0 onwards), uploaded on `stream`.  None where the Params are fixed."""
    import torch
    if params.fixed:
        return None
    if model is None:
        raise ValueError("denoise: no noise levels -- give Params(shot=, read=), or a noise= model whose per-frame levels are taken")
    with torch.cuda.stream(stream):
        return torch.from_numpy(model.levels(N)).to(device)


def _levels(params: Params, levels, N: int, device):
    """(shot, read, pointer | None) as the C entries take them."""
    import torch
    if levels is None:
        if not params.fixed:
            raise ValueError("denoise: no noise levels -- give Params(shot=, read=) or a device (N, 2) float32 `levels` tensor")
        return float(params.shot), float(params.read), None
    if (not isinstance(levels, torch.Tensor) or levels.dtype != torch.float32 or tuple(levels.shape) != (N, 2) or levels.device != device
            or not levels.is_contiguous()):
        raise ValueError(f"denoise: levels must be a contiguous float32 tensor of shape ({N}, 2) on {device}")
    return 0.0, 0.0, levels.data_ptr()


def _out(out, shape, device):
    """A caller's output is written through its data_ptr(): only a contiguous fp32 tensor of the output shape on the device will do."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != device
            or not out.is_contiguous()):
        raise ValueError(f"denoise: out must be a contiguous float32 tensor of the output shape {tuple(shape)} on {device}")
    return out


def launch(fmt, params: Params, raw, W, S, out, stream, levels=None):
    """Enqueue the denoiser on the contiguous (N, H, S bytes) `raw` of W pixels a row in `fmt` into the caller-owned `out`."""
    cf = fmt.c()
    shot, read, lv = _levels(params, levels, raw.shape[0], raw.device)
    if lib().sesrq_denoise_raw(C.byref(cf), raw.data_ptr(), S, shot, read, lv, float(params.h), out.data_ptr(), raw.shape[0],
                               raw.shape[1], W, stream.cuda_stream) != 0:
        raise ValueError(last_error())


def launch_spread(cfa: str, params: Params, spread, out, stream, levels=None):
    """Enqueue the denoiser on the contiguous (N, 3, H, W) fp32 `spread` of CFA order `cfa` into the caller-owned `out`."""
    N, _, H, W = spread.shape
    shot, read, lv = _levels(params, levels, N, spread.device)
    if lib().sesrq_denoise_spread(sensor.CFAS.index(cfa), spread.data_ptr(), shot, read, lv, float(params.h), out.data_ptr(), N, H, W,
                                  stream.cuda_stream) != 0:
        raise ValueError(last_error())


def run(raw, fmt, params: Params = None, levels=None, out=None, stream=None, stride: int = None, width: int = None):
    """raw in `fmt` (a sesrq.sensor.Format) on a HIP device, as sensor.unpack takes it (see sensor.frames; `stride` and `width` for
    padded rows) -> the denoised spread frame (N, 3, H, W) fp32.  params: a Params with the levels, or, with a device (N, 2) fp32
    `levels` tensor of per-frame (shot, read) pairs, one without.  One kernel, enqueued on `stream` (default: current), not
    synchronised."""
    import torch
    params, fmt = params_of(True if params is None else params), sensor._fmt(fmt)
    if not isinstance(raw, torch.Tensor) or raw.device.type != "cuda":
        raise ValueError("the raw frame must be a tensor on a HIP device")
    dev = raw.device
    raw, W, S = sensor.frames(raw, fmt, dev, stride, width)
    with torch.cuda.device(dev):
        raw = raw.contiguous()
        out = _out(out, (raw.shape[0], 3, raw.shape[1], W), dev)
        launch(fmt, params, raw, W, S, out, _lib.enter_stream(dev, stream, raw, out, levels), levels)
    return out


def run_spread(spread, cfa="rggb", params: Params = None, levels=None, out=None, stream=None):
    """spread: (N, 3, H, W) fp32 on a HIP device, a frame of CFA order `cfa` with each pixel's sample in the plane of its site channel
    (what sensor.unpack, noise.apply and unprocess.run write with want_spread) -> the denoised spread frame (N, 3, H, W) fp32.  The two
    other planes' values at a pixel do not matter.  params, levels: as run takes them.  One kernel, enqueued on `stream` (default:
    current), not synchronised."""
    import torch
    params, cfa = params_of(True if params is None else params), str(cfa).lower()
    if cfa not in sensor.CFAS:
        raise ValueError(f"cfa {cfa!r}: one of {sensor.CFAS}")
    if (not isinstance(spread, torch.Tensor) or spread.dtype != torch.float32 or spread.dim() != 4 or spread.shape[1] != 3
            or spread.device.type != "cuda"):
        raise ValueError("the spread frame must be a (N, 3, H, W) float32 tensor on a HIP device")
    dev = spread.device
    with torch.cuda.device(dev):
        spread = spread.contiguous()
        out = _out(out, tuple(spread.shape), dev)
        if out.data_ptr() == spread.data_ptr():
            raise ValueError("denoise: out must not be the spread frame (a pixel's neighbours are read after it is written)")
        launch_spread(cfa, params, spread, out, _lib.enter_stream(dev, stream, spread, out, levels), levels)
    return out
