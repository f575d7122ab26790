"""The classical demosaic of a Bayer frame on the device: the baseline the raw nets (MFLAG 2, 3, 4) are measured against.

The SR nets have their classical yardstick in sesrq.resize (Pillow's bicubic); this is the one of the raw side: bilinear interpolation
and the 5 x 5 linear filters of Malvar, He and Cutler, as one kernel of libsesrq_demosaic.so (C ABI include/sesrq_demosaic.h, which
states the per-pixel arithmetic; tests/demosaic_oracle.py restates it in numpy).  The input is the packed sensor frame as
sesrq.sensor takes it, or the fp32 spread frame the sensor, noise and unprocess routes write -- the noisy frame a denoising net saw,
for instance.  The output is (N, 3, H, W) fp32, planes R, G, B, in the layout of the nets' ground truth: quality.score and
develop.export take it as it is.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _lib, sensor

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_demosaic.so"))

BILINEAR, MALVAR = 0, 1                                  # SESRQ_DEMOSAIC_*
METHODS = ("bilinear", "malvar")

# every symbol include/sesrq_demosaic.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_demosaic_raw": (C.c_int, [C.POINTER(sensor.CFormat), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p]),
    "sesrq_demosaic_spread": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_demosaic_instance_count": (C.c_int, []),
    "sesrq_demosaic_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_demosaic_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_demosaic_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.demosaic", "sesrq_demosaic")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


def method_of(method) -> int:
    """SESRQ_DEMOSAIC_* of "bilinear" / "malvar" (or of the constant itself)."""
    if isinstance(method, str) and method.lower() in METHODS:
        return METHODS.index(method.lower())
    if method in (BILINEAR, MALVAR) and not isinstance(method, bool):
        return int(method)
    raise ValueError(f"demosaic method {method!r}: one of {METHODS}")


def _out(out, shape, device):
    """A caller's output is written through its data_ptr(): only a contiguous fp32 tensor of the output shape on the device will do."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != device
            or not out.is_contiguous()):
        raise ValueError(f"demosaic: out must be a contiguous float32 tensor of the output shape {tuple(shape)} on {device}")
    return out


def launch(fmt, method: int, raw, W, S, out, stream):
    """Enqueue the demosaic of the contiguous (N, H, S bytes) `raw` of W pixels a row in `fmt` into the caller-owned `out`."""
    cf = fmt.c()
    if lib().sesrq_demosaic_raw(C.byref(cf), raw.data_ptr(), S, method, out.data_ptr(), raw.shape[0], raw.shape[1], W,
                                stream.cuda_stream) != 0:
        raise ValueError(last_error())


def launch_spread(cfa: str, method: int, spread, out, stream):
    """Enqueue the demosaic of the contiguous (N, 3, H, W) fp32 `spread` of CFA order `cfa` into the caller-owned `out`."""
    N, _, H, W = spread.shape
    if lib().sesrq_demosaic_spread(sensor.CFAS.index(cfa), spread.data_ptr(), method, out.data_ptr(), N, H, W, stream.cuda_stream) != 0:
        raise ValueError(last_error())


def run(raw, fmt, method="malvar", out=None, stream=None, stride: int = None, width: int = None):
    """raw in `fmt` (a sesrq.sensor.Format) on a HIP device, as sensor.unpack takes it (see sensor.frames; `stride` and `width` for
    padded rows) -> the demosaiced frame (N, 3, H, W) fp32.  One kernel, enqueued on `stream` (default: current), not synchronised."""
    import torch
    m, fmt = method_of(method), sensor._fmt(fmt)
    if not isinstance(raw, torch.Tensor) or raw.device.type != "cuda":
        raise ValueError("the raw frame must be a tensor on a HIP device")
    dev = raw.device
    raw, W, S = sensor.frames(raw, fmt, dev, stride, width)
    with torch.cuda.device(dev):
        raw = raw.contiguous()
        out = _out(out, (raw.shape[0], 3, raw.shape[1], W), dev)
        launch(fmt, m, raw, W, S, out, _lib.enter_stream(dev, stream, raw, out))
    return out


def run_spread(spread, cfa="rggb", method="malvar", out=None, stream=None):
    """spread: (N, 3, H, W) fp32 on a HIP device, a frame of CFA order `cfa` with each pixel's sample in the plane of its site channel
    (what sensor.unpack, noise.apply and unprocess.run write with want_spread) -> the demosaiced frame (N, 3, H, W) fp32.  The two
    other planes' values at a pixel do not matter.  One kernel, enqueued on `stream` (default: current), not synchronised."""
    import torch
    m, cfa = method_of(method), str(cfa).lower()
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
            raise ValueError("demosaic: out must not be the spread frame (a pixel's neighbours are read after it is written)")
        launch_spread(cfa, m, spread, out, _lib.enter_stream(dev, stream, spread, out))
    return out
