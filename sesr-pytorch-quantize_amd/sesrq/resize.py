"""Predictions out at any size: the nets' output, or any 8-bit image, resampled bicubically to a free size on the device.

Every other way out of the nets writes the prediction at the net's own size, r x the input.  Filling a display or a delivery size
(720p -> 1080p through the x2 net, a 4K result fitted to a 3840 x 1600 panel) took a host resize of the exported bytes or an fp32
``F.interpolate``.  libsesrq_resize.so (C ABI include/sesrq_resize.h) does it in one kernel, from the int8 or fp32 prediction
itself: the prediction's byte (``image.export``'s), a horizontal and a vertical pass with per-axis tables of integer weights built
on the host.  The arithmetic is Pillow's ``Image.resize(size, Image.BICUBIC)`` on 8-bit images, byte for byte, edges included.
There is no CPU path.

Sizes are (rows, columns) = (Ho, Wo), as in the tensors' shapes (PIL's ``size`` is (Wo, Ho)).  A downscale ratio above 4 on either
axis is refused; upscales are unbounded.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_resize.so"))

MAX_TAPS, MAX_RATIO, BITS = 17, 4, 22          # SESRQ_RESIZE_MAX_TAPS / _MAX_RATIO / _BITS
U8, F32, I8 = 0, 1, 2                          # SESRQ_RESIZE_U8 / _F32 / _I8
ORDERS = _lib.ORDERS

# every symbol include/sesrq_resize.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_resize_coeffs": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sesrq_resize_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_resize_destroy": (None, [C.c_void_p]),
    "sesrq_resize_tile": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sesrq_resize_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_resize_instance_count": (C.c_int, []),
    "sesrq_resize_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_resize_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_resize_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.resize", "sesrq_resize")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances
_order = _lib.byte_order
check_out = _lib.check_u8_out
_plans = {}                                    # (H, W, Ho, Wo, device index) -> Plan; lives as long as the process


def coeffs(n_in: int, n_out: int):
    """The table of one axis (host, no device): (xmin int32 (n_out,), count int32 (n_out,), weights int32 (n_out, 17)); output i is
    clamp((2^21 + sum_x weights[i, x] * src[xmin[i] + x]) >> 22, 0, 255) over x < count[i]."""
    n = max(int(n_out), 0)
    xmin, count, w = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, MAX_TAPS), np.int32)
    if lib().sesrq_resize_coeffs(int(n_in), int(n_out), xmin.ctypes.data, count.ctypes.data, w.ctypes.data) != 0:
        raise ValueError(last_error())
    return xmin, count, w


class Plan:
    """The device context of one H x W -> Ho x Wo resize on one device: both tables, uploaded once, and the output tile."""

    def __init__(self, H, W, Ho, Wo, device):
        import torch
        self.H, self.W, self.Ho, self.Wo, self.device = int(H), int(W), int(Ho), int(Wo), device
        self.handle = C.c_void_p()
        with torch.cuda.device(device):
            if lib().sesrq_resize_create(self.H, self.W, self.Ho, self.Wo, C.byref(self.handle)) != 0:
                raise ValueError(last_error())
        tw, th = C.c_int(), C.c_int()
        lib().sesrq_resize_tile(self.handle, C.byref(tw), C.byref(th))
        self.tile = (tw.value, th.value)       # output pixels of a tile for C = 1 (a third as wide for C = 3), output rows


def plan(H, W, Ho, Wo, device) -> Plan:
    """The Plan of a size pair on `device`, created once per (H, W, Ho, Wo, device)."""
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("resize: a plan lives on a HIP device")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(H), int(W), int(Ho), int(Wo), device.index)
    p = _plans.get(key)
    if p is None:
        p = _plans[key] = Plan(H, W, Ho, Wo, device)
    return p


def run(p: Plan, src, scale=None, zero=None, order: str = "rgb", out=None, stream=None):
    """src on the plan's device: an interleaved (N, H, W, C) uint8 image in RGB order, or a prediction (N, C, H, W), fp32 or int8 with
    the net's output domain (scale, zero) -> device uint8 (N, Ho, Wo, C), C = 1 or 3, interleaved in `order`.  out: a contiguous
    uint8 tensor of that shape to write into.  One kernel on `stream` (default: current), not synchronised."""
    import torch
    o = _order(order)
    if not isinstance(src, torch.Tensor) or src.dim() != 4 or min(src.shape) < 1:
        raise ValueError("resize: the source is a (N, H, W, C) uint8 image or a (N, C, H, W) prediction")
    if src.device != p.device:
        raise ValueError(f"resize: the source is on {src.device}, the plan on {p.device}")
    if src.dtype == torch.uint8:
        dt, (N, H, W, Ch), s, z = U8, src.shape, 0.0, 0
    else:
        s, z = _lib.pred_domain(src, scale, zero, "prediction")
        dt, (N, Ch, H, W) = (F32 if src.dtype == torch.float32 else I8), src.shape
    if Ch not in (1, 3):
        raise ValueError(f"resize: {Ch} channels; an 8-bit image has 1 or 3")
    shape = (N, p.Ho, p.Wo, Ch)
    if out is not None:
        check_out(out, shape, p.device, "resize")
    with torch.cuda.device(p.device):
        src = src.contiguous()
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=p.device)
        st = _lib.enter_stream(p.device, stream, src, out)
        rc = lib().sesrq_resize_run(p.handle, src.data_ptr(), dt, float(np.float32(s)), int(z), Ch, o, out.data_ptr(), N, H, W, p.Ho, p.Wo,
                                    st.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())
    return out


def _size(size):
    try:
        Ho, Wo = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"resize: size {size!r}: (rows, columns)") from None
    return Ho, Wo


def export(pred, size, scale=None, zero=None, order: str = "rgb", out=None, stream=None):
    """image.export at a free size: pred (N, C, H, W) fp32, or int8 with the net's output domain -> device uint8 (N, Ho, Wo, C),
    size = (Ho, Wo): Pillow's bicubic resize of the bytes image.export writes, without those bytes reaching memory.  A uint8
    (N, H, W, C) image is resized as it is."""
    import torch
    if not isinstance(pred, torch.Tensor) or pred.dim() != 4:
        raise ValueError("resize: the prediction is a (N, C, H, W) tensor")
    if pred.device.type != "cuda":
        raise ValueError("resize: the prediction must be on a HIP device")
    Ho, Wo = _size(size)
    H, W = (pred.shape[1], pred.shape[2]) if pred.dtype == torch.uint8 else (pred.shape[2], pred.shape[3])
    return run(plan(H, W, Ho, Wo, pred.device), pred, scale, zero, order, out, stream)
