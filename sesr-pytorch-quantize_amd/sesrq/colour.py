"""Colour out of the luma super-resolution nets: the net super-resolves Y, the LR image's Cb and Cr are upscaled bicubically, and
YCbCr goes back to RGB bytes -- the standard completion of a Y-channel SR net, in one fused kernel on the HR side.

The reference stops at the Y score (self_dataset_sr.py: Y in, Y out), so there is nothing of its own to match; include/sesrq_colour.h
fixes the arithmetic (BT.601 studio chroma in Q6 fixed point from the float64 d(v) = v / 255.0, the Keys a = -1/2 bicubic in exact
integers, the inverse matrix in fp32) and libsesrq_colour.so (a library of its own) runs it.  There is no CPU path.

``chroma`` gives the Q6 (Cb, Cr) planes of an image, ``export`` the colour image from the net's luma and the LR image, ``weights``
the bicubic weight table.  Byte order: ``"rgb"`` (PIL) or ``"bgr"`` (cv2); the output is in the order of the input.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import FACTORS, Y_F32, Y_I8

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_colour.so"))

ORDERS = {"rgb": 0, "bgr": 1}
TILE_W, TILE_H = 32, 8              # SESRQ_COLOUR_TILE_W / _H: the export's LR tile at r = 4 (twice that each way at r = 2)

# every symbol include/sesrq_colour.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_colour_weights": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
    "sesrq_colour_chroma": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_colour_export": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p]),
    "sesrq_colour_instance_count": (C.c_int, []),
    "sesrq_colour_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_colour_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_colour_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.colour", "sesrq_colour")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


def _order(order) -> int:
    o = ORDERS.get(str(order).lower())
    if o is None:
        raise ValueError(f"byte order {order!r}: 'rgb' (PIL) or 'bgr' (cv2)")
    return o


def _factor(r) -> int:
    return _lib.chroma_factor(r, "colour")


def weights(r: int):
    """The bicubic weight table (host): (w int16 (r, 4), first int8 (r,)) -- output column r j + phi takes the LR taps
    j + first[phi] + k, k = 0 .. 3, with weights w[phi, k] / 1024."""
    w, first = np.empty((int(r) if r in FACTORS else 1, 4), np.int16), np.empty(int(r) if r in FACTORS else 1, np.int8)
    if lib().sesrq_colour_weights(int(r), w.ctypes.data, first.ctypes.data) != 0:
        raise ValueError(last_error())
    return w, first


def _images(img):
    from .image import _images as images
    return images(img, None)


def chroma(img_u8, order: str = "rgb", stream=None):
    """img_u8: (N, H, W, 3) or (H, W, 3) torch.uint8 on a HIP device -> (N, 2, H, W) torch.int16: the Q6 (Cb, Cr) planes
    (64 * the BT.601 studio chroma, rounded to nearest even).  Enqueued on `stream` (default: current), not synchronised."""
    import torch
    o = _order(order)
    img = _images(img_u8)
    dev = img.device
    N, H, W, _ = img.shape
    with torch.cuda.device(dev):
        img = img.contiguous()
        out = torch.empty((N, 2, H, W), dtype=torch.int16, device=dev)
        st = _lib.enter_stream(dev, stream, img, out)
        rc = lib().sesrq_colour_chroma(img.data_ptr(), o, out.data_ptr(), N, H, W, st.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())
    return out


def check_out(out, shape, device, who: str = "export"):
    """A caller-supplied output is written through its data_ptr(): anything but a contiguous uint8 tensor of the output shape on the
    device is refused before any launch."""
    import torch
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or out.device != device
            or not out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous uint8 tensor of the output shape {tuple(shape)} on {device}")


def launch(y, scale, zero, img, order, r, out, stream):
    """Enqueue one export of the contiguous luma `y` (N, 1, rH, rW) and LR image `img` (N, H, W, 3) into caller-owned `out` on `stream`."""
    import torch
    N, H, W, _ = img.shape
    dt = Y_F32 if y.dtype == torch.float32 else Y_I8
    rc = lib().sesrq_colour_export(y.data_ptr(), dt, float(np.float32(scale)), int(zero), img.data_ptr(), _order(order), int(r),
                                   out.data_ptr(), N, H, W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def export(y, img_u8, r: int, order: str = "rgb", scale=None, zero=None, out=None, stream=None):
    """y: the net's luma (N, 1, rH, rW) fp32, or int8 with the net's output domain (scale = f32(input.L.scale), zero = zero[L]);
    img_u8: the LR image (N, H, W, 3) or (H, W, 3) torch.uint8 in `order`; r: 2 or 4 -> device uint8 (N, rH, rW, 3) in `order`:
    the colour image whose luma is the net's and whose chroma is the LR image's, upscaled bicubically (include/sesrq_colour.h).
    out: a contiguous uint8 tensor of that shape to write into.  Enqueued on `stream` (default: current), not synchronised."""
    import torch
    _order(order)
    r = _factor(r)
    img = _images(img_u8)
    dev = img.device
    N, H, W, _ = img.shape
    s, z = _lib.luma_domain(y, (N, 1, r * H, r * W), dev, scale, zero, "image")
    shape = (N, r * H, r * W, 3)
    if out is not None:
        check_out(out, shape, dev)
    with torch.cuda.device(dev):
        y, img = y.contiguous(), img.contiguous()
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        launch(y, s, z, img, order, r, out, _lib.enter_stream(dev, stream, y, img, out))
    return out
