"""The super-resolution nets' input from the HR image: a bicubic x2 / x4 downscale of the 8-bit ground truth, fused with the image
decode into the net's q0 / fp32 input.

The reference's dataset (self_dataset_sr.py) reads a pre-made LR file (LRbicx4 / LRbicx2, made by MATLAB's imresize from the
mod-12-cropped HR image) next to every HR image.  Here the HR image -- which goes to the device anyway, to be scored -- is the only
upload: libsesrq_downscale.so (C ABI include/sesrq_downscale.h, which fixes the arithmetic: Keys a = -1/2 stretched by r, exact
integer weights, mirrored edges, the vertical pass first, a uint8 intermediate between the passes) makes the LR image, and in the
same kernel decodes it exactly as sesrq.image does, so the LR image need not exist in memory at all.  There is no CPU path.

That arithmetic is meant to reproduce MATLAB's ``imresize(img, 1 / r, 'bicubic')`` on uint8; that is intent, not a pinned fact (no
MATLAB output has been compared).  The one outside anchor is PIL's BICUBIC resize, which it equals away from the border.

``weights`` gives the integer weights, ``modcrop`` the top-left crop the datasets' GTmod12 folders were made with, ``downscale`` the
LR image, ``decode`` the net's q0 / fp32 input straight from the HR image.  Byte order: ``"rgb"`` (PIL) or ``"bgr"`` (cv2).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_downscale.so"))

Y, RGB = 0, 1                       # SESRQ_DOWNSCALE_Y / SESRQ_DOWNSCALE_RGB: sesrq.image's forms
FORMS = {"y": Y, "rgb": RGB}
CHANNELS = {Y: 1, RGB: 3}
ORDERS = {"rgb": 0, "bgr": 1}
FACTORS = (2, 4)
MFLAG_FACTORS = {5: 4, 6: 2}        # SESR-x4 (Y), SESR-x2 (RGB)
TILE_W, TILE_H = 32, 8              # SESRQ_DOWNSCALE_TILE_W / _H: the kernel's LR tile at r = 4 (twice that each way at r = 2)

# every symbol include/sesrq_downscale.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_downscale_weights": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "sesrq_downscale_create": (C.c_int, [C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_downscale_destroy": (None, [C.c_void_p]),
    "sesrq_downscale_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p]),
    "sesrq_downscale_instance_count": (C.c_int, []),
    "sesrq_downscale_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_downscale_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_downscale_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.downscale", "sesrq_downscale")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


def factor_of(mflag: int) -> int:
    """The downscale factor of a network's input: 5 (SESR-x4) -> 4, 6 (SESR-x2) -> 2."""
    if mflag not in MFLAG_FACTORS:
        raise ValueError(f"MFLAG {mflag}: an HR image is downscaled for the super-resolution nets only (5: SESR-x4, 6: SESR-x2)")
    return MFLAG_FACTORS[mflag]


def _factor(r) -> int:
    if r not in FACTORS:
        raise ValueError(f"scale factor {r!r}: the HR image is downscaled by 2 or 4")
    return int(r)


def _form(form) -> int:
    f = FORMS.get(str(form).lower()) if not isinstance(form, int) else (form if form in (Y, RGB) else None)
    if f is None:
        raise ValueError(f"image form {form!r}: 'y' (MFLAG 5) or 'rgb' (MFLAG 6)")
    return f


def _order(order) -> int:
    o = ORDERS.get(str(order).lower())
    if o is None:
        raise ValueError(f"byte order {order!r}: 'rgb' (PIL) or 'bgr' (cv2)")
    return o


def weights(r: int):
    """The integer weights (host): (w int16 (4 r,), D) -- LR index d takes the HR taps r d - 3 r / 2 + k, k = 0 .. 4 r - 1, with
    weights w[k] / D."""
    w, D = np.empty(4 * int(r) if r in FACTORS else 1, np.int16), C.c_int()
    if lib().sesrq_downscale_weights(int(r), w.ctypes.data, C.byref(D)) != 0:
        raise ValueError(last_error())
    return w, int(D.value)


def modcrop(img, m: int = 12):
    """The top-left crop of a (H, W, 3) or (N, H, W, 3) image (numpy or torch) to multiples of `m` each way, as a view: how the
    datasets' GTmod12 folders were made (12 is a multiple of every factor)."""
    if int(m) < 1:
        raise ValueError(f"modcrop: m = {m!r} must be a positive integer")
    if img.ndim not in (3, 4) or img.shape[-1] != 3:
        raise ValueError(f"modcrop: an image is interleaved (H, W, 3) or (N, H, W, 3), got {tuple(img.shape)}")
    H, W = img.shape[-3], img.shape[-2]
    if H < m or W < m:
        raise ValueError(f"modcrop: an image of {H} x {W} has no {m} x {m} pixels to keep")
    return img[..., :H - H % m, :W - W % m, :]


def hr_images(hr_u8, r, device=None, who: str = "downscale"):
    """(N, H, W, 3) view of an HR image (N, H, W, 3) / (H, W, 3) torch.uint8 whose size is a multiple of r each way; the device is
    checked last (`device` None: any HIP device), so that every other refusal needs none."""
    import torch
    r = _factor(r)
    if not isinstance(hr_u8, torch.Tensor) or hr_u8.dtype != torch.uint8:
        raise ValueError(f"{who}: an 8-bit image must be a torch.uint8 tensor (N, H, W, 3) or (H, W, 3)")
    img = hr_u8.unsqueeze(0) if hr_u8.dim() == 3 else hr_u8
    if img.dim() != 4 or img.shape[3] != 3 or min(img.shape) < 1:
        raise ValueError(f"{who}: an 8-bit image is interleaved (N, H, W, 3) or (H, W, 3), got {tuple(hr_u8.shape)}")
    if img.shape[1] % r or img.shape[2] % r:
        raise ValueError(f"{who}: an HR image of {img.shape[1]} x {img.shape[2]} is no multiple of r = {r} each way; crop it first "
                         "(sesrq.downscale.modcrop)")
    return img


def _on_device(img, device, who):
    if device is not None and img.device != device:
        raise ValueError(f"{who}: image is on {img.device}, expected {device}")
    if img.device.type != "cuda":
        raise ValueError(f"{who}: the image must be on a HIP device")


def check_out(out, shape, device, who: str = "downscale"):
    """A caller-supplied output is written through its data_ptr(): anything but a contiguous uint8 tensor of the output shape on the
    image's device is refused before any launch."""
    import torch
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or out.device != device
            or not out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous uint8 tensor of the output shape {tuple(shape)} on {device}")


def launch(device, scale_in, zero_in, exact_div, img, order, r, form, lr, q0, x, stream):
    """Enqueue one run on the (N, H, W, 3) contiguous uint8 HR `img` into caller-owned lr / q0 / x (any may be None) on `stream`."""
    N, H, W, _ = img.shape
    dec = q0 is not None or x is not None
    h = _so.context(device, scale_in, zero_in, exact_div) if dec else None
    rc = lib().sesrq_downscale_run(h, img.data_ptr(), _order(order), int(r), _form(form) if dec else 0,
                                   lr.data_ptr() if lr is not None else None, q0.data_ptr() if q0 is not None else None,
                                   x.data_ptr() if x is not None else None, N, H, W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def downscale(hr_u8, r: int, order: str = "rgb", out=None, stream=None):
    """hr_u8: (N, H, W, 3) or (H, W, 3) torch.uint8 on a HIP device, H and W multiples of r (2 or 4) -> the LR image, device uint8
    (N, H / r, W / r, 3) in the same order.  out: a contiguous uint8 tensor of that shape to write into.  Enqueued on `stream`
    (default: current), not synchronised."""
    import torch
    _order(order)
    img = hr_images(hr_u8, r)
    N, H, W, _ = img.shape
    shape = (N, H // r, W // r, 3)
    if out is not None:
        check_out(out, shape, img.device)
    _on_device(img, None, "downscale")
    dev = img.device
    with torch.cuda.device(dev):
        img = img.contiguous()
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        launch(dev, 1.0, 0, 0, img, order, r, None, out, None, None, _lib.enter_stream(dev, stream, img, out))
    return out


def decode(engine_or_bundle, hr_u8, r: int, form, order: str = "rgb", want_q: bool = True, want_f: bool = False, stream=None):
    """hr_u8: (N, H, W, 3) or (H, W, 3) torch.uint8 HR images on a HIP device -> (q0 int8 (N, C, H / r, W / r) | None, x fp32 likewise |
    None): sesrq.image.decode of the downscaled image, which is never written.  C = 1 for form "y", 3 for "rgb"; the input domain
    comes from engine_or_bundle as in sesrq.image.decode (None when only x is asked for).  Enqueued on `stream`, not synchronised."""
    import torch
    f = _form(form)
    _order(order)
    if not (want_q or want_f):
        raise ValueError("decode: ask for q0, x or both")
    img = hr_images(hr_u8, r, who="decode")
    b, scale_in, zero_in, exact_div, dev = _lib.input_domain(engine_or_bundle, want_q, "decode")
    if b is not None and b.in_channels != CHANNELS[f]:
        raise ValueError(f"image form {form!r} gives {CHANNELS[f]} channel(s); this net takes {b.in_channels}")
    _on_device(img, dev, "decode")
    dev = img.device
    N, H, W, _ = img.shape
    shape = (N, CHANNELS[f], H // r, W // r)
    with torch.cuda.device(dev):
        img = img.contiguous()
        q0 = torch.empty(shape, dtype=torch.int8, device=dev) if want_q else None
        x = torch.empty(shape, dtype=torch.float32, device=dev) if want_f else None
        launch(dev, scale_in, zero_in, exact_div, img, order, r, f, None, q0, x, _lib.enter_stream(dev, stream, img, q0, x))
    return q0, x
