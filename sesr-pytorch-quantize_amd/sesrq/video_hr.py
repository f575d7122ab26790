"""The super-resolution nets' video input from the HR clip alone: a bicubic x2 / x4 downscale of an 8-bit YUV 4:2:0 surface (NV12 /
I420), fused with the decode of its LR luma into the net's q0 / fp32 input.

Video SR test sets ship HR sequences; the LR side is a bicubic downscale.  Here the HR surface -- which goes to the device anyway, to
be scored -- is the only upload: libsesrq_video_hr.so (C ABI include/sesrq_video_hr.h) downscales each plane (Y, Cb, Cr: centre sited
images of their own) with the arithmetic sesrq.downscale fixed for images -- Keys a = -1/2 stretched by r, exact integer weights,
mirrored edges, the vertical pass first, a uint8 intermediate -- and decodes the LR luma as sesrq.video decodes a surface's, all in ONE
kernel, so image and video scores of one net are comparable.  There is no CPU path.

The HR luma must be a multiple of 2 r each way (``modcrop``), so that the LR luma and both chroma planes divide exactly; odd LR sizes
stay the province of ready-made LR clips (sesrq.video).  ``weights`` gives the integer weights, ``run`` the LR surface and / or the
net's q0 / fp32 input, ``launch`` enqueues into caller-owned buffers.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib, video
from .video import I420, NV12, Surface, SurfaceDesc  # noqa: F401  (public names of this module too)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_video_hr.so"))

FACTORS = (2, 4)
MFLAG_FACTORS = {5: 4, 6: 2}        # SESR-x4 (luma), SESR-x2 (RGB)
TILE_HR_W, TILE_HR_H = 128, 32      # SESRQ_VIDEO_HR_TILE_HR_W / _H: a workgroup's tile in HR luma pixels

# every symbol include/sesrq_video_hr.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_video_hr_weights": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "sesrq_video_hr_create": (C.c_int, [C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_video_hr_destroy": (None, [C.c_void_p]),
    "sesrq_video_hr_run": (C.c_int, [C.c_void_p, C.POINTER(SurfaceDesc), C.c_int, C.POINTER(SurfaceDesc), C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p]),
    "sesrq_video_hr_instance_count": (C.c_int, []),
    "sesrq_video_hr_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_video_hr_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_video_hr_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.video_hr", "sesrq_video_hr")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


def _factor(r) -> int:
    if r not in FACTORS:
        raise ValueError(f"scale factor {r!r}: the HR surface is downscaled by 2 or 4")
    return int(r)


def factor_of(mflag: int) -> int:
    """The downscale factor of a network's input: 5 (SESR-x4) -> 4, 6 (SESR-x2) -> 2."""
    if mflag not in MFLAG_FACTORS:
        raise ValueError(f"MFLAG {mflag}: an HR surface is downscaled for the super-resolution nets only (5: SESR-x4, 6: SESR-x2)")
    return MFLAG_FACTORS[mflag]


def weights(r: int):
    """The integer weights (host): (w int16 (4 r,), D) -- sesrq.downscale.weights: LR index d of a plane takes the HR taps
    r d - 3 r / 2 + k, k = 0 .. 4 r - 1, with weights w[k] / D."""
    w, D = np.empty(4 * int(r) if r in FACTORS else 1, np.int16), C.c_int()
    if lib().sesrq_video_hr_weights(int(r), w.ctypes.data, C.byref(D)) != 0:
        raise ValueError(last_error())
    return w, int(D.value)


def modcrop(surface_or_size, r: int):
    """The top-left crop to multiples of 2 r each way -- what both the LR luma and the chroma planes need to divide exactly: of a
    Surface as views of its planes, of a (H, W) size as the cropped size."""
    m = 2 * _factor(r)
    s = surface_or_size
    H, W = (s.H, s.W) if isinstance(s, Surface) else (int(s[0]), int(s[1]))
    if H < m or W < m:
        raise ValueError(f"modcrop: a frame of {H} x {W} has no {m} x {m} pixels to keep")
    h, w = H - H % m, W - W % m
    if not isinstance(s, Surface):
        return h, w
    if (h, w) == (H, W):
        return s
    cw = w if s.fmt == NV12 else w // 2
    return Surface(s.fmt, h, w, s.y[:, :h, :w], *[p[:, :h // 2, :cw] for p in s.planes()[1:]])


def lr_size(hr: Surface, r: int, who: str = "video_hr"):
    """(H, W) of the LR luma of an HR Surface whose luma is a multiple of 2 r each way."""
    r = _factor(r)
    if not isinstance(hr, Surface):
        raise ValueError(f"{who}: a sesrq.video.Surface, got {type(hr).__name__}")
    if hr.H % (2 * r) or hr.W % (2 * r):
        raise ValueError(f"{who}: an HR frame of {hr.H} x {hr.W} is no multiple of 2 r = {2 * r} each way; crop it first "
                         "(sesrq.video_hr.modcrop)")
    return hr.H // r, hr.W // r


def launch(device, scale_in, zero_in, exact_div, hr: Surface, r, lr, q0, x, stream, lr_luma: bool = True) -> None:
    """Enqueue one run on the device Surface `hr` into the caller-owned LR Surface `lr` (lr_luma False: its chroma planes only), q0
    and x (any may be None) on `stream`."""
    dec = q0 is not None or x is not None
    h = _so.context(device, scale_in, zero_in, exact_div) if dec else None
    dh = hr.desc()
    dl = None
    if lr is not None:
        dl = lr.desc()
        if not lr_luma:
            dl.y = None
    rc = lib().sesrq_video_hr_run(h, C.byref(dh), int(r), C.byref(dl) if dl is not None else None,
                                  q0.data_ptr() if q0 is not None else None, x.data_ptr() if x is not None else None, hr.N, hr.H // int(r),
                                  hr.W // int(r), stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def run(engine_or_bundle, hr: Surface, r: int, fmt=None, want_lr: bool = True, want_q: bool = False, want_f: bool = False, stream=None):
    """hr: a Surface of N HR frames on a HIP device, its luma a multiple of 2 r each way -> (lr Surface | None, q0 int8 (N, 1, H, W) |
    None, x fp32 (N, 1, H, W) | None), H x W = the HR size over r: every plane downscaled bicubically by r, and sesrq.video.decode of the
    LR luma, which need not be written.  fmt: the LR surface's pixel format (default: hr's).  The input domain of q0 comes from
    engine_or_bundle as in sesrq.video.decode (None when q0 is not asked for).  Enqueued on `stream` (default: current), not
    synchronised."""
    import torch
    r = _factor(r)
    if not (want_lr or want_q or want_f):
        raise ValueError("video_hr: ask for the LR surface, q0, x or any of them")
    H, W = lr_size(hr, r)
    b, scale_in, zero_in, exact_div, dev = _lib.input_domain(engine_or_bundle, want_q, "video_hr")
    if b is not None and b.in_channels != 1 and (want_q or want_f):
        raise ValueError(f"video_hr: the LR luma feeds luma nets (1 channel in); this net takes {b.in_channels}: RGB nets decode the LR "
                         "surface through sesrq.video_rgb")
    f = video._format(fmt) if fmt is not None else hr.fmt
    s = video._on_device(hr, dev, "video_hr")
    dev = s.device
    with torch.cuda.device(dev):
        lr = Surface.alloc(f, s.N, H, W, dev) if want_lr else None
        q0 = torch.empty((s.N, 1, H, W), dtype=torch.int8, device=dev) if want_q else None
        x = torch.empty((s.N, 1, H, W), dtype=torch.float32, device=dev) if want_f else None
        st = _lib.enter_stream(dev, stream, *s.planes(), *(lr.planes() if lr is not None else ()), q0, x)
        launch(dev, scale_in, zero_in, exact_div, s, r, lr, q0, x, st)
    return lr, q0, x
