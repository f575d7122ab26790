"""YUV 4:2:0 video frames (NV12 / I420) into and out of the RGB super-resolution nets (SESR-x2, MFLAG 6: 3 channels in, 3 out; BT.601
studio range, chroma centre sited).  A decoder's surface goes to the device as it is (1.5 B/px) and one kernel makes the net's input
of it: chroma upscaled bicubically to 4:4:4, YCbCr -> RGB bytes, each byte through the net's per-code table.  One kernel takes the
net's prediction back to a 4:2:0 surface: RGB bytes as the PNG export forms them, BT.601 luma, chroma averaged over 2 x 2 blocks.  No
RGB image and no full-resolution chroma plane is held in memory on the way.

The reference has no video path; include/sesrq_video_rgb.h fixes the arithmetic, every step taken from a sibling where one exists, and
libsesrq_video_rgb.so (a library of its own) runs it.  There is no CPU path.  Surfaces, files and uploads are sesrq.video's:
``Surface``, ``load_yuv``, ``save_yuv``, ``to_device``, ``check_out``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import Y_F32, Y_I8  # noqa: F401  (the dtype codes of a prediction: SESRQ_VIDEO_F32 / _I8)
from .video import FORMATS, I420, NV12, Surface, SurfaceDesc, _format, _on_device, check_out, load_yuv, save_yuv, to_device  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_video_rgb.so"))

CODES = 256
TILE_W, TILE_H = 128, 32            # SESRQ_VIDEO_RGB_TILE_W / _H: the luma tile of a decode workgroup
EXPORT_BLOCK_W, EXPORT_LANES = 16, 256      # SESRQ_VIDEO_RGB_EXPORT_BLOCK_W / _LANES: a lane's 16 x 2 block, blocks a workgroup

# every symbol include/sesrq_video_rgb.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_video_rgb_table": (C.c_int, [C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sesrq_video_rgb_create": (C.c_int, [C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_video_rgb_destroy": (None, [C.c_void_p]),
    "sesrq_video_rgb_decode": (C.c_int, [C.c_void_p, C.POINTER(SurfaceDesc), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p]),
    "sesrq_video_rgb_export": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.POINTER(SurfaceDesc), C.c_int, C.c_int, C.c_int,
                                         C.c_void_p]),
    "sesrq_video_rgb_instance_count": (C.c_int, []),
    "sesrq_video_rgb_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_video_rgb_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_video_rgb_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.video_rgb", "sesrq_video_rgb")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


def table(scale_in: float, zero_in: int, exact_div: int = 0):
    """Every RGB byte code (host): (q0 int8 (256,), x fp32 (256,)) with x = clip(fl32(v / 255.0), 0, 1) -- sesrq.image.table's."""
    q, x = np.empty(CODES, np.int8), np.empty(CODES, np.float32)
    if lib().sesrq_video_rgb_table(float(np.float32(scale_in)), int(zero_in), int(exact_div), q.ctypes.data, x.ctypes.data) != 0:
        raise ValueError(last_error())
    return q, x


def launch_decode(device, scale_in, zero_in, exact_div, src: Surface, q0, x, stream) -> None:
    """Enqueue one decode of `src` into caller-owned contiguous q0 / x (N, 3, H, W) (either may be None) on `stream`."""
    h = _so.context(device, scale_in, zero_in, exact_div)
    d = src.desc()
    rc = lib().sesrq_video_rgb_decode(h, C.byref(d), q0.data_ptr() if q0 is not None else None, x.data_ptr() if x is not None else None,
                                      src.N, src.H, src.W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def decode(engine_or_bundle, surface: Surface, want_q: bool = True, want_f: bool = False, stream=None):
    """surface: a Surface on a HIP device -> (q0 int8 (N, 3, H, W) | None, x fp32 (N, 3, H, W) | None), planes R, G, B.

    q0 is in the input domain of the net (engine.bundle or the bundle itself: scale[0], zero[0]; an Engine also fixes how x / s0 is
    formed, its exact_div); x = clip(fl32(v / 255.0), 0, 1) of each RGB byte v is the fp32 frame (engine_or_bundle may be None when
    only x is asked for).  Enqueued on `stream` (default: current), not synchronised."""
    import torch
    if not (want_q or want_f):
        raise ValueError("decode: ask for q0, x or both")
    b, scale_in, zero_in, exact_div, dev = _lib.input_domain(engine_or_bundle, want_q, "decode")
    if b is not None and b.in_channels != 3:
        raise ValueError(f"decode: the RGB decode of a video surface feeds RGB nets (3 channels in); this net takes {b.in_channels}: "
                         "luma nets go through sesrq.video")
    s = _on_device(surface, dev, "decode")
    dev = s.device
    with torch.cuda.device(dev):
        q0 = torch.empty((s.N, 3, s.H, s.W), dtype=torch.int8, device=dev) if want_q else None
        x = torch.empty((s.N, 3, s.H, s.W), dtype=torch.float32, device=dev) if want_f else None
        launch_decode(dev, scale_in, zero_in, exact_div, s, q0, x, _lib.enter_stream(dev, stream, *s.planes(), q0, x))
    return q0, x


def launch_export(pred, scale, zero, out: Surface, stream) -> None:
    """Enqueue one export of the contiguous prediction `pred` (N, 3, H, W) into the caller-owned `out` of H x W on `stream`."""
    import torch
    dt = Y_F32 if pred.dtype == torch.float32 else Y_I8
    do = out.desc()
    rc = lib().sesrq_video_rgb_export(pred.data_ptr(), dt, float(np.float32(scale)), int(zero), C.byref(do), out.N, out.H, out.W,
                                      stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def _pred_domain(pred, scale, zero):
    """(scale, zero) an export passes on with the prediction: (N, 3, H, W) on a HIP device, fp32 -- (0.0, 0) -- or int8 with the
    net's output domain."""
    import torch
    if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or pred.shape[1] != 3 or min(pred.shape) < 1:
        raise ValueError(f"export: the prediction is a (N, 3, H, W) tensor, got "
                         f"{tuple(pred.shape) if isinstance(pred, torch.Tensor) else type(pred).__name__}")
    if pred.device.type != "cuda":
        raise ValueError("export: the prediction must be on a HIP device")
    if pred.dtype == torch.float32:
        return 0.0, 0
    if pred.dtype != torch.int8:
        raise ValueError("export: the prediction must be float32 or int8")
    if scale is None or zero is None:
        raise ValueError("export: an int8 prediction needs the output domain: scale and zero")
    return scale, zero


def export(pred, fmt=None, scale=None, zero=None, out=None, stream=None) -> Surface:
    """pred: the net's prediction (N, 3, H, W) on a HIP device, fp32, or int8 with the net's output domain (scale =
    f32(input.L.scale), zero = zero[L]) -> the Surface of H x W: RGB bytes as sesrq.image.export forms them, converted to BT.601
    studio YCbCr, chroma averaged over 2 x 2 blocks (include/sesrq_video_rgb.h).  fmt: the output's pixel format (default: out's,
    else nv12); out: a Surface of that size on the same device to write into.  Enqueued on `stream` (default: current), not
    synchronised."""
    import torch
    s, z = _pred_domain(pred, scale, zero)
    dev = pred.device
    N, _, H, W = pred.shape
    f = _format(fmt) if fmt is not None else (out.fmt if isinstance(out, Surface) else NV12)
    if out is not None:
        check_out(out, f, N, H, W, dev)
    with torch.cuda.device(dev):
        pred = pred.contiguous()
        if out is None:
            out = Surface.alloc(f, N, H, W, dev)
        launch_export(pred, s, z, out, _lib.enter_stream(dev, stream, pred, *out.planes()))
    return out
