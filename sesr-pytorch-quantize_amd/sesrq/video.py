"""YUV 4:2:0 video frames (NV12 / I420) into and out of the luma super-resolution nets (SESR-x4, MFLAG 5: Y in, Y out, BT.601 studio
range).  A decoder's surface goes to the device as it is (1.5 B/px): its Y plane is the net's input, its chroma planes are upscaled
bicubically on the HR side and leave with the net's luma as a 4:2:0 surface again -- no RGB on the way.

The reference has no video path; include/sesrq_video.h fixes the arithmetic, every step taken from a sibling (the image library's
per-code decode and byte export, the colour library's exact-integer Keys bicubic), and libsesrq_video.so (a library of its own) runs
it.  There is no CPU path.  Bytes are taken as they are: studio range is what the net was trained on, a full-range stream is the
caller's to convert.  Chroma is centre sited.

``Surface`` describes a batch of frames as planes with pitches (a contiguous ``.yuv`` file frame and a decoder's pitched surface alike),
``load_yuv`` / ``save_yuv`` read and write raw ``.yuv`` files, ``decode`` gives the net's q0 (and the fp32 frame) of a surface's Y plane,
``export`` the HR surface from the net's luma and the LR surface's chroma.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import FACTORS, Y_F32, Y_I8  # noqa: F401  (FACTORS: a public name of this module)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_video.so"))

CODES = 256
NV12, I420 = 0, 1                   # SESRQ_VIDEO_NV12 / SESRQ_VIDEO_I420
FORMATS = {"nv12": NV12, "i420": I420}
TILE_OUT_W, TILE_OUT_H = 128, 32    # SESRQ_VIDEO_TILE_OUT_W / _H: the output-luma tile of an export workgroup


class SurfaceDesc(C.Structure):
    """sesrq_video_surface (include/sesrq_video.h)."""
    _fields_ = [("format", C.c_int), ("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p), ("pitch_y", C.c_int64),
                ("pitch_c", C.c_int64), ("frame_y", C.c_int64), ("frame_c", C.c_int64)]


# every symbol include/sesrq_video.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_video_table": (C.c_int, [C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sesrq_video_create": (C.c_int, [C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_video_destroy": (None, [C.c_void_p]),
    "sesrq_video_decode": (C.c_int, [C.c_void_p, C.POINTER(SurfaceDesc), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_video_export": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.POINTER(SurfaceDesc), C.c_int, C.POINTER(SurfaceDesc),
                                     C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_video_instance_count": (C.c_int, []),
    "sesrq_video_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_video_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_video_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.video", "sesrq_video")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


def _format(fmt) -> int:
    f = FORMATS.get(str(fmt).lower()) if not isinstance(fmt, int) else (fmt if fmt in (NV12, I420) else None)
    if f is None:
        raise ValueError(f"pixel format {fmt!r}: 'nv12' (Y, then interleaved Cb,Cr) or 'i420' (Y, Cb, Cr)")
    return f


def _factor(r) -> int:
    return _lib.chroma_factor(r, "video")


def _size(H, W):
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"a frame is at least 1 x 1, got {H} x {W}")
    return int(H), int(W)


def chroma_size(H: int, W: int):
    """(rows, samples a row) of each chroma plane of an H x W frame: halves, rounded up."""
    return (int(H) + 1) // 2, (int(W) + 1) // 2


def plane_shapes(fmt, H: int, W: int):
    """[(rows, bytes a row)] of the planes of one frame in file order: Y, then Cb,Cr interleaved (NV12) or Cb and Cr (I420)."""
    hc, wc = chroma_size(H, W)
    return [(H, W), (hc, 2 * wc)] if _format(fmt) == NV12 else [(H, W), (hc, wc), (hc, wc)]


def frame_bytes(fmt, H: int, W: int) -> int:
    """Bytes of one unpadded H x W frame of a raw .yuv file: H W + 2 ceil(H / 2) ceil(W / 2)."""
    H, W = _size(H, W)
    return sum(r * b for r, b in plane_shapes(fmt, H, W))


def table(scale_in: float, zero_in: int, exact_div: int = 0):
    """Every Y byte code (host): (q0 int8 (256,), x fp32 (256,)) with x = clip(fl32(v / 255.0), 0, 1) -- sesrq.image.table's."""
    q, x = np.empty(CODES, np.int8), np.empty(CODES, np.float32)
    if lib().sesrq_video_table(float(np.float32(scale_in)), int(zero_in), int(exact_div), q.ctypes.data, x.ctypes.data) != 0:
        raise ValueError(last_error())
    return q, x


def weights(r: int):
    """The bicubic weight table of the chroma upscale (host): sesrq.colour.weights -- one table serves both libraries."""
    from . import colour
    return colour.weights(r)


# ------------------------------------------------------------------------------------------------------------------ surfaces
def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def _strides(a):
    """Strides of a plane in bytes (uint8: elements)."""
    return tuple(a.stride()) if _is_torch(a) else tuple(a.strides)


class Surface:
    """A batch of N 4:2:0 frames of H x W luma: planes plus layout.

    y: (N, H, W) uint8; NV12: c0 (N, ceil(H/2), 2 ceil(W/2)) interleaved Cb,Cr; I420: c0, c1 (N, ceil(H/2), ceil(W/2)) Cb and Cr.
    Planes are numpy arrays (host) or torch tensors (host or device), all of one kind and on one device; they may be views: the last
    stride must be 1, the row stride is the pitch and the batch stride the frame stride, so a decoder's pitched surface and a
    contiguous .yuv file frame are both described.  The two planes of I420 share pitch and frame stride.  `buf` is the one buffer the
    planes are views of, where there is one (load_yuv, alloc): it moves between host and device in one copy."""

    def __init__(self, fmt, H: int, W: int, y, c0, c1=None, buf=None):
        self.fmt = _format(fmt)
        self.H, self.W = _size(H, W)
        self.y, self.c0, self.c1, self.buf = y, c0, (c1 if self.fmt == I420 else None), buf
        planes = self.planes()
        if any(p is None for p in planes):
            raise ValueError(f"surface: {'nv12 has the planes y and c0' if self.fmt == NV12 else 'i420 has the planes y, c0 and c1'}")
        if len({_is_torch(p) for p in planes}) != 1 or not all(_is_torch(p) or isinstance(p, np.ndarray) for p in planes):
            raise ValueError("surface: the planes are numpy arrays or torch tensors, all of one kind")
        if y.ndim != 3:
            raise ValueError(f"surface: the Y plane is (N, H, W), got {tuple(y.shape)}")
        self.N = int(y.shape[0])
        if self.N < 1:
            raise ValueError("surface: no frames")
        for p, (rows, nbytes), name in zip(planes, plane_shapes(self.fmt, self.H, self.W), ("y", "c0", "c1")):
            if tuple(p.shape) != (self.N, rows, nbytes):
                raise ValueError(f"surface: plane {name} of {self.N} {self.fmt_name} frames of {self.H} x {self.W} is "
                                 f"{(self.N, rows, nbytes)} uint8, got {tuple(p.shape)}")
            if str(p.dtype).split(".")[-1] != "uint8":
                raise ValueError(f"surface: plane {name} must be uint8, got {p.dtype}")
            st = _strides(p)
            if st[2] != 1 or st[1] < nbytes or st[0] < 0:
                raise ValueError(f"surface: plane {name} has strides {st}: bytes of a row are adjacent, the pitch is at least the "
                                 f"row's {nbytes} bytes")
            if self.N > 1 and st[0] < (rows - 1) * st[1] + nbytes and st[0] != 0:
                raise ValueError(f"surface: plane {name} has a frame stride of {st[0]}, below the plane's extent")
        if self.is_torch and len({p.device for p in planes}) != 1:
            raise ValueError("surface: the planes are on different devices")
        if self.fmt == I420 and _strides(self.c0)[0 if self.N > 1 else 1:2] != _strides(self.c1)[0 if self.N > 1 else 1:2]:
            raise ValueError("surface: the Cb and Cr planes of i420 share one pitch and one frame stride")

    fmt_name = property(lambda s: "nv12" if s.fmt == NV12 else "i420")
    is_torch = property(lambda s: _is_torch(s.y))
    device = property(lambda s: s.y.device if _is_torch(s.y) else None)
    pitch_y = property(lambda s: _strides(s.y)[1])
    pitch_c = property(lambda s: _strides(s.c0)[1])
    frame_y = property(lambda s: _strides(s.y)[0])
    frame_c = property(lambda s: _strides(s.c0)[0])

    def planes(self):
        return [self.y, self.c0] + ([self.c1] if self.fmt == I420 else [])

    tensors = planes

    @staticmethod
    def views(buf, fmt, N: int, H: int, W: int, pitch_y=None, pitch_c=None) -> "Surface":
        """The surface laid over the 1-D uint8 buffer `buf` (numpy or torch) in file order, frame after frame: each frame its Y rows,
        then its chroma rows.  pitch_y / pitch_c: bytes between rows (default: the row's bytes, a raw .yuv file)."""
        f = _format(fmt)
        H, W = _size(H, W)
        shapes = plane_shapes(f, H, W)
        pitches = [int(pitch_y or W)] + [int(pitch_c or shapes[1][1])] * (len(shapes) - 1)
        if any(p < s[1] for p, s in zip(pitches, shapes)):
            raise ValueError(f"surface: a pitch of {pitches} is below its row's bytes")
        frame = sum(s[0] * p for s, p in zip(shapes, pitches))
        if buf.ndim != 1 or buf.shape[0] < N * frame or N < 1:
            raise ValueError(f"surface: {N} frames of {frame} bytes need a 1-D buffer of {N * frame} bytes, got {tuple(buf.shape)}")
        planes, off = [], 0
        for (rows, nbytes), pitch in zip(shapes, pitches):
            if _is_torch(buf):
                planes.append(buf.as_strided((N, rows, nbytes), (frame, pitch, 1), buf.storage_offset() + off))
            else:
                planes.append(np.lib.stride_tricks.as_strided(buf[off:], (N, rows, nbytes), (frame, pitch, 1)))
            off += rows * pitch
        return Surface(f, H, W, *planes, buf=buf)

    @staticmethod
    def alloc(fmt, N: int, H: int, W: int, device=None, pitch_y=None, pitch_c=None) -> "Surface":
        """An uninitialised surface in one buffer: torch on `device`, numpy when device is None."""
        f = _format(fmt)
        H, W = _size(H, W)
        shapes = plane_shapes(f, H, W)
        n = int(N) * (H * int(pitch_y or W) + sum(s[0] for s in shapes[1:]) * int(pitch_c or shapes[1][1]))
        if device is None:
            buf = np.empty(n, np.uint8)
        else:
            import torch
            buf = torch.empty(n, dtype=torch.uint8, device=device)
        return Surface.views(buf, f, int(N), H, W, pitch_y, pitch_c)

    def desc(self) -> SurfaceDesc:
        """The C struct of a torch surface."""
        if not self.is_torch:
            raise ValueError("surface: the planes must be torch tensors on a HIP device")
        return SurfaceDesc(self.fmt, self.y.data_ptr(), self.c0.data_ptr(), self.c1.data_ptr() if self.c1 is not None else None,
                           self.pitch_y, self.pitch_c, self.frame_y, self.frame_c)

    def cpu(self) -> "Surface":
        """The surface with numpy planes (a torch surface is copied to the host)."""
        if not self.is_torch:
            return self
        if self.buf is not None:
            return Surface.views(self.buf.cpu().numpy(), self.fmt, self.N, self.H, self.W, self.pitch_y, self.pitch_c)
        return Surface(self.fmt, self.H, self.W, *[p.cpu().numpy() for p in self.planes()])

    def tobytes(self) -> bytes:
        """The frames as a raw .yuv file holds them: unpadded rows, plane after plane, frame after frame."""
        s = self.cpu()
        return b"".join(np.ascontiguousarray(p[n]).tobytes() for n in range(s.N) for p in s.planes())

    def __getitem__(self, frames) -> "Surface":
        """The frames of a slice, as views."""
        if not isinstance(frames, slice):
            raise TypeError("surface[a:b]: a slice of frames")
        return Surface(self.fmt, self.H, self.W, *[p[frames] for p in self.planes()])


def load_yuv(path: str, W: int, H: int, fmt, frames=None) -> Surface:
    """A raw .yuv file of unpadded W x H frames in `fmt` as a host Surface.  frames: (first, end) to read a part of the sequence."""
    f = _format(fmt)
    H, W = _size(H, W)
    fb = frame_bytes(f, H, W)
    size = os.path.getsize(path)
    if size == 0 or size % fb:
        raise ValueError(f"{path}: {size} bytes are no whole number of {W}x{H} {'nv12' if f == NV12 else 'i420'} frames of {fb} bytes")
    total = size // fb
    a, b = (0, total) if frames is None else (int(frames[0]), total if frames[1] is None else int(frames[1]))
    if not 0 <= a < b <= total:
        raise ValueError(f"{path}: frames {a}:{b} of a file of {total}")
    buf = np.fromfile(path, dtype=np.uint8, count=(b - a) * fb, offset=a * fb)
    return Surface.views(buf, f, b - a, H, W)


def save_yuv(path: str, surface: Surface, append: bool = False) -> None:
    """Write (or append) the frames of a surface (host or device) as a raw .yuv file: unpadded rows."""
    with open(path, "ab" if append else "wb") as fh:
        fh.write(surface.tobytes())


def to_device(surface: Surface, device=None) -> Surface:
    """The surface on a HIP device (default: the current one).  A surface in one buffer goes up in one copy and keeps its layout;
    any other is copied plane by plane into unpadded planes.  A surface already there is returned as it is."""
    import torch
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if surface.is_torch and surface.device == dev:
        return surface
    if surface.buf is not None:
        return Surface.views(_lib.host_tensor(surface.buf).to(dev, non_blocking=True), surface.fmt, surface.N, surface.H, surface.W,
                             surface.pitch_y, surface.pitch_c)
    return Surface(surface.fmt, surface.H, surface.W, *[_lib.host_tensor(p).to(dev).contiguous() for p in surface.planes()])


def _on_device(surface, device, who: str) -> Surface:
    if not isinstance(surface, Surface):
        raise ValueError(f"{who}: a sesrq.video.Surface, got {type(surface).__name__}")
    if not surface.is_torch or surface.device.type != "cuda":
        raise ValueError(f"{who}: the surface must be on a HIP device (video.to_device)")
    if device is not None and surface.device != device:
        raise ValueError(f"{who}: the surface is on {surface.device}, expected {device}")
    return surface


def check_out(out, fmt, N: int, H: int, W: int, device, who: str = "export") -> None:
    """A caller-supplied output surface is written through its pointers: anything but a surface of N frames of H x W on the device is
    refused before any launch (shape, dtype and pitches are the Surface's own checks)."""
    if not isinstance(out, Surface) or not out.is_torch or (out.N, out.H, out.W) != (N, H, W) or out.device != device or \
            (fmt is not None and out.fmt != _format(fmt)) or (N > 1 and (out.frame_y == 0 or out.frame_c == 0)):
        raise ValueError(f"{who}: out must be a Surface of {N} frame(s) of {H} x {W}"
                         f"{'' if fmt is None else ' in ' + ('nv12' if _format(fmt) == NV12 else 'i420')} on {device}")


# ------------------------------------------------------------------------------------------------------------------ device
def launch_decode(device, scale_in, zero_in, exact_div, src: Surface, q0, x, stream) -> None:
    """Enqueue one decode of the Y plane of `src` into caller-owned q0 / x (either may be None) on `stream`."""
    h = _so.context(device, scale_in, zero_in, exact_div)
    d = src.desc()
    rc = lib().sesrq_video_decode(h, C.byref(d), q0.data_ptr() if q0 is not None else None, x.data_ptr() if x is not None else None,
                                  src.N, src.H, src.W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def decode(engine_or_bundle, surface: Surface, want_q: bool = True, want_f: bool = False, stream=None):
    """surface: a Surface on a HIP device -> (q0 int8 (N, 1, H, W) | None, x fp32 (N, 1, H, W) | None) of its Y plane.

    q0 is in the input domain of the net (engine.bundle or the bundle itself: scale[0], zero[0]; an Engine also fixes how x / s0 is
    formed, its exact_div); x = clip(fl32(v / 255.0), 0, 1) is the fp32 frame (engine_or_bundle may be None when only x is asked
    for).  Enqueued on `stream` (default: current), not synchronised."""
    import torch
    if not (want_q or want_f):
        raise ValueError("decode: ask for q0, x or both")
    b, scale_in, zero_in, exact_div, dev = _lib.input_domain(engine_or_bundle, want_q, "decode")
    if b is not None and b.in_channels != 1:
        raise ValueError(f"decode: a video surface feeds luma nets (1 channel in); this net takes {b.in_channels}: RGB nets decode a "
                         "surface through sesrq.video_rgb")
    s = _on_device(surface, dev, "decode")
    dev = s.device
    with torch.cuda.device(dev):
        q0 = torch.empty((s.N, 1, s.H, s.W), dtype=torch.int8, device=dev) if want_q else None
        x = torch.empty((s.N, 1, s.H, s.W), dtype=torch.float32, device=dev) if want_f else None
        launch_decode(dev, scale_in, zero_in, exact_div, s, q0, x, _lib.enter_stream(dev, stream, s.y, q0, x))
    return q0, x


def launch_export(y, scale, zero, lr: Surface, r, out: Surface, stream) -> None:
    """Enqueue one export of the contiguous luma `y` (N, 1, rH, rW) and the chroma of `lr` into the caller-owned `out` on `stream`."""
    import torch
    dt = Y_F32 if y.dtype == torch.float32 else Y_I8
    dl, do = lr.desc(), out.desc()
    rc = lib().sesrq_video_export(y.data_ptr(), dt, float(np.float32(scale)), int(zero), C.byref(dl), int(r), C.byref(do), lr.N, lr.H,
                                  lr.W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def export(y, lr: Surface, r: int, fmt=None, scale=None, zero=None, out=None, stream=None) -> Surface:
    """y: the net's luma (N, 1, rH, rW) fp32, or int8 with the net's output domain (scale = f32(input.L.scale), zero = zero[L]); lr:
    the LR Surface on the same device (its chroma planes are read); r: 2 or 4 -> the HR Surface of rH x rW: the net's luma as bytes
    and lr's chroma upscaled bicubically (include/sesrq_video.h).  fmt: the output's pixel format (default: lr's); out: a Surface
    of that size to write into (its format decides).  Enqueued on `stream` (default: current), not synchronised."""
    import torch
    r = _factor(r)
    lr = _on_device(lr, None, "export")
    dev = lr.device
    N, H, W = lr.N, lr.H, lr.W
    s, z = _lib.luma_domain(y, (N, 1, r * H, r * W), dev, scale, zero, "surface")
    f = _format(fmt) if fmt is not None else (out.fmt if isinstance(out, Surface) else lr.fmt)
    if out is not None:
        check_out(out, f, N, r * H, r * W, dev)
    with torch.cuda.device(dev):
        y = y.contiguous()
        if out is None:
            out = Surface.alloc(f, N, r * H, r * W, dev)
        launch_export(y, s, z, lr, r, out, _lib.enter_stream(dev, stream, y, *lr.planes()[1:], *out.planes()))
    return out
