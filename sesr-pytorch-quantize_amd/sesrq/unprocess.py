"""Raw-net inputs and their ground truth from an sRGB image: the unprocessing step in front of the raw nets (MFLAG 1-4).

The reference's raw frames and 16-bit ground truths come from an external unprocessing project: inverse tone curve, gamma expansion,
rgb2cam, inverse white-balance gains, mosaic.  libsesrq_unprocess.so (C ABI include/sesrq_unprocess.h, which fixes the arithmetic) is
that step as one kernel: an 8-bit image becomes the Bayer frame a sensor would have written, the ground truth, the net's q0 and its
fp32 input frame -- whichever are asked for.  It is the counterpart of sesrq.develop, which takes a net's output back to display bytes.
There is no CPU path.

A `Profile` holds rgb2cam, the inverse gains, the 256-entry table of the inverse tone curve and whether highlights are preserved
(the unprocessing paper's safe_invert_gains); `from_colormatrix` builds one from camera metadata as the reference's
``metadata2tensor`` does, `from_develop` the inverse of a sesrq.develop.Profile.  Byte order: ``"rgb"`` (PIL) or ``"bgr"`` (cv2).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib, sensor
from .develop import RGB2XYZ

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_unprocess.so"))

CODES = 256
PAPER, GAMMA22, SRGB, LINEAR = 0, 1, 2, 3          # SESRQ_UNPROCESS_*
CURVES = {"paper": PAPER, "gamma": GAMMA22, "srgb": SRGB, "linear": LINEAR}
ORDERS = _lib.ORDERS

# every symbol include/sesrq_unprocess.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_unprocess_curve": (C.c_int, [C.c_int, C.c_void_p]),
    "sesrq_unprocess_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                         C.POINTER(C.c_void_p)]),
    "sesrq_unprocess_destroy": (None, [C.c_void_p]),
    "sesrq_unprocess_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p]),
    "sesrq_unprocess_instance_count": (C.c_int, []),
    "sesrq_unprocess_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_unprocess_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_unprocess_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.unprocess", "sesrq_unprocess")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances
_order = _lib.byte_order
_ctx = {}           # (profile bytes, format, input domain, device index) -> context handle; lives as long as the process


def curve(kind) -> np.ndarray:
    """A built-in table (host): fp32 (256,), L[b] the linear value of byte b.  kind: "paper" (the unprocessing paper's inverse
    smoothstep, then ^2.2), "gamma" ((b / 255)^2.2), "srgb" (the piecewise sRGB EOTF) or "linear" (b / 255)."""
    k = CURVES.get(str(kind).lower()) if not isinstance(kind, (int, np.integer)) else int(kind)
    if k is None:
        raise ValueError(f"curve {kind!r}: 'paper', 'gamma', 'srgb', 'linear' or an array of 256 values")
    L = np.empty(CODES, np.float32)
    if lib().sesrq_unprocess_curve(k, L.ctypes.data) != 0:
        raise ValueError(last_error())
    return L


_table = curve          # Profile's `curve` argument shadows the function


class Profile:
    """How a display image becomes linear camera RGB: the table of the inverse tone curve ("paper", "gamma", "srgb", "linear" or an
    array of 256 finite fp32 values), the row-major 3 x 3 rgb2cam, the inverse gains (d_R, d_G, d_B) and whether highlights are
    preserved while the gains are inverted.  Everything is held as fp32; what the library would refuse is refused here."""

    def __init__(self, rgb2cam=((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), inv_gains=(1.0, 1.0, 1.0), curve="paper",
                 highlight: bool = True):
        m = np.asarray(rgb2cam, np.float64)
        d = np.asarray(inv_gains, np.float64)
        if d.shape != (3,) or m.size != 9:
            raise ValueError(f"Profile: a 3 x 3 matrix and three inverse gains, got {m.shape} and {d.shape}")
        with np.errstate(over="ignore"):
            self.rgb2cam = np.ascontiguousarray(m.reshape(3, 3), np.float32)
            self.inv_gains = np.ascontiguousarray(d, np.float32)
        if isinstance(curve, (str, int, np.integer)):
            self.curve = _table(curve)
        else:
            t = np.asarray(curve)
            if t.shape != (CODES,):
                raise ValueError(f"Profile: a curve is a name or {CODES} values, got shape {t.shape}")
            with np.errstate(over="ignore"):
                self.curve = np.ascontiguousarray(t, np.float32)
        self.highlight = bool(highlight)
        if not np.isfinite(self.rgb2cam).all():
            raise ValueError("Profile: the matrix must be finite")
        if not np.isfinite(self.inv_gains).all() or (self.inv_gains < 0).any():
            raise ValueError("Profile: inverse gains must be finite and not negative")
        if not np.isfinite(self.curve).all():
            raise ValueError("Profile: the curve's values must be finite")
        for a in (self.rgb2cam, self.inv_gains, self.curve):
            a.setflags(write=False)
        self.key = self.rgb2cam.tobytes() + self.inv_gains.tobytes() + self.curve.tobytes() + bytes([self.highlight])

    def __eq__(self, other):
        return isinstance(other, Profile) and other.key == self.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return (f"Profile(rgb2cam={self.rgb2cam.tolist()}, inv_gains={self.inv_gains.tolist()}, curve=<{CODES} values>, "
                f"highlight={self.highlight})")


def from_colormatrix(xyz2cam, red_gain=1.0, blue_gain=1.0, rgb_gain=1.0, curve="paper", highlight: bool = True) -> Profile:
    """The profile of a camera's metadata: rgb2cam = xyz2cam x rgb2xyz (sRGB / D65), every row divided by its sum, as the reference's
    ``metadata2tensor`` (self_dataset.py) forms it; inverse gains (1 / (rgb_gain red_gain), 1 / rgb_gain, 1 / (rgb_gain blue_gain)).
    Evaluated in float64 and rounded once to fp32."""
    x = np.asarray(xyz2cam, np.float64)
    if x.size != 9:
        raise ValueError(f"from_colormatrix: xyz2cam is a 3 x 3 matrix, got shape {x.shape}")
    a = x.reshape(3, 3) @ np.asarray(RGB2XYZ, np.float64)
    a = a / a.sum(axis=-1, keepdims=True)
    rg, bg, g = float(red_gain), float(blue_gain), float(rgb_gain)
    if not all(np.isfinite(v) and v > 0 for v in (rg, bg, g)):
        raise ValueError("from_colormatrix: the gains must be positive and finite")
    return Profile(a, (1.0 / (g * rg), 1.0 / g, 1.0 / (g * bg)), curve, highlight)


_INVERSE_OF = {"gamma": "gamma", "srgb": "srgb", "trunc255": "linear"}


def from_develop(profile, curve: str = "gamma", highlight: bool = False) -> Profile:
    """The inverse of a sesrq.develop.Profile: the closed-form inverse of its matrix, the reciprocals of its gains (float64, rounded
    once) and the table that undoes the develop curve named `curve` ("gamma", "srgb" or "trunc255": a develop profile keeps its
    thresholds, not their name).  Highlights are not preserved by default: the exact inverse of develop's gains is their reciprocal."""
    from . import develop
    if not isinstance(profile, develop.Profile):
        raise ValueError("from_develop: profile must be a sesrq.develop.Profile")
    if curve not in _INVERSE_OF:
        raise ValueError(f"from_develop: develop curve {curve!r}: 'gamma', 'srgb' or 'trunc255'")
    a = profile.ccm.astype(np.float64)
    cof = np.array([[a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]],
                    [a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]],
                    [a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0], a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]])
    det = a[0, 0] * cof[0, 0] + a[0, 1] * cof[1, 0] + a[0, 2] * cof[2, 0]
    g = profile.gains.astype(np.float64)
    if not np.isfinite(det) or det == 0 or (g == 0).any():
        raise ValueError("from_develop: the develop profile's matrix is singular or a gain is zero")
    return Profile(cof / det, 1.0 / g, _INVERSE_OF[curve], highlight)


def save_png16(path: str, rgb_u16) -> None:
    """Write a (H, W, 3) uint16 array as a 16-bit RGB PNG (the container of the raw nets' ground truths): one zlib stream, filter 0."""
    import struct
    import zlib
    a = np.ascontiguousarray(rgb_u16)
    if a.dtype != np.uint16 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"save_png16: a (H, W, 3) uint16 image, got {a.dtype} {a.shape}")
    H, W, _ = a.shape
    rows = np.concatenate([np.zeros((H, 1), np.uint8), a.astype(">u2").view(np.uint8).reshape(H, 6 * W)], 1).tobytes()
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows, 6)) +
                chunk(b"IEND", b""))


def _profile(profile) -> Profile:
    if not isinstance(profile, Profile):
        raise ValueError("unprocess: profile must be a sesrq.unprocess.Profile")
    return profile


def _format(fmt) -> sensor.Format:
    """The frame's format: None is the reference's dataset format; the frame is written in 16-bit containers."""
    f = sensor.REFERENCE if fmt is None else sensor._fmt(fmt)
    if f.packing != "u16":
        raise ValueError(f"unprocess: the frame is written in 16-bit containers; pack it with sensor.pack for {f.packing}")
    return f


def images(img_u8, device=None):
    """(N, H, W, 3) view of a uint8 image tensor (N, H, W, 3) or (H, W, 3) on a HIP device (`device`, when given)."""
    import torch
    if not isinstance(img_u8, torch.Tensor) or img_u8.dtype != torch.uint8:
        raise ValueError("unprocess: the image must be a torch.uint8 tensor")
    img = img_u8.unsqueeze(0) if img_u8.dim() == 3 else img_u8
    if img.dim() != 4 or img.shape[3] != 3 or min(img.shape) < 1:
        raise ValueError(f"unprocess: an image is (N, H, W, 3) or (H, W, 3), got {tuple(img_u8.shape)}")
    if img.device.type != "cuda" or (device is not None and img.device != device):
        raise ValueError(f"unprocess: the image is on {img.device}, expected {device if device is not None else 'a HIP device'}")
    return img


def context(profile: Profile, fmt: sensor.Format, scale_in, zero_in, exact_div, device):
    """The device context (sesrq_unprocess_create) of one (profile, format, input domain) on `device`, created once."""
    import torch
    key = (profile.key, fmt, np.float32(scale_in).tobytes(), int(zero_in), int(exact_div), device.index)
    h = _ctx.get(key)
    if h is None:
        h = C.c_void_p()
        with torch.cuda.device(device):
            rc = lib().sesrq_unprocess_create(profile.curve.ctypes.data, profile.rgb2cam.ctypes.data, profile.inv_gains.ctypes.data,
                                              int(profile.highlight), sensor.CFAS.index(fmt.cfa), fmt.black, fmt.white,
                                              float(np.float32(scale_in)), int(zero_in), int(exact_div), C.byref(h))
        if rc != 0:
            raise ValueError(last_error())
        _ctx[key] = h
    return h


def launch(profile, fmt, scale_in, zero_in, exact_div, img, order, raw, gt, q0, spread, stream):
    """Enqueue one run on the contiguous (N, H, W, 3) `img` into caller-owned outputs (any may be None, not all) on `stream`."""
    N, H, W, _ = img.shape
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = lib().sesrq_unprocess_run(context(profile, fmt, scale_in, zero_in, exact_div, img.device), img.data_ptr(), _order(order), ptr(raw),
                                   ptr(gt), ptr(q0), ptr(spread), N, H, W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def run(img_u8, profile, fmt=None, engine_or_bundle=None, order: str = "rgb", want_raw: bool = True, want_gt: bool = True,
        want_q: bool = False, want_spread: bool = False, stream=None):
    """img_u8: (N, H, W, 3) or (H, W, 3) torch.uint8 on a HIP device, interleaved in `order` -> dict of the tensors asked for:
    "raw" (N, H, W) uint16 in `fmt` (a sesrq.sensor.Format in 16-bit containers; None: the reference's 12-bit RGGB), "gt" (N, 3, H, W)
    fp32, "q0" (N, 3, H, W) int8 in the input domain of the net (engine.bundle or the bundle itself; an Engine also fixes exact_div)
    and "spread" (N, 3, H, W) fp32, the net's input frame.  One kernel, enqueued on `stream` (default: current), not synchronised."""
    import torch
    if not (want_raw or want_gt or want_q or want_spread):
        raise ValueError("unprocess: ask for raw, gt, q0 or spread")
    _order(order)
    profile, fmt = _profile(profile), _format(fmt)
    b, scale_in, zero_in, exact_div, dev = _lib.input_domain(engine_or_bundle, want_q, "unprocess")
    if b is not None and b.in_channels != 3:
        raise ValueError(f"a raw Bayer frame feeds 3-channel nets; this one takes {b.in_channels}")
    img = images(img_u8, dev)
    dev = img.device
    N, H, W, _ = img.shape
    with torch.cuda.device(dev):
        img = img.contiguous()
        new = lambda want, shape, dt: torch.empty(shape, dtype=dt, device=dev) if want else None
        out = dict(raw=new(want_raw, (N, H, W), torch.uint16), gt=new(want_gt, (N, 3, H, W), torch.float32),
                   q0=new(want_q, (N, 3, H, W), torch.int8), spread=new(want_spread, (N, 3, H, W), torch.float32))
        st = _lib.enter_stream(dev, stream, img, *out.values())
        launch(profile, fmt, scale_in, zero_in, exact_div, img, order, out["raw"], out["gt"], out["q0"], out["spread"], st)
    return {k: v for k, v in out.items() if v is not None}
