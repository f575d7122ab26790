"""Display images out of the raw nets (MFLAG 2, 3, 4: dm, nrdm_3, nrdm_6): white-balance gains, colour-correction matrix, tone curve.

What these nets return is linear camera RGB in [0, 1]: the reference's frames come from an unprocessing pipeline that inverts the
white-balance gains and the colour matrix before the net sees them, and its ``metadata2tensor`` (self_dataset.py) prepares ``cam2rgb``,
``red_gain`` and ``blue_gain`` without ever applying them.  libsesrq_develop.so (C ABI include/sesrq_develop.h, which fixes the
arithmetic) is the tail of that pipeline's ``process`` as one kernel: gains, clip, 3 x 3 matrix, clip, tone curve, interleaved bytes.
There is no CPU path.

A `Profile` holds the gains, the matrix and the 255 thresholds of the tone curve; `from_colormatrix` builds one from camera metadata
as the reference's ``metadata2tensor`` does.  `export` takes the int8 output of a net with its output domain, or any fp32 (N, 3, H, W)
frame: the ground truth of ``raw.load_gt`` developed with the same profile gives the side-by-side of a prediction.
Byte order: ``"rgb"`` (PIL) or ``"bgr"`` (cv2).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_develop.so"))

LEVELS = 255
GAMMA22, SRGB, TRUNC255 = 0, 1, 2           # SESRQ_DEVELOP_GAMMA22 / _SRGB / _TRUNC255
CURVES = {"gamma": GAMMA22, "srgb": SRGB, "trunc255": TRUNC255}
ORDERS = {"rgb": 0, "bgr": 1}
PRED_F32, PRED_I8 = 0, 1
MFLAGS = (2, 3, 4)                          # the nets whose output is a linear camera-RGB image
RGB2XYZ = ((0.4124564, 0.3575761, 0.1804375), (0.2126729, 0.7151522, 0.0721750), (0.0193339, 0.1191920, 0.9503041))

# every symbol include/sesrq_develop.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_develop_curve": (C.c_int, [C.c_int, C.c_void_p]),
    "sesrq_develop_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "sesrq_develop_destroy": (None, [C.c_void_p]),
    "sesrq_develop_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p]),
    "sesrq_develop_instance_count": (C.c_int, []),
    "sesrq_develop_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_develop_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_develop_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.develop", "sesrq_develop")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances
_ctx = {}           # (profile bytes, device index) -> context handle; lives as long as the process


def _order(order) -> int:
    o = ORDERS.get(str(order).lower())
    if o is None:
        raise ValueError(f"byte order {order!r}: 'rgb' (PIL) or 'bgr' (cv2)")
    return o


def check_mflag(mflag: int) -> int:
    """The nets a developed image comes out of: 2 (dm), 3 (nrdm_3), 4 (nrdm_6).  MFLAG 1's output is a mosaic, 5 and 6 are not raw nets."""
    if mflag not in MFLAGS:
        raise ValueError(f"MFLAG {mflag}: a developed image comes out of the raw nets with an RGB output (2: dm, 3: nrdm_3, 4: nrdm_6); "
                         "MFLAG 1 (nr) returns a mosaic, 5 and 6 export through sesrq.image")
    return mflag


def curve(kind) -> np.ndarray:
    """A built-in threshold table (host): fp32 (255,), T[k] at index k - 1.  kind: "gamma" (o^(1/2.2), the unprocessing paper's),
    "srgb" (the piecewise sRGB OETF) or "trunc255" (image.export's truncation)."""
    k = CURVES.get(str(kind).lower()) if not isinstance(kind, (int, np.integer)) else int(kind)
    if k is None:
        raise ValueError(f"tone curve {kind!r}: 'gamma', 'srgb', 'trunc255' or an array of 255 thresholds")
    T = np.empty(LEVELS, np.float32)
    if lib().sesrq_develop_curve(k, T.ctypes.data) != 0:
        raise ValueError(last_error())
    return T


_table = curve          # Profile's `curve` argument shadows the function


class Profile:
    """How a linear camera-RGB frame becomes a display image: gains (g_R, g_G, g_B) -- white balance with any exposure gain folded
    in --, the row-major 3 x 3 colour-correction matrix, and the tone curve: "gamma", "srgb", "trunc255" or an array of 255
    non-decreasing fp32 thresholds (byte = the number of thresholds at or below the value).  Everything is held as fp32; what the
    library would refuse is refused here."""

    def __init__(self, gains=(1.0, 1.0, 1.0), ccm=((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), curve="gamma"):
        g = np.asarray(gains, np.float64)
        m = np.asarray(ccm, np.float64)
        if g.shape != (3,) or m.size != 9:
            raise ValueError(f"Profile: three gains and a 3 x 3 matrix, got {g.shape} and {m.shape}")
        with np.errstate(over="ignore"):
            self.gains = np.ascontiguousarray(g, np.float32)
            self.ccm = np.ascontiguousarray(m.reshape(3, 3), np.float32)
        if isinstance(curve, str) or isinstance(curve, (int, np.integer)):
            self.curve = _table(curve)
        else:
            t = np.asarray(curve)
            if t.shape != (LEVELS,):
                raise ValueError(f"Profile: a tone curve is a name or {LEVELS} thresholds, got shape {t.shape}")
            with np.errstate(over="ignore"):
                self.curve = np.ascontiguousarray(t, np.float32)
        if not np.isfinite(self.gains).all() or (self.gains < 0).any():
            raise ValueError("Profile: gains must be finite and not negative")
        if not np.isfinite(self.ccm).all():
            raise ValueError("Profile: the matrix must be finite")
        if not np.isfinite(self.curve).all() or (np.diff(self.curve) < 0).any():
            raise ValueError("Profile: the thresholds must be finite and must not decrease")
        for a in (self.gains, self.ccm, self.curve):
            a.setflags(write=False)
        self.key = self.gains.tobytes() + self.ccm.tobytes() + self.curve.tobytes()

    def __eq__(self, other):
        return isinstance(other, Profile) and other.key == self.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return f"Profile(gains={self.gains.tolist()}, ccm={self.ccm.tolist()}, curve=<{LEVELS} thresholds>)"


def from_colormatrix(xyz2cam, red_gain=1.0, blue_gain=1.0, rgb_gain=1.0, curve="gamma") -> Profile:
    """The profile of a camera's metadata, as the reference's ``metadata2tensor`` (self_dataset.py) prepares it: rgb2cam = xyz2cam x
    rgb2xyz (sRGB / D65), every row divided by its sum, cam2rgb = its inverse; gains (rgb_gain red_gain, rgb_gain, rgb_gain
    blue_gain).  Evaluated in float64 (the inverse in closed form) and rounded once to fp32, where the reference works in fp32
    throughout."""
    x = np.asarray(xyz2cam, np.float64)
    if x.size != 9:
        raise ValueError(f"from_colormatrix: xyz2cam is a 3 x 3 matrix, got shape {x.shape}")
    a = x.reshape(3, 3) @ np.asarray(RGB2XYZ, np.float64)
    a = a / a.sum(axis=-1, keepdims=True)
    cof = np.array([[a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]],
                    [a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]],
                    [a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0], a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]])
    det = a[0, 0] * cof[0, 0] + a[0, 1] * cof[1, 0] + a[0, 2] * cof[2, 0]
    if not np.isfinite(det) or det == 0:
        raise ValueError("from_colormatrix: rgb2cam is singular")
    rg, bg, g = float(red_gain), float(blue_gain), float(rgb_gain)
    return Profile((g * rg, g, g * bg), cof / det, curve)


def _profile(profile) -> Profile:
    if not isinstance(profile, Profile):
        raise ValueError("export: profile must be a sesrq.develop.Profile")
    return profile


def context(profile: Profile, device):
    """The device context (sesrq_develop_create) of one profile on `device`, created once."""
    import torch
    key = (profile.key, device.index)
    h = _ctx.get(key)
    if h is None:
        h = C.c_void_p()
        with torch.cuda.device(device):
            if lib().sesrq_develop_create(profile.gains.ctypes.data, profile.ccm.ctypes.data, profile.curve.ctypes.data, C.byref(h)) != 0:
                raise ValueError(last_error())
        _ctx[key] = h
    return h


def check_out(out, shape, device, who: str = "export"):
    """A caller-supplied output is written through its data_ptr(): anything but a contiguous uint8 tensor of the output shape on the
    device is refused before any launch."""
    import torch
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or out.device != device
            or not out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous uint8 tensor of the output shape {tuple(shape)} on {device}")


def launch(profile, pred, scale, zero, order, out, stream):
    """Enqueue one export of the contiguous (N, 3, H, W) `pred` into caller-owned `out` on `stream`."""
    import torch
    N, _, H, W = pred.shape
    dt = PRED_F32 if pred.dtype == torch.float32 else PRED_I8
    rc = lib().sesrq_develop_export(context(profile, pred.device), pred.data_ptr(), dt, float(np.float32(scale)), int(zero), _order(order),
                                    out.data_ptr(), N, H, W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def export(pred, profile, scale=None, zero=None, order: str = "rgb", out=None, stream=None):
    """pred: (N, 3, H, W) fp32 linear camera RGB, or int8 with the net's output domain (scale = f32(input.L.scale), zero = zero[L]) ->
    device uint8 (N, H, W, 3) in `order`: the frame developed with `profile` (include/sesrq_develop.h).  An fp32 frame need not be a
    net's output: the ground truth (raw.load_gt) developed with the same profile is the side-by-side of a prediction.  out: a
    contiguous uint8 tensor of that shape to write into.  Enqueued on `stream` (default: current), not synchronised."""
    import torch
    _order(order)
    profile = _profile(profile)
    if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or min(pred.shape) < 1:
        raise ValueError("export: the prediction is a (N, 3, H, W) tensor")
    N, Ch, H, W = pred.shape
    if Ch != 3:
        raise ValueError(f"export: {Ch} channels; a developed image comes from the 3 planes R, G, B")
    if pred.device.type != "cuda":
        raise ValueError("export: the prediction must be on a HIP device")
    if pred.dtype == torch.float32:
        s, z = 0.0, 0
    elif pred.dtype == torch.int8:
        if scale is None or zero is None:
            raise ValueError("export: an int8 prediction needs the output domain: scale and zero")
        s, z = scale, zero
    else:
        raise ValueError("export: the prediction must be float32 or int8")
    dev = pred.device
    shape = (N, H, W, 3)
    if out is not None:
        check_out(out, shape, dev)
    with torch.cuda.device(dev):
        pred = pred.contiguous()
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        launch(profile, pred, s, z, order, out, _lib.enter_stream(dev, stream, pred, out))
    return out
