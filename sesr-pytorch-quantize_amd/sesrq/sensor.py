"""Bayer raw frames as sensors deliver them into the 3-channel nets: any of the four CFA orders, a black pedestal, a white level of up
to 16 bits, in 16-bit containers or MIPI CSI-2 packed (RAW10: 4 px in 5 bytes, RAW12: 2 px in 3 bytes).

sesrq.raw takes the reference's synthetic dataset format alone (uint16, RGGB, black 0, white 4095: self_dataset.py TestDataset).  This
module is the same route with the format as a parameter: the frame goes to the device as the sensor wrote it (1.25 / 1.5 / 2 B/px) and
libsesrq_sensor.so (C ABI include/sesrq_sensor.h, which states the per-pixel arithmetic) turns it into the net's q0 -- the int8 input
of sesrq_forward -- and, when asked, into the fp32 input frame.  At Format() every byte is the one sesrq.raw gives.  The reference has
no format knob, so other formats are pinned to a restatement of the header's arithmetic (tests/sensor_oracle.py).  pack / unpack_host
are host-side numpy, for files and tests; there is no CPU path to q0.

The route's code lives here once.  Everything that takes `fmt` also takes None -- the reference's dataset format on libsesrq_raw.so,
decided in route() and nowhere else -- and sesrq.raw's load_raw / load_gt / unpack are calls of these with fmt=None; its launch is the
binding of sesrq_raw_unpack that launch() here calls for fmt=None.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

from . import _lib, raw as _raw
from .raw import raw_size

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_sensor.so"))

CFAS = ("rggb", "grbg", "gbrg", "bggr")                  # SESRQ_CFA_*
PACKINGS = ("u16", "raw10", "raw12")                     # SESRQ_PACK_*
# site channel (0 R, 1 G, 2 B) of the parities (0,0) (0,1) (1,0) (1,1)
SITES = {"rggb": (0, 1, 1, 2), "grbg": (1, 0, 2, 1), "gbrg": (1, 2, 0, 1), "bggr": (2, 1, 1, 0)}
_GROUP = {"u16": (1, 2), "raw10": (4, 5), "raw12": (2, 3)}      # packing -> (pixels, bytes) of a pack group
_TOP = {"u16": 65535, "raw10": 1023, "raw12": 4095}


class CFormat(C.Structure):
    _fields_ = [("cfa", C.c_int32), ("black", C.c_int32), ("white", C.c_int32), ("packing", C.c_int32)]


@dataclasses.dataclass(frozen=True)
class Format:
    """A sensor's raw format: CFA order, black and white level (codes are clamped to [black, white] and mapped to [0, 1]) and packing.
    The default is the reference's dataset format, the one sesrq.raw takes."""
    cfa: str = "rggb"
    black: int = 0
    white: int = 4095
    packing: str = "u16"

    def __post_init__(self):
        cfa, packing = str(self.cfa).lower(), str(self.packing).lower()
        if cfa not in CFAS:
            raise ValueError(f"cfa {self.cfa!r}: one of {CFAS}")
        if packing not in PACKINGS:
            raise ValueError(f"packing {self.packing!r}: one of {PACKINGS}")
        for name in ("black", "white"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} level {v!r} is not an integer")
        black, white = int(self.black), int(self.white)
        if not 0 <= black < white <= 65535:
            raise ValueError(f"levels need 0 <= black < white <= 65535, got black {black}, white {white}")
        if white > _TOP[packing]:
            raise ValueError(f"white {white} is above the range of {packing} ({_TOP[packing]})")
        for name, v in (("cfa", cfa), ("packing", packing), ("black", black), ("white", white)):
            object.__setattr__(self, name, v)

    @property
    def levels(self) -> int:
        return self.white - self.black + 1

    def row_bytes(self, W: int) -> int:
        """Bytes of a row of W pixels without padding; W must be a whole number of pack groups."""
        px, nb = _GROUP[self.packing]
        if W < 1 or W % px:
            raise ValueError(f"a {self.packing} row is a whole number of groups of {px} pixels, got W = {W}")
        return W // px * nb

    def width_of(self, nbytes: int) -> int:
        """Pixels of an unpadded row of `nbytes` bytes."""
        px, nb = _GROUP[self.packing]
        if nbytes < 1 or nbytes % nb:
            raise ValueError(f"an unpadded {self.packing} row is a whole number of groups of {nb} bytes, got {nbytes}; give the width")
        return nbytes // nb * px

    def c(self) -> CFormat:
        return CFormat(CFAS.index(self.cfa), self.black, self.white, PACKINGS.index(self.packing))


_FMT = C.POINTER(CFormat)
# every symbol include/sesrq_sensor.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_sensor_row_bytes": (C.c_size_t, [_FMT, C.c_int]),
    "sesrq_sensor_table": (C.c_int, [_FMT, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "sesrq_sensor_create": (C.c_int, [_FMT, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_sensor_destroy": (None, [C.c_void_p]),
    "sesrq_sensor_unpack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_sensor_instance_count": (C.c_int, []),
    "sesrq_sensor_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_sensor_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_sensor_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.sensor", "sesrq_sensor")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


def _fmt(fmt) -> Format:
    if not isinstance(fmt, Format):
        raise ValueError(f"fmt must be a sesrq.sensor.Format, got {type(fmt).__name__}")
    return fmt


REFERENCE = Format()


def route(fmt, who: str = "", stride=None, width=None):
    """The raw route's one decision: (the frames' Format, whether libsesrq_raw.so unpacks them).  fmt=None is the reference's dataset
    format on libsesrq_raw.so, whose rows are unpadded; a Format, the default one included, goes to libsesrq_sensor.so."""
    if fmt is None:
        if stride is not None or width is not None:
            raise ValueError(f"{who}stride and width belong to a sensor format (fmt=...)")
        return REFERENCE, True
    return _fmt(fmt), False


def table(fmt: Format, scale_in: float, zero_in: int, exact_div: int = 0) -> np.ndarray:
    """q0 of every d = clamp(code, black, white) - black = 0 .. white - black (host): clamp8(rint(x / s0 + z0)) with x = clamp(fl32(d) /
    fl32(white - black), 0, 1).  exact_div as sesrq_options.exact_div (0 / 1: the true quotient, 2: x * fl(1 / s0))."""
    out = np.empty(_fmt(fmt).levels, np.int8)
    cf = fmt.c()
    if lib().sesrq_sensor_table(C.byref(cf), float(np.float32(scale_in)), int(zero_in), int(exact_div), out.ctypes.data, out.size) != 0:
        raise ValueError(last_error())
    return out


def levels(fmt: Format) -> np.ndarray:
    """x(d) for every d = 0 .. white - black: the fp32 quotients fl32(d) / fl32(white - black), formed on the host."""
    d = np.arange(_fmt(fmt).levels, dtype=np.float32)
    return np.clip(d / np.float32(fmt.white - fmt.black), np.float32(0), np.float32(1))


# ------------------------------------------------------------------------------------------------------------------ host packing
def pack(frame_u16, fmt: Format, stride: int = None, pad: int = 0) -> np.ndarray:
    """(..., H, W) uint16 codes -> (..., H, stride) uint8 rows as the sensor writes them (stride >= fmt.row_bytes(W), default that;
    padding bytes hold `pad`).  Codes must fit the packing's bits."""
    a = np.asarray(frame_u16)
    if a.dtype != np.uint16 or a.ndim < 2:
        raise ValueError("pack: need a (..., H, W) uint16 array")
    W = a.shape[-1]
    nb = _fmt(fmt).row_bytes(W)
    stride = nb if stride is None else int(stride)
    if stride < nb:
        raise ValueError(f"pack: stride {stride} is less than the {nb} bytes of a row of {W} pixels")
    if a.size and int(a.max()) > _TOP[fmt.packing]:
        raise ValueError(f"pack: code {int(a.max())} does not fit {fmt.packing}")
    out = np.full(a.shape[:-1] + (stride,), pad, np.uint8)
    if fmt.packing == "u16":
        out[..., 0:nb:2], out[..., 1:nb:2] = a & 0xff, a >> 8
    elif fmt.packing == "raw10":
        g = a.reshape(a.shape[:-1] + (W // 4, 4))
        rows = np.empty(a.shape[:-1] + (W // 4, 5), np.uint8)
        rows[..., :4] = g >> 2
        rows[..., 4] = (g[..., 0] & 3) | (g[..., 1] & 3) << 2 | (g[..., 2] & 3) << 4 | (g[..., 3] & 3) << 6
        out[..., :nb] = rows.reshape(a.shape[:-1] + (nb,))
    else:
        g = a.reshape(a.shape[:-1] + (W // 2, 2))
        rows = np.empty(a.shape[:-1] + (W // 2, 3), np.uint8)
        rows[..., :2] = g >> 4
        rows[..., 2] = (g[..., 0] & 15) | (g[..., 1] & 15) << 4
        out[..., :nb] = rows.reshape(a.shape[:-1] + (nb,))
    return out


def unpack_host(rows_u8, fmt: Format, width: int = None) -> np.ndarray:
    """(..., H, stride) uint8 rows -> (..., H, W) uint16 codes: the inverse of pack.  width: W (default: the rows are unpadded)."""
    r = np.asarray(rows_u8)
    if r.dtype != np.uint8 or r.ndim < 2:
        raise ValueError("unpack_host: need a (..., H, stride) uint8 array")
    W = _fmt(fmt).width_of(r.shape[-1]) if width is None else int(width)
    nb = fmt.row_bytes(W)
    if r.shape[-1] < nb:
        raise ValueError(f"unpack_host: rows of {r.shape[-1]} bytes are shorter than the {nb} bytes of {W} pixels")
    r = r[..., :nb].astype(np.uint16)
    if fmt.packing == "u16":
        return r[..., 0::2] | r[..., 1::2] << 8
    if fmt.packing == "raw10":
        g = r.reshape(r.shape[:-1] + (W // 4, 5))
        px = [g[..., k] << 2 | (g[..., 4] >> (2 * k)) & 3 for k in range(4)]
    else:
        g = r.reshape(r.shape[:-1] + (W // 2, 3))
        px = [g[..., 0] << 4 | g[..., 2] & 15, g[..., 1] << 4 | g[..., 2] >> 4]
    return np.stack(px, -1).reshape(r.shape[:-1] + (W,)).astype(np.uint16)


def load_raw(path: str, fmt) -> np.ndarray:
    """A raw frame file ``<name>_<rows>_<cols>.raw`` (the reference's naming) in `fmt`: (rows, cols) uint16 for u16 (little-endian),
    (rows, fmt.row_bytes(cols)) uint8 for the packed formats.  The file holds exactly rows x row_bytes bytes."""
    fmt, _ = route(fmt)
    rows, cols = raw_size(path)
    nb = fmt.row_bytes(cols)
    nbytes = os.path.getsize(path)
    if nbytes != rows * nb:
        raise ValueError(f"{path}: {nbytes} bytes, a {rows} x {cols} {fmt.packing} frame has {rows * nb}")
    if fmt.packing == "u16":
        return np.fromfile(path, dtype="<u2").reshape(rows, cols).astype(np.uint16, copy=False)
    return np.fromfile(path, dtype=np.uint8).reshape(rows, nb)


_levels = {}


def load_gt(array_u16, fmt, device=None):
    """Ground truth of the raw route at the format's levels: a 16-bit RGB frame (N, 3, H, W) or (3, H, W), numpy or torch uint16, as
    device fp32 (N, 3, H, W) = x(clamp(v, black, white) - black).  The quotients are formed on the host and looked up on the device (a
    GPU tensor / scalar division would multiply by a reciprocal)."""
    import torch
    fmt, _ = route(fmt)
    g = _lib.host_tensor(array_u16)
    if not isinstance(g, torch.Tensor) or g.dtype != torch.uint16:
        raise ValueError("load_gt: the ground truth must be a uint16 array or tensor")
    if g.dim() == 3:
        g = g.unsqueeze(0)
    if g.dim() != 4 or g.shape[1] != 3:
        raise ValueError(f"load_gt: expected an RGB frame (N, 3, H, W), got {tuple(g.shape)}")
    dev = torch.device(device) if device is not None else (g.device if g.device.type == "cuda" else
                                                           torch.device("cuda", torch.cuda.current_device()))
    key = (dev, fmt.black, fmt.white)
    lv = _levels.get(key)
    if lv is None:
        lv = _levels[key] = torch.from_numpy(levels(fmt)).to(dev)
    idx = g.to(dev, non_blocking=True).to(torch.int32).clamp_(min=fmt.black, max=fmt.white).sub_(fmt.black)
    return lv[idx.long()]


# ------------------------------------------------------------------------------------------------------------------ device
def frames(raw, fmt, device, stride: int = None, width: int = None, who: str = ""):
    """((N, H, S) view of the frames, W, row stride in bytes) of a device tensor in `fmt`; `who` goes in front of route()'s refusal.

    u16: torch.uint16 (N, 1, H, S) / (N, H, S) / (H, S); packed: torch.uint8 (N, H, S) / (H, S), S bytes per row.  Without `stride` the
    rows are unpadded and W follows from S; a padded frame gives its row stride in bytes (it must be the tensor's) and its `width`."""
    import torch
    fmt, _ = route(fmt, who, stride, width)
    want = torch.uint16 if fmt.packing == "u16" else torch.uint8
    if not isinstance(raw, torch.Tensor) or raw.dtype != want:
        raise ValueError(f"a {fmt.packing} raw frame must be a torch.{'uint16' if want == torch.uint16 else 'uint8'} tensor")
    if raw.dim() == 4:
        if raw.shape[1] != 1 or fmt.packing != "u16":
            raise ValueError(f"a raw frame has one channel, got {tuple(raw.shape)}")
        raw = raw.reshape(raw.shape[0], raw.shape[2], raw.shape[3])
    elif raw.dim() == 2:
        raw = raw.unsqueeze(0)
    if raw.dim() != 3 or min(raw.shape) < 1:
        raise ValueError(f"a raw frame is (N, H, row) or (H, row), got {tuple(raw.shape)}")
    if raw.device != device:
        raise ValueError(f"raw frame is on {raw.device}, expected {device}")
    S = raw.shape[2] * raw.element_size()
    if stride is None:
        if width is not None and fmt.row_bytes(int(width)) != S:
            raise ValueError(f"rows of {S} bytes are not unpadded rows of {width} pixels; give the stride")
        W = fmt.width_of(S)
    else:
        if int(stride) != S:
            raise ValueError(f"stride {stride}: the tensor's rows are {S} bytes apart")
        if width is None:
            raise ValueError("a frame with a row stride needs its width")
        W = int(width)
        if fmt.row_bytes(W) > S:
            raise ValueError(f"stride {S} is less than the {fmt.row_bytes(W)} bytes of a row of {W} pixels")
    return raw, W, S


_ctx = {}          # (device index, f32 scale bits, zero, exact_div, format) -> context handle; lives as long as the process


def context(device, fmt: Format, scale_in, zero_in, exact_div):
    """The device context (sesrq_sensor_create) of one (device, input domain, format), created once."""
    import torch
    key = (device.index, np.float32(scale_in).tobytes(), int(zero_in), int(exact_div), _fmt(fmt))
    h = _ctx.get(key)
    if h is None:
        h, cf = C.c_void_p(), fmt.c()
        with torch.cuda.device(device):
            if lib().sesrq_sensor_create(C.byref(cf), float(np.float32(scale_in)), int(zero_in), int(exact_div), C.byref(h)) != 0:
                raise ValueError(last_error())
        _ctx[key] = h
    return h


def launch(device, fmt, scale_in, zero_in, exact_div, raw, W, S, q0, spread, stream):
    """Enqueue one unpack of the contiguous (N, H, S bytes) `raw` of W pixels a row into caller-owned q0 / spread (either may be None)."""
    fmt, reference = route(fmt)
    if reference:          # libsesrq_raw.so: the (N, H, W) uint16 tensor says its own W and rows are unpadded
        return _raw.launch(device, scale_in, zero_in, exact_div, raw, q0, spread, stream)
    N, H = raw.shape[0], raw.shape[1]
    h = context(device, fmt, scale_in, zero_in, exact_div)
    rc = lib().sesrq_sensor_unpack(h, raw.data_ptr(), S, q0.data_ptr() if q0 is not None else None,
                                   spread.data_ptr() if spread is not None else None, N, H, W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def unpack(engine_or_bundle, raw, fmt, want_q: bool = True, want_spread: bool = False, stride: int = None, stream=None,
           width: int = None):
    """raw in `fmt` on a HIP device (see frames()) -> (q0 int8 (N, 3, H, W) | None, spread fp32 (N, 3, H, W) | None).

    q0 is in the input domain of the net (engine.bundle or the bundle itself; an Engine also fixes exact_div); spread is the fp32 input
    frame (engine_or_bundle may be None when only spread is asked for).  Enqueued on `stream` (default: current), not synchronised."""
    import torch
    if not (want_q or want_spread):
        raise ValueError("unpack: ask for q0, spread or both")
    b, scale_in, zero_in, exact_div, dev = _lib.input_domain(engine_or_bundle, want_q, "unpack")
    if b is not None and b.in_channels != 3:
        raise ValueError(f"a raw Bayer frame feeds 3-channel nets; this one takes {b.in_channels}")
    if dev is None:
        dev = raw.device if isinstance(raw, torch.Tensor) else None
    raw, W, S = frames(raw, fmt, dev, stride, width)
    if dev is None or dev.type != "cuda":
        raise ValueError("the raw frame must be on a HIP device")
    N, H = raw.shape[0], raw.shape[1]
    with torch.cuda.device(dev):
        raw = raw.contiguous()
        q0 = torch.empty((N, 3, H, W), dtype=torch.int8, device=dev) if want_q else None
        sp = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev) if want_spread else None
        launch(dev, fmt, scale_in, zero_in, exact_div, raw, W, S, q0, sp, _lib.enter_stream(dev, stream, raw, q0, sp))
    return q0, sp
