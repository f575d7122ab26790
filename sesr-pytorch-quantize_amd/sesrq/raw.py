"""12-bit RGGB Bayer raw frames into the 3-channel nets: the input side of the reference's evaluation loop.

The reference (self_dataset.py TestDataset.__getitem__) reads ``<name>_<rows>_<cols>.raw`` (uint16, row-major), spreads it into a
sparse 3-channel RGGB mosaic (R at (even, even), G at (even, odd) and (odd, even), B at (odd, odd), zeros elsewhere), divides by
2**12 - 1 in fp32 and clamps to [0, 1]; its ground truth is a 16-bit RGB image treated the same way.  Here the raw frame goes to
the device as it is (2 B/px) and libsesrq_raw.so (C ABI include/sesrq_raw.h) turns it into the net's q0 -- the int8 input of
sesrq_forward -- and, when asked, into the reference's fp32 ``inp``, bit for bit.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_raw.so"))

CODES = 4096
WHITE = CODES - 1           # 2**12 - 1

# every symbol include/sesrq_raw.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_raw_table": (C.c_int, [C.c_float, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_raw_create": (C.c_int, [C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_raw_destroy": (None, [C.c_void_p]),
    "sesrq_raw_unpack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_raw_instance_count": (C.c_int, []),
    "sesrq_raw_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_raw_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_raw_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.raw", "sesrq_raw")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


def table(scale_in: float, zero_in: int, exact_div: int = 0) -> np.ndarray:
    """q0 of every code 0 .. 4095 (host): clamp8(rint(x / s0 + z0)) with x = clamp(fl32(code) / 4095, 0, 1).  exact_div as
    sesrq_options.exact_div (0 / 1: the true quotient, 2: x * fl(1 / s0))."""
    out = np.empty(CODES, np.int8)
    if lib().sesrq_raw_table(float(np.float32(scale_in)), int(zero_in), int(exact_div), out.ctypes.data) != 0:
        raise ValueError(last_error())
    return out


# ------------------------------------------------------------------------------------------------------------------ files
def raw_size(path: str):
    """(rows, cols) from a reference raw file name ``<name>_<rows>_<cols>.raw``: the basename's last two '_' fields."""
    base = os.path.basename(path)
    stem, ext = os.path.splitext(base)
    parts = stem.split("_")
    if ext.lower() != ".raw" or len(parts) < 3:
        raise ValueError(f"{path}: a raw frame is named <name>_<rows>_<cols>.raw")
    try:
        rows, cols = int(parts[-2]), int(parts[-1])
    except ValueError:
        raise ValueError(f"{path}: rows / cols in <name>_<rows>_<cols>.raw are not integers") from None
    if rows < 1 or cols < 1:
        raise ValueError(f"{path}: empty frame {rows} x {cols}")
    return rows, cols


def load_raw(path: str) -> np.ndarray:
    """A reference raw frame as a (rows, cols) uint16 array (little-endian file, row-major, as np.fromfile reads it there)."""
    from . import sensor
    return sensor.load_raw(path, None)


def load_gt(array_u16, device=None):
    """Ground truth of the raw route: a 16-bit RGB frame (N, 3, H, W) or (3, H, W), numpy or torch uint16, as device fp32 (N, 3, H, W)
    = clamp(fl32(v) / 4095, 0, 1), the reference's true fp32 quotient (self_dataset.py:235-243): codes are uploaded at 2 B/px and mapped
    on the device through the 4096 quotients formed on the host (a GPU tensor / scalar division would multiply by fl(1 / 4095))."""
    from . import sensor
    return sensor.load_gt(array_u16, None, device)


# ------------------------------------------------------------------------------------------------------------------ device
def launch(device, scale_in, zero_in, exact_div, raw, q0, spread, stream):
    """Enqueue one unpack of the (N, H, W) contiguous uint16 `raw` into caller-owned q0 / spread (either may be None) on `stream`."""
    N, H, W = raw.shape
    h = _so.context(device, scale_in, zero_in, exact_div)
    rc = lib().sesrq_raw_unpack(h, raw.data_ptr(), q0.data_ptr() if q0 is not None else None,
                                spread.data_ptr() if spread is not None else None, N, H, W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def unpack(engine_or_bundle, raw, want_q: bool = True, want_spread: bool = False, stream=None):
    """raw: (N, 1, H, W) or (N, H, W) torch.uint16 on a HIP device -> (q0 int8 (N, 3, H, W) | None, spread fp32 (N, 3, H, W) | None).

    q0 is in the input domain of the net (engine.bundle or the bundle itself: scale[0], zero[0]; an Engine also fixes how x / s0 is
    formed, its exact_div); spread is the reference's fp32 input frame (engine_or_bundle may be None when only spread is asked for).  Enqueued on `stream` (default: current), not synchronised."""
    from . import sensor
    return sensor.unpack(engine_or_bundle, raw, None, want_q, want_spread, stream=stream)
