"""8-bit images into and out of the super-resolution nets (MFLAG 5 / 6): the image side of the reference's evaluation loop.

The reference (self_dataset_sr.py TestDataset.__getitem__) reads its LR / HR PNGs as uint8, divides by 255 in float64 and, for
SESR-x4 (MFLAG 5), forms the luma ``(65.481 R + 128.553 G + 24.966 B + 16) / 255`` in float64 before it casts to fp32; SESR-x2
(MFLAG 6) takes the three channels.  Its PNG export (sim.py) clips the fp32 output to [0, 1], multiplies by 255 in fp32 and truncates
to uint8.  Here the image goes to the device as it is (3 B/px) and libsesrq_image.so (C ABI include/sesrq_image.h) turns it into
the net's q0 -- the int8 input of sesrq_forward -- and, when asked, into the reference's fp32 ``inp``, bit for bit; the export reads
the fp32 or int8 output planes and writes the interleaved uint8 image.  There is no CPU path.

Forms: ``"y"`` (1 plane, MFLAG 5) and ``"rgb"`` (3 planes, MFLAG 6).  Byte order: ``"rgb"`` (PIL) or ``"bgr"`` (cv2).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_image.so"))

CODES = 256
Y, RGB = 0, 1                       # SESRQ_IMAGE_Y / SESRQ_IMAGE_RGB
FORMS = {"y": Y, "rgb": RGB}
CHANNELS = {Y: 1, RGB: 3}
ORDERS = {"rgb": 0, "bgr": 1}
PRED_F32, PRED_I8 = 0, 1
MFLAG_FORMS = {5: "y", 6: "rgb"}

# every symbol include/sesrq_image.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_image_table": (C.c_int, [C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sesrq_image_create": (C.c_int, [C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_image_destroy": (None, [C.c_void_p]),
    "sesrq_image_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p]),
    "sesrq_image_export": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p]),
    "sesrq_image_instance_count": (C.c_int, []),
    "sesrq_image_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_image_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_image_last_error": (C.c_char_p, []),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.image", "sesrq_image")
lib, last_error, instances = _so.lib, _so.last_error, _so.instances


def form_of(mflag: int) -> str:
    """The decode form of a network: 5 (SESR-x4, Y in / Y out) -> "y", 6 (SESR-x2, RGB) -> "rgb"."""
    if mflag not in MFLAG_FORMS:
        raise ValueError(f"MFLAG {mflag}: 8-bit images feed the super-resolution nets only (5: SESR-x4, Y; 6: SESR-x2, RGB)")
    return MFLAG_FORMS[mflag]


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


def table(scale_in: float, zero_in: int, exact_div: int = 0):
    """The RGB form of every byte code (host): (q0 int8 (256,), x fp32 (256,)) with x = clip(fl32(v / 255.0), 0, 1)."""
    q, x = np.empty(CODES, np.int8), np.empty(CODES, np.float32)
    if lib().sesrq_image_table(float(np.float32(scale_in)), int(zero_in), int(exact_div), q.ctypes.data, x.ctypes.data) != 0:
        raise ValueError(last_error())
    return q, x


# ------------------------------------------------------------------------------------------------------------------ files
def load_image(path: str) -> np.ndarray:
    """An 8-bit image file as a (H, W, 3) uint8 RGB array ((N, H, W, 3) for an .npy that holds a batch).  ``.npy``: a uint8 array of
    shape (H, W, 3) or (N, H, W, 3), taken as it is (its byte order is the caller's).  ``.png``: read through PIL (imported here
    only), converted to RGB as the reference's cv2.imread converts to its 3-channel BGR (grey is repeated, alpha dropped); 16-bit
    PNGs are refused."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path, allow_pickle=False)
        if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
            raise ValueError(f"{path}: an 8-bit image .npy holds uint8 (H, W, 3) or (N, H, W, 3), got {a.dtype} {a.shape}")
        return a
    if ext == ".png":
        try:
            from PIL import Image
        except ImportError:
            raise RuntimeError(f"{path}: reading PNG files needs Pillow (PIL), which is not installed; pass the image as a uint8 "
                               ".npy of shape (H, W, 3) instead") from None
        with Image.open(path) as im:
            if im.mode not in ("L", "P", "RGB", "RGBA", "LA"):
                raise ValueError(f"{path}: PNG mode {im.mode}: only 8-bit images are read (16-bit data takes the raw route)")
            return np.array(im.convert("RGB"), dtype=np.uint8)      # a writable copy
    raise ValueError(f"{path}: an 8-bit image is a .png or a uint8 .npy")


def save_png(path: str, img_u8) -> None:
    """Write a (H, W, 3) or (H, W, 1) uint8 RGB / grey array (numpy, or a tensor moved to the host) as a PNG through PIL."""
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError(f"{path}: writing PNG files needs Pillow (PIL), which is not installed; save the uint8 array as .npy "
                           "instead") from None
    a = img_u8.cpu().numpy() if hasattr(img_u8, "cpu") else np.asarray(img_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError(f"save_png: a (H, W, 1 | 3) uint8 image, got {a.dtype} {a.shape}")
    Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(path)


# ------------------------------------------------------------------------------------------------------------------ device
def _images(img, device):
    """(N, H, W, 3) view of a (N, H, W, 3) / (H, W, 3) uint8 tensor on `device` (None: any HIP device)."""
    import torch
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8:
        raise ValueError("an 8-bit image must be a torch.uint8 tensor (N, H, W, 3) or (H, W, 3)")
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[3] != 3 or min(img.shape) < 1:
        raise ValueError(f"an 8-bit image is interleaved (N, H, W, 3) or (H, W, 3), got {tuple(img.shape)}")
    if device is not None and img.device != device:
        raise ValueError(f"image is on {img.device}, expected {device}")
    if img.device.type != "cuda":
        raise ValueError("the image must be on a HIP device")
    return img


def launch(device, scale_in, zero_in, exact_div, img, form, order, q0, x, stream):
    """Enqueue one decode of the (N, H, W, 3) contiguous uint8 `img` into caller-owned q0 / x (either may be None) on `stream`."""
    N, H, W, _ = img.shape
    h = _so.context(device, scale_in, zero_in, exact_div)
    rc = lib().sesrq_image_decode(h, img.data_ptr(), _form(form), _order(order), q0.data_ptr() if q0 is not None else None,
                                  x.data_ptr() if x is not None else None, N, H, W, stream.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())


def decode(engine_or_bundle, img_u8, form, order: str = "rgb", want_q: bool = True, want_f: bool = False, stream=None):
    """img_u8: (N, H, W, 3) or (H, W, 3) torch.uint8 on a HIP device -> (q0 int8 (N, C, H, W) | None, x fp32 (N, C, H, W) | None),
    C = 1 for form "y", 3 for "rgb".

    q0 is in the input domain of the net (engine.bundle or the bundle itself: scale[0], zero[0]; an Engine also fixes how x / s0 is
    formed, its exact_div); x is the reference's fp32 input frame (engine_or_bundle may be None when only x is asked for).  Enqueued
    on `stream` (default: current), not synchronised."""
    import torch
    f = _form(form)
    _order(order)
    if not (want_q or want_f):
        raise ValueError("decode: ask for q0, x or both")
    b, scale_in, zero_in, exact_div, dev = _lib.input_domain(engine_or_bundle, want_q, "decode")
    if b is not None and b.in_channels != CHANNELS[f]:
        raise ValueError(f"image form {form!r} gives {CHANNELS[f]} channel(s); this net takes {b.in_channels}")
    img = _images(img_u8, dev)
    dev = img.device
    N, H, W, _ = img.shape
    Ch = CHANNELS[f]
    with torch.cuda.device(dev):
        img = img.contiguous()
        q0 = torch.empty((N, Ch, H, W), dtype=torch.int8, device=dev) if want_q else None
        x = torch.empty((N, Ch, H, W), dtype=torch.float32, device=dev) if want_f else None
        launch(dev, scale_in, zero_in, exact_div, img, f, order, q0, x, _lib.enter_stream(dev, stream, img, q0, x))
    return q0, x


def load_gt(img_u8, mflag: int, device=None, order: str = "rgb"):
    """The ground truth of the image route: an 8-bit HR image (N, H, W, 3) / (H, W, 3), numpy or torch uint8, as the device fp32
    (N, C, H, W) frame quality.score takes -- the reference's gt (self_dataset_sr.py: MFLAG 5 the clipped float64 luma, MFLAG 6
    clip(HR / 255.)), uploaded at 3 B/px and formed on the device."""
    import torch
    g = _lib.host_tensor(img_u8)
    if not isinstance(g, torch.Tensor) or g.dtype != torch.uint8:
        raise ValueError("load_gt: the ground truth must be a uint8 image array or tensor")
    dev = torch.device(device) if device is not None else (g.device if g.device.type == "cuda" else
                                                           torch.device("cuda", torch.cuda.current_device()))
    _, x = decode(None, g.to(dev, non_blocking=True), form_of(mflag), order=order, want_q=False, want_f=True)
    return x


def export(pred, order: str = "rgb", scale=None, zero=None, stream=None):
    """pred: (N, C, H, W) fp32, or int8 with the net's output domain (scale = f32(input.L.scale), zero = zero[L]) -> device uint8
    (N, H, W, C) = trunc(fl32(clip(p, 0, 1) * 255)), C = 1 or 3, interleaved in `order` -- the reference's PNG export (sim.py).
    For MFLAG 6 pass the anchored fp32 output (Engine(anchor_add=True)): the anchor does not exist in the int8 output.
    Enqueued on `stream` (default: current), not synchronised."""
    import torch
    o = _order(order)
    if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or min(pred.shape) < 1:
        raise ValueError("export: the prediction is a (N, C, H, W) tensor")
    N, Ch, H, W = pred.shape
    if Ch not in (1, 3):
        raise ValueError(f"export: {Ch} channels; an 8-bit image has 1 or 3")
    if pred.device.type != "cuda":
        raise ValueError("export: the prediction must be on a HIP device")
    if pred.dtype == torch.float32:
        dt, s, z = PRED_F32, 0.0, 0
    elif pred.dtype == torch.int8:
        if scale is None or zero is None:
            raise ValueError("export: an int8 prediction needs the output domain: scale and zero")
        dt, s, z = PRED_I8, float(np.float32(scale)), int(zero)
    else:
        raise ValueError("export: the prediction must be float32 or int8")
    dev = pred.device
    with torch.cuda.device(dev):
        pred = pred.contiguous()
        out = torch.empty((N, H, W, Ch), dtype=torch.uint8, device=dev)
        st = _lib.enter_stream(dev, stream, pred, out)
        rc = lib().sesrq_image_export(pred.data_ptr(), dt, s, z, Ch, o, out.data_ptr(), N, H, W, st.cuda_stream)
    if rc != 0:
        raise ValueError(last_error())
    return out
