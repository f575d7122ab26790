"""numpy restatement of the 8-bit image route (include/sesrq_image.h): the checker for inputs no fixture holds.

  d(v)   = v / 255.0 in float64
  Y      = clip((((65.481 d(R) + 128.553 d(G)) + 24.966 d(B)) + 16.0) / 255.0, 0, 1) in float64, then fl32 (one plane)
  RGB    = clip(fl32(d(v_c)), 0, 1) (three planes, R, G, B)
  q0     = the input quantiser on that frame (oracle.sesrq_oracle.quantize_input; exact_div 2 = the reciprocal form)
  export = trunc(fl32(clip(p, 0, 1) * 255.0f)) interleaved (N, H, W, C), RGB or BGR; int8 p dequantised as (q - zero) * scale in fp32
numpy evaluates the float64 expressions left to right, one rounding per operation, without fused multiply-add -- the reference's
self_dataset_sr.py arithmetic."""
import numpy as np

F32 = np.float32


def rgb_planes(img, order="rgb"):
    """(N, H, W, 3) or (H, W, 3) uint8 -> (N, 3, H, W) uint8 in R, G, B plane order."""
    a = np.asarray(img)
    if a.ndim == 3:
        a = a[None]
    a = a.transpose(0, 3, 1, 2)
    return a[:, ::-1] if order == "bgr" else a


def decode_y(img, order="rgb"):
    p = rgb_planes(img, order).astype(np.float64) / 255.0
    s = 65.481 * p[:, 0] + 128.553 * p[:, 1] + 24.966 * p[:, 2] + 16.0
    return np.clip(s / 255.0, 0, 1).astype(F32)[:, None]


def decode_rgb(img, order="rgb"):
    return np.clip((rgb_planes(img, order).astype(np.float64) / 255.0).astype(F32), F32(0), F32(1))


def decode(img, form, order="rgb"):
    return decode_y(img, order) if form == "y" else decode_rgb(img, order)


def q0(x, scale_in, zero_in, exact_div=0):
    from oracle import sesrq_oracle as O
    return O.quantize_input(x, scale_in, zero_in, reciprocal=exact_div == 2)


def dequant(q, scale, zero):
    return ((np.asarray(q).astype(F32) - F32(zero)) * F32(scale)).astype(F32)


def export(pred, order="rgb"):
    """(N, C, H, W) fp32 -> (N, H, W, C) uint8, the reference's sim.py PNG export (clip, * 255.0 in fp32, channel flip, astype)."""
    g = np.clip(np.asarray(pred, F32).transpose(0, 2, 3, 1), 0, 1) * F32(255.0)
    assert g.dtype == np.float32
    if order == "bgr" and g.shape[3] == 3:
        g = g[:, :, :, ::-1]
    return np.ascontiguousarray(g.astype(np.uint8))


def upsample2(x):
    """The x2 anchor: nearest-neighbour upsampling of the input (test.py:148-153)."""
    return np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)
