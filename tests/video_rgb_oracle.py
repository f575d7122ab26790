"""numpy restatement of the RGB video route (include/sesrq_video_rgb.h), built from the restatements that exist:

  decode  D1  video_oracle.chroma_q6 at r = 2 (colour_oracle.upscale of 64 c) BEFORE its byte, cropped to H x W
          D2  colour_oracle.to_rgb (step 4 of sesrq_colour.h) on Y = fl32(y byte) and the Q6 chroma
          D3  image_oracle.decode_rgb / q0 on those bytes (the per-code table)
  export  E1  image_oracle.export: trunc(fl32(clip(p, 0, 1) * 255)), int8 p dequantised first
          E2  Y  = (65481 R + 128553 G + 24966 B + 4207500) // 255000
          E3  Cb = (2 S + 262140000) // 2040000 with S the sum of -37797 R - 74203 G + 112000 B over the 2 x 2 block, pixel indices
              clamped to the frame; Cr likewise with 112000 R - 93786 G - 18214 B
A frame is video_oracle's dict of planes {"y", "cb", "cr"}; an RGB image is (N, H, W, 3) uint8."""
import os
import re

import numpy as np

import colour_oracle as CO
import image_oracle as IO
import video_oracle as VO

F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sesrq_video_rgb.h")

KY = (65481, 128553, 24966)
KCB = (-37797, -74203, 112000)
KCR = (112000, -93786, -18214)


def header_defines():
    """{name: value} of the header's SESRQ_VIDEO_RGB_* integer defines."""
    return {k: int(v) for k, v in re.findall(r"#define SESRQ_VIDEO_RGB_(\w+)\s+(\d+)", open(HEADER).read())}


def tile():
    """(TILE_W, TILE_H) of the decode kernel, luma pixels."""
    d = header_defines()
    return d["TILE_W"], d["TILE_H"]


# ------------------------------------------------------------------------------------------------------------------ decode
def chroma444(c, H, W, keep=False):
    """D1: a chroma plane (..., ceil(H / 2), ceil(W / 2)) uint8 -> the Q6 plane (..., H, W) int64 (keep: and the horizontal pass)."""
    v, h = VO.chroma_q6(c, 2, keep=True)
    v = v[..., :H, :W]
    return (v, h) if keep else v


def rgb_bytes(fr):
    """D1 + D2: the frames -> the RGB image (N, H, W, 3) uint8."""
    y = np.asarray(fr["y"])
    _, H, W = y.shape
    R, G, B = CO.to_rgb(y.astype(F32), chroma444(fr["cb"], H, W), chroma444(fr["cr"], H, W))
    return np.ascontiguousarray(np.stack([R, G, B], -1))


def decode(fr, scale_in=None, zero_in=None, exact_div=0):
    """D1 - D3: the frames -> (q0 int8 (N, 3, H, W) | None without a domain, x fp32 (N, 3, H, W))."""
    x = IO.decode_rgb(rgb_bytes(fr))
    if scale_in is None:
        return None, x
    return IO.q0(x, scale_in, zero_in, exact_div), x


# ------------------------------------------------------------------------------------------------------------------ export
def luma_of(rgb):
    """E2 on (..., 3) integer RGB."""
    r = np.asarray(rgb).astype(np.int64)
    return (KY[0] * r[..., 0] + KY[1] * r[..., 1] + KY[2] * r[..., 2] + 4207500) // 255000


def chroma_term(rgb, k):
    r = np.asarray(rgb).astype(np.int64)
    return k[0] * r[..., 0] + k[1] * r[..., 1] + k[2] * r[..., 2]


def ycbcr(img):
    """E2 + E3: an RGB image (N, H, W, 3) uint8 -> the frames."""
    img = np.asarray(img)
    N, H, W, _ = img.shape
    yi = np.minimum(np.arange(2 * ((H + 1) // 2)), H - 1)
    xi = np.minimum(np.arange(2 * ((W + 1) // 2)), W - 1)
    out = {"y": luma_of(img).astype(np.uint8)}
    for name, k in (("cb", KCB), ("cr", KCR)):
        t = chroma_term(img, k)[:, yi][:, :, xi]
        S = t[:, 0::2, 0::2] + t[:, 0::2, 1::2] + t[:, 1::2, 0::2] + t[:, 1::2, 1::2]
        num = 2 * S + 262140000
        assert num.min() > 0 and num.max() < 1 << 31
        out[name] = (num // 2040000).astype(np.uint8)
    return out


def export(pred, scale=None, zero=None):
    """E1 - E3: the prediction (N, 3, H, W), fp32 or int8 with (scale, zero) -> the frames."""
    p = np.asarray(pred)
    if p.dtype == np.int8:
        p = CO.dequant(p, scale, zero)
    with np.errstate(invalid="ignore"):
        return ycbcr(IO.export(np.nan_to_num(p, nan=0.0, posinf=np.inf, neginf=-np.inf)))
