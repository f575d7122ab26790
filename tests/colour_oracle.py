"""numpy restatement of the colour export (include/sesrq_colour.h): integers for steps 1 - 2, np.float32 operations for steps 3 - 4.

  1. chroma   d(v) = v / 255.0 in float64;  cb = ((-37.797 d(R) + -74.203 d(G)) + 112.0 d(B)) + 128.0,
              cr = ((112.0 d(R) + -93.786 d(G)) + -18.214 d(B)) + 128.0;  Cb = rint(64 cb), Cr = rint(64 cr)  (Q6, ties to even)
  2. upscale  Keys a = -1/2, half-pixel centres, edge replicate, horizontal pass then vertical pass, each floor((sum w c + 512) / 1024)
  3. luma     Y = fmin(fmax(p, 0), 1) * 255 in fp32; an int8 p is (q - zero) * scale in fp32
  4. colour   a = 1.16438356 (Y - 16); R = a + 1.59602679 crf; G = (a - 0.39176229 cbf) - 0.81296765 crf; B = a + 2.01723214 cbf
              with cbf = (Cb - 8192) / 64; bytes clamp(rint(.), 0, 255)
numpy evaluates the float64 and float32 expressions left to right, one rounding per operation, without fused multiply-add.  The
weights below are the header's table, typed in; tests/test_colour_oracle.py derives them from the Keys polynomial."""
import os
import re

import numpy as np

F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sesrq_colour.h")

WEIGHTS = {4: ((-45, 399, 745, -75), (-7, 93, 987, -49), (-49, 987, 93, -7), (-75, 745, 399, -45)),
           2: ((-24, 232, 888, -72), (-72, 888, 232, -24))}
FIRST = {4: (-2, -2, -1, -1), 2: (-2, -1)}


def header_tile():
    """(SESRQ_COLOUR_TILE_W, SESRQ_COLOUR_TILE_H) as the header exports them."""
    src = open(HEADER).read()
    return tuple(int(re.search(rf"#define SESRQ_COLOUR_TILE_{d}\s+(\d+)", src).group(1)) for d in "WH")


def tile(r):
    """The LR tile (w, h) of the export kernel at factor r: the header's output tile over r (at r = 4 SESRQ_COLOUR_TILE_W / _H)."""
    src = open(HEADER).read()
    ow, oh = (int(re.search(rf"#define SESRQ_COLOUR_TILE_OUT_{d}\s+(\d+)", src).group(1)) for d in "WH")
    assert ow % r == 0 and oh % r == 0
    return ow // r, oh // r


def rgb_planes(img, order="rgb"):
    """(N, H, W, 3) or (H, W, 3) uint8 -> (N, 3, H, W) uint8 in R, G, B plane order."""
    a = np.asarray(img)
    if a.ndim == 3:
        a = a[None]
    a = a.transpose(0, 3, 1, 2)
    return a[:, ::-1] if order == "bgr" else a


def chroma(img, order="rgb"):
    """Step 1: (N, H, W, 3) uint8 -> (N, 2, H, W) int16, plane 0 = Cb, plane 1 = Cr in Q6."""
    p = rgb_planes(img, order).astype(np.float64) / 255.0
    cb = -37.797 * p[:, 0] + -74.203 * p[:, 1] + 112.0 * p[:, 2] + 128.0
    cr = 112.0 * p[:, 0] + -93.786 * p[:, 1] + -18.214 * p[:, 2] + 128.0
    return np.stack([np.rint(64.0 * cb), np.rint(64.0 * cr)], 1).astype(np.int16)


def upscale_axis(c, r, axis):
    """One pass of step 2 along `axis` of an integer array: length L -> r L."""
    c = np.moveaxis(np.asarray(c).astype(np.int64), axis, -1)
    L = c.shape[-1]
    j = np.arange(L)
    out = np.empty(c.shape[:-1] + (r * L,), np.int64)
    for phi in range(r):
        s = np.full(c.shape, 512, np.int64)
        for k in range(4):
            s += WEIGHTS[r][phi][k] * c[..., np.clip(j + FIRST[r][phi] + k, 0, L - 1)]
        out[..., phi::r] = s >> 10                       # arithmetic shift: floor, of negative sums as well
    return np.moveaxis(out, -1, axis)


def upscale(c, r, keep=False):
    """Step 2: (..., H, W) integer planes -> (..., r H, r W) int64, the horizontal pass first.  keep: also the horizontal pass."""
    h = upscale_axis(c, r, -1)
    v = upscale_axis(h, r, -2)
    return (v, h) if keep else v


def dequant(q, scale, zero):
    with np.errstate(over="ignore"):                     # a huge scale may reach inf: step 3 clips it
        return ((np.asarray(q).astype(F32) - F32(zero)) * F32(scale)).astype(F32)


def luma(p):
    """Step 3: fp32 prediction -> Y in [0, 255] fp32; a NaN gives 0."""
    with np.errstate(invalid="ignore"):
        y = np.fmin(np.fmax(np.asarray(p, F32), F32(0)), F32(1)) * F32(255.0)
    assert y.dtype == F32
    return y


def colour_f32(Y, Cb, Cr):
    """Step 4 before the bytes: Y fp32 and upscaled Q6 chroma (same shape) -> (R, G, B) fp32 arrays."""
    a = F32(1.16438356) * (Y - F32(16.0))
    cbf = (Cb - 8192).astype(F32) * F32(0.015625)
    crf = (Cr - 8192).astype(F32) * F32(0.015625)
    R = a + F32(1.59602679) * crf
    G = (a - F32(0.39176229) * cbf) - F32(0.81296765) * crf
    B = a + F32(2.01723214) * cbf
    assert R.dtype == G.dtype == B.dtype == F32
    return R, G, B


def to_rgb(Y, Cb, Cr):
    """Step 4: Y fp32 and upscaled Q6 chroma (same shape) -> (R, G, B) uint8 arrays."""
    return tuple(np.clip(np.rint(v), 0, 255).astype(np.uint8) for v in colour_f32(Y, Cb, Cr))


def export(y, img, r, order="rgb", scale=None, zero=None):
    """y (N, 1, rH, rW) fp32, or int8 with (scale, zero); img (N, H, W, 3) uint8 in `order` -> (N, rH, rW, 3) uint8 in `order`."""
    y = np.asarray(y)
    p = dequant(y, scale, zero) if y.dtype == np.int8 else y
    up = upscale(chroma(img, order), r)
    R, G, B = to_rgb(luma(p)[:, 0], up[:, 0], up[:, 1])
    return np.ascontiguousarray(np.stack((B, G, R) if order == "bgr" else (R, G, B), -1))
