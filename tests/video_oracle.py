"""numpy restatement of the video route (include/sesrq_video.h): integers for the chroma, np.float32 operations for the luma.

  1. decode   x = clip(fl32(v / 255.0), 0, 1) with v / 255.0 in float64; q0 = the input quantiser on x (oracle.sesrq_oracle)
  2. luma     u = trunc(fl32(clip(p, 0, 1) * 255)); an int8 p is (q - zero) * scale in fp32; a NaN gives 0
  3. chroma   C = 64 c; colour_oracle.upscale (the Keys a = -1/2 integers, horizontal pass first); byte = clamp((C^ + 32) >> 6, 0, 255);
              the HR plane is the top-left (rH / 2) x (rW / 2) of the upscaled r ceil(H / 2) x r ceil(W / 2) plane
The weights, the upscale and the dequantisation are colour_oracle's: one table serves both restatements.

A frame is a dict of planes {"y": (N, H, W), "cb": (N, Hc, Wc), "cr": (N, Hc, Wc)} uint8, whatever the pixel format; pack / unpack
turn it into the bytes of a raw .yuv file and back."""
import os
import re

import numpy as np

import colour_oracle as CO

F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sesrq_video.h")


def header_tile():
    """(SESRQ_VIDEO_TILE_OUT_W, SESRQ_VIDEO_TILE_OUT_H) as the header exports them."""
    src = open(HEADER).read()
    return tuple(int(re.search(rf"#define SESRQ_VIDEO_TILE_OUT_{d}\s+(\d+)", src).group(1)) for d in "WH")


def tile(r):
    """The LR luma tile (w, h) of the export kernel at factor r: the header's output tile over r."""
    ow, oh = header_tile()
    assert ow % r == 0 and oh % r == 0
    return ow // r, oh // r


def chroma_size(H, W):
    return (H + 1) // 2, (W + 1) // 2


def frame_bytes(H, W):
    hc, wc = chroma_size(H, W)
    return H * W + 2 * hc * wc


def random_frames(rng, N, H, W, kind="random"):
    """N frames of H x W: random bytes, or bytes drawn from {0, 255}."""
    hc, wc = chroma_size(H, W)
    draw = (lambda s: rng.integers(0, 256, s).astype(np.uint8)) if kind == "random" else \
        (lambda s: (rng.integers(0, 2, s) * 255).astype(np.uint8))
    return {"y": draw((N, H, W)), "cb": draw((N, hc, wc)), "cr": draw((N, hc, wc))}


def pack(fr, fmt):
    """The frames as the bytes of a raw .yuv file: per frame Y, then Cb,Cr interleaved (nv12) or Cb, Cr (i420); unpadded rows."""
    out = []
    for n in range(fr["y"].shape[0]):
        out.append(fr["y"][n].tobytes())
        if fmt == "nv12":
            out.append(np.stack([fr["cb"][n], fr["cr"][n]], -1).tobytes())
        else:
            out += [fr["cb"][n].tobytes(), fr["cr"][n].tobytes()]
    return b"".join(out)


def unpack(data, fmt, H, W):
    """The inverse of pack: the bytes of a raw .yuv file -> the dict of planes."""
    hc, wc = chroma_size(H, W)
    a = np.frombuffer(data, np.uint8).reshape(-1, frame_bytes(H, W))
    y = a[:, :H * W].reshape(-1, H, W)
    c = a[:, H * W:]
    if fmt == "nv12":
        c = c.reshape(-1, hc, wc, 2)
        return {"y": y, "cb": c[..., 0], "cr": c[..., 1]}
    c = c.reshape(-1, 2, hc, wc)
    return {"y": y, "cb": c[:, 0], "cr": c[:, 1]}


# ------------------------------------------------------------------------------------------------------------------ arithmetic
def code_x():
    """x of every byte code: clip(fl32(v / 255.0), 0, 1)."""
    return np.clip((np.arange(256, dtype=np.float64) / 255.0).astype(F32), F32(0), F32(1))


def table(scale_in, zero_in, exact_div=0):
    """(q0 int8 (256,), x fp32 (256,)) of every byte code."""
    from oracle import sesrq_oracle as O
    x = code_x()
    return O.quantize_input(x, scale_in, zero_in, reciprocal=exact_div == 2), x


def decode(y, scale_in=None, zero_in=None, exact_div=0):
    """Step 1: Y planes (N, H, W) uint8 -> (q0 int8 (N, 1, H, W) | None without a domain, x fp32 (N, 1, H, W))."""
    y = np.asarray(y)
    x = code_x()[y][:, None]
    if scale_in is None:
        return None, x
    from oracle import sesrq_oracle as O
    return O.quantize_input(x, scale_in, zero_in, reciprocal=exact_div == 2), x


def luma(p, scale=None, zero=None):
    """Step 2: the net's luma (N, 1, rH, rW), fp32 or int8 with (scale, zero) -> the Y plane (N, rH, rW) uint8."""
    p = np.asarray(p)
    if p.dtype == np.int8:
        p = CO.dequant(p, scale, zero)
    with np.errstate(invalid="ignore"):
        g = np.fmin(np.fmax(p.astype(F32), F32(0)), F32(1)) * F32(255.0)
    assert g.dtype == F32
    return g.astype(np.uint8)[:, 0]


def chroma_q6(c, r, keep=False):
    """Step 3 before the bytes: a chroma plane (..., Hc, Wc) uint8 -> the upscaled Q6 plane (..., r Hc, r Wc) int64 (keep: and the
    horizontal pass)."""
    return CO.upscale(np.asarray(c).astype(np.int64) * 64, r, keep=keep)


def chroma_bytes(q6):
    return np.clip((np.asarray(q6) + 32) >> 6, 0, 255).astype(np.uint8)


def chroma(c, r, H, W):
    """Step 3: the LR chroma plane (N, Hc, Wc) of H x W frames -> the HR chroma plane (N, rH / 2, rW / 2) uint8."""
    return np.ascontiguousarray(chroma_bytes(chroma_q6(c, r))[..., :r * H // 2, :r * W // 2])


def export(y, lr, r, scale=None, zero=None):
    """The net's luma (N, 1, rH, rW) and the LR frames (dict of planes) -> the HR frames (dict of planes)."""
    N, H, W = lr["y"].shape
    assert tuple(np.asarray(y).shape) == (N, 1, r * H, r * W)
    return {"y": luma(y, scale, zero), "cb": chroma(lr["cb"], r, H, W), "cr": chroma(lr["cr"], r, H, W)}
