"""numpy restatement of include/sesrq_downscale.h: the checker of the bicubic x2 / x4 downscale and of its fused decode.

  taps     LR index d of an axis of length n takes HR indices j = r d - 3 r / 2 + k, k = 0 .. 4 r - 1, weights WEIGHTS[r][k] / D[r]
  edges    an index outside the frame is mirrored with the edge sample repeated: p = 2 n, i = j mod p, i if i < n else p - 1 - i
  a pass   clamp(floor((sum w v + D / 2) / D), 0, 255) as uint8
  order    the vertical pass (axis H) first, then the horizontal one, a uint8 image in between
  decode   tests/image_oracle.py on the LR bytes (the Y or the RGB form, q0 by the oracle's input quantiser)
tests/test_downscale_oracle.py anchors it outside itself (the Keys polynomial in fractions, PIL's BICUBIC resize)."""
import numpy as np

import image_oracle as IO

WEIGHTS = {2: (-3, -9, 29, 111, 111, 29, -9, -3),
           4: (-7, -45, -75, -49, 93, 399, 745, 987, 987, 745, 399, 93, -49, -75, -45, -7)}
D = {2: 256, 4: 4096}
HR_TILE = (128, 32)                 # SESRQ_DOWNSCALE_TILE_HR_W / _H: a workgroup's tile in HR pixels


def tile(r):
    """(width, height) of the kernel's tile in LR pixels at factor r."""
    return HR_TILE[0] // r, HR_TILE[1] // r


def header_tile():
    """(SESRQ_DOWNSCALE_TILE_W, SESRQ_DOWNSCALE_TILE_H) and the HR tile as include/sesrq_downscale.h exports them."""
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "sesrq_downscale.h")).read()
    v = {k: int(x) for k, x in re.findall(r"#define SESRQ_DOWNSCALE_TILE_(\w+) (\d+)", src)}
    return (v["W"], v["H"]), (v["HR_W"], v["HR_H"])


def mirror(j, n):
    i = np.mod(j, 2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def taps(n, r):
    """(n / r, 4 r) int64: the mirrored HR index of every tap of every LR index of an axis of length n."""
    assert n % r == 0 and n >= r
    return mirror(r * np.arange(n // r, dtype=np.int64)[:, None] - 3 * r // 2 + np.arange(4 * r, dtype=np.int64)[None, :], n)


def one_pass(a, r, axis, sums=False):
    """One pass along `axis` of a uint8 array: uint8 (or, sums=True, the int64 sums before rounding)."""
    a = np.moveaxis(np.asarray(a), axis, 0)
    assert a.dtype == np.uint8
    idx = taps(a.shape[0], r)
    w = np.asarray(WEIGHTS[r], np.int64).reshape((1, 4 * r) + (1,) * (a.ndim - 1))
    s = (a.astype(np.int64)[idx] * w).sum(1)
    assert np.abs(s).max(initial=0) <= 255 * 4448
    out = s if sums else np.clip((s + D[r] // 2) // D[r], 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def downscale(img, r, keep=False):
    """(N, H, W, 3) or (H, W, 3) uint8 -> the LR image (N, H / r, W / r, 3) uint8 (byte order does not matter: channels are
    independent); keep=True also returns the uint8 intermediate (N, H / r, W, 3)."""
    a = np.asarray(img)
    if a.ndim == 3:
        a = a[None]
    assert a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3 and a.shape[1] % r == 0 and a.shape[2] % r == 0
    v = one_pass(a, r, 1)
    h = np.ascontiguousarray(one_pass(v, r, 2))
    return (h, v) if keep else h


def decode(img, r, form, order="rgb", scale_in=None, zero_in=None, exact_div=0):
    """(lr uint8, x fp32 (N, C, H / r, W / r), q0 int8 | None): the LR image and sesrq_image.h's decode of it."""
    lr = downscale(img, r)
    x = np.ascontiguousarray(IO.decode(lr, form, order))
    q = None if scale_in is None else np.ascontiguousarray(IO.q0(x, scale_in, zero_in, exact_div)).astype(np.int8)
    return lr, x, q


def clamp_pattern(n, r, d, high):
    """(n,) uint8 along one axis: 255 where the weight of LR index d's tap is positive and 0 elsewhere (high=True: the sum is
    D + 2 * 255 * |negative weights|, far above 255 D) or the inverse (far below 0).  d's taps must lie inside the axis."""
    j0 = r * d - 3 * r // 2
    assert j0 >= 0 and j0 + 4 * r <= n
    line = np.full(n, 0 if high else 255, np.uint8)
    w = np.asarray(WEIGHTS[r])
    line[j0:j0 + 4 * r] = np.where((w > 0) == high, 255, 0)
    return line
