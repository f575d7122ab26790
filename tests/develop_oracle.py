"""numpy restatement of include/sesrq_develop.h: the develop export, step by step, in explicit np.float32 operations (numpy rounds
every fp32 operation once and never fuses), with searchsorted for the threshold count.  tests/test_develop_oracle.py anchors the
tables and the count outside this file; tests/test_develop.py compares the device with it byte for byte.

The built-in tables are restated here from their definitions: gamma and sRGB as the fp32 nearest to the exact preimage, found from a
float64 guess and settled in exact rational arithmetic; TRUNC255 by bisection on np.float32 multiplication."""
from fractions import Fraction

import numpy as np

F32 = np.float32
LEVELS = 255
IDENTITY = np.eye(3, dtype=F32)
UNIT = np.ones(3, F32)


# --------------------------------------------------------------------------------------------------------------------- tables
def nearest_f32(x: Fraction) -> np.float32:
    """The fp32 nearest to a positive rational, ties to even, in exact arithmetic (normal range)."""
    assert x > 0
    e = 0
    while x >= 2:
        x, e = x / 2, e + 1
    while x < 1:
        x, e = x * 2, e - 1
    assert -126 <= e <= 127
    m = x * (1 << 23)                        # in [2^23, 2^24)
    n, r = divmod(m.numerator, m.denominator)
    twice = 2 * r
    if twice > m.denominator or (twice == m.denominator and n & 1):
        n += 1
    return F32(np.ldexp(np.float64(n), e - 23))


def preimage_power(k: int, kind: str):
    """(y, a, b) with T[k]^b = y^a exactly: the power branches of the two curves."""
    v = Fraction(2 * k - 1, 510)
    if kind == "gamma":
        return v, 11, 5
    return (v + Fraction(55, 1000)) / Fraction(1055, 1000), 12, 5


def srgb_is_linear(k: int) -> bool:
    return Fraction(2 * k - 1, 510) <= Fraction(4045, 100000)


def table(kind: str) -> np.ndarray:
    """The 255 thresholds of a built-in curve, T[k] at index k - 1."""
    T = np.empty(LEVELS, F32)
    for k in range(1, LEVELS + 1):
        if kind == "trunc255":
            lo, hi = F32(0), F32(2)              # fl(lo * 255) < k <= fl(hi * 255); bisect on the bit patterns
            a, b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
            while b - a > 1:
                mid = (a + b) // 2
                if np.uint32(mid).view(F32) * F32(255.0) >= F32(k):
                    b = mid
                else:
                    a = mid
            T[k - 1] = np.uint32(b).view(F32)
        elif kind == "srgb" and srgb_is_linear(k):
            T[k - 1] = nearest_f32(Fraction(2 * k - 1, 510) / Fraction(1292, 100))
        else:
            y, a, b = preimage_power(k, kind)
            t = F32(float(y) ** (a / b))         # a float64 guess; settled exactly below
            while True:                          # the nearest float t satisfies m_-^b < y^a < m_+^b on its two neighbouring midpoints
                fr = Fraction(float(t))
                below = (fr + Fraction(float(np.nextafter(t, F32(0))))) / 2
                above = (fr + Fraction(float(np.nextafter(t, F32(2))))) / 2
                if y ** a <= below ** b:
                    t = np.nextafter(t, F32(0))
                elif y ** a >= above ** b:
                    t = np.nextafter(t, F32(2))
                else:
                    break
            T[k - 1] = t
    return T


def curve_f64(kind: str, o):
    """255 f(o) of the built-in curves in float64: what the count rounds."""
    o = np.asarray(o, np.float64)
    if kind == "gamma":
        return 255.0 * np.maximum(o, 1e-8) ** (1 / 2.2)
    if kind == "srgb":
        return 255.0 * np.where(o <= 0.0031308, 12.92 * o, 1.055 * np.maximum(o, 1e-12) ** (1 / 2.4) - 0.055)
    return np.floor((o.astype(F32) * F32(255.0)).astype(np.float64)) + 0.0      # trunc255: no rounding involved


# --------------------------------------------------------------------------------------------------------------------- steps
def dequant(q, scale, zero):
    """p = fl((q - zero) * scale), as sesrq_forward forms out_f."""
    return (q.astype(np.int32) - np.int32(zero)).astype(F32) * F32(scale)


def clip01(v):
    """fminf(fmaxf(v, 0), 1): a NaN gives 0."""
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(v, F32(0)), F32(1)).astype(F32)


def steps(pred, gains=UNIT, ccm=IDENTITY, scale=None, zero=None):
    """The intermediates of steps 1 .. 3 of a (N, 3, H, W) prediction: dict p, l (step 1), u (the product of step 2 before its
    clip), w (step 2), s (the sum of step 3 before its clip), o (step 3)."""
    p = dequant(pred, scale, zero) if pred.dtype == np.int8 else np.asarray(pred, F32)
    g = np.asarray(gains, F32).reshape(1, 3, 1, 1)
    m = np.asarray(ccm, F32).reshape(3, 3)
    l = clip01(p)
    with np.errstate(over="ignore", invalid="ignore"):
        u = (l * g).astype(F32)
        w = np.fmin(u, F32(1)).astype(F32)
        s = np.stack([((m[c, 0] * w[:, 0]).astype(F32) + (m[c, 1] * w[:, 1]).astype(F32)).astype(F32) + (m[c, 2] * w[:, 2]).astype(F32)
                      for c in range(3)], 1).astype(F32)
    return dict(p=p, l=l, u=u, w=w, s=s, o=clip01(s))


def count(o, T):
    """byte = #{k : o >= T[k]} of a non-decreasing table."""
    return np.searchsorted(np.asarray(T, F32), o, side="right").astype(np.uint8)


def export(pred, gains=UNIT, ccm=IDENTITY, T=None, order="rgb", scale=None, zero=None):
    """(N, 3, H, W) fp32 / int8 -> (N, H, W, 3) uint8 in `order`."""
    b = count(steps(pred, gains, ccm, scale, zero)["o"], T)
    out = np.ascontiguousarray(b.transpose(0, 2, 3, 1))
    return np.ascontiguousarray(out[..., ::-1]) if order == "bgr" else out


# --------------------------------------------------------------------------------------------------------------------- metadata
RGB2XYZ = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]])


def cam2rgb_f64(xyz2cam):
    """The reference's metadata2tensor in float64, the inverse by Cramer's rule with exact-order cofactors."""
    a = np.asarray(xyz2cam, np.float64).reshape(3, 3) @ RGB2XYZ
    a = a / a.sum(axis=-1, keepdims=True)
    inv = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            r = [x for x in range(3) if x != j]
            c = [x for x in range(3) if x != i]
            inv[i, j] = (-1) ** (i + j) * (a[r[0], c[0]] * a[r[1], c[1]] - a[r[0], c[1]] * a[r[1], c[0]])
    det = sum(a[0, j] * inv[j, 0] for j in range(3))
    return inv / det


# --------------------------------------------------------------------------------------------------------------------- test frames
# What the device tests (tests/test_develop.py) develop, kept here so that tests/test_develop_oracle.py can show that the oracle's own
# clips fire on them: gains up to 4, a matrix with negative off-diagonals whose rows sum to 1, an int8 output domain whose
# dequantised range overshoots [0, 1] on both sides.
GAINS = (2.0, 1.0, 4.0)
CCM = ((1.9, -0.7, -0.2), (-0.25, 1.6, -0.35), (-0.1, -0.6, 1.7))
DOMAIN = (0.0047, -119)


def frame(rng, shape, dtype):
    """A random prediction of `shape`: every int8 code, or fp32 values dense near 0, around and outside [0, 1]."""
    if dtype == "i8":
        return rng.integers(-128, 128, shape).astype(np.int8)
    return (rng.random(shape) ** 2 * 1.3 - 0.15).astype(F32)
