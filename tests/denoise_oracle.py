"""A numpy restatement of include/sesrq_denoise.h, written from the header's text and sharing no code with sesrq.denoise: the staged
sample, the fold, the per-sample g, the 49 candidates in their order, the row sums and their sum, the weight and the true quotient.
With dtype float32 every operation below is one numpy operation on float32 operands, so each is rounded once, as the header demands;
dtype float64 evaluates the same formulas for the rounding bound."""
import numpy as np

from sensor_oracle import sites

F32 = np.float32


def fold(t, n):
    """Reflection about the first and the last sample without repeating it; period 2 (n - 1)."""
    u = np.mod(t, 2 * (n - 1))
    return np.where(u < n, u, 2 * (n - 1) - u)


def samples_raw(codes, black, white):
    """(N, H, W) codes -> x(v) of sesrq_sensor.h."""
    return (np.clip(np.asarray(codes).astype(np.int64), black, white) - black).astype(F32) / F32(white - black)


def samples_spread(spread, cfa):
    """(N, 3, H, W) fp32 -> each pixel's value in the plane of its site channel, as it is."""
    N, _, H, W = spread.shape
    return np.take_along_axis(spread, np.broadcast_to(sites(cfa, H, W), (N, 1, H, W)), 1)[:, 0]


def nlm(s, levels, h=1.0, dtype=F32):
    """(N, H, W) samples, levels (shot, read) or (N, 2) -> the (N, H, W) denoised samples."""
    N, H, W = s.shape
    with np.errstate(invalid="ignore"):
        c = np.where(s > 0, np.minimum(s, F32(1)), F32(0)).astype(dtype)
    lv = np.broadcast_to(np.asarray(levels, F32), (N, 2)).astype(dtype)
    v = c * lv[:, 0, None, None] + lv[:, 1, None, None]
    g = dtype(1) / np.fmax(v * dtype(2), dtype(2.0 ** -100))
    yy, xx = fold(np.arange(-8, H + 8), H), fold(np.arange(-8, W + 8), W)
    cp, gp = c[:, yy][:, :, xx], g[:, yy][:, :, xx]
    at = lambda a, dy, dx: a[:, 8 + dy:8 + dy + H, 8 + dx:8 + dx + W]
    rh, k004 = dtype(F32(1.0) / F32(h)), dtype(F32(0.04))
    num, den = np.zeros((N, H, W), dtype), np.zeros((N, H, W), dtype)
    for j in range(-3, 4):
        for i in range(-3, 4):
            r = []
            for a in range(-2, 3):
                e = [np.square(at(cp, a, b) - at(cp, 2 * j + a, 2 * i + b)) * at(gp, a, b) for b in range(-2, 3)]
                r.append((((e[0] + e[1]) + e[2]) + e[3]) + e[4])
            Dp = (((r[0] + r[1]) + r[2]) + r[3]) + r[4]
            k = np.fmax(dtype(1) - np.fmax(Dp * k004 - dtype(1), dtype(0)) * rh, dtype(0))
            w = k * k if (i, j) != (0, 0) else np.ones_like(k)
            num, den = num + w * at(cp, 2 * j, 2 * i), den + w
    return num / den


def place(vals, cfa):
    """(N, H, W) -> the spread frame (N, 3, H, W): the value in the plane of the site channel, +0.0 in the two others."""
    N, H, W = vals.shape
    out = np.zeros((N, 3, H, W), vals.dtype)
    np.put_along_axis(out, np.broadcast_to(sites(cfa, H, W), (N, 1, H, W)), vals[:, None], 1)
    return out


def denoise_raw(codes, cfa, black, white, levels, h=1.0):
    return place(nlm(samples_raw(codes, black, white), levels, h), cfa)


def denoise_spread(spread, cfa, levels, h=1.0):
    return place(nlm(samples_spread(np.asarray(spread, F32), cfa), levels, h), cfa)
