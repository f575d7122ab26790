"""A numpy restatement of include/sesrq_demosaic.h, written from the header's text and sharing no code with sesrq.demosaic: the fold,
the group sums in their order, the two methods' numerators, the clamp and the true fp32 quotient.  Every array is float32 and every
operation below is one numpy operation on float32 operands, so each is rounded once, as the header demands."""
import numpy as np

from sensor_oracle import sites

F32 = np.float32


def fold(t, n):
    """Reflection about the first and the last sample without repeating it; period 2 (n - 1)."""
    u = np.mod(t, 2 * (n - 1))
    return np.where(u < n, u, 2 * (n - 1) - u)


def samples_raw(codes, black, white):
    """(N, H, W) codes -> (the fp32 samples d(v), K = 16 D)."""
    return (np.clip(np.asarray(codes).astype(np.int64), black, white) - black).astype(F32), F32(16 * (white - black))


def samples_spread(spread, cfa):
    """(N, 3, H, W) fp32 -> (each pixel's value in the plane of its site channel, as it is; K = 16)."""
    N, _, H, W = spread.shape
    return np.take_along_axis(spread, np.broadcast_to(sites(cfa, H, W), (N, 1, H, W)), 1)[:, 0], F32(16)


@np.errstate(all="ignore")
def numerators(s, cfa, method):
    """(N, H, W) fp32 samples -> (N, 3, H, W) fp32 numerators S of the planes R, G, B.  Overflow and NaN are legal results."""
    N, H, W = s.shape
    yy, xx = np.arange(H), np.arange(W)
    at = lambda j, i: s[:, fold(yy + j, H)][:, :, fold(xx + i, W)]
    c = s
    n, so, w, e = at(-1, 0), at(1, 0), at(0, -1), at(0, 1)
    A1 = ((n + so) + w) + e
    Dg = ((at(-1, -1) + at(-1, 1)) + at(1, -1)) + at(1, 1)
    V2, H2, Hn, Vn = at(-2, 0) + at(2, 0), at(0, -2) + at(0, 2), w + e, n + so
    site = F32(16) * c
    if method == "malvar":
        green = (F32(8) * c + F32(4) * A1) - F32(2) * (V2 + H2)
        horiz = (((F32(10) * c + F32(8) * Hn) - F32(2) * Dg) - F32(2) * H2) + V2
        vert = (((F32(10) * c + F32(8) * Vn) - F32(2) * Dg) - F32(2) * V2) + H2
        diag = (F32(12) * c + F32(4) * Dg) - F32(3) * (V2 + H2)
    else:
        green, horiz, vert, diag = F32(4) * A1, F32(8) * Hn, F32(8) * Vn, F32(4) * Dg
    ch = sites(cfa, H, W)                                   # the pixel's own channel ...
    mate = sites(cfa, H, W + 1)[:, 1:]                      # ... and the channel of its left and right neighbours
    S = np.empty((N, 3, H, W), F32)
    for k in (0, 2):                                        # R, then B
        S[:, k] = np.where(ch == k, site, np.where(ch == 2 - k, diag, np.where(mate == k, horiz, vert)))
    S[:, 1] = np.where(ch == 1, site, green)
    return S


def finish(S, K):
    """clamp(S) / K: a NaN and a -0.0 give +0.0; the quotient is numpy's float32 division, a true IEEE one."""
    with np.errstate(invalid="ignore"):
        return (np.where(S > 0, np.minimum(S, K), F32(0)).astype(F32) / K).astype(F32)


def demosaic_raw(codes, cfa, black, white, method):
    s, K = samples_raw(codes, black, white)
    return finish(numerators(s, cfa, method), K)


def demosaic_spread(spread, cfa, method):
    s, K = samples_spread(np.asarray(spread, F32), cfa)
    return finish(numerators(s, cfa, method), K)
