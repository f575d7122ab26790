"""A numpy restatement of include/sesrq_noise.h, written from the header's text and sharing no code with sesrq.noise: Philox4x32-10 in
uint64 arithmetic, the two uniforms, the Box-Muller deviates in float64, the reference's add_noise sequence in float32 (`combine`,
pinned to the reference bit for bit by tests/golden/noise/add_noise.npz) and the whole frame (`frame`: tests/sensor_oracle.py's clean
frame, the combine, the clamp and the oracle's input quantiser)."""
import numpy as np

import sensor_oracle as SO
from oracle import sesrq_oracle as O

F32 = np.float32
U64 = np.uint64
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = U64(0xFFFFFFFF)
Z_MAX = float(np.sqrt(48 * np.log(2.0)))          # u_r >= 2^-24: |z| <= sqrt(-2 ln 2^-24) = 5.77


def philox(counter, key):
    """Philox4x32-10.  counter: four uint32 arrays (broadcast against each other), key: two -> the four result words (uint64 arrays
    holding 32-bit values)."""
    c = [np.asarray(v, U64) & MASK for v in np.broadcast_arrays(*counter)]
    k = [U64(int(key[0]) & 0xFFFFFFFF), U64(int(key[1]) & 0xFFFFFFFF)]
    for r in range(10):
        if r:
            k = [(k[0] + U64(W0)) & MASK, (k[1] + U64(W1)) & MASK]
        p0, p1 = U64(M0) * c[0], U64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> U64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> U64(32)) ^ c[3] ^ k[1], p0 & MASK]
    return c


def words(seed, frame, H, W):
    """(w0, w1, w2, w3), each (H, W), of one frame."""
    seed, frame = int(seed) & (2 ** 64 - 1), int(frame) & (2 ** 64 - 1)
    x, y = np.arange(W, dtype=U64)[None, :], np.arange(H, dtype=U64)[:, None]
    return philox((x, y, U64(frame & 0xFFFFFFFF), U64(frame >> 32)), (seed & 0xFFFFFFFF, seed >> 32))


def words_at(seed, frame, y, x):
    """(w0, w1, w2, w3) of one pixel, as ints."""
    seed, frame = int(seed) & (2 ** 64 - 1), int(frame) & (2 ** 64 - 1)
    w = philox([np.array([v], U64) for v in (x, y, frame & 0xFFFFFFFF, frame >> 32)], (seed & 0xFFFFFFFF, seed >> 32))
    return tuple(int(v[0]) for v in w)


def u_r(w):
    return ((w >> U64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def u_t(w):
    return (w >> U64(8)).astype(np.float64) * 2.0 ** -24


def deviates(seed, frame0, N, H, W):
    """(N, 3, H, W) float64: z[c] of every pixel of frames frame0 .. frame0 + N - 1."""
    out = np.empty((N, 3, H, W), np.float64)
    for n in range(N):
        w = words(seed, int(frame0) + n, H, W)
        ra, rb = np.sqrt(-2.0 * np.log(u_r(w[0]))), np.sqrt(-2.0 * np.log(u_r(w[2])))
        ta, tb = 2.0 * np.pi * u_t(w[1]), 2.0 * np.pi * u_t(w[3])
        out[n, 0], out[n, 1], out[n, 2] = ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb)
    return out


def variance(x, shot, read):
    """v = fl(fl(x * shot) + read) in float32."""
    return ((np.asarray(x, F32) * np.asarray(shot, F32)).astype(F32) + np.asarray(read, F32)).astype(F32)


def combine(x, shot, read, z, sigma=None):
    """The reference's add_noise in float32, one IEEE operation a step: x + sqrt(x * shot + read) * z.  shot / read: scalars or arrays
    that broadcast against x.  sigma: a square root to take in place of the correctly rounded one (a reference build whose vector
    sqrt is not: tests/test_noise_oracle.py)."""
    x, z = np.asarray(x, F32), np.asarray(z, F32)
    if sigma is None:
        sigma = np.sqrt(variance(x, shot, read)).astype(F32)
    return (x + (sigma * z).astype(F32)).astype(F32)


def clean(codes, cfa, black, white):
    """(N, H, W) codes -> the clean (N, 3, H, W) fp32 frame of tests/sensor_oracle.py."""
    return SO.spread(codes, SO.levels(black, white), F32(0), cfa, black, white)


def frame(codes, cfa, black, white, levels, z, s0, z0, exact_div=0):
    """(spread, q0) of the noisy frame.  levels: (shot, read), or an (N, 2) array of them per frame; z: (N, 3, H, W) deviates.  The
    clamp is the header's fminf(fmaxf(y, 0), 1): a NaN y (sigma = inf times a deviate that is exactly 0) gives 0, never a NaN."""
    x = clean(codes, cfa, black, white)
    lv = np.asarray(levels, F32)
    shot, read = (lv[0], lv[1]) if lv.ndim == 1 else (lv[:, 0].reshape(-1, 1, 1, 1), lv[:, 1].reshape(-1, 1, 1, 1))
    with np.errstate(over="ignore", invalid="ignore"):          # levels at the top of what the header accepts: v = inf, inf * 0
        y = combine(x, shot, read, z)
    sp = np.fmin(np.fmax(y, F32(0)), F32(1)).astype(F32)
    return sp, O.quantize_input(sp, s0, z0, reciprocal=exact_div == 2)

