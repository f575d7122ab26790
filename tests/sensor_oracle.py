"""A numpy restatement of include/sesrq_sensor.h, written from the header's text and sharing no code with sesrq.sensor: CFA sites,
levels, the q0 map (through the oracle's input quantiser) and the MIPI RAW10 / RAW12 byte layouts, pixel group by pixel group.

The reference has no format knob (its / (2**12 - 1) is hard-coded), so formats other than (rggb, 0, 4095, u16) are pinned to this
restatement, and the restatement is pinned to the reference at that format (tests/test_sensor.py, CPU test 1)."""
import numpy as np

from oracle import sesrq_oracle as O

F32 = np.float32
# site channel of (y & 1, x & 1), as the header's comment lists them
SITE = {"rggb": ((0, 1), (1, 2)), "grbg": ((1, 0), (2, 1)), "gbrg": ((1, 2), (0, 1)), "bggr": ((2, 1), (1, 0))}


def sites(cfa, H, W):
    t = np.array(SITE[cfa])
    return t[(np.arange(H) & 1)[:, None], (np.arange(W) & 1)[None, :]]


def levels(black, white):
    """x(d), d = 0 .. white - black: the true fp32 quotient, clamped to [0, 1]."""
    d = np.arange(white - black + 1).astype(F32)
    return np.minimum(np.maximum(d / F32(white - black), F32(0)), F32(1)).astype(F32)


def q_table(black, white, s0, z0, exact_div=0):
    """q0(d): the oracle's input quantiser on the levels; exact_div 2 multiplies by fl(1 / s0)."""
    return O.quantize_input(levels(black, white), s0, z0, reciprocal=exact_div == 2)


def spread(codes, per_d, fill, cfa, black, white):
    """(N, H, W) codes -> (N, 3, H, W): per_d[clamp(code, black, white) - black] at the site channel, `fill` elsewhere."""
    codes = np.asarray(codes)
    N, H, W = codes.shape
    d = np.clip(codes.astype(np.int64), black, white) - black
    out = np.full((N, 3, H, W), fill, per_d.dtype)
    s = sites(cfa, H, W)
    for c in range(3):
        m = s == c
        out[:, c][:, m] = per_d[d][:, m]
    return out


def pack_rows(codes, packing, stride=None, pad=0):
    """(N, H, W) codes -> (N, H, stride) bytes, one pack group at a time as the header spells the layout out."""
    codes = np.asarray(codes).astype(np.int64)
    N, H, W = codes.shape
    nb = {"u16": 2 * W, "raw10": W // 4 * 5, "raw12": W // 2 * 3}[packing]
    out = np.full((N, H, nb if stride is None else stride), pad, np.uint8)
    if packing == "u16":
        for x in range(W):
            out[:, :, 2 * x], out[:, :, 2 * x + 1] = codes[:, :, x] & 255, codes[:, :, x] >> 8
    elif packing == "raw10":
        for g in range(W // 4):
            p = [codes[:, :, 4 * g + k] for k in range(4)]
            for k in range(4):
                out[:, :, 5 * g + k] = p[k] >> 2
            out[:, :, 5 * g + 4] = (p[3] & 3) << 6 | (p[2] & 3) << 4 | (p[1] & 3) << 2 | (p[0] & 3)
    else:
        for g in range(W // 2):
            p0, p1 = codes[:, :, 2 * g], codes[:, :, 2 * g + 1]
            out[:, :, 3 * g], out[:, :, 3 * g + 1] = p0 >> 4, p1 >> 4
            out[:, :, 3 * g + 2] = (p1 & 15) << 4 | (p0 & 15)
    return out
