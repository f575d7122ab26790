"""numpy restatement of include/sesrq_unprocess.h: steps 1 .. 5 in explicit np.float32 operations (numpy rounds every fp32 operation
once and never fuses), and the four outputs -- q0 and spread as tests/sensor_oracle.py forms them from the raw frame, which is what the
header promises.  tests/test_unprocess_oracle.py anchors it in float64; tests/test_unprocess.py compares the device with it bit for bit."""
import numpy as np

import sensor_oracle as SO

F32 = np.float32
CFAS = ("rggb", "grbg", "gbrg", "bggr")
# what the tests unprocess: a camera-like rgb2cam whose rows sum to 1, inverse gains of a daylight white balance
RGB2CAM = ((0.75, 0.30, -0.05), (-0.20, 1.10, 0.10), (0.05, -0.45, 1.40))
INV_GAINS = (1 / 2.5, 1 / 1.25, 1 / 2.125)
DOMAIN = (1 / 255.0, -128)             # the q0 domain of the cases that run without a net


def steps(img, L, m=RGB2CAM, d=INV_GAINS, highlight=True, order="rgb"):
    """(N, H, W, 3) uint8 -> dict c (step 2), g (step 3's mean or None), u (step 4 before its clamp), r (step 4): (N, H, W, 3) fp32."""
    m, d = np.asarray(m, F32).reshape(3, 3), np.asarray(d, F32)
    l = np.asarray(L, F32)[img[..., ::-1] if order == "bgr" else img]
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.stack([(m[i, 0] * l[..., 0] + m[i, 1] * l[..., 1]) + m[i, 2] * l[..., 2] for i in range(3)], -1)
        g, s = None, np.broadcast_to(d, c.shape)
        if highlight:
            g = ((c[..., 0] + c[..., 1]) + c[..., 2]) / F32(3.0)
            t = np.fmax(g - F32(0.9), F32(0)) / F32(0.1)
            k = (t * t)[..., None]
            s = np.fmax(k + (F32(1) - k) * d, d)
        u = c * s
        r = np.fmin(np.fmax(u, F32(0)), F32(1))               # fmaxf first: a NaN gives 0
    assert c.dtype == s.dtype == r.dtype == F32
    return dict(c=c, g=g, u=u, r=r)


def codes(img, L, m=RGB2CAM, d=INV_GAINS, highlight=True, order="rgb", D=4095):
    """k_c of step 5: (N, 3, H, W) int32."""
    r = steps(img, L, m, d, highlight, order)["r"]
    return np.rint(r * F32(D)).astype(np.int32).transpose(0, 3, 1, 2)


def outputs(k, cfa="rggb", black=0, white=4095, s0=DOMAIN[0], z0=DOMAIN[1], exact_div=0):
    """The four outputs of codes k (N, 3, H, W): dict raw uint16 (N, H, W), gt fp32, q0 int8, spread fp32 (N, 3, H, W)."""
    N, _, H, W = k.shape
    D = white - black
    ks = np.take_along_axis(k, np.broadcast_to(SO.sites(cfa, H, W), (N, 1, H, W)), 1)[:, 0]
    raw = (black + ks).astype(np.uint16)
    qt = SO.q_table(black, white, s0, z0, exact_div).astype(np.int8)
    return dict(raw=raw, gt=(k.astype(F32) / F32(D)).astype(F32), q0=SO.spread(raw, qt, qt[0], cfa, black, white),
                spread=SO.spread(raw, SO.levels(black, white), F32(0), cfa, black, white))


def run(img, L, m=RGB2CAM, d=INV_GAINS, highlight=True, order="rgb", cfa="rggb", black=0, white=4095, **domain):
    return outputs(codes(img, L, m, d, highlight, order, white - black), cfa, black, white, **domain)


def all_codes():
    """(1, 2, 1024, 3) uint8: all 256 codes per channel and Bayer phase; a grey ramp (mask, white level) and opposed channels (lower clamp)."""
    b = np.arange(1024) // 4                                     # every code at column phases 0 and 1 (and twice over)
    grey = np.stack([b, b, b], -1)
    mixed = np.stack([(b * 7 + 31) % 256, 255 - b, b], -1)
    return np.stack([grey, mixed])[None].astype(np.uint8)
