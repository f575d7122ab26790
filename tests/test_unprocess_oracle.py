"""tests/unprocess_oracle.py anchored outside itself (60-digit tables, float64 codes) and the library's refusals before any HIP call."""
import ctypes as C
import os

import mpmath
import numpy as np
import pytest

from conftest import GOLDEN

import unprocess_oracle as UO
from sesrq import develop, unprocess

F32 = np.float32
META = np.load(os.path.join(GOLDEN, "develop", "metadata.npz"))


@pytest.mark.parametrize("kind", ["paper", "gamma", "srgb", "linear"])
def test_every_table_entry_is_correctly_rounded(kind):
    L = unprocess.curve(kind)
    assert L.dtype == F32 and L.shape == (256,) and (np.diff(L) > 0).all()
    mp = mpmath.mp.clone()
    mp.dps = 60
    for b in range(256):
        v = mp.mpf(b) / 255
        if kind == "paper":
            u = mp.mpf(1) / 2 - mp.sin(mp.asin(1 - 2 * v) / 3)
            x = max(u, mp.mpf("1e-8")) ** mp.mpf("2.2")
        elif kind == "gamma":
            x = v ** mp.mpf("2.2")
        elif kind == "srgb":
            x = v / mp.mpf("12.92") if v <= mp.mpf("0.04045") else ((v + mp.mpf("0.055")) / mp.mpf("1.055")) ** mp.mpf("2.4")
        else:
            x = v
        err = abs(mp.mpf(float(L[b])) - x)
        for other in (np.nextafter(L[b], F32(-1)), np.nextafter(L[b], F32(2))):
            assert err < abs(mp.mpf(float(other)) - x), (kind, b, L[b])


def _image():
    rng = np.random.default_rng(64)
    img = rng.integers(0, 256, (1, 64, 64, 3), dtype=np.uint8)
    img[0, 8:16] = rng.integers(0, 2, (8, 64, 3)) * 255
    img[0, 24:32] = rng.integers(225, 256, (8, 64, 3))
    return img


def test_oracle_codes_against_float64():
    """Codes may differ only where float64's r D is within 0.02 of a half-integer (about 16 roundings x 2^-24 x 4095 x sum|m| <= 0.004).
    The mask and the upper clamp fire under every matrix; the lower clamp needs a row negative enough, which the first matrix has."""
    img = _image()
    live = []
    for cam in range(6):
        p = unprocess.from_colormatrix(META["xyz2cam"][cam], 2.5 / 1.25, 2.125 / 1.25, 1.25)
        a = META["xyz2cam"][cam] @ np.asarray(develop.RGB2XYZ)             # metadata2tensor's rgb2cam, rounded once
        assert np.array_equal(p.rgb2cam, (a / a.sum(-1, keepdims=True)).astype(F32)) and np.array_equal(p.inv_gains, np.array(UO.INV_GAINS, F32))
        inv = unprocess.from_develop(develop.from_colormatrix(META["xyz2cam"][cam], 2.0, 1.7, 1.25))
        assert np.allclose(inv.rgb2cam, p.rgb2cam, atol=2e-6) and np.allclose(inv.inv_gains, p.inv_gains, rtol=3e-7)
        s = UO.steps(img, p.curve, p.rgb2cam, p.inv_gains)
        k = UO.codes(img, p.curve, p.rgb2cam, p.inv_gains)
        m, d = p.rgb2cam.astype(np.float64), p.inv_gains.astype(np.float64)
        c = p.curve.astype(np.float64)[img] @ m.T
        t = np.maximum(c.sum(-1) / 3.0 - 0.9, 0) / 0.1
        sc = np.maximum((t * t)[..., None] * (1 - d) + d, d)              # k + (1 - k) d
        rD = np.clip(c * sc, 0, 1) * 4095.0
        k64 = np.rint(rD).astype(np.int32).transpose(0, 3, 1, 2)
        off = np.abs(rD - np.floor(rD) - 0.5).transpose(0, 3, 1, 2)
        assert (off[k != k64] < 0.02).all() and (np.abs(k - k64) <= 1).all(), (cam, int((k != k64).sum()))
        live.append(((s["g"] > 0.9).mean(), (s["u"] > 1).mean(), (s["u"] < 0).mean()))
        assert live[-1][0] > 0 and live[-1][1] > 0, (cam, live[-1])
    assert live[0][2] > 0 and sum(v[2] for v in live) > 0, live


def test_create_and_curve_refuse_before_any_hip_call():
    lib, h = unprocess.lib(), C.c_void_p()
    ok = dict(L=unprocess.curve("paper"), m=np.eye(3, dtype=F32), d=np.ones(3, F32), highlight=1, cfa=0, black=0, white=4095, scale=0.004, zero=-128, exact_div=0)
    bad = lambda a, i, v: np.array([v if j == i else x for j, x in enumerate(a.ravel())], F32).reshape(a.shape)
    for kw, word in ((dict(L=bad(ok["L"], 7, np.nan)), "table entry 7"), (dict(m=bad(ok["m"], 5, np.inf)), "matrix entry 5"),
                     (dict(d=bad(ok["d"], 1, -0.5)), "inverse gain 1"), (dict(d=bad(ok["d"], 2, np.nan)), "inverse gain 2"), (dict(highlight=2), "highlight"),
                     (dict(cfa=4), "cfa"), (dict(black=4095), "levels"), (dict(white=65536), "levels"), (dict(black=-1), "levels"),
                     (dict(scale=0.0), "scale_in"), (dict(scale=np.inf), "scale_in"), (dict(exact_div=3), "exact_div")):
        a = [v.ctypes.data if isinstance(v, np.ndarray) else v for v in {**ok, **kw}.values()]
        assert lib.sesrq_unprocess_create(*a, C.byref(h)) != 0 and h.value is None and word in unprocess.last_error(), (word, unprocess.last_error())
    assert lib.sesrq_unprocess_curve(4, ok["L"].ctypes.data) != 0 and "kind 4" in unprocess.last_error()
