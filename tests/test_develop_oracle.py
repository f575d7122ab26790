"""The develop export's restatement (tests/develop_oracle.py) anchored outside itself, and the host side of libsesrq_develop.so
(include/sesrq_develop.h): no test here needs a device.

  tables      every gamma / sRGB threshold is the fp32 nearest to the exact preimage, shown in integer arithmetic on the two
              neighbouring midpoints (m_-^5 < y^11 < m_+^5, resp. y^12): no libm involved; the linear branch of sRGB and its knee
              likewise; TRUNC255 by bisection on np.float32 multiplication; sesrq_develop_curve returns exactly these tables
  rounding    on 2^20 seeded values per curve the count is rint(255 f(o)) in float64, except within 1e-6 of a half-integer (and at
              samples that are a threshold themselves, see the test)
  metadata    from_colormatrix against the reference's metadata2tensor (tests/golden/develop/metadata.npz)
  ABI         the library exports exactly the header's symbols and links no other library of the project; every refusal of create and
              export is reached on pointers that are never dereferenced; sim.py's argument errors
  liveness    on the frames the device tests use every clip of the oracle fires, and does not fire, on >= 1 % of the samples"""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import develop_oracle as DO
from sesrq import develop

F32 = np.float32
HEADER = os.path.join(ROOT, "include", "sesrq_develop.h")
KINDS = ("gamma", "srgb", "trunc255")


def _frac(t):
    return Fraction(float(t))


def _midpoints(t):
    t = F32(t)
    return (_frac(t) + _frac(np.nextafter(t, F32(-1)))) / 2, (_frac(t) + _frac(np.nextafter(t, F32(2)))) / 2


# ------------------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("kind", ["gamma", "srgb"])
def test_thresholds_are_the_nearest_floats_of_the_exact_preimages(kind):
    T = develop.curve(kind)
    assert T.dtype == F32 and T.shape == (255,)
    powers = 0
    for k in range(1, 256):
        below, above = _midpoints(T[k - 1])
        v = Fraction(2 * k - 1, 510)
        if kind == "srgb" and v <= Fraction(4045, 100000):
            x = v * Fraction(100, 1292)                              # v / 12.92
            assert below < x < above, (kind, k)
            continue
        y = v if kind == "gamma" else (v + Fraction(55, 1000)) * Fraction(1000, 1055)
        a = 11 if kind == "gamma" else 12
        # T = y^(a/5): T^5 = y^a.  Integers on both sides: (num_m / den_m)^5 vs (num_y / den_y)^a
        for m, sign in ((below, -1), (above, 1)):
            lhs = m.numerator ** 5 * y.denominator ** a
            rhs = y.numerator ** a * m.denominator ** 5
            assert (lhs < rhs) if sign < 0 else (lhs > rhs), (kind, k, sign)
        powers += 1
    assert powers == (255 if kind == "gamma" else 245)               # sRGB: k = 1 .. 10 lie on the linear branch
    if kind == "srgb":                                               # the knee: both branches' thresholds bracket it, in order
        assert Fraction(2 * 10 - 1, 510) <= Fraction(4045, 100000) < Fraction(2 * 11 - 1, 510)
        assert T[9] < F32(0.0031308) < T[10]


def test_trunc255_thresholds_by_bisection():
    T = develop.curve("trunc255")
    for k in range(1, 256):
        t = F32(T[k - 1])
        assert t * F32(255.0) >= F32(k) and np.nextafter(t, F32(-1)) * F32(255.0) < F32(k), k
        assert int(t * F32(255.0)) == k
    # so the count is image_export's byte for every value between the thresholds
    o = np.random.default_rng(255).random(1 << 16).astype(F32)
    assert np.array_equal(DO.count(o, T), (o * F32(255.0)).astype(np.uint8))
    assert T[254] == F32(1.0)


@pytest.mark.parametrize("kind", KINDS)
def test_library_tables_are_the_oracles_and_increase(kind):
    T = develop.curve(kind)
    assert np.array_equal(T.view(np.uint32), DO.table(kind).view(np.uint32))
    assert (np.diff(T.astype(np.float64)) > 0).all() and T[0] > 0 and T[-1] <= 1
    assert np.array_equal(develop.curve(develop.CURVES[kind]), T)
    assert np.array_equal(develop.Profile(curve=kind).curve, T)


def test_curve_refusals():
    for bad in ("gama", 3, -1):
        with pytest.raises(ValueError, match="curve|kind"):
            develop.curve(bad)
    assert develop.lib().sesrq_develop_curve(0, None) != 0 and "NULL" in develop.last_error()


# ------------------------------------------------------------------------------------------------------------------------ rounding
SAMPLES = 1 << 20


@pytest.mark.parametrize("kind", KINDS)
def test_count_is_the_rounding_it_claims(kind):
    """byte == rint(255 f(o)) in float64 wherever 255 f(o) is not within 1e-6 of a half-integer -- for every sample that is not itself
    a threshold.  A threshold is the NEAREST fp32 to the exact preimage, so where it was rounded down the sample o == T[k] counts
    as k while 255 f(o) still lies below k - 1/2, by up to half an ulp of o through the curve's slope: 2.8e-6 (sRGB, o = 0.5118943)
    and 2.1e-6 (o = 0.48808023) on this seed, which 1e-6 cannot cover.  Those samples are held to what the table's definition gives:
    the byte is the larger neighbour and the half-integer lies within half an ulp of o."""
    rng = np.random.default_rng(20)
    T = develop.curve(kind)
    o = np.concatenate([rng.random(SAMPLES // 2).astype(F32),                                   # uniform
                        np.exp2(rng.uniform(-24, 0, SAMPLES // 2)).astype(F32)])               # and every octave down to 2^-24
    o[:4] = (0.0, 1.0, np.nextafter(F32(1), F32(0)), np.finfo(F32).tiny)
    byte = DO.count(o, T).astype(np.int64)
    v = DO.curve_f64(kind, o)
    near = np.abs(v - np.floor(v) - 0.5) < 1e-6
    bad = byte != np.rint(v).astype(np.int64)
    on = np.isin(o, T)
    print(f"{kind}: {int(near.sum())} of {o.size} samples within 1e-6 of a half-integer, {int(on.sum())} are thresholds themselves, "
          f"{int(bad.sum())} differ from rint, {int((bad & on).sum())} of them on a threshold")
    assert near.sum() + (bad & on).sum() < 1e-3 * o.size
    rest = bad & ~near & ~on
    assert not rest.any(), (kind, o[rest][:4], byte[rest][:4], v[rest][:4])
    at = bad & on
    if at.any():
        half_ulp = (DO.curve_f64(kind, np.nextafter(o[at], F32(2))) - DO.curve_f64(kind, np.nextafter(o[at], F32(-1)))) / 4
        assert (byte[at] == np.rint(v[at]).astype(np.int64) + 1).all() and (np.abs(byte[at] - 0.5 - v[at]) <= half_ulp).all()
        assert np.array_equal(T[byte[at] - 1], o[at])
    assert byte.min() == 0 and byte.max() == 255 and len(np.unique(byte)) == 256


# ------------------------------------------------------------------------------------------------------------------------ metadata
def test_from_colormatrix_against_the_reference():
    z = np.load(os.path.join(GOLDEN, "develop", "metadata.npz"), allow_pickle=False)
    assert len(z["xyz2cam"]) >= 4
    for i, x in enumerate(z["xyz2cam"]):
        p = develop.from_colormatrix(x, z["red_gain"][i], z["blue_gain"][i])
        want, ref, e_ref = z["cam2rgb"][i], z["ref_cam2rgb"][i], float(z["e_ref"][i])
        assert e_ref <= 1e-4 * np.abs(want).max()
        assert p.ccm.dtype == F32 and p.ccm.shape == (3, 3)
        ulp = np.spacing(np.abs(want).astype(F32)).astype(np.float64)
        assert (np.abs(p.ccm.astype(np.float64) - want) <= ulp).all(), i
        assert (np.abs(p.ccm.astype(np.float64) - ref.astype(np.float64)) <= e_ref + ulp).all(), i
        assert (np.abs(p.ccm.astype(np.float64).sum(1) - 1) <= 3 * (e_ref + ulp.max())).all(), i
        assert np.array_equal(p.gains, np.array([z["ref_red"][i], 1.0, z["ref_blue"][i]], F32)), i
        assert np.array_equal(p.ccm, DO.cam2rgb_f64(x).astype(F32)) or (np.abs(p.ccm - DO.cam2rgb_f64(x).astype(F32)) <= ulp).all()
        # what a misreading moves: far more than the bound
        assert np.abs(DO.cam2rgb_f64(np.asarray(x).T) - want).max() > 1000 * (e_ref + ulp.max())
    g = develop.from_colormatrix(z["xyz2cam"][0], 2.0, 1.5, rgb_gain=1.25, curve="srgb")
    assert np.array_equal(g.gains, np.array([2.5, 1.25, 1.875], F32)) and np.array_equal(g.curve, develop.curve("srgb"))
    with pytest.raises(ValueError, match="3 x 3"):
        develop.from_colormatrix(np.ones((2, 3)))
    with pytest.raises(ValueError, match="singular"):
        develop.from_colormatrix(np.ones((3, 3)))


def test_profile_refusals_and_identity():
    T = develop.curve("gamma")
    for kw, msg in ((dict(gains=(1, -0.5, 1)), "gains"), (dict(gains=(1, np.nan, 1)), "gains"), (dict(gains=(1, np.inf, 1)), "gains"),
                    (dict(gains=(1, 1)), "three gains"), (dict(ccm=np.ones(8)), "3 x 3"), (dict(ccm=np.full((3, 3), np.inf)), "matrix"),
                    (dict(curve=T[:200]), "255 thresholds"), (dict(curve=T[::-1]), "decrease"),
                    (dict(curve=np.where(np.arange(255) == 7, np.nan, T)), "finite")):
        with pytest.raises(ValueError, match=msg):
            develop.Profile(**kw)
    a, b = develop.Profile((2, 1, 1.5), np.eye(3), "srgb"), develop.Profile([2.0, 1.0, 1.5], np.eye(3).ravel(), develop.curve("srgb"))
    assert a == b and hash(a) == hash(b) and a != develop.Profile((2, 1, 1.5), np.eye(3), "gamma")
    flat = np.repeat(T[::5], 5)[:255]                                # equal neighbours, entries <= 0 and > 1: legal
    flat[:3], flat[-3:] = (-1.0, 0.0, 0.0), (1.5, 1.5, 2.0)
    develop.Profile(curve=flat)
    for m in (1, 5, 6):
        with pytest.raises(ValueError, match="MFLAG"):
            develop.check_mflag(m)
    assert [develop.check_mflag(m) for m in (2, 3, 4)] == [2, 3, 4]


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_develop_library_exports_exactly_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_develop[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 8, names
    assert sorted(develop.SYMBOLS) == names, "python binding and header disagree"
    develop.lib()                                                    # binds every one of them
    nm = subprocess.run(["nm", "-D", "--defined-only", develop.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r" T (sesrq\w*)", nm))) == names
    ldd = subprocess.run(["ldd", develop.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libsesrq" not in ldd, "the develop library links another library of the project"
    dyn = subprocess.run(["readelf", "-d", develop.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libsesrq" not in dyn.replace("libsesrq_develop.so", "")
    assert sorted(develop.instances()) == ["develop_export<f32>", "develop_export<i8>"]
    lib = develop.lib()
    assert lib.sesrq_develop_instance_count() == 2
    assert lib.sesrq_develop_instance_name(2) is None and lib.sesrq_develop_instance_name(-1) is None
    assert lib.sesrq_develop_instance_launches(-1) == -1 and lib.sesrq_develop_instance_launches(2) == -1


def test_other_libraries_instances_unchanged_by_the_develop_library():
    from sesrq import _lib, image
    assert len(_lib.instances()) == 258 and len(image.instances()) == 10
    assert not any("develop" in n for n in list(_lib.instances()) + list(image.instances()))


def _arr(a):
    a = np.ascontiguousarray(a, F32)
    return a, a.ctypes.data


def test_create_refusals_without_a_device():
    lib = develop.lib()
    g, m, T = np.ones(3, F32), np.eye(3, dtype=F32).ravel(), develop.curve("gamma")
    h = C.c_void_p(0x1234)
    nan, inf = np.nan, np.inf

    def create(gains=g, ccm=m, curve=T, out=h):
        keep = [_arr(x) if x is not None else (None, None) for x in (gains, ccm, curve)]
        return lib.sesrq_develop_create(keep[0][1], keep[1][1], keep[2][1], C.byref(out) if out is not None else None)

    cases = [(dict(out=None), "ctx is NULL"), (dict(gains=None), "NULL"), (dict(ccm=None), "NULL"), (dict(curve=None), "NULL")]
    for bad in (nan, inf, -inf, -1.0, -1e-30):
        for c in range(3):
            cases.append((dict(gains=np.where(np.arange(3) == c, bad, g)), f"gain {c}"))
    for bad in (nan, inf, -inf):
        for j in (0, 4, 8):
            cases.append((dict(ccm=np.where(np.arange(9) == j, bad, m)), f"matrix entry {j}"))
    for bad in (nan, inf, -inf):
        for k in (0, 100, 254):
            cases.append((dict(curve=np.where(np.arange(255) == k, bad, T)), f"threshold {k + 1} is not finite"))
    dec = T.copy()
    dec[100] = np.nextafter(dec[99], F32(0))
    cases.append((dict(curve=dec), "threshold 101 is below threshold 100"))
    cases.append((dict(curve=T[::-1]), "decreases"))
    for kw, msg in cases:
        h.value = 0x1234
        assert create(**kw) != 0 and msg in develop.last_error(), (msg, develop.last_error())
        assert kw.get("out", h) is None or h.value is None, "a refused create must leave *ctx NULL"


def test_export_refusals_without_a_device():
    lib = develop.lib()
    ctx = C.c_void_p(4096)                        # never dereferenced: every failing check comes before any HIP call
    fake, odd = C.c_void_p(4096), C.c_void_p(4098)
    nan, inf = float("nan"), float("inf")
    for args, msg in (((None, fake, 0, 1.0, 0, 0, fake, 1, 8, 8, None), "ctx is NULL"),
                      ((ctx, None, 0, 1.0, 0, 0, fake, 1, 8, 8, None), "pred is NULL"),
                      ((ctx, fake, 0, 1.0, 0, 0, None, 1, 8, 8, None), "out is NULL"),
                      ((ctx, fake, 2, 1.0, 0, 0, fake, 1, 8, 8, None), "pred_dtype"),
                      ((ctx, fake, -1, 1.0, 0, 0, fake, 1, 8, 8, None), "pred_dtype"),
                      ((ctx, fake, 1, 0.0, 0, 0, fake, 1, 8, 8, None), "scale"),
                      ((ctx, fake, 1, -0.01, 0, 0, fake, 1, 8, 8, None), "scale"),
                      ((ctx, fake, 1, nan, 0, 0, fake, 1, 8, 8, None), "scale"),
                      ((ctx, fake, 1, inf, 0, 0, fake, 1, 8, 8, None), "scale"),
                      ((ctx, fake, 1, 0.01, 128, 0, fake, 1, 8, 8, None), "int8 range"),
                      ((ctx, fake, 1, 0.01, -129, 0, fake, 1, 8, 8, None), "int8 range"),
                      ((ctx, odd, 0, 1.0, 0, 0, fake, 1, 8, 8, None), "4-byte aligned"),
                      ((ctx, fake, 0, 1.0, 0, 2, fake, 1, 8, 8, None), "order"),
                      ((ctx, fake, 0, 1.0, 0, -1, fake, 1, 8, 8, None), "order"),
                      ((ctx, fake, 0, 1.0, 0, 0, fake, 0, 8, 8, None), "empty frame"),
                      ((ctx, fake, 0, 1.0, 0, 0, fake, 1, 0, 8, None), "empty frame"),
                      ((ctx, fake, 0, 1.0, 0, 0, fake, 1, 8, -1, None), "empty frame"),
                      ((ctx, fake, 0, 1.0, 0, 0, fake, 1, 1 << 16, 1 << 15, None), "too large"),                # H W = 2^31
                      ((ctx, fake, 1, 0.01, 0, 0, fake, 1 << 11, 1 << 12, 1 << 12, None), "too large"),         # the runs: 2^31
                      ((ctx, fake, 1, 0.01, 0, 0, fake, 1023, 1 << 13, 1 << 12, None), "too large")):           # ... plus a grid round
        assert lib.sesrq_develop_export(*args) != 0 and msg in develop.last_error(), (msg, develop.last_error())


def test_python_refusals_without_a_device():
    import torch
    p = develop.Profile()
    x = torch.zeros((1, 3, 4, 4))
    for args, kw, msg in (((x, p), {}, "HIP device"), ((x[:, :2], p), {}, "2 channels"), ((x[0], p), {}, r"\(N, 3, H, W\)"),
                          ((x, "gamma"), {}, "Profile"), ((x, p), dict(order="rbg"), "order")):
        with pytest.raises(ValueError, match=msg):
            develop.export(*args, **kw)


BASE = ["--params", "p.npz", "--mflag", "3"]


@pytest.mark.parametrize("argv, msg", [
    (["--mflag", "1", "--input", "a_4_4.raw", "--develop", "--save-png", "o.png"], "mosaic"),
    (["--mflag", "5", "--input", "a_4_4.raw", "--develop", "--save-png", "o.png"], "MFLAG 5"),
    (["--mflag", "6", "--input", "a_4_4.raw", "--develop", "--save-png", "o.png"], "MFLAG 6"),
    (BASE + ["--input", "a.npy", "--develop", "--save-png", "o.png"], r"\*\.raw"),
    (BASE + ["--develop", "--save-png", "o.png"], r"\*\.raw"),
    (BASE + ["--input", "a_4_4.raw", "--develop"], "--save-png"),
    (BASE + ["--input", "a_4_4.raw", "--save-png", "o.png", "--curve", "srgb"], "belong to --develop"),
    (BASE + ["--input", "a_4_4.raw", "--save-png", "o.png", "--wb", "2,1,1.5"], "belong to --develop"),
    (BASE + ["--input", "a_4_4.raw", "--develop", "--save-png", "o.png", "--wb", "2,1"], "three gains"),
    (BASE + ["--input", "a_4_4.raw", "--develop", "--save-png", "o.png", "--wb", "2,-1,1"], "gains"),
    (BASE + ["--input", "a_4_4.raw", "--develop", "--save-png", "o.png", "--ccm"] + ["1"] * 9 + ["--colormatrix"] + ["1"] * 9, "either --ccm"),
    (BASE + ["--input", "a_4_4.raw", "--develop", "--save-png", "o.png", "--red-gain", "2"], "belong to --colormatrix"),
    (BASE + ["--input", "a_4_4.raw", "--develop", "--save-png", "o.png", "--colormatrix"] + ["1"] * 9, "singular"),
    (BASE + ["--input", "a_4_4.raw", "--develop", "--save-png", "o.png", "--curve", "linear"], "invalid choice"),
])
def test_sim_argument_errors(argv, msg, capsys):
    import sim
    with pytest.raises(SystemExit) as e:
        sim.main(argv)
    assert e.value.code == 2                                         # an argparse error
    assert re.search(msg, capsys.readouterr().err), msg


# ------------------------------------------------------------------------------------------------------------------------ liveness
@pytest.mark.parametrize("dtype", ["f32", "i8"])
def test_oracle_is_live_on_the_device_tests_frames(dtype):
    rng = np.random.default_rng(3)
    pred = DO.frame(rng, (2, 3, 64, 96), dtype)
    dom = dict(scale=DO.DOMAIN[0], zero=DO.DOMAIN[1]) if dtype == "i8" else {}
    s = DO.steps(pred, DO.GAINS, DO.CCM, **dom)
    sites = {"step 1 low": s["p"] < 0, "step 1 high": s["p"] > 1, "step 2 high": s["u"] > 1, "step 3 low": s["s"] < 0,
             "step 3 high": s["s"] > 1}
    for name, fired in sites.items():
        share = float(fired.mean())
        print(f"{dtype} {name}: fires on {100 * share:.1f} %")
        assert 0.01 <= share <= 0.99, (name, share)
    assert np.array_equal(s["w"], np.minimum(s["u"], F32(1))) and np.array_equal(s["o"], np.clip(s["s"], 0, 1))
    for kind in KINDS:
        b = DO.export(pred, DO.GAINS, DO.CCM, develop.curve(kind), **dom)
        assert b.shape == (2, 64, 96, 3) and b.dtype == np.uint8
        share = np.bincount(b.ravel(), minlength=256).max() / b.size
        assert share <= 0.6, (kind, share)
        assert np.array_equal(DO.export(pred, DO.GAINS, DO.CCM, develop.curve(kind), "bgr", **dom), b[..., ::-1])
    # a NaN is 0 at step 1; the int8 route is the fp32 route on its dequantised values
    assert (DO.export(np.full((1, 3, 1, 1), np.nan, F32), T=develop.curve("gamma")) == 0).all()
    if dtype == "i8":
        assert np.array_equal(DO.export(pred, DO.GAINS, DO.CCM, develop.curve("srgb"), **dom),
                              DO.export(DO.dequant(pred, *DO.DOMAIN), DO.GAINS, DO.CCM, develop.curve("srgb")))
