"""CPU tests of the noise route: tests/noise_oracle.py (the numpy restatement of include/sesrq_noise.h) against the generator's known
answers, the normal distribution, the reference's add_noise (tests/golden/noise/add_noise.npz) and tests/sensor_oracle.py; and
sesrq.noise's host side (levels_from, random_levels, NoiseModel) against the reference's random_noise_levels.

The reference and the square root.  add_noise's eps is reproducible (the same-seed torch.normal(zeros, ones), recorded), and every
step of combine is pinned to it bit for bit but one: torch's vectorised CPU sqrt, in the build the fixture was made with, is off by one
ulp for about 0.4 % of its arguments, where numpy's, the C library's and the device's sqrtf are correctly rounded (the header's "each
step one IEEE fp32 operation").  So the fixture also holds the reference's own sigma, and the test asserts: the variance bit for bit;
sigma within one ulp of the correctly rounded root; combine on the reference's sigma == out bit for bit at every sample; and combine
== out bit for bit wherever the reference's sigma is the correctly rounded one.  (A bound in ulps of `out` on the remaining 0.4 % would
bound nothing: x + sigma * eps cancels at the dark end of the ramp, where one ulp of sigma is many ulps of out -- up to 4 here.)"""
import os

import numpy as np
import pytest

import noise_oracle as NO
import sensor_oracle as SO
from conftest import GOLDEN

F32 = np.float32
SEED, FRAME = 0x0123456789ABCDEF, 7


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. Philox
KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = NO.philox([np.array([c], np.uint64) for c in counter], key)
    assert tuple(int(w[0]) for w in got) == want


def test_words_are_the_counter_layout_of_the_header():
    """counter = (x, y, lo32(f), hi32(f)), key = (lo32(seed), hi32(seed)): one pixel of words() against a direct philox call."""
    f = (5 << 32) | 9
    w = NO.words(SEED, f, 4, 6)
    one = NO.philox([np.array([v], np.uint64) for v in (3, 2, 9, 5)], (SEED & 0xffffffff, SEED >> 32))
    assert [int(w[k][2, 3]) for k in range(4)] == [int(v[0]) for v in one]


# ---------------------------------------------------------------------------------------------------------------- 2. deviates
def test_uniforms_are_exact_in_fp32_and_inside_their_ranges():
    w = np.array([0, 1, 0x1ff, 0x200, 0xffffffff, 0x80000000], np.uint64)
    for u in (NO.u_r(w), NO.u_t(w)):
        assert np.array_equal(u.astype(F32).astype(np.float64), u)
    assert NO.u_r(w).min() == 2.0 ** -24 and NO.u_r(w).max() == 1 - 2.0 ** -24
    assert NO.u_t(w).min() == 0 and NO.u_t(w).max() == 1 - 2.0 ** -24


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_moments_and_correlations_at_six_standard_errors():
    H = W = 64
    z = NO.deviates(SEED, FRAME, 1, H, W)[0]          # (3, 64, 64)
    n = z.size
    assert np.abs(z).max() <= NO.Z_MAX
    m, v = z.mean(), z.var()
    assert abs(m) <= 6 / np.sqrt(n)
    assert abs(v - 1) <= 6 * np.sqrt(2 / n)
    assert abs((z ** 3).mean()) <= 6 * np.sqrt(15 / n)
    assert abs((z ** 4).mean() - 3) <= 6 * np.sqrt(96 / n)
    bound = 6 / np.sqrt(H * W)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert abs(_corr(z[a], z[b])) <= bound, ("channels", a, b)
    for c in range(3):
        assert abs(_corr(z[c][:, :-1], z[c][:, 1:])) <= bound, ("x-neighbours", c)
        assert abs(_corr(z[c][:-1, :], z[c][1:, :])) <= bound, ("y-neighbours", c)
    nxt = NO.deviates(SEED, FRAME + 1, 1, H, W)[0]
    prv = NO.deviates(SEED - 1, FRAME, 1, H, W)[0]
    for c in range(3):
        assert abs(_corr(z[c], nxt[c])) <= bound, ("frames f, f + 1", c)
        assert abs(_corr(z[c], prv[c])) <= bound, ("seeds s, s - 1", c)


def test_kolmogorov_smirnov_against_the_normal():
    from math import erf
    z = np.sort(NO.deviates(SEED, FRAME, 1, 512, 512).ravel())
    n = z.size
    cdf = 0.5 * (1 + np.vectorize(erf)(z / np.sqrt(2.0)))
    d = max(np.abs(cdf - np.arange(1, n + 1) / n).max(), np.abs(cdf - np.arange(n) / n).max())
    assert d <= 1.95 / np.sqrt(n), d


def test_a_batch_is_its_frames():
    z = NO.deviates(SEED, 2 ** 32 - 1, 3, 4, 5)
    for n in range(3):
        assert np.array_equal(z[n], NO.deviates(SEED, 2 ** 32 - 1 + n, 1, 4, 5)[0])
    assert not np.array_equal(z[0], z[1])


# ---------------------------------------------------------------------------------------------------------------- 3. combine
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "noise", "add_noise.npz"), allow_pickle=False)


def test_combine_is_the_references_add_noise(golden):
    x = golden["x"]
    assert np.array_equal(x[:4096], (np.arange(4096).astype(F32) / F32(4095))) and not x[4096:].any()
    lv = golden["levels"]
    assert (lv[:, 0] == 0).any() and (lv[:, 1] == 0).any()
    off = 0
    for p, (shot, read) in enumerate(lv):
        eps, out, sigma = golden[f"eps_{p}"], golden[f"out_{p}"], golden[f"sigma_{p}"]
        v = NO.variance(x, shot, read)
        root = np.sqrt(v.astype(np.float64)).astype(F32)
        assert np.array_equal(bits(np.sqrt(v)), bits(root))                      # numpy's fp32 sqrt is the correctly rounded one
        assert np.abs(bits(sigma).astype(np.int64) - bits(root)).max() <= 1
        assert np.array_equal(bits(NO.combine(x, shot, read, eps, sigma=sigma)), bits(out)), p
        same = sigma == root
        off += int((~same).sum())
        assert np.array_equal(bits(NO.combine(x, shot, read, eps))[same], bits(out)[same]), p
    assert off <= 0.005 * lv.shape[0] * x.size          # the reference's sqrt is off at well under 1 % of the samples
    p = int(np.nonzero((lv == 0).all(1))[0][0])
    assert np.array_equal(bits(golden[f"out_{p}"]), bits(x))                     # zero levels leave the frame as it is


# ---------------------------------------------------------------------------------------------------------------- 4. levels
def test_levels_from_is_random_noise_levels(golden):
    from sesrq import noise
    shot, read = noise.levels_from(golden["log_shot"], golden["g"])
    assert shot.dtype == F32 and read.dtype == F32
    for got, want in ((shot, golden["shot"]), (read, golden["read"])):
        assert (np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all()      # two exps and a multiply-add, each within an ulp
    one = noise.levels_from(golden["log_shot"][3], golden["g"][3])
    assert one[0] == shot[3] and one[1] == read[3]


def test_random_levels_stay_inside_the_references_range():
    from sesrq import noise
    lv = noise.random_levels(np.random.default_rng(11), 20000)
    assert lv.shape == (20000, 2) and lv.dtype == F32
    assert lv[:, 0].min() >= F32(1e-4) and lv[:, 0].max() <= F32(0.012)
    assert lv[:, 0].min() < 1.1e-4 and lv[:, 0].max() > 0.011             # and reach both ends
    # ln read - (2.18 ln shot + 1.20) ~ N(0, 0.26): mean and deviation at 6 standard errors
    r = np.log(lv[:, 1].astype(np.float64)) - (2.18 * np.log(lv[:, 0].astype(np.float64)) + 1.20)
    assert abs(r.mean()) <= 6 * 0.26 / np.sqrt(r.size) and abs(r.std() - 0.26) <= 6 * 0.26 / np.sqrt(2 * r.size)
    assert np.array_equal(lv, noise.random_levels(np.random.default_rng(11), 20000))
    with pytest.raises(ValueError):
        noise.random_levels(np.random.RandomState(1), 2)


def test_noise_model_is_a_value():
    from sesrq import noise
    m = noise.NoiseModel(seed=5)
    assert not m.fixed and m.advance(3).frame0 == 3 and m.frame0 == 0
    assert np.array_equal(m.levels(5)[3:], m.advance(3).levels(2))             # per-frame levels depend on (seed, frame) alone
    assert not np.array_equal(m.levels(2), noise.NoiseModel(seed=6).levels(2))
    f = noise.NoiseModel(0.003, 1e-5, seed=2 ** 64 - 1, frame0=2 ** 64 - 1)
    assert f.fixed and f.advance(2).frame0 == 1 and np.array_equal(f.levels(2), np.array([[0.003, 1e-5]] * 2, F32))
    assert f.plan(2)[:2] == (0.003, 1e-5) and f.plan(2)[2] is None
    for bad in (dict(shot=0.1), dict(read=0.1), dict(shot=-1.0, read=0.0), dict(shot=0.0, read=float("nan")),
                dict(shot=float("inf"), read=0.0), dict(seed=-1), dict(seed=2 ** 64), dict(frame0=1.5), dict(seed=True)):
        with pytest.raises(ValueError):
            noise.NoiseModel(**bad)


# ---------------------------------------------------------------------------------------------------------------- 5. sensor oracle
@pytest.mark.parametrize("cfa", ["rggb", "grbg", "gbrg", "bggr"])
@pytest.mark.parametrize("packing,black,white", [("u16", 64, 1023), ("u16", 4096, 65535), ("raw10", 16, 1023), ("raw12", 0, 4095)])
def test_zero_levels_give_the_sensor_oracles_frame(cfa, packing, black, white):
    """shot = read = 0: the oracle's spread and q0 are tests/sensor_oracle.py's, for every CFA order and packing (the packing only
    bounds the codes: both oracles work on codes)."""
    rng = np.random.default_rng(white)
    top = {"u16": 65535, "raw10": 1023, "raw12": 4095}[packing]
    codes = rng.integers(0, top + 1, (2, 5, 8)).astype(np.uint16)
    codes[0, 0, :2] = (white, black)
    z = NO.deviates(3, 0, 2, 5, 8)
    for s0, z0, ed in ((0.00392155787524055, -128, 0), (0.003686274624630517, -136, 2)):
        sp, q = NO.frame(codes, cfa, black, white, (0.0, 0.0), z, s0, z0, ed)
        t = SO.q_table(black, white, s0, z0, ed)
        assert np.array_equal(bits(sp), bits(SO.spread(codes, SO.levels(black, white), F32(0), cfa, black, white)))
        assert np.array_equal(q, SO.spread(codes, t, t[0], cfa, black, white))
    lv = np.array([[0, 0], [0.01, 1e-4]], F32)                                 # per-frame levels: frame 0 clean, frame 1 not
    sp, _ = NO.frame(codes, cfa, black, white, lv, z, 0.0039, -128)
    cl = NO.clean(codes, cfa, black, white)
    assert np.array_equal(sp[0], cl[0]) and not np.array_equal(sp[1], cl[1])


# ---------------------------------------------------------------------------------------------------------------- CLI flags
def test_cli_noise_flags(monkeypatch):
    """--add-noise defaults to define.TEST_RAW_ADD_NOISE, read when the flags are resolved; noise goes onto *.raw inputs only."""
    import argparse

    import define
    import sim
    from sesrq import noise
    ap = argparse.ArgumentParser()
    sim.add_noise_flags(ap)
    raw, npy = ["a_4_4.raw"], ["a.npy"]
    assert define.TEST_RAW_ADD_NOISE is False
    assert sim.noise_model(ap.parse_args([]), "t", raw) is None
    m = sim.noise_model(ap.parse_args(["--add-noise", "--shot", "0.003", "--read", "1e-5", "--noise-seed", "3"]), "t", raw)
    assert m == noise.NoiseModel(0.003, 1e-5, seed=3)
    assert sim.noise_model(ap.parse_args(["--add-noise"]), "t", raw) == noise.NoiseModel()
    for argv, inputs, word in ((["--shot", "0.003", "--read", "1e-5"], raw, "belong to --add-noise"), (["--noise-seed", "1"], raw, "belong to"),
                               (["--add-noise"], npy, "raw inputs"), (["--add-noise", "--shot", "0.1"], raw, "both shot and read"),
                               (["--add-noise", "--shot", "-1", "--read", "0"], raw, "not negative")):
        with pytest.raises(SystemExit, match=word):
            sim.noise_model(ap.parse_args(argv), "t", inputs)
    monkeypatch.setattr(define, "TEST_RAW_ADD_NOISE", True)
    assert sim.noise_model(ap.parse_args([]), "t", raw) == noise.NoiseModel()
    assert sim.noise_model(ap.parse_args([]), "t", npy) is None            # the reference adds noise to raw frames only
    assert sim.noise_model(ap.parse_args(["--no-add-noise"]), "t", raw) is None
    assert sim.noise_model(ap.parse_args(["--shot", "0.01", "--read", "0"]), "t", raw) == noise.NoiseModel(0.01, 0.0)


def test_noise_library_exports_exactly_the_header():
    """Every function include/sesrq_noise.h declares is bound by sesrq.noise.SYMBOLS, and nothing else."""
    import re

    from conftest import ROOT
    from sesrq import noise
    text = open(os.path.join(ROOT, "include", "sesrq_noise.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sesrq_noise_[a-z_]+)\s*\(", text))
    assert declared == set(noise.SYMBOLS), declared ^ set(noise.SYMBOLS)
