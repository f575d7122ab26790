"""The classical denoise baseline (sesrq.denoise, libsesrq_denoise.so) against tests/denoise_oracle.py, the numpy restatement of
include/sesrq_denoise.h.  Tolerance zero on the device: every fp32 word is compared as bits.  The oracle itself is anchored first (a
constant frame, the noise it removes, its float64 evaluation).  The kernel's tile is 64 x 32 with a halo of 8, so the sizes sit on 2, 3
(several reflections inside the halo), 9 (the first size above it), a tile - 2, a tile and two tiles + 2 per axis (the nearest legal
width for RAW10 / RAW12)."""
import ctypes as C
import os

import numpy as np
import pytest

import demosaic_oracle as DO
import denoise_oracle as NO
import sensor_oracle as SO
from conftest import GOLDEN
from helpers import Arena, device, same, score, stream_ptr
from sesrq import denoise, sensor as S

gpu = pytest.mark.gpu
F32 = np.float32
CFAS = ("rggb", "grbg", "gbrg", "bggr")
FORMATS = {"u16": (256, 65535), "raw10": (64, 1023), "raw12": (0, 4095)}
LEVELS = ((0.01, 5e-4), (0.0, 1e-3), (0.01, 0.0))          # read = 0: black samples have v = 0 and the 2^-100 floor fires
HS, WS = (2, 3, 9, 30, 32, 66), (2, 3, 9, 62, 64, 130)
LEGAL = {"u16": {}, "spread": {}, "raw10": {2: 4, 3: 4, 9: 8, 62: 60, 66: 68, 130: 132}, "raw12": {3: 2, 9: 10}}
BOUND64 = 4 * 2.548e-7     # 4 x the largest |float32 - float64 evaluation| measured on the synthetic frame (profiles/denoise_probe.txt)


def synthetic(levels, seed=0, H=96, W=128):
    """(clean, noisy) RGGB samples (1, H, W): a smooth sinusoid times 16 x 24 blocks, per-colour gains; the model's noise, clipped."""
    y, x = np.mgrid[0:H, 0:W]
    gain = np.array([0.8, 1.0, 0.6])[SO.sites("rggb", H, W)]
    clean = ((0.5 + 0.3 * np.sin(2 * np.pi * x / 64) * np.cos(2 * np.pi * y / 48)) * (0.6 + 0.4 * ((y // 16 + x // 24) & 1)) * gain)[None]
    z = np.random.default_rng(seed).standard_normal(clean.shape)
    return clean.astype(F32), np.clip(clean + np.sqrt(clean * levels[0] + levels[1]) * z, 0, 1).astype(F32)


def frame(rng, N, H, W):
    """Samples in [0, 1] whose patches are neither equal nor unrelated, so weights land strictly inside (0, 1) as well as on both
    ends: a ramp with noise near the model's, one black corner, one saturated sample."""
    y, x = np.mgrid[0:H, 0:W]
    s = np.clip(0.2 + 0.5 * (x + 2 * y) / (W + 2 * H) + 0.04 * rng.standard_normal((N, H, W)), 0, 1)
    s[:, :H // 2, :W // 3] = 0
    s[:, -1, -1] = 1
    return s.astype(F32)


def levels_of(kind, N, k):
    """Scalars, or an (N, 2) array whose frames differ."""
    return LEVELS[k % 3] if kind == "scalar" else np.array([LEVELS[(k + n) % 3] for n in range(N)], F32)


def run(src, cfa, packing, lv, h=1.0, stride=None, pad=0):
    """The kernel on (N, H, W) codes in `packing`, or on a spread frame ("spread"); lv: a pair, or an (N, 2) array."""
    import torch
    arr = isinstance(lv, np.ndarray)
    p = denoise.Params(h=h) if arr else denoise.Params(*lv, h=h)
    dlv = torch.from_numpy(lv).to(device()) if arr else None
    if packing == "spread":
        out = denoise.run_spread(torch.from_numpy(src).to(device()), cfa, p, levels=dlv)
    else:
        t = torch.from_numpy(SO.pack_rows(src, packing, stride, pad)).to(device())
        kw = {} if stride is None else dict(stride=stride, width=src.shape[2])
        out = denoise.run(t.view(torch.uint16) if packing == "u16" else t, S.Format(cfa, *FORMATS[packing], packing), p, levels=dlv, **kw)
    torch.cuda.synchronize()
    return out


def codes_of(s, packing):
    black, white = FORMATS[packing]
    return np.rint(black + s * (white - black)).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------- no device
def test_oracle_keeps_a_constant_and_removes_noise():
    same("constant", NO.nlm(np.full((1, 7, 9), 0.25, F32), LEVELS[0]), np.full((1, 7, 9), 0.25, F32))      # every w is 1; 49 / 4 / 49 is exact
    clean, noisy = synthetic(LEVELS[0])
    got = NO.nlm(noisy, LEVELS[0])
    mse = lambda a: float(np.mean((a.astype(np.float64) - clean) ** 2))
    print(f"synthetic frame: mse noisy {mse(noisy):.3e}, denoised {mse(got):.3e}")
    assert mse(got) < 0.5 * mse(noisy)
    w = np.abs(got - noisy)
    assert got.min() >= 0 and got.max() <= 1 and w.max() > 0


def test_oracle_against_its_float64_evaluation():
    """w is continuous in Dp, so float32 against float64 is rounding alone."""
    _, noisy = synthetic(LEVELS[0])
    diff = float(np.abs(NO.nlm(noisy, LEVELS[0]) - NO.nlm(noisy, LEVELS[0], dtype=np.float64)).max())
    print(f"largest |float32 - float64|: {diff:.3e}")
    assert diff <= BOUND64


def test_refusals_through_the_c_abi_without_a_device():
    """Pointers that are never dereferenced: every refusal comes before any HIP call."""
    lib, fake = denoise.lib(), 4096
    raw = lambda f=S.Format().c(), src=fake, st=64, shot=0.01, read=1e-4, lv=None, h=1.0, out=fake, N=1, H=8, W=8: \
        lib.sesrq_denoise_raw(C.byref(f), src, st, shot, read, lv, h, out, N, H, W, None)
    for kw, msg in ((dict(src=None), "raw is NULL"), (dict(out=None), "out is NULL"), (dict(out=4098), "4-byte"), (dict(N=0), "empty batch"),
                    (dict(H=1), "H, W >= 2"), (dict(W=1), "H, W >= 2"), (dict(st=15), "row_stride_bytes 15"), (dict(shot=-1.0), "shot"),
                    (dict(read=float("nan")), "read"), (dict(shot=float("inf")), "shot"), (dict(h=0.0), "strength"), (dict(h=-1.0), "strength"),
                    (dict(h=float("nan")), "strength"), (dict(h=float("inf")), "strength"), (dict(lv=4098), "levels is not 4-byte"),
                    (dict(f=S.CFormat(4, 0, 1, 0)), "cfa 4"), (dict(f=S.CFormat(0, 0, 1023, 1), W=6), "multiple of the 4")):
        assert raw(**kw) != 0 and msg in denoise.last_error(), (kw, denoise.last_error())
    for args, msg in (((4, fake, 0.01, 0.0, None, 1.0, fake, 1, 8, 8), "cfa 4"), ((0, None, 0.01, 0.0, None, 1.0, fake, 1, 8, 8), "spread is NULL"),
                      ((0, 4098, 0.01, 0.0, None, 1.0, fake, 1, 8, 8), "4-byte"), ((0, fake, 0.01, 0.0, None, 1.0, fake, 1, 8, 1), "H, W >= 2"),
                      ((0, fake, -0.01, 0.0, None, 1.0, fake, 1, 8, 8), "shot"), ((0, fake, 0.01, 0.0, None, 0.0, fake, 1, 8, 8), "strength")):
        assert lib.sesrq_denoise_spread(*args, None) != 0 and msg in denoise.last_error(), (args, denoise.last_error())
    with pytest.raises(ValueError, match="both shot and read"):
        denoise.Params(shot=0.01)


# ------------------------------------------------------------------------------------------------------------------- device
@gpu
@pytest.mark.parametrize("kind", ("scalar", "array"))
@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("packing", (*FORMATS, "spread"))
def test_matrix(packing, cfa, kind):
    rng, k = np.random.default_rng(len(cfa + packing)), CFAS.index(cfa)
    for N in (1, 3):
        for H, w in zip(HS, WS if N == 1 else WS[::-1]):
            W = LEGAL[packing].get(w, w)
            lv, s = levels_of(kind, N, k + H), frame(rng, N, H, W)
            if packing == "spread":
                sp = np.where(NO.place(np.ones_like(s), cfa) > 0, NO.place(s, cfa), F32(np.nan))      # NaN at the non-sites
                same(f"{N} x {H} x {W}", run(sp, cfa, packing, lv), NO.denoise_spread(sp, cfa, lv))
            else:
                codes = codes_of(s, packing)
                codes[:, 0, 0], codes[:, -1, 0] = 0, FORMATS[packing][1]                         # below black (where there is one), at white
                same(f"{N} x {H} x {W}", run(codes, cfa, packing, lv), NO.denoise_raw(codes, cfa, *FORMATS[packing], lv))


@gpu
def test_spread_nan_negative_zero_and_values_outside_0_1():
    rng = np.random.default_rng(11)
    s = frame(rng, 2, 34, 66)
    s = np.where(rng.random(s.shape) < 0.1, rng.choice(np.array([np.nan, -0.0, 1.5, -0.25, np.inf], F32), s.shape), s)
    sp = np.where(NO.place(np.ones_like(s), "grbg") > 0, NO.place(s, "grbg"), F32(np.nan))
    want = NO.denoise_spread(sp, "grbg", LEVELS[0])
    assert np.isfinite(want).all()
    same("odd values", run(sp, "grbg", "spread", LEVELS[0]), want)


@gpu
@pytest.mark.parametrize("packing,stride", [("u16", 160), ("raw10", 97), ("raw12", 108)])
def test_padded_rows_with_a_canary(packing, stride):
    """Padding behind the wide loads (strides of 160 and 108 bytes keep them) and behind the per-sample ones (97); per-frame levels."""
    codes, lv = codes_of(frame(np.random.default_rng(stride), 2, 34, 68), packing), levels_of("array", 2, stride)
    same(packing, run(codes, "gbrg", packing, lv, stride=stride, pad=0xA5), NO.denoise_raw(codes, "gbrg", *FORMATS[packing], lv))


@gpu
def test_odd_addresses_in_a_canary_arena():
    """raw at an odd address with an odd stride, out at 4 mod 16: the per-sample loads and per-pixel stores; nothing beside out."""
    import torch
    fmt, (N, H, W), stride = S.Format("bggr", *FORMATS["raw10"], "raw10"), (2, 34, 68), 87
    codes = codes_of(frame(np.random.default_rng(3), N, H, W), "raw10")
    arena = Arena(device(), Arena.room(N * H * stride, N * 3 * H * W * 4))
    raw = arena.place((N, H, stride), torch.uint8, 1, SO.pack_rows(codes, "raw10", stride, 0x5A), "raw")
    out = arena.place((N, 3, H, W), torch.float32, 4, name="out")
    cf = fmt.c()
    assert denoise.lib().sesrq_denoise_raw(C.byref(cf), raw.data_ptr(), stride, 0.01, 5e-4, None, 1.0, out.data_ptr(), N, H, W, stream_ptr()) == 0
    torch.cuda.synchronize()
    same("odd addresses", out, NO.denoise_raw(codes, "bggr", *FORMATS["raw10"], LEVELS[0]))
    assert arena.check() == []


@gpu
@pytest.mark.parametrize("h", (0.5, 4.0))
def test_strength(h):
    codes = codes_of(frame(np.random.default_rng(5), 1, 34, 66), "u16")
    same(f"h = {h}", run(codes, "rggb", "u16", LEVELS[0], h=h), NO.denoise_raw(codes, "rggb", *FORMATS["u16"], LEVELS[0], h))


@gpu
def test_zz_every_instantiation_ran():
    """After the cases above: every (input, levels, path) is named by the library's own launch counters."""
    counts = denoise.instances()
    assert len(counts) == 16 and all(counts.values()), [n for n, c in counts.items() if not c]


@gpu
def test_sim_prints_the_denoise_baseline_lines(capsys, tmp_path):
    import sim
    from helpers import raw_frame
    from sesrq.store import STORE
    codes, gt16 = raw_frame("c")
    rawp, gtp = str(tmp_path / f"c_{codes.shape[0]}_{codes.shape[1]}.raw"), str(tmp_path / "gt.npy")
    codes.astype("<u2").tofile(rawp), np.save(gtp, gt16)
    base = ["--input", rawp, "--gt", gtp, "--add-noise", "--shot", "0.01", "--read", "0.0005", "--denoise"]
    nrdm, nr = ["--params", os.path.join(GOLDEN, "nrdm_3_nat.params.npz")], ["--params", os.path.join(GOLDEN, "nr_dm", "nr.params.npz")]
    for flags, line in ((["--mflag", "3", "--baseline", "malvar"] + nrdm, "nlm + malvar baseline mean psnr is:"),
                        (["--mflag", "1", "--denoise-strength", "2"] + nr, "nlm denoise baseline mean psnr is:")):
        STORE.clear()
        sim.main(flags + base)
        assert line in capsys.readouterr().out
    STORE.clear()
    with pytest.raises(SystemExit, match="--baseline too"):
        sim.main(["--mflag", "3"] + nrdm + base)


@gpu
def test_public_entries():
    import torch
    import sesrq
    from sesrq import noise, quality
    from sesrq.bundle import Bundle
    e = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "raw", "nrdm_3.npz")), device())
    fmt, p = S.Format("rggb", 64, 1023), denoise.Params(0.01, 5e-4)
    rng = np.random.default_rng(5)
    codes = codes_of(frame(rng, 2, 34, 66), "raw10").astype(np.uint16)
    gt16 = rng.integers(0, 1100, (2, 3, 34, 66)).astype(np.uint16)
    x = torch.from_numpy(codes).to(device())
    q2, y2 = e.forward_raw(x, fmt=fmt)
    q, y, den = e.forward_raw(x, fmt=fmt, denoise=p)
    want = NO.denoise_raw(codes, "rggb", 64, 1023, LEVELS[0])
    same("denoised", den, want), same("q beside denoise", q, q2), same("y beside denoise", y, y2)
    q, y, base, den = e.forward_raw(x, fmt=fmt, denoise=p, baseline="malvar")
    same("denoised beside a baseline", den, want), same("nlm + malvar", base, DO.demosaic_spread(want, "rggb", "malvar"))
    same("q beside both", q, q2), same("y beside both", y, y2)
    m = noise.NoiseModel(seed=3)                              # levels drawn per frame: denoise=True takes them
    q, y, den = e.forward_raw(x, fmt=fmt, noise=m, denoise=True)
    q3, sp = noise.apply(e, x, fmt, m, want_q=True, want_spread=True)
    torch.cuda.synchronize()
    same("noisy frame denoised", den, NO.denoise_spread(sp.cpu().numpy(), "rggb", m.levels(2)))
    same("q of the noisy frame", q, e.forward(q3)[0])
    with pytest.raises(ValueError, match="noise levels"):
        e.forward_raw(x, fmt=fmt, denoise=True)
    lv = SO.levels(64, 1023)
    gts = [lv[np.clip(g.astype(np.int64), 64, 1023) - 64][None] for g in gt16]
    net, rows = quality.evaluate_raw(e, list(codes), list(gt16), 1, fmt=fmt, denoise=p)
    same("the net's rows, MFLAG 1", net, quality.evaluate_raw(e, list(codes), list(gt16), 1, fmt=fmt))
    net3, rows3 = quality.evaluate_raw(e, list(codes), list(gt16), 3, fmt=fmt, denoise=p, baseline="malvar")
    for k in range(2):
        same(f"nlm rows, frame {k}", rows[k:k + 1], score(want[k:k + 1], gts[k], 1))
        same(f"nlm + malvar rows, frame {k}", rows3[k:k + 1], score(DO.demosaic_spread(want[k:k + 1], "rggb", "malvar"), gts[k], 3))
    with pytest.raises(ValueError, match="baseline="):
        quality.evaluate_raw(e, list(codes), list(gt16), 3, fmt=fmt, denoise=p)
    with pytest.raises(ValueError, match="^MFLAG 1"):
        quality.evaluate_raw(e, [], [], 1, baseline="malvar", denoise=p)
