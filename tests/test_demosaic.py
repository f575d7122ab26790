"""The classical demosaic baseline (sesrq.demosaic, libsesrq_demosaic.so) against tests/demosaic_oracle.py, the numpy restatement of
include/sesrq_demosaic.h.  Tolerance zero: every fp32 word is compared as bits.  The oracle itself is anchored outside itself first
(constants, ramps, the sensor oracle's x(v)); the kernel's tile is 64 x 32, so the sizes sit on 2, 3, a tile - 2, a tile, a tile + 2
and two tiles + 2 per axis (the nearest legal width for RAW10 / RAW12)."""
import ctypes as C
import os

import numpy as np
import pytest

import demosaic_oracle as DO
import sensor_oracle as SO
from conftest import GOLDEN
from helpers import Arena, device, same, score, stream_ptr
from sesrq import demosaic, sensor as S

gpu = pytest.mark.gpu
F32 = np.float32
CFAS, METHODS = ("rggb", "grbg", "gbrg", "bggr"), ("malvar", "bilinear")
LEVELS = {"u16": (256, 65535), "raw10": (64, 1023), "raw12": (0, 4095)}
TOP = {"u16": 65535, "raw10": 1023, "raw12": 4095}
HS, WS = (2, 3, 30, 32, 34, 66), (2, 3, 62, 64, 66, 130)
LEGAL = {"u16": {}, "raw10": {2: 4, 3: 4, 62: 60, 66: 68, 130: 132}, "raw12": {3: 2}}


def sizes(packing, N):
    """(H, W) on the seams of both axes; the batch of 3 pairs the heights with the widths in reverse."""
    return [(h, LEGAL[packing].get(w, w)) for h, w in zip(HS, WS if N == 1 else WS[::-1])]


def fmt_of(cfa, packing):
    return S.Format(cfa, *LEVELS[packing], packing)


def run_raw(codes, fmt, method, stride=None, pad=0):
    import torch
    t = torch.from_numpy(SO.pack_rows(codes, fmt.packing, stride, pad)).to(device())
    kw = {} if stride is None else dict(stride=stride, width=codes.shape[2])
    out = demosaic.run(t.view(torch.uint16) if fmt.packing == "u16" else t, fmt, method, **kw)
    torch.cuda.synchronize()
    return out


def spread_frame(rng, cfa, shape):
    """Random fp32 in [0, 1] at every pixel's site plane, NaN in its two other planes."""
    N, H, W = shape
    sp = np.full((N, 3, H, W), np.nan, F32)
    np.put_along_axis(sp, np.broadcast_to(SO.sites(cfa, H, W), (N, 1, H, W)), rng.random((N, 1, H, W), F32), 1)
    return sp


# ------------------------------------------------------------------------------------------------------------------- no device
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("cfa", CFAS)
def test_oracle_on_constants_ramps_and_the_site_channel(cfa, method):
    rng = np.random.default_rng(7)
    const = DO.demosaic_raw(np.full((1, 7, 9), 1234), cfa, 100, 60000, method)
    assert (const == F32(1134) / F32(59900)).all()                      # every channel, edges included
    y, x = np.mgrid[0:11, 0:13]
    ramp = DO.demosaic_raw((3 * x + 5 * y + 7)[None], cfa, 0, 65535, method)
    same("ramp", ramp[0, :, 2:-2, 2:-2], np.broadcast_to(((3 * x + 5 * y + 7).astype(F32) / F32(65535))[2:-2, 2:-2], (3, 7, 9)))
    codes = rng.integers(0, 65536, (2, 9, 10))
    got, site = DO.demosaic_raw(codes, cfa, 256, 60000, method), SO.sites(cfa, 9, 10)[None, None]
    want = SO.spread(codes, SO.levels(256, 60000), F32(0), cfa, 256, 60000)
    same("site channel", np.take_along_axis(got, np.broadcast_to(site, (2, 1, 9, 10)), 1), want.sum(1, keepdims=True, dtype=F32))


def test_refusals_through_the_c_abi_without_a_device():
    """Pointers that are never dereferenced: every refusal comes before any HIP call."""
    lib, fake = demosaic.lib(), 4096
    raw = lambda f=S.Format().c(), src=fake, st=64, m=1, out=fake, N=1, H=8, W=8: lib.sesrq_demosaic_raw(C.byref(f), src, st, m, out, N, H, W, None)
    for kw, msg in ((dict(src=None), "raw is NULL"), (dict(out=None), "out is NULL"), (dict(out=4098), "4-byte"), (dict(m=2), "method 2"),
                    (dict(N=0), "empty batch"), (dict(H=1), "H, W >= 2"), (dict(W=1), "H, W >= 2"), (dict(st=15), "row_stride_bytes 15"),
                    (dict(f=S.CFormat(4, 0, 1, 0)), "cfa 4"), (dict(f=S.CFormat(0, 0, 1023, 1), W=6), "multiple of the 4")):
        assert raw(**kw) != 0 and msg in demosaic.last_error(), (kw, demosaic.last_error())
    for args, msg in (((4, fake, 1, fake, 1, 8, 8), "cfa 4"), ((0, None, 1, fake, 1, 8, 8), "spread is NULL"), ((0, 4098, 1, fake, 1, 8, 8), "4-byte"),
                      ((0, fake, 1, fake, 1, 8, 1), "H, W >= 2")):
        assert lib.sesrq_demosaic_spread(*args, None) != 0 and msg in demosaic.last_error(), (args, demosaic.last_error())
    with pytest.raises(ValueError, match="one of"):
        demosaic.method_of("ahd")


# ------------------------------------------------------------------------------------------------------------------- device
@gpu
@pytest.mark.parametrize("packing", list(LEVELS))
@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("method", METHODS)
def test_raw_matrix(method, cfa, packing):
    rng, fmt = np.random.default_rng(len(cfa + packing)), fmt_of(cfa, packing)
    for N in (1, 3):
        for H, W in sizes(packing, N):
            codes = rng.integers(0, TOP[packing] + 1, (N, H, W))          # below black and above white included
            same(f"{N} x {H} x {W}", run_raw(codes, fmt, method), DO.demosaic_raw(codes, cfa, fmt.black, fmt.white, method))


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_checkerboard_reaches_the_clamps(method):
    """{0, white} in 2 x 2 cells.  Malvar's negative lobes take S below 0 and above K; the bilinear numerators are sums of samples
    with positive weights that add up to 16, so they cannot leave [0, K] on any frame: that is what is asserted of them."""
    y, x = np.mgrid[0:34, 0:66]
    codes = (((y // 2 + x // 2) & 1) * 4095)[None]
    s, K = DO.samples_raw(codes, 0, 4095)
    num = DO.numerators(s, "rggb", method)
    assert ((num < 0).any() and (num > K).any()) if method == "malvar" else (num.min() == 0 and num.max() == K)
    same(method, run_raw(codes, S.Format(), method), DO.demosaic_raw(codes, "rggb", 0, 4095, method))


@gpu
@pytest.mark.parametrize("packing,stride", [("u16", 160), ("raw10", 97), ("raw12", 108)])
def test_padded_rows_with_a_canary(packing, stride):
    """Padding behind the wide loads (strides of 160 and 108 bytes keep them) and behind the per-sample ones (97)."""
    fmt = fmt_of("gbrg", packing)
    codes = np.random.default_rng(stride).integers(0, TOP[packing] + 1, (2, 34, 68))
    same(packing, run_raw(codes, fmt, "malvar", stride, pad=0xA5), DO.demosaic_raw(codes, "gbrg", fmt.black, fmt.white, "malvar"))


@gpu
@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("method", METHODS)
def test_spread_frames(method, cfa):
    import torch
    rng = np.random.default_rng(len(cfa + method))
    for N in (1, 3):
        for H, W in sizes("u16", N):
            sp = spread_frame(rng, cfa, (N, H, W))
            got = demosaic.run_spread(torch.from_numpy(sp).to(device()), cfa, method)
            torch.cuda.synchronize()
            same(f"{N} x {H} x {W}", got, DO.demosaic_spread(sp, cfa, method))


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_spread_nan_negative_zero_and_values_outside_0_1(method):
    import torch
    rng = np.random.default_rng(11)
    sp = spread_frame(rng, "grbg", (2, 34, 66))
    odd = rng.choice(np.array([np.nan, -0.0, 1.5, -0.25, 3e38, np.inf], F32), sp.shape)
    sp = np.where(~np.isnan(sp) & (rng.random(sp.shape) < 0.15), odd, sp)
    num = DO.numerators(DO.samples_spread(sp, "grbg")[0], "grbg", method)
    assert (num < 0).any() and (num > 16).any() and np.isnan(num).any()
    got = demosaic.run_spread(torch.from_numpy(sp).to(device()), "grbg", method)
    torch.cuda.synchronize()
    same(method, got, DO.demosaic_spread(sp, "grbg", method))


@gpu
def test_odd_addresses_in_a_canary_arena():
    """raw at an odd address with an odd stride, out at 4 mod 16: the per-sample loads and per-pixel stores; nothing beside out."""
    import torch
    fmt, (N, H, W), stride = fmt_of("bggr", "raw12"), (2, 34, 68), 105
    codes = np.random.default_rng(3).integers(0, 4096, (N, H, W))
    arena = Arena(device(), Arena.room(N * H * stride, N * 3 * H * W * 4))
    raw = arena.place((N, H, stride), torch.uint8, 1, SO.pack_rows(codes, "raw12", stride, 0x5A), "raw")
    out = arena.place((N, 3, H, W), torch.float32, 4, name="out")
    cf = fmt.c()
    assert demosaic.lib().sesrq_demosaic_raw(C.byref(cf), raw.data_ptr(), stride, demosaic.MALVAR, out.data_ptr(), N, H, W, stream_ptr()) == 0
    torch.cuda.synchronize()
    same("odd addresses", out, DO.demosaic_raw(codes, "bggr", fmt.black, fmt.white, "malvar"))
    assert arena.check() == []


@gpu
def test_zz_every_instantiation_ran():
    """After the matrices above: every (method, input, green diagonal) is named by the library's own launch counters."""
    counts = demosaic.instances()
    assert len(counts) == 16 and all(counts.values()), [n for n, c in counts.items() if not c]


@gpu
def test_public_entries():
    import torch
    import sesrq
    from sesrq import noise, quality
    from sesrq.bundle import Bundle
    e = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "raw", "nrdm_3.npz")), device())
    fmt = S.Format("grbg", 64, 1023)
    rng = np.random.default_rng(5)
    codes, gt16 = rng.integers(0, 1100, (2, 34, 66)).astype(np.uint16), rng.integers(0, 1100, (2, 3, 34, 66)).astype(np.uint16)
    x = torch.from_numpy(codes).to(device())
    q, y, base = e.forward_raw(x, fmt=fmt, baseline="malvar")
    q2, y2 = e.forward_raw(x, fmt=fmt)
    same("baseline", base, DO.demosaic_raw(codes, "grbg", 64, 1023, "malvar"))
    same("q beside a baseline", q, q2), same("y beside a baseline", y, y2)
    m = noise.NoiseModel(shot=0.01, read=0.001, seed=3)
    q, y, base = e.forward_raw(x, fmt=fmt, noise=m, baseline="bilinear")
    q2, sp = noise.apply(e, x, fmt, m, want_q=True, want_spread=True)
    torch.cuda.synchronize()
    same("noisy baseline", base, DO.demosaic_spread(sp.cpu().numpy(), "grbg", "bilinear"))
    same("q of the noisy frame", q, e.forward(q2)[0])
    net, rows = quality.evaluate_raw(e, list(codes), list(gt16), 3, fmt=fmt, baseline="malvar")
    same("the net's rows", net, quality.evaluate_raw(e, list(codes), list(gt16), 3, fmt=fmt))
    lv = SO.levels(64, 1023)
    for k in range(2):
        gt = lv[np.clip(gt16[k].astype(np.int64), 64, 1023) - 64][None]
        same(f"baseline rows, frame {k}", rows[k:k + 1], score(DO.demosaic_raw(codes[k:k + 1], "grbg", 64, 1023, "malvar"), gt, 3))
    with pytest.raises(ValueError, match="^MFLAG 1"):
        quality.evaluate_raw(e, [], [], 1, baseline="malvar")
