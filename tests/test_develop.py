"""The develop export on the device (sesrq.develop, libsesrq_develop.so, Engine.forward_develop, sim.py --develop) against the numpy
restatement of include/sesrq_develop.h (tests/develop_oracle.py; tests/test_develop_oracle.py anchors it outside itself).  Every byte
is compared with the oracle: there is no tolerance anywhere; frames are small.

  thresholds       each built-in curve and custom tables (equal neighbours, entries <= 0 and > 1; all thresholds in one bucket of the
                   search index): one frame holds T[k], its predecessor and its successor in every plane -- bytes k, k - 1, k
  search           the index-narrowed search and the plain 8-step search (SESRQ_DEVELOP_SEARCH=full) give the same bytes
  anchor           TRUNC255 + unit gains + identity == image.export on every int8 code under five domains, every 4099th fp32 bit
                   pattern and the specials
  shapes           H in {1, 2, 3} x every W from 1 to two runs + 2, N in {1, 3}, fp32 and int8, both byte orders
  extremes         frames of opposite extremes side by side, {0, 1} frames, every int8 code under overshooting domains
  int8 == fp32     the export from q with (scale, zero) equals the export from the fp32 output sesrq_forward wrote
  grid             a frame just above one trip and one just above two trips of the grid, ragged and aligned; a wrapping batch
  caller buffers   pred at element-aligned offsets, out at odd addresses, in canary arenas
  large output     one batch whose output crosses 2^32 bytes
  engine           forward_develop on the nrdm_3 raw fixture frames, with fmt= RAW10 and noise=; the refusals
  command line     sim.py --develop --save-png
  instances        LAST: every instantiation was launched by a checked case"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import Arena, device, raw_frame, same, stream_ptr

import develop_oracle as DO

pytestmark = pytest.mark.gpu

F32 = np.float32
RAW = os.path.join(GOLDEN, "raw")
SEG = 16                                      # pixels of a run (csrc/sesrq_develop.hip)
THREADS, BLOCKS_PER_CU = 256, 8
KINDS = ("gamma", "srgb", "trunc255")


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


def _profile(kind="gamma", gains=DO.GAINS, ccm=DO.CCM):
    from sesrq import develop
    return develop.Profile(gains, ccm, kind)


def _export(pred, profile, order="rgb", **kw):
    """(device bytes, oracle bytes) of one export; an int8 prediction takes DO.DOMAIN unless scale / zero are given."""
    import torch
    from sesrq import develop
    dom = dict(scale=DO.DOMAIN[0], zero=DO.DOMAIN[1]) if pred.dtype == np.int8 else {}
    dom.update(kw)
    got = develop.export(_t(pred), profile, order=order, **dom)
    torch.cuda.synchronize()
    return got.cpu().numpy(), DO.export(pred, profile.gains, profile.ccm, profile.curve, order, **dom)


def _posterised():
    """Equal neighbours (runs of five), entries <= 0 at the bottom and > 1 at the top: legal, they skip codes."""
    from sesrq import develop
    T = np.repeat(develop.curve("gamma")[::5], 5)[:255].copy()
    T[:3], T[-3:] = (-1.0, 0.0, 0.0), (1.5, 1.5, 2.0)
    return T


def _clustered():
    """All 255 thresholds an ulp apart: they share one bucket of the search index, so every count takes all eight steps."""
    return (F32(0.5).view(np.uint32) + np.arange(255, dtype=np.uint32)).view(F32)


def _tables():
    from sesrq import develop
    return [(k, develop.curve(k)) for k in KINDS] + [("posterised", _posterised()), ("clustered", _clustered())]


# ------------------------------------------------------------------------------------------------------------------- thresholds
@pytest.mark.parametrize("name", KINDS + ("posterised", "clustered"))
def test_every_threshold_with_its_neighbours(name):
    from sesrq import develop
    T = dict(_tables())[name]
    p = develop.Profile(curve=T)                                        # unit gains, the identity
    vals = np.concatenate([T, np.nextafter(T, F32(-np.inf)), np.nextafter(T, F32(np.inf))]).astype(F32)
    pred = np.stack([vals, np.roll(vals, 255), np.roll(vals, 510)]).reshape(1, 3, 15, 51)
    got, want = _export(pred, p)
    same(f"thresholds {name}", got, want)
    if name in KINDS:                                                   # strictly increasing inside (0, 1]: k, k - 1, k by construction
        k = np.arange(1, 256)
        flat = got.reshape(765, 3)
        assert np.array_equal(flat[:255, 0], k) and np.array_equal(flat[255:510, 0], k - 1) and np.array_equal(flat[510:, 0], k)
        assert np.array_equal(flat[:255, 1], k) and np.array_equal(flat[255:510, 2], k)       # plane G holds T at 255 .., B at 510 ..
    else:
        assert len(np.unique(got)) < 120 or name == "clustered"
    q = np.arange(-128, 128).astype(np.int8)
    pred8 = np.stack([q, q[::-1], np.roll(q, 77)]).reshape(1, 3, 16, 16)
    got, want = _export(pred8, p)
    same(f"thresholds {name} int8", got, want)


def test_full_search_gives_the_same_bytes():
    """A context made with SESRQ_DEVELOP_SEARCH=full (an empty index, eight steps) against the cached contexts of the same profiles."""
    import torch
    from sesrq import develop
    rng = np.random.default_rng(8)
    pred = DO.frame(rng, (2, 3, 33, 47), "f32")
    lib = develop.lib()
    for name, T in _tables():
        p = develop.Profile(DO.GAINS, DO.CCM, T)
        want = DO.export(pred, p.gains, p.ccm, p.curve)
        same(f"indexed {name}", develop.export(_t(pred), p), want)
        h = C.c_void_p()
        os.environ["SESRQ_DEVELOP_SEARCH"] = "full"
        try:
            assert lib.sesrq_develop_create(p.gains.ctypes.data, p.ccm.ctypes.data, p.curve.ctypes.data, C.byref(h)) == 0, develop.last_error()
        finally:
            del os.environ["SESRQ_DEVELOP_SEARCH"]
        d, out = _t(pred), torch.empty((2, 33, 47, 3), dtype=torch.uint8, device=device())
        assert lib.sesrq_develop_export(h, d.data_ptr(), 0, 0.0, 0, 0, out.data_ptr(), 2, 33, 47, stream_ptr()) == 0, develop.last_error()
        torch.cuda.synchronize()
        lib.sesrq_develop_destroy(h)
        same(f"full search {name}", out, want)


# ------------------------------------------------------------------------------------------------------------------- anchor
SPECIALS = np.array([0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x00000001,
                     0x80000001, 0x007fffff, 0x807fffff, 0x3f800000, 0x3f800001, 0x3f7fffff, 0xbf800000, 0x7f7fffff, 0xff7fffff],
                    np.uint32).view(F32)


def test_trunc255_identity_is_image_export():
    import torch
    from sesrq import develop, image
    p = develop.Profile(curve="trunc255")
    q = np.arange(-128, 128).astype(np.int8)
    pred8 = np.stack([q, q[::-1], np.roll(q, 101)]).reshape(1, 3, 16, 16)
    for scale, zero in (DO.DOMAIN, (0.0047, -128), (0.0047, 127), (1.0, 0), (3e38, -128)):
        d = _t(pred8)
        got = develop.export(d, p, scale=scale, zero=zero)
        ref = image.export(d, scale=scale, zero=zero)
        torch.cuda.synchronize()
        same(f"anchor int8 scale={scale} zero={zero}", got, ref)
        same(f"anchor int8 oracle scale={scale} zero={zero}", got, DO.export(pred8, T=p.curve, scale=scale, zero=zero))
    bits = np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(np.uint32)
    vals = np.concatenate([SPECIALS, np.nextafter(F32(1), F32(0))[None], np.nextafter(F32(1), F32(2))[None], bits.view(F32)])
    side = int(np.ceil(np.sqrt(len(vals) / 3)))
    pred = np.resize(vals, 3 * side * side).reshape(1, 3, side, side)
    assert pred.size >= len(vals) and np.isnan(pred).any() and np.isinf(pred).any()
    for order in ("rgb", "bgr"):
        d = _t(pred)
        got = develop.export(d, p, order=order)
        ref = image.export(d, order=order)
        torch.cuda.synchronize()
        same(f"anchor fp32 {order}", got, ref)
    with np.errstate(invalid="ignore"):
        same("anchor fp32 oracle", got, DO.export(pred, T=p.curve, order="bgr"))
    flat = develop.export(_t(pred), p).cpu().numpy().reshape(-1, 3)[:, 0]
    assert (flat[:4] == 0).all() and flat[4] == 255 and flat[5] == 0 and flat[12] == 255 and flat[13] == 255 and flat[14] == 254


# ------------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("dtype", ["f32", "i8"])
def test_every_width_across_the_run_seams(dtype):
    from sesrq import develop
    rng = np.random.default_rng(5 + len(dtype))
    widths = list(range(1, 2 * SEG + 3))
    assert widths[-1] == 34
    name = f"develop_export<{dtype}>"
    before = develop.instances()
    calls = 0
    for kind in ("gamma", "srgb"):
        p = _profile(kind)
        for N in (1, 3):
            for H in (1, 2, 3):
                for W in widths:
                    pred = DO.frame(rng, (N, 3, H, W), dtype)
                    order = ("rgb", "bgr")[(H + W + N) % 2]
                    got, want = _export(pred, p, order)
                    same(f"{kind} {dtype} N={N} {H}x{W} {order}", got, want)
                    calls += 1
    after = develop.instances()
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: calls}


# ------------------------------------------------------------------------------------------------------------------- extremes
def test_opposite_extremes_side_by_side_and_binary_frames():
    rng = np.random.default_rng(23)
    p = _profile("srgb")
    for H, W in ((3, 5), (4, 16), (1, 1)):
        for lo, hi in ((-1e30, 1e30), (0.0, 1.0), (-0.0, np.inf)):
            pred = np.empty((5, 3, H, W), F32)
            pred[0::2], pred[1::2] = lo, hi
            got, want = _export(pred, p)
            same(f"extremes {H}x{W} {lo} {hi}", got, want)
            for n in range(5):
                assert np.array_equal(got[n:n + 1], DO.export(pred[n:n + 1], p.gains, p.ccm, p.curve)), (H, W, n)
            assert (got[0] == got[0, 0, 0]).all() and (got[1] == got[1, 0, 0]).all() and (got[0] != got[1]).any()
        binary = rng.integers(0, 2, (3, 3, H, W)).astype(F32)
        got, want = _export(binary, p)
        same(f"binary {H}x{W}", got, want)
        planes = np.zeros((3, 3, H, W), F32)                             # one primary per frame: the matrix's columns, clipped
        for c in range(3):
            planes[c, c] = 1.0
        got, want = _export(planes, p, "bgr")
        same(f"primaries {H}x{W}", got, want)


def test_every_int8_code_under_overshooting_domains():
    q = np.arange(-128, 128).astype(np.int8)
    rng = np.random.default_rng(77)
    pred = np.stack([np.stack([q, q[::-1], rng.permutation(q)]), np.stack([rng.permutation(q), q, q]),
                     np.stack([q, rng.permutation(q), q[::-1]])]).reshape(3, 3, 16, 16)
    for kind in KINDS:
        p = _profile(kind)
        for scale, zero in (DO.DOMAIN, (0.0047, -128), (0.0047, 127), (0.006, -100), (0.012, 0), (1.0, 0), (3e38, -128), (1e-38, 127)):
            lo, hi = (-128 - zero) * F32(scale), (127 - zero) * F32(scale)
            got, want = _export(pred, p, scale=scale, zero=zero)
            same(f"codes {kind} scale={scale} zero={zero} [{lo}, {hi}]", got, want)
    assert (-128 - DO.DOMAIN[1]) * DO.DOMAIN[0] < 0 and (127 - DO.DOMAIN[1]) * DO.DOMAIN[0] > 1


# ------------------------------------------------------------------------------------------------------------------- int8 == fp32
def _raw_engine(net="nrdm_3", **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(os.path.join(RAW, net + ".npz")), device(), **kw)


def test_export_from_q_equals_export_from_out_f():
    import torch
    from sesrq import develop
    e = _raw_engine()
    b = e.bundle
    for f in ("a", "c"):
        raw = _t(raw_frame(f)[0])[None, None]
        q, y = e.forward_raw(raw)
        for kind in KINDS:
            p = _profile(kind)
            from_q = develop.export(q, p, scale=b.scale[b.L], zero=b.zero[b.L])
            from_f = develop.export(y, p)
            torch.cuda.synchronize()
            same(f"int8 == fp32 {f} {kind}", from_q, from_f)
            same(f"int8 == oracle {f} {kind}", from_q, DO.export(q.cpu().numpy(), p.gains, p.ccm, p.curve, scale=F32(b.scale[b.L]),
                                                                 zero=b.zero[b.L]))


# ------------------------------------------------------------------------------------------------------------------- grid
def _trip():
    import torch
    return torch.cuda.get_device_properties(device()).multi_processor_count * BLOCKS_PER_CU * THREADS * SEG       # pixels of one grid round


@pytest.mark.parametrize("dtype", ["i8", "f32"])
def test_frames_just_above_one_and_two_trips_of_the_grid(dtype):
    """One row of trip + 3 runs (aligned) and of 2 trips + 37 pixels (ragged: the per-pixel path everywhere), tiled from a pattern of
    4099 pixels and compared on the device against the tiled oracle bytes."""
    import torch
    from sesrq import develop
    P = 4099
    rng = np.random.default_rng(41)
    pat = DO.frame(rng, (1, 3, 1, P), dtype)
    p = _profile("gamma")
    dom = dict(scale=DO.DOMAIN[0], zero=DO.DOMAIN[1]) if dtype == "i8" else {}
    small = _t(DO.export(pat, p.gains, p.ccm, p.curve, **dom))           # (1, 1, P, 3)
    dpat = _t(pat)
    before = develop.instances()
    for HW in (_trip() + 3 * SEG, 2 * _trip() + 37):
        idx = torch.arange(HW, device=device()) % P
        pred = dpat[:, :, :, idx].contiguous()
        out = develop.export(pred, p, **dom)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (1, 1, HW, 3)
        assert bool((out == small[:, :, idx]).all()), f"{dtype} HW = {HW}"
        del pred, out
    after = develop.instances()
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {f"develop_export<{dtype}>": 2}


def test_wrapping_batch_equals_its_single_frame_calls():
    import torch
    from sesrq import develop
    H, W = 33, 31                                                        # 1023 pixels: 64 runs a frame, the last one partial
    runs = -(-H * W // SEG)
    N = _trip() // SEG // runs + 9
    assert N * runs > _trip() // SEG
    rng = np.random.default_rng(43)
    three = DO.frame(rng, (3, 3, H, W), "i8")
    p = _profile("srgb")
    ones = []
    for k in range(3):
        got, want = _export(three[k:k + 1], p)
        same(f"single frame {k}", got, want)
        ones.append(_t(got))
    idx = torch.arange(N, device=device()) % 3
    out = develop.export(_t(three)[idx], p, scale=DO.DOMAIN[0], zero=DO.DOMAIN[1])
    torch.cuda.synchronize()
    for k in range(3):
        assert bool((out[k::3] == ones[k]).all()), f"frames {k} mod 3 differ"


# ------------------------------------------------------------------------------------------------------------------- buffers
I8_OFFS = (0, 1, 3, 7)
F32_OFFS = (0, 4, 12)
OUT_OFFS = (0, 1, 3, 5, 15)
ROUNDS = ((0x5A, bytes([0x7F])), (0xA5, bytes([0x80])))


@pytest.mark.parametrize("dtype", ["i8", "f32"])
def test_export_in_hostile_surroundings(dtype):
    """pred at every element-aligned address class and out at odd addresses, in arenas whose every other byte is a canary (around an
    fp32 pred: NaNs): the bytes equal the oracle's, nothing beside the buffers changes.  H W = 48 gives whole 16-pixel runs (the
    16-byte path when the addresses allow: offsets 0), 5 x 7 only the per-pixel path; both are launches of the same instantiation."""
    import torch
    from sesrq import develop
    name = f"develop_export<{dtype}>"
    rng = np.random.default_rng(31 + len(dtype))
    p = _profile("gamma")
    h = develop.context(p, device())
    offs = I8_OFFS if dtype == "i8" else F32_OFFS
    seen = {"pred": set(), "out": set()}
    for H, W in ((3, 16), (5, 7)):
        N = 2
        pred = DO.frame(rng, (N, 3, H, W), dtype)
        want = DO.export(pred, p.gains, p.ccm, p.curve, scale=DO.DOMAIN[0], zero=DO.DOMAIN[1])
        places = [(0, 0)] + [(offs[i % len(offs)], OUT_OFFS[(i + 1) % 5]) for i in range(5)] + [(offs[1], 0), (0, 1)]
        for po, oo in places:
            for rnd, (canary, around) in enumerate(ROUNDS):
                what = f"{name} {H}x{W} pred@{po} out@{oo} run {rnd + 1}"
                before = develop.instances()
                ain = Arena(device(), Arena.room(pred.nbytes), around if dtype == "i8" else np.array([np.nan], F32).tobytes())
                dp = ain.place(pred.shape, torch.int8 if dtype == "i8" else torch.float32, po, fill=pred, name="pred")
                aout = Arena(device(), Arena.room(want.nbytes), canary)
                out = aout.place(want.shape, torch.uint8, oo, name="out")
                rc = develop.lib().sesrq_develop_export(h, dp.data_ptr(), 1 if dtype == "i8" else 0, DO.DOMAIN[0], DO.DOMAIN[1], 0,
                                                        out.data_ptr(), N, H, W, stream_ptr())
                assert rc == 0, (what, develop.last_error())
                torch.cuda.synchronize()
                for a in (ain, aout):
                    stray = a.check()
                    assert not stray, f"{what}: bytes outside the caller's buffers changed: {stray[:6]}"
                same(what, out, want)
                same(what + " pred untouched", dp, pred)
                after = develop.instances()
                assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}, what
                seen["pred"].add(po), seen["out"].add(oo)
    assert seen["pred"] == set(offs) and seen["out"] == set(OUT_OFFS), seen


# ------------------------------------------------------------------------------------------------------------------- large
def test_output_crossing_four_gib():
    """One int8 batch whose output crosses 2^32 bytes: the frames are copies of three distinct frames, compared on the device against
    the oracle of those three."""
    import torch
    from sesrq import develop
    H = W = 256
    per = H * W * 3
    N = (1 << 32) // per + 2
    assert N * per > 1 << 32 and (N - 1) * per > 1 << 32                 # the last frame lies wholly behind 2^32
    rng = np.random.default_rng(4096)
    p3 = DO.frame(rng, (3, 3, H, W), "i8")
    p = _profile("gamma")
    want3 = _t(DO.export(p3, p.gains, p.ccm, p.curve, scale=DO.DOMAIN[0], zero=DO.DOMAIN[1]))
    idx = torch.arange(N, device=device()) % 3
    pred = _t(p3)[idx]
    out = torch.full((N, H, W, 3), 0x5A, dtype=torch.uint8, device=device())
    got = develop.export(pred, p, scale=DO.DOMAIN[0], zero=DO.DOMAIN[1], out=out)
    torch.cuda.synchronize()
    assert got is out
    for k in range(3):
        assert bool((out[k::3] == want3[k]).all()), f"frames {k} mod 3 differ"
    same("last frame", out[N - 1], want3[(N - 1) % 3])


# ------------------------------------------------------------------------------------------------------------------- engine
def test_forward_develop_equals_the_export_of_forward_raws_output():
    import torch
    from sesrq import develop, noise, sensor
    e = _raw_engine()
    b = e.bundle
    scale, zero = b.scale[b.L], b.zero[b.L]
    side = torch.cuda.Stream(device=device())
    p = develop.from_colormatrix([[1.0234, -0.2969, -0.2266], [-0.5625, 1.6328, -0.0469], [-0.0703, 0.2188, 0.6406]], 2.1, 1.6, curve="srgb")
    r10 = sensor.Format(cfa="grbg", black=64, white=1023, packing="raw10")
    model = noise.NoiseModel(0.004, 1e-4, seed=1)
    for f in ("a", "b", "c"):
        codes = raw_frame(f)[0]
        packed = sensor.pack((np.minimum(codes, 4095) >> 2).astype(np.uint16)[:, :codes.shape[1] // 4 * 4], r10)      # 10-bit, whole groups
        for what, raw, kw in (("plain", _t(codes)[None, None], {}), ("raw10", _t(packed)[None], dict(fmt=r10)),
                              ("noise", _t(codes)[None, None], dict(noise=model))):
            q, _ = e.forward_raw(raw, want_f=False, **kw)
            for order in ("rgb", "bgr"):
                got = e.forward_develop(raw, p, order=order, **kw)
                two = develop.export(q, p, scale=scale, zero=zero, order=order)
                torch.cuda.synchronize()
                assert got.dtype == torch.uint8 and tuple(got.shape) == (1, q.shape[2], q.shape[3], 3)
                same(f"forward_develop {f} {what} {order} == export", got, two)
                same(f"forward_develop {f} {what} {order} == oracle", got,
                     DO.export(q.cpu().numpy(), p.gains, p.ccm, p.curve, order, scale=F32(scale), zero=zero))
        want = e.forward_develop(_t(codes)[None, None], p)
        x = (_t(codes.astype(np.int32)) * 1).to(torch.uint16)[None, None]      # produced on the current stream just before the call
        got_side = e.forward_develop(x, p, stream=side, slot=1)
        side.synchronize()
        same(f"forward_develop {f} side stream", got_side, want)
        out = torch.full(tuple(want.shape), 0x5A, dtype=torch.uint8, device=device())
        assert e.forward_develop(_t(codes)[None, None], p, out=out) is out
        torch.cuda.synchronize()
        same(f"forward_develop {f} caller out", out, want)
        assert len(np.unique(want.cpu().numpy())) > 50
    # the ground truth developed with the same profile: the side-by-side
    from sesrq import raw as rawmod
    gt = rawmod.load_gt(raw_frame("c")[1], device())
    same("developed ground truth", develop.export(gt, p), DO.export(gt.cpu().numpy(), p.gains, p.ccm, p.curve))


def test_forward_develop_refusals():
    import sesrq
    import torch
    from sesrq import _lib, develop
    from sesrq.bundle import Bundle
    e = _raw_engine()
    codes = raw_frame("c")[0]
    raw = _t(codes)[None, None]
    p = _profile()
    x4 = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "sesr_x4.crop.npz")), device())
    x2 = sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "sesr_x2_rand.crop.npz")), device())
    torch.cuda.synchronize()
    launches = sum(develop.instances().values()) + sum(_lib.instances().values())
    shp = (1, codes.shape[0], codes.shape[1], 3)
    for name, bad in (("short", torch.empty((1, shp[1] - 1, shp[2], 3), dtype=torch.uint8, device=device())),
                      ("planar", torch.empty((1, 3, shp[1], shp[2]), dtype=torch.uint8, device=device())),
                      ("int8", torch.empty(shp, dtype=torch.int8, device=device())),
                      ("strided", torch.empty((1, shp[1], 2 * shp[2], 3), dtype=torch.uint8, device=device())[:, :, ::2]),
                      ("host", torch.empty(shp, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="out must be a contiguous uint8 tensor of the output shape"):
            e.forward_develop(raw, p, out=bad)
    with pytest.raises(ValueError, match="order"):
        e.forward_develop(raw, p, order="rbg")
    with pytest.raises(ValueError, match="Profile"):
        e.forward_develop(raw, "gamma")
    with pytest.raises(ValueError, match="1 channel"):
        x4.forward_develop(raw, p)
    with pytest.raises(ValueError, match="PixelShuffle factor 2"):
        x2.forward_develop(raw, p)
    with pytest.raises(ValueError, match="uint16"):                      # forward_raw's own refusals stay forward_raw's
        e.forward_develop(raw.to(torch.int32), p)
    with pytest.raises(ValueError, match="one channel"):
        e.forward_develop(raw.expand(1, 2, *raw.shape[2:]).contiguous(), p)
    # the nr-shaped misuse: MFLAG 1's output is a mosaic, refused where the task is known
    with pytest.raises(ValueError, match="mosaic"):
        develop.check_mflag(1)
    with pytest.raises(ValueError, match="scale and zero"):
        develop.export(torch.zeros(shp, dtype=torch.int8, device=device()).permute(0, 3, 1, 2), p)
    with pytest.raises(ValueError, match="float32 or int8"):
        develop.export(torch.zeros((1, 3, 4, 4), dtype=torch.float16, device=device()), p)
    with pytest.raises(ValueError, match="out must be"):
        develop.export(torch.zeros((1, 3, 4, 4), device=device()), p, out=torch.empty((1, 4, 4, 4), dtype=torch.uint8, device=device()))
    torch.cuda.synchronize()
    assert sum(develop.instances().values()) + sum(_lib.instances().values()) == launches, "a refused call launched a kernel"


# ------------------------------------------------------------------------------------------------------------------- command line
def test_sim_develop_save_png(capsys, tmp_path):
    pytest.importorskip("PIL")
    import sim
    from sesrq import develop, image
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "nrdm_3_nat.params.npz")
    codes = raw_frame("c")[0]
    rawp = str(tmp_path / f"c_{codes.shape[0]}_{codes.shape[1]}.raw")
    codes.astype("<u2").tofile(rawp)
    xyz2cam = [1.0234, -0.2969, -0.2266, -0.5625, 1.6328, -0.0469, -0.0703, 0.2188, 0.6406]
    STORE.clear()
    y = sim.main(["--mflag", "3", "--params", params, "--input", rawp, "--develop", "--colormatrix"] + [str(v) for v in xyz2cam] +
                 ["--red-gain", "2.1", "--blue-gain", "1.6", "--curve", "srgb", "--save-png", str(tmp_path / "dev.png")])
    assert capsys.readouterr().out.strip().split("\n")[-1].startswith("png:")
    p = develop.from_colormatrix(xyz2cam, 2.1, 1.6, curve="srgb")
    want = DO.export(y.cpu().numpy(), p.gains, p.ccm, p.curve)[0]
    got = image.load_image(str(tmp_path / "dev.png"))
    assert got.shape == codes.shape + (3,) and np.array_equal(got, want)
    STORE.clear()
    sim.main(["--mflag", "3", "--params", params, "--input", rawp, "--develop", "--wb", "2,1,1.5", "--ccm", "1.6", "-0.4", "-0.2", "-0.3",
              "1.5", "-0.2", "0", "-0.5", "1.5", "--save-png", str(tmp_path / "dev2.png")])
    STORE.clear()
    sim.main(["--mflag", "3", "--params", params, "--input", rawp, "--save-png", str(tmp_path / "linear.png")])
    capsys.readouterr()
    p2 = develop.Profile((2, 1, 1.5), (1.6, -0.4, -0.2, -0.3, 1.5, -0.2, 0, -0.5, 1.5), "gamma")
    assert np.array_equal(image.load_image(str(tmp_path / "dev2.png")), DO.export(y.cpu().numpy(), p2.gains, p2.ccm, p2.curve)[0])
    # without the flag everything is as before: the linear camera RGB, truncated
    assert np.array_equal(image.load_image(str(tmp_path / "linear.png")), DO.export(y.cpu().numpy(), T=develop.curve("trunc255"))[0])
    assert (got != image.load_image(str(tmp_path / "linear.png"))).any()


def test_zz_every_develop_instance_ran():
    """LAST in this file: every kernel instantiation libsesrq_develop.so can launch was launched by a checked case above."""
    from sesrq import develop
    k = develop.instances()
    assert sorted(k) == ["develop_export<f32>", "develop_export<i8>"], k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
