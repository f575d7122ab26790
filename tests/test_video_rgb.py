"""YUV 4:2:0 video in and out of the RGB nets on the device (sesrq.video_rgb, libsesrq_video_rgb.so, Engine.forward_video_rgb,
quality.evaluate_video_rgb, sim.py --mflag 6 --yuv) against the numpy restatement of include/sesrq_video_rgb.h
(tests/video_rgb_oracle.py; tests/test_video_rgb_oracle.py anchors it outside itself).  Every comparison is exact and covers every
byte and fp32 word; frames are small.

  decode codes     all 256 Y codes x the chroma extremes, padded pitches and frame strides, each output set, three input domains
  decode geometry  every W from 1 to two decode tiles and two, every H likewise; both formats, N = 1 and 3; random frames, studio
                   extremes {16, 240} and {0, 255}: both clamps of the RGB byte fire
  odd sizes        H, W in {1, 3, 5}: chroma planes rounded up, the upscaled plane cropped; the export's clamped 2 x 2 blocks
  export geometry  every W and H from 1 to 2 x 16 + 3 and the seams of the grid (256 blocks a workgroup); int8 and fp32, both formats
  export values    every int8 code under three output domains; fp32 NaN, +-inf, -0.0 and the truncation steps k / 255 +- 1 ulp; the
                   194 luma and 12 chroma tie triples as constant 2 x 2 blocks
  batch            neighbouring frames of opposite extremes
  caller buffers   every plane and tensor at odd addresses in canary arenas: the same bytes, padding and surroundings intact
  large            one decoded tensor and one output surface that cross 2^32 bytes, on frames of period 7
  engine           forward_video_rgb against forward_image on the restated RGB bytes and the restated export; the anchored engine's
                   fp32 instantiations; a side stream and a second slot; a caller's out; the refusals; evaluate_video_rgb; sim.py
  instances        LAST: every one of the ten instantiations was launched by a checked case"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import Arena, device, same, stream_ptr

import colour_oracle as CO
import image_oracle as IO
import video_oracle as VO
import video_rgb_oracle as RO
from test_video import Laid, _same_frames, _t      # the hand-laid surface over canary-filled buffers

pytestmark = pytest.mark.gpu

F32 = np.float32
IMG = os.path.join(GOLDEN, "image")
FMTS = ("nv12", "i420")
OUTS = {"q0": (True, False), "x": (False, True), "q0,x": (True, True)}
DOMAINS = ((0.0032141484320163728, -146, 0), (0.0047, -119, 1), (0.0052, -120, 2))       # the golden x2 net's, and two more
DOMAIN = (0.0047, -119)                       # an int8 output domain for the cases that need no particular one
TW, TH = RO.tile()
BLOCK_W, LANES = (RO.header_defines()[k] for k in ("EXPORT_BLOCK_W", "EXPORT_LANES"))
ROUNDS = ((0x5A, bytes([0x7F])), (0xA5, bytes([0x80])))


def _delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _decode(fr, fmt, outs, dom=DOMAINS[0], pads=(0, 0), gap=0):
    """Decode on the device through the C ABI into poisoned tensors -> {"q0": tensor, "x": tensor} of what was asked for; the launch
    counter, the padding and the source are checked on the way."""
    import torch
    from sesrq import video_rgb
    N, H, W = fr["y"].shape
    want_q, want_f = OUTS[outs]
    src = Laid(fmt, N, H, W, pads=pads, gap=gap).fill(fr)
    q0 = torch.full((N, 3, H, W), 0x5A, dtype=torch.int8, device=device()) if want_q else None
    x = torch.full((N, 3, H, W), float("nan"), device=device()) if want_f else None
    h = video_rgb._so.context(device(), *dom)
    d = src.s.desc()
    before = video_rgb.instances()
    rc = video_rgb.lib().sesrq_video_rgb_decode(h, C.byref(d), q0.data_ptr() if want_q else None, x.data_ptr() if want_f else None,
                                                N, H, W, stream_ptr())
    assert rc == 0, video_rgb.last_error()
    torch.cuda.synchronize()
    assert _delta(before, video_rgb.instances()) == {f"vrgb_decode<{fmt},{outs}>": 1}
    assert src.padding_intact()
    _same_frames("src untouched", src.frames(), fr)
    return {"q0": q0, "x": x}


def _check_decode(what, fr, fmt, outs, dom=DOMAINS[0], **kw):
    got = _decode(fr, fmt, outs, dom, **kw)
    wq, wx = RO.decode(fr, *dom)
    if got["q0"] is not None:
        same(what + " q0", got["q0"], wq)
    if got["x"] is not None:
        same(what + " x", got["x"], wx)


def _export(p, fmt, pads=(0, 0), gap=0, scale=None, zero=None):
    """Export on the device -> (the frames as a dict of planes, the oracle's); launch counter and padding checked on the way."""
    import torch
    from sesrq import video_rgb
    N, _, H, W = p.shape
    i8 = p.dtype == np.int8
    dom = dict(scale=DOMAIN[0] if scale is None else scale, zero=DOMAIN[1] if zero is None else zero) if i8 else {}
    out = Laid(fmt, N, H, W, pads=pads, gap=gap)
    t = _t(p)
    before = video_rgb.instances()
    got = video_rgb.export(t, out=out.s, **dom)
    torch.cuda.synchronize()
    assert got is out.s
    assert _delta(before, video_rgb.instances()) == {f"vrgb_export<{'i8' if i8 else 'f32'},{fmt}>": 1}
    assert out.padding_intact(), f"padding bytes written ({fmt}, pads {pads}, gap {gap})"
    same("pred untouched", t, p)
    return out.frames(), RO.export(p, dom.get("scale"), dom.get("zero"))


def _pred(rng, shape, dtype):
    """A random prediction of `shape`: int8 codes, or fp32 values around and outside [0, 1]."""
    if dtype == "i8":
        return rng.integers(-128, 128, shape).astype(np.int8)
    return (rng.random(shape) * 1.3 - 0.15).astype(F32)


def _frames(rng, N, H, W, kind):
    """random: random bytes; studio: {16, 240}; extreme: {0, 255}."""
    if kind == "studio":
        fr = VO.random_frames(rng, N, H, W, "extreme")
        return {k: np.where(v == 0, 16, 240).astype(np.uint8) for k, v in fr.items()}
    return VO.random_frames(rng, N, H, W, kind)


def _clamps(fr):
    """(a channel falls below 0, a channel rises above 255) before the byte of D2."""
    _, H, W = fr["y"].shape
    v = np.stack(CO.colour_f32(fr["y"].astype(F32), RO.chroma444(fr["cb"], H, W), RO.chroma444(fr["cr"], H, W)))
    return bool((np.rint(v) < 0).any()), bool((np.rint(v) > 255).any())


# ------------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("outs", list(OUTS))
def test_decode_every_y_code_with_the_chroma_extremes(outs):
    ext = (0, 16, 128, 240, 255)
    pairs = [(a, b) for a in ext for b in ext]
    N, H, W = len(pairs), 16, 16
    y = np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(1, H, W), (N, H, W)).copy()
    cb = np.stack([np.full((8, 8), a, np.uint8) for a, _ in pairs])
    cr = np.stack([np.full((8, 8), b, np.uint8) for _, b in pairs])
    fr = {"y": y, "cb": cb, "cr": cr}
    img = RO.rgb_bytes(fr)
    assert img.min() == 0 and img.max() == 255 and len(np.unique(img)) > 200
    for i, dom in enumerate(DOMAINS):
        for j, (pads, gap) in enumerate((((0, 0), 0), ((1, 3), 7), ((13, 16), 0))):
            _check_decode(f"codes {outs} {dom} pads {pads}", fr, FMTS[(i + j) % 2], outs, dom, pads=pads, gap=gap)
    # the same codes under random chroma: the upscale's overshoot reaches the matrix
    rng = np.random.default_rng(len(outs))
    fr2 = VO.random_frames(rng, 3, H, W, "extreme")
    fr2["y"][:] = y[:3]
    for fmt in FMTS:
        _check_decode(f"codes {outs} extreme chroma {fmt}", fr2, fmt, outs, pads=(5, 1), gap=3)


def _decode_sizes():
    ws, hs = list(range(1, 2 * TW + 3)), list(range(1, 2 * TH + 3))
    return [(5, w) for w in ws] + [(h, 7) for h in hs]


@pytest.mark.parametrize("kind", ["random", "studio", "extreme"])
def test_decode_every_width_and_height_across_the_tile_seams(kind):
    sizes = _decode_sizes()
    assert {1, 2, 15, 16, 17, TW - 1, TW, TW + 1, 2 * TW, 2 * TW + 1, 2 * TW + 2} <= {w for _, w in sizes}
    assert {1, 2, 3, TH - 1, TH, TH + 1, 2 * TH, 2 * TH + 1, 2 * TH + 2} <= {h for h, _ in sizes}
    rng = np.random.default_rng(len(kind))
    low = high = False
    used = set()
    names = list(OUTS)
    for i, (H, W) in enumerate(sizes):
        N, fmt, outs, padded = (1, 3)[i % 2], FMTS[(i // 2) % 2], names[(i // 4) % 3], (i // 12) % 2 == 1
        fr = _frames(rng, N, H, W, kind)
        _check_decode(f"{kind} {N}x{H}x{W} {fmt} {outs} padded={padded}", fr, fmt, outs, pads=(3, 5) if padded else (0, 0),
                      gap=11 if padded and N > 1 else 0)
        used.add((N, fmt, outs, padded))
        lo, hi = _clamps(fr)
        low, high = low or lo, high or hi
    assert len(used) == 24
    if kind != "random":
        assert low and high, f"the {kind} frames did not reach both clamps of the RGB byte"


def test_decode_odd_sizes_round_the_chroma_planes_up_and_crop():
    rng = np.random.default_rng(7)
    i = 0
    for H in (1, 3, 5):
        for W in (1, 3, 5):
            for fmt in FMTS:
                fr = VO.random_frames(rng, 2, H, W)
                assert fr["cb"].shape == (2, (H + 1) // 2, (W + 1) // 2) and 2 * ((W + 1) // 2) > W
                _check_decode(f"odd {H}x{W} {fmt}", fr, fmt, list(OUTS)[i % 3], pads=(1, 1) if i % 2 else (0, 0))
                i += 1


def test_decode_batch_frames_do_not_leak_into_their_neighbours():
    """Frames of opposite extremes side by side: a constant chroma plane upscales to itself, so every pixel of a frame is the inverse
    matrix of that frame's own three bytes."""
    for H, W in ((3, 5), (TH + 1, TW + 1), (1, 1)):
        N = 5
        hc, wc = VO.chroma_size(H, W)
        fr = {"y": np.zeros((N, H, W), np.uint8), "cb": np.zeros((N, hc, wc), np.uint8), "cr": np.zeros((N, hc, wc), np.uint8)}
        for n in range(N):
            fr["y"][n], fr["cb"][n], fr["cr"][n] = (255, 0, 255) if n % 2 else (0, 255, 0)
        for fmt in FMTS:
            got = _decode(fr, fmt, "q0,x", gap=3)
            wq, wx = RO.decode(fr, *DOMAINS[0])
            same("batch q0", got["q0"], wq)
            same("batch x", got["x"], wx)
            x = got["x"].cpu().numpy()
            for n in range(N):
                assert all(len(np.unique(x[n, c])) == 1 for c in range(3)), (H, W, n)
                alone = RO.decode({k: v[n:n + 1] for k, v in fr.items()})[1]
                assert x[n:n + 1].tobytes() == alone.tobytes()


# ------------------------------------------------------------------------------------------------------------------- export
def _export_sizes():
    top = 2 * BLOCK_W + 3
    sizes = [(h, w) for h in (1, 2, 5) for w in range(1, top + 1)] + [(h, w) for w in (1, 7, 16) for h in range(1, top + 1)]
    # the grid's seams: N ceil(H / 2) ceil(W / 16) blocks just below, on and beyond one and two workgroups of LANES
    seams = [(1, 2 * 16, 16 * 16), (1, 2 * 16, 16 * 16 - 1), (1, 2 * 16 + 1, 16 * 16), (1, 2 * 16, 16 * 16 + 1), (3, 2 * 17 - 1, 5 * 16),
             (1, 4 * 16, 16 * 16), (2, 2 * 16, 16 * 16 + 5), (1, 2 * (LANES + 1), 16)]
    return sizes, seams


@pytest.mark.parametrize("dtype", ["i8", "f32"])
def test_export_every_width_and_height_and_the_grid_seams(dtype):
    sizes, seams = _export_sizes()
    blocks = [n * ((h + 1) // 2) * ((w + 15) // 16) for n, h, w in seams]
    assert {LANES, LANES + 1, 2 * LANES} <= set(blocks) and any(b < LANES for b in blocks) and any(b > 2 * LANES for b in blocks)
    rng = np.random.default_rng(len(dtype))
    used = set()
    for i, (N, H, W) in enumerate([((1, 3)[k % 2], h, w) for k, (h, w) in enumerate(sizes)] + seams):
        fmt, padded = FMTS[(i // 2) % 2], (i // 4) % 2 == 1
        p = _pred(rng, (N, 3, H, W), dtype)
        got, want = _export(p, fmt, pads=(5, 3) if padded else (0, 0), gap=11 if padded and N > 1 else 0)
        assert want["cb"].shape == (N, (H + 1) // 2, (W + 1) // 2)
        _same_frames(f"export {dtype} {N}x{H}x{W} {fmt} padded={padded}", got, want)
        used.add((N > 1, fmt, padded))
    assert len(used) == 8


@pytest.mark.parametrize("fmt", FMTS)
def test_export_every_int8_code_under_three_output_domains(fmt):
    import json
    meta = json.loads(str(np.load(os.path.join(IMG, "sesr_x2_rand.npz"), allow_pickle=False)["meta"]))
    s_fix, z_fix = float(np.float32(meta["scale"][-1])), int(meta["zero"][-1])
    rng = np.random.default_rng(11)
    codes = np.arange(-128, 128).astype(np.int8)
    p = np.stack([np.stack([codes, codes[::-1], rng.permutation(codes)]), np.stack([rng.permutation(codes) for _ in range(3)])])
    p = p.reshape(2, 3, 16, 16)
    for scale, zero in ((s_fix, z_fix), (s_fix, 127), (0.0047, -119), (1.0, 0), (3e38, -128)):
        got, want = _export(p, fmt, scale=scale, zero=zero)
        _same_frames(f"codes {fmt} scale={scale} zero={zero}", got, want)
    assert len(np.unique(_export(p, fmt, scale=0.0047, zero=-119)[0]["y"])) > 100


@pytest.mark.parametrize("fmt", FMTS)
def test_export_fp32_specials_and_truncation_steps(fmt):
    special = np.array([0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000000,
                        0x00000001, 0x80000001, 0x3f800000, 0x3f800001, 0x3f7fffff, 0xbf800000, 0x7f7fffff, 0xff7fffff],
                       np.uint32).view(F32)
    steps = (np.arange(256, dtype=np.float64) / 255).astype(F32)                  # on the steps, one ulp below and one above
    around = np.concatenate([steps, np.nextafter(steps, F32(-1)), np.nextafter(steps, F32(2))])
    vals = np.concatenate([special, np.array([-0.25, 1.5, 16 / 255, 235 / 255, 0.5], F32), around])
    assert len(vals) <= 32 * 32
    g = np.resize(vals, 32 * 32).astype(F32).reshape(32, 32)
    # channel G carries the values (its weight is the largest), R and B a permutation and the reverse
    p = np.stack([np.stack([g[::-1], g, g[:, ::-1]]), np.stack([g, g, g])]).copy()
    got, want = _export(p, fmt, pads=(1, 1))
    _same_frames(f"fp32 specials {fmt}", got, want)
    img = IO.export(np.nan_to_num(p, nan=0.0, posinf=np.inf, neginf=-np.inf))
    assert img[1, 0, :8, 1].tolist() == [0, 0, 0, 0, 255, 0, 0, 0]                 # NaNs as 0.0, +inf, -inf, -0.0, 0.0
    assert got["y"][1, 0, :8].tolist() == [16, 16, 16, 16, 235, 16, 16, 16]        # grey pixels: Y of (v, v, v)


@functools.lru_cache(maxsize=None)
def _tie_triples():
    """The 194 triples whose exact luma ends in 1/2, the 12 of the one-pixel Cr (Cb has none)."""
    v = np.arange(256, dtype=np.int64)
    t = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    ly = t[(RO.chroma_term(t, RO.KY) + 4207500) % 255000 == 0]
    lb = t[(2 * RO.chroma_term(t, RO.KCB) + 65535000) % 510000 == 0]
    lr = t[(2 * RO.chroma_term(t, RO.KCR) + 65535000) % 510000 == 0]
    assert (len(ly), len(lb), len(lr)) == (194, 0, 12)
    return np.concatenate([ly, lr])


@pytest.mark.parametrize("dtype", ["i8", "f32"])
def test_export_luma_and_chroma_ties_as_constant_blocks(dtype):
    t = _tie_triples()                                                              # (206, 3)
    cols = 2 * len(t)
    img = np.repeat(np.repeat(t.astype(np.uint8).reshape(1, 1, len(t), 3), 2, axis=2), 2, axis=1)      # (1, 2, 412, 3): 2 x 2 blocks
    img = np.concatenate([img, img[:, :, ::-1]], 1)                                                     # (1, 4, 412, 3)
    if dtype == "f32":
        p = ((img.astype(np.float64) + 0.5) / 255.0).astype(F32).transpose(0, 3, 1, 2).copy()
        kw = {}
    else:                                         # scale 1 / 255 with zero -128: code q is the byte q + 128 (+ 0.5 keeps the truncation off the step)
        p = (img.astype(np.int16) - 128).astype(np.int8).transpose(0, 3, 1, 2).copy()
        kw = dict(scale=float(np.float32(1.0 / 255.0 * (1 + 2.0 ** -10))), zero=-128)
    assert np.array_equal(IO.export(p if dtype == "f32" else IO.dequant(p, kw["scale"], kw["zero"])), img), "the bytes are the triples"
    assert p.shape == (1, 3, 4, cols)
    for fmt in FMTS:
        got, want = _export(p, fmt, **kw)
        _same_frames(f"ties {dtype} {fmt}", got, want)
        y = got["y"][0, 0, 0::2].astype(np.int64)
        exact2 = 2 * (RO.chroma_term(t, RO.KY) + 4080000)                                               # twice the exact luma x 255000
        assert np.array_equal(y[:194] * 510000, exact2[:194] + 255000), "a luma tie rounds half up"
        assert np.array_equal(got["cr"][0, 0].astype(np.int64)[194:] * 510000, 2 * RO.chroma_term(t[194:], RO.KCR) + 65535000)


@pytest.mark.parametrize("dtype", ["i8", "f32"])
def test_export_batch_frames_do_not_leak_into_their_neighbours(dtype):
    for H, W in ((3, 5), (4, 33), (1, 1)):
        N = 5
        lo, hi = (-128, 127) if dtype == "i8" else (-1.0, 2.0)
        p = np.zeros((N, 3, H, W), np.int8 if dtype == "i8" else F32)
        for n in range(N):
            for c in range(3):
                p[n, c] = hi if (n + c) % 2 else lo
        for fmt in FMTS:
            got, want = _export(p, fmt, gap=3)
            _same_frames(f"batch {dtype} {H}x{W} {fmt}", got, want)
            for n in range(N):
                assert all(len(np.unique(got[k][n])) == 1 for k in got), (H, W, n)


# ------------------------------------------------------------------------------------------------------------------- buffers
I8_OFFS = (0, 1, 2, 3, 7)
F32_OFFS = (0, 4, 8, 12)


def test_decode_in_hostile_surroundings():
    """Every plane of the source and both outputs at every address class, in arenas whose every other byte is a canary.  W = 32 gives
    whole 16-pixel runs (the 16-byte path when the addresses allow), W = 7 only the per-element path."""
    import torch
    from sesrq import video, video_rgb
    rng = np.random.default_rng(9)
    dom = DOMAINS[0]
    h = video_rgb._so.context(device(), *dom)
    i = 0
    for H, W in ((4, 32), (5, 7)):
        fr = VO.random_frames(rng, 2, H, W)
        wq, wx = RO.decode(fr, *dom)
        for so, qo, xo, pad in ((0, 0, 0, 0), (1, 2, 4, 1), (2, 6, 8, 16), (3, 14, 12, 5), (7, 16, 0, 0), (0, 1, 0, 0), (0, 0, 4, 0)):
            for canary, around in ROUNDS:
                fmt = FMTS[i % 2]
                i += 1
                room_in = [(2 * (rows + 1) * (nb + pad + 8) + 64) for rows, nb in video.plane_shapes(fmt, H, W)]
                ain = Arena(device(), Arena.room(*room_in), around)
                src = Laid(fmt, 2, H, W, pads=(pad, pad), gap=pad, offs=(so, (so + 3) % 8, (so + 6) % 8), arena=ain, canary=around[0]).fill(fr)
                aout = Arena(device(), Arena.room(wq.nbytes, wx.nbytes), canary)
                q0 = aout.place(wq.shape, torch.int8, qo, name="q0")
                x = aout.place(wx.shape, torch.float32, xo, name="x")
                d = src.s.desc()
                rc = video_rgb.lib().sesrq_video_rgb_decode(h, C.byref(d), q0.data_ptr(), x.data_ptr(), 2, H, W, stream_ptr())
                assert rc == 0, video_rgb.last_error()
                torch.cuda.synchronize()
                what = f"decode {fmt} {H}x{W} src@{so} q0@{qo} x@{xo} pad {pad}"
                assert not ain.check() and not aout.check(), what
                same(what + " q0", q0, wq)
                same(what + " x", x, wx)
                _same_frames(what + " src untouched", src.frames(), fr)
                assert src.padding_intact()


@pytest.mark.parametrize("dtype", ["i8", "f32"])
def test_export_in_hostile_surroundings(dtype):
    """The prediction and every plane of out at every address class, in arenas whose every other byte is a canary (a NaN around an
    fp32 prediction): the bytes equal the oracle's, nothing beside the buffers changes, no padding byte is written."""
    import torch
    from sesrq import video, video_rgb
    rng = np.random.default_rng(31 + len(dtype))
    p_offs = I8_OFFS if dtype == "i8" else F32_OFFS
    seen = {"out": set(), "p": set()}
    i = 0
    for H, W in ((4, 32), (5, 7)):
        N = 2
        p = _pred(rng, (N, 3, H, W), dtype)
        want = RO.export(p, *DOMAIN)
        places = [(0, 0, 0)] + [(I8_OFFS[(k + 2) % 5], p_offs[k % len(p_offs)], 1 + k) for k in range(5)] + [(0, p_offs[1], 0), (1, 0, 16), (8, 0, 0)]
        for oo, po, pad in places:
            for canary, around in ROUNDS:
                fmt = FMTS[i % 2]
                i += 1
                name = f"vrgb_export<{dtype},{fmt}>"
                what = f"{name} {H}x{W} out@{oo} pred@{po} pad {pad}"
                ain = Arena(device(), Arena.room(p.nbytes), around if dtype == "i8" else np.array([np.nan], F32).tobytes())
                dp = ain.place(p.shape, torch.int8 if dtype == "i8" else torch.float32, po, fill=p, name="pred")
                room_out = [(N * (rows + 1) * (nb + pad + 8) + 64) for rows, nb in video.plane_shapes(fmt, H, W)]
                aout = Arena(device(), Arena.room(*room_out), canary)
                out = Laid(fmt, N, H, W, pads=(pad, pad), gap=pad, offs=(oo, (oo + 3) % 8, (oo + 6) % 8), arena=aout, canary=canary)
                do = out.s.desc()
                before = video_rgb.instances()
                rc = video_rgb.lib().sesrq_video_rgb_export(dp.data_ptr(), video_rgb.Y_I8 if dtype == "i8" else video_rgb.Y_F32, DOMAIN[0],
                                                            DOMAIN[1], C.byref(do), N, H, W, stream_ptr())
                assert rc == 0, (what, video_rgb.last_error())
                torch.cuda.synchronize()
                for a in (ain, aout):
                    stray = a.check()
                    assert not stray, f"{what}: bytes outside the caller's buffers changed: {stray[:6]}"
                assert out.padding_intact(), f"{what}: a padding byte of out was written"
                _same_frames(what, out.frames(), want)
                same(what + " pred untouched", dp, p)
                assert _delta(before, video_rgb.instances()) == {name: 1}, what
                seen["out"].add(oo), seen["p"].add(po)
    assert set(I8_OFFS) <= seen["out"] and seen["p"] == set(p_offs), seen


# ------------------------------------------------------------------------------------------------------------------- large
PERIOD = 7


def _bundle():
    from sesrq.bundle import Bundle
    return Bundle.load(os.path.join(IMG, "sesr_x2_rand.npz"))


def _periodic_equal(t, first):
    """Every frame n of tensor t (N, ...) equals frame n % PERIOD of `first` (PERIOD, ...), compared on the device."""
    N = t.shape[0]
    whole = N // PERIOD * PERIOD
    ok = bool((t[:whole].view(N // PERIOD, PERIOD, *t.shape[1:]) == first[None]).all())
    return ok and bool((t[whole:] == first[:N - whole]).all())


def test_decoded_tensor_crossing_four_gib():
    """One batch whose fp32 frame (N, 3, H, W) crosses 2^32 bytes; frame n is frame n % 7 of seven random ones."""
    import torch
    from sesrq import video, video_rgb
    H, W = 64, 96
    per = 3 * H * W * 4
    N = (1 << 32) // per + 3
    assert (N - 1) * per > 1 << 32                 # the last frame lies wholly behind 2^32
    rng = np.random.default_rng(4097)
    fr = VO.random_frames(rng, PERIOD, H, W)
    wq, wx = RO.decode(fr, *DOMAINS[0])
    one = video.Surface.views(_t(np.frombuffer(bytearray(VO.pack(fr, "nv12")), np.uint8)), "nv12", PERIOD, H, W)
    reps = -(-N // PERIOD)
    src = video.Surface.views(one.buf.repeat(reps), "nv12", N, H, W)
    q0, x = video_rgb.decode(_bundle(), src, want_q=True, want_f=True)
    torch.cuda.synchronize()
    assert x.numel() * 4 > 1 << 32 and tuple(x.shape) == (N, 3, H, W)
    same("first period x", x[:PERIOD], wx)
    same("first period q0", q0[:PERIOD], wq)
    assert _periodic_equal(x.view(torch.int32), x[:PERIOD].view(torch.int32)), "a frame of x differs from its period"
    assert _periodic_equal(q0, q0[:PERIOD]), "a frame of q0 differs from its period"


def test_output_surface_crossing_four_gib():
    """One batch whose output surface (one buffer, frame after frame) crosses 2^32 bytes; frame n is frame n % 7."""
    import torch
    from sesrq import video, video_rgb
    H, W = 128, 192
    per = video.frame_bytes("nv12", H, W)
    N = (1 << 32) // per + 3
    assert (N - 1) * per > 1 << 32
    rng = np.random.default_rng(4098)
    p7 = _pred(rng, (PERIOD, 3, H, W), "i8")
    want = RO.export(p7, *DOMAIN)
    reps = -(-N // PERIOD)
    p = _t(p7).repeat(reps, 1, 1, 1)[:N].contiguous()
    out = video.Surface.alloc("nv12", N, H, W, device())
    assert out.buf.numel() == N * per and out.frame_y == per
    out.buf.fill_(0x5A)
    got = video_rgb.export(p, scale=DOMAIN[0], zero=DOMAIN[1], out=out)
    torch.cuda.synchronize()
    assert got is out
    first = video.Surface("nv12", H, W, out.y[:PERIOD], out.c0[:PERIOD])
    _same_frames("first period", VO.unpack(first.tobytes(), "nv12", H, W), want)
    assert _periodic_equal(out.y, out.y[:PERIOD]) and _periodic_equal(out.c0, out.c0[:PERIOD]), "a frame differs from its period"


# ------------------------------------------------------------------------------------------------------------------- engine
def _engine(net="sesr_x2_rand", **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(os.path.join(IMG, net + ".npz")), device(), **kw)


def _golden_frames():
    """Three video frames of the golden LR size: the golden LR image's channels as Y, Cb and Cr planes in turn, so that every code
    occurs in the luma, with chroma subsampled from them."""
    lr = np.load(os.path.join(IMG, "frames.npz"), allow_pickle=False)["lr_a"]          # (24, 64, 3) uint8
    H, W = lr.shape[:2]
    fr = VO.random_frames(np.random.default_rng(5), 3, H, W)
    for n in range(3):
        fr["y"][n] = lr[..., n]
        fr["cb"][n] = lr[0::2, 0::2, (n + 1) % 3] // 2 + 64
        fr["cr"][n] = lr[1::2, 1::2, (n + 2) % 3] // 2 + 64
    return fr


def test_forward_video_rgb_equals_forward_image_on_the_restated_rgb_and_the_restated_export():
    import torch
    from sesrq import video_rgb
    e = _engine()
    b = e.bundle
    scale, zero = b.scale[b.L], b.zero[b.L]
    fr = _golden_frames()
    N, H, W = fr["y"].shape
    img = RO.rgb_bytes(fr)
    assert len(np.unique(img)) > 200
    q, _ = e.forward_image(_t(img), want_q=True, want_f=False)
    torch.cuda.synchronize()
    want = RO.export(q.cpu().numpy(), np.float32(scale), zero)
    assert (want["cb"] != want["cr"]).any() and len(np.unique(want["y"])) > 30       # the un-anchored x2 output is dark, not flat
    side = torch.cuda.Stream(device=device())
    for i, (fi, fo) in enumerate([(a, c) for a in FMTS for c in FMTS]):
        src = Laid(fi, N, H, W, pads=(3, 1) if i % 2 else (0, 0)).fill(fr).s
        q0, _ = video_rgb.decode(e, src)
        same("q0", q0, RO.decode(fr, b.scale[0], b.zero[0], e.exact_div)[0])
        before = video_rgb.instances()
        got, pred = e.forward_video_rgb(src, want_q=True)
        torch.cuda.synchronize()
        assert _delta(before, video_rgb.instances()) == {f"vrgb_decode<{fi},q0>": 1, f"vrgb_export<i8,{fi}>": 1}
        assert got.fmt_name == fi and (got.N, got.H, got.W) == (N, 2 * H, 2 * W) and torch.equal(pred, q)
        _same_frames(f"forward_video_rgb {fi}", VO.unpack(got.tobytes(), fi, 2 * H, 2 * W), want)
        # into a caller's out of the other format, behind pitches; then on a side stream with a second slot
        out = Laid(fo, N, 2 * H, 2 * W, pads=(16, 2), gap=9)
        assert e.forward_video_rgb(src, out=out.s) is out.s
        torch.cuda.synchronize()
        _same_frames(f"forward_video_rgb {fi} -> caller's {fo}", out.frames(), want)
        assert out.padding_intact()
        moved = video_rgb.Surface(fi, H, W, *[(p.to(torch.int32) * 1).to(torch.uint8) for p in src.planes()])      # produced on the current stream
        got_side = e.forward_video_rgb(moved, stream=side, slot=1)
        side.synchronize()
        _same_frames(f"forward_video_rgb {fi} side stream", VO.unpack(got_side.tobytes(), fi, 2 * H, 2 * W), want)


def test_forward_video_rgb_takes_the_fp32_instantiations_on_an_anchored_engine():
    import torch
    from sesrq import video_rgb
    e = _engine(anchor_add=True)
    assert e.anchor_add
    fr = _golden_frames()
    N, H, W = fr["y"].shape
    img = RO.rgb_bytes(fr)
    _, y = e.forward_image(_t(img), want_q=False, want_f=True)
    torch.cuda.synchronize()
    want = RO.export(y.cpu().numpy())
    plain = _engine().forward_video_rgb(Laid("nv12", N, H, W).fill(fr).s)
    torch.cuda.synchronize()
    for fi, fo in (("nv12", "i420"), ("i420", "nv12")):
        src = Laid(fi, N, H, W, pads=(1, 1)).fill(fr).s
        out = Laid(fo, N, 2 * H, 2 * W, pads=(3, 5), gap=2)
        before = video_rgb.instances()
        got, pred = e.forward_video_rgb(src, out=out.s, want_q=True)
        torch.cuda.synchronize()
        assert _delta(before, video_rgb.instances()) == {f"vrgb_decode<{fi},x>": 1, f"vrgb_export<f32,{fo}>": 1}
        assert got is out.s and pred.dtype == torch.float32 and torch.equal(pred, y)
        _same_frames(f"forward_video_rgb anchored {fi} -> {fo}", out.frames(), want)
        assert out.padding_intact()
    assert VO.pack(want, "nv12") != plain.tobytes(), "the anchored output is the plain one: the case would not tell the branches apart"


def test_forward_video_rgb_refusals():
    import torch
    import sesrq
    from sesrq import _lib, video_rgb
    from sesrq.bundle import Bundle
    fr = _golden_frames()
    N, H, W = fr["y"].shape
    src = Laid("nv12", N, H, W).fill(fr).s
    e = _engine()
    e5 = _engine("sesr_x4")
    chained = sesrq.Engine(Bundle.load(os.path.join(IMG, "sesr_x2_rand.npz")), device(),
                           upstream=Bundle.load(os.path.join(GOLDEN, "raw", "nrdm_3.npz")))
    torch.cuda.synchronize()
    launches = sum(video_rgb.instances().values()) + sum(_lib.instances().values())
    for bad in (Laid("nv12", N, 2 * H - 1, 2 * W).s, Laid("nv12", N + 1, 2 * H, 2 * W).s, video_rgb.Surface.alloc("nv12", N, 2 * H, 2 * W),
                torch.empty((N, 2 * H, 2 * W), dtype=torch.uint8, device=device())):
        with pytest.raises(ValueError, match="out must be a Surface"):
            e.forward_video_rgb(src, out=bad)
    with pytest.raises(ValueError, match="Surface"):
        e.forward_video_rgb(src.y)
    with pytest.raises(ValueError, match="HIP device"):
        e.forward_video_rgb(src.cpu())
    with pytest.raises(ValueError, match="upstream"):
        chained.forward_video_rgb(src)
    with pytest.raises(ValueError, match="RGB net"):
        e5.forward_video_rgb(src)
    with pytest.raises(ValueError, match="3 channels in"):
        video_rgb.decode(e5, src)
    p = torch.zeros((N, 3, 2 * H, 2 * W), device=device())
    with pytest.raises(ValueError, match=r"\(N, 3, H, W\)"):
        video_rgb.export(p[:, :1])
    with pytest.raises(ValueError, match="scale and zero"):
        video_rgb.export(p.to(torch.int8))
    with pytest.raises(ValueError, match="float32 or int8"):
        video_rgb.export(p.to(torch.float16))
    with pytest.raises(ValueError, match="out must be a Surface"):
        video_rgb.export(p, fmt="i420", out=Laid("nv12", N, 2 * H, 2 * W).s)
    with pytest.raises(ValueError, match="out must be a Surface"):
        video_rgb.export(p, out=Laid("nv12", N, 2 * H, 2 * W + 1).s)
    with pytest.raises(ValueError, match="pixel format"):
        video_rgb.export(p, fmt="yuyv")
    torch.cuda.synchronize()
    assert sum(video_rgb.instances().values()) + sum(_lib.instances().values()) == launches, "a refused call launched a kernel"


def test_evaluate_video_rgb_equals_score_on_the_frames_made_by_hand():
    import torch
    from sesrq import quality, video_rgb
    e = _engine(anchor_add=True)
    rng = np.random.default_rng(21)
    fr = _golden_frames()
    N, H, W = fr["y"].shape
    hr = VO.random_frames(rng, N, 2 * H, 2 * W)
    lrs = [video_rgb.Surface.views(np.frombuffer(bytearray(VO.pack({k: v[n:n + 1] for k, v in fr.items()}, "nv12")), np.uint8), "nv12", 1, H, W)
           for n in range(N)]
    hrs = [video_rgb.Surface.views(np.frombuffer(bytearray(VO.pack({k: v[n:n + 1] for k, v in hr.items()}, "i420")), np.uint8), "i420", 1,
                                   2 * H, 2 * W) for n in range(N)]
    got = quality.evaluate_video_rgb(e, lrs, hrs)
    x, gt = RO.decode(fr)[1], RO.decode(hr)[1]
    rows = []
    for n in range(N):
        _, y = e.forward(_t(x[n:n + 1]), want_q=False, want_f=True)
        rows.append(quality.score(y, _t(gt[n:n + 1]), 6))
    torch.cuda.synchronize()
    want = torch.cat(rows).cpu().numpy()
    assert got.shape == (N, 3) and got.dtype == np.float64 and np.array_equal(got, want)
    with pytest.raises(ValueError, match="MFLAG 5"):
        quality.evaluate_video_rgb(e, lrs, hrs, mflag=5)
    with pytest.raises(ValueError, match="anchor_add"):
        quality.evaluate_video_rgb(_engine(), lrs, hrs)


def test_sim_mflag6_yuv_save_yuv(capsys, tmp_path):
    import sim
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "sesr_x2_rand_nat.params.npz")
    rng = np.random.default_rng(33)
    H, W = 9, 13
    fr = VO.random_frames(rng, 2, H, W)
    hr = VO.random_frames(rng, 2, 2 * H, 2 * W)
    with open(tmp_path / "lr.yuv", "wb") as f:
        f.write(VO.pack(fr, "nv12"))
    with open(tmp_path / "hr.yuv", "wb") as f:
        f.write(VO.pack(hr, "nv12"))
    STORE.clear()
    y = sim.main(["--mflag", "6", "--params", params, "--yuv", str(tmp_path / "lr.yuv"), "--size", f"{W}x{H}", "--pix-fmt", "nv12",
                  "--save-yuv", str(tmp_path / "sr.yuv"), "--out-pix-fmt", "i420", "--gt-yuv", str(tmp_path / "hr.yuv")])
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[-1].startswith("yuv:") and "srx2 mean psnr is" in lines[-2] and float(lines[-3]) > 0 and float(lines[-4]) > 0
    assert tuple(y.shape) == (2, 3, 2 * H, 2 * W)
    x = RO.decode(fr)[1]
    want = RO.export((y.cpu().numpy() + IO.upsample2(x)).astype(F32))
    assert open(tmp_path / "sr.yuv", "rb").read() == VO.pack(want, "i420"), "the written file differs from the oracle's bytes"
    STORE.clear()
    sim.main(["--mflag", "6", "--params", params, "--yuv", str(tmp_path / "lr.yuv"), "--size", f"{W}x{H}", "--pix-fmt", "nv12",
              "--frames", "1:2", "--save-yuv", str(tmp_path / "one.yuv")])
    capsys.readouterr()
    assert open(tmp_path / "one.yuv", "rb").read() == VO.pack({k: v[1:] for k, v in want.items()}, "nv12")
    STORE.clear()
    with pytest.raises(SystemExit, match="--yuv"):
        sim.main(["--mflag", "3", "--params", params, "--yuv", str(tmp_path / "lr.yuv"), "--size", f"{W}x{H}", "--pix-fmt", "nv12"])


def test_zz_every_video_rgb_instance_ran():
    """LAST in this file: every kernel instantiation libsesrq_video_rgb.so can launch was launched by a checked case above, by name."""
    from sesrq import video_rgb
    k = video_rgb.instances()
    names = [f"vrgb_decode<{f},{o}>" for f in FMTS for o in OUTS] + [f"vrgb_export<{d},{f}>" for d in ("f32", "i8") for f in FMTS]
    assert len(names) == 10 and sorted(k) == sorted(names), k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
