"""YUV 4:2:0 video on the device (sesrq.video, libsesrq_video.so, Engine.forward_video, quality.evaluate_video, sim.py --yuv) against
the numpy restatement of include/sesrq_video.h (tests/video_oracle.py; tests/test_video_oracle.py anchors it outside itself).  Every
comparison is exact and covers every byte; frames are small.

  decode           all 256 codes in frames of 1 x 1, 1 x 17, 3 x 5 and 33 x 31; pitches W, W + 1, W + 13; N = 1 and 3 with a frame stride
                   beyond the frame; q0, x, both; three input domains
  geometry         every LR W from 1 to two tiles and two at H = 5, every H likewise at W = 7; r = 2 and 4, int8 and fp32 Y, N = 1
                   and 3, the four format pairs cycled, output pitches exact and padded; random chroma and chroma drawn from
                   {0, 255} (both clamps of the chroma byte, negative sums of the horizontal pass)
  odd sizes        H, W in {1, 3, 5}: the rounded-up chroma planes and the crop of the upscaled plane
  batch            neighbouring frames of opposite extremes: nothing of a frame reaches its neighbour
  luma extremes    every int8 code under three output domains; fp32 specials and values on the truncation steps k / 255
  caller buffers   every plane and the luma at odd addresses in canary-filled arenas: the same bytes, no canary touched, no padding
                   byte of a row or between frames written, inputs unchanged
  sibling          the exported Y plane equals sesrq.image.export at C = 1 of the same luma
  large output     one batch whose output surface crosses 2^32 bytes
  sweeps           (tests/test_resampler_sweep_device.py) both edges of every reachable Q6 value of each pass at every phase
  loop, strips     (tests/test_resampler_limits.py) the decode's loop into its third trip; one LR row and one LR column, one and two
                   wide, of 2^22 + 5 pixels through the export, r = 2 and 4
  forward_video    on the golden LR frames, a side stream, a caller's out, the fp32 branch on an anchored engine, the refusals;
                   evaluate_video; sim.py --yuv --save-yuv
  instances        LAST: every instantiation was launched by a checked case"""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import Arena, device, same, stream_ptr

import video_oracle as VO

pytestmark = pytest.mark.gpu

F32 = np.float32
IMG = os.path.join(GOLDEN, "image")
DOMAIN = (0.0047, -119)                       # an int8 output domain for the cases that need no particular one
FMTS = ("nv12", "i420")
PAIRS = [(a, b) for a in FMTS for b in FMTS]  # (lr format, out format)
CANARY = 0x5A


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


def _luma(rng, shape, dtype):
    """A random luma of `shape`: int8 codes, or fp32 values around and outside [0, 1]."""
    if dtype == "i8":
        return rng.integers(-128, 128, shape).astype(np.int8)
    return (rng.random(shape) * 1.3 - 0.15).astype(F32)


class Laid:
    """A device Surface laid out by hand over canary-filled buffers: each plane in a buffer of its own (an Arena placement, or a plain
    tensor), rows `pads` bytes apart beyond their own bytes, frames `gap` bytes apart beyond their extent."""

    def __init__(self, fmt, N, H, W, pads=(0, 0), gap=0, offs=(0, 0, 0), arena=None, canary=CANARY):
        import torch
        from sesrq import video
        self.canary, self.flat, planes = canary, [], []
        for k, (rows, nbytes) in enumerate(video.plane_shapes(fmt, H, W)):
            pitch = nbytes + pads[min(k, 1)]
            frame = rows * pitch + gap
            n = (N - 1) * frame + (rows - 1) * pitch + nbytes
            if arena is None:
                flat = torch.full((n,), canary, dtype=torch.uint8, device=device())
            else:
                flat = arena.place((n,), torch.uint8, offs[k], name=f"{fmt}{k}")
            self.flat.append(flat)
            planes.append(flat.as_strided((N, rows, nbytes), (frame, pitch, 1), flat.storage_offset()))
        self.s = video.Surface(fmt, H, W, *planes)

    def fill(self, fr):
        """Copy the dict of planes in."""
        if self.s.fmt_name == "nv12":
            self.s.y.copy_(_t(fr["y"]))
            self.s.c0.copy_(_t(np.stack([fr["cb"], fr["cr"]], -1).reshape(self.s.c0.shape)))
        else:
            for p, k in zip(self.s.planes(), ("y", "cb", "cr")):
                p.copy_(_t(fr[k]))
        return self

    def frames(self):
        """The dict of planes, from the device."""
        s = self.s
        if s.fmt_name == "nv12":
            c = s.c0.cpu().numpy()
            return {"y": s.y.cpu().numpy(), "cb": np.ascontiguousarray(c[..., 0::2]), "cr": np.ascontiguousarray(c[..., 1::2])}
        return {k: p.cpu().numpy() for p, k in zip(s.planes(), ("y", "cb", "cr"))}

    def padding_intact(self):
        """No byte between a row's end and the pitch, or between frames, differs from the canary."""
        for flat, p in zip(self.flat, self.s.planes()):
            c = flat.clone()
            c.as_strided(tuple(p.shape), tuple(p.stride()), 0).fill_(self.canary)
            if not bool((c == self.canary).all()):
                return False
        return True


def _same_frames(what, got, want):
    for k in ("y", "cb", "cr"):
        same(f"{what} {k}", got[k], want[k])


def _export(y, lr_fr, r, pair=("nv12", "nv12"), pads=(0, 0), gap=0, **kw):
    """Export on the device -> (the HR frames as a dict of planes, the oracle's); padding bytes checked on the way."""
    import torch
    from sesrq import video
    N, H, W = lr_fr["y"].shape
    dom = dict(scale=DOMAIN[0], zero=DOMAIN[1]) if y.dtype == np.int8 else {}
    dom.update(kw)
    lr = Laid(pair[0], N, H, W, pads=(1, 3) if pads != (0, 0) else (0, 0), gap=5 if gap else 0).fill(lr_fr)
    out = Laid(pair[1], N, r * H, r * W, pads=pads, gap=gap)
    got = video.export(_t(y), lr.s, r, out=out.s, **dom)
    torch.cuda.synchronize()
    assert got is out.s
    assert out.padding_intact() and lr.padding_intact(), f"padding bytes written ({pair}, pads {pads}, gap {gap})"
    _same_frames("lr untouched", lr.frames(), lr_fr)
    return out.frames(), VO.export(y, lr_fr, r, scale=dom.get("scale"), zero=dom.get("zero"))


# ------------------------------------------------------------------------------------------------------------------- decode
def _domains():
    out = []
    for name in ("sesr_x4.crop.npz", os.path.join("image", "sesr_x4.npz")):
        meta = json.loads(str(np.load(os.path.join(GOLDEN, name), allow_pickle=False)["meta"]))
        out.append((meta["scale"][0], meta["zero"][0], len(out)))
    return out + [(0.0052, -120, 2)]


@pytest.mark.parametrize("outs", ["q0", "x", "q0,x"])
def test_decode_every_code_through_pitches_and_frame_strides(outs):
    import torch
    from sesrq import video
    want_q, want_f = "q0" in outs, "x" in outs
    rng = np.random.default_rng(len(outs))
    name = f"video_decode<{outs}>"
    for s0, z0, ed in _domains():
        h = video._so.context(device(), s0, z0, ed)
        for H, W in ((1, 1), (1, 17), (3, 5), (33, 31), (2, 32)):
            for N in (1, 3):
                for pad in (0, 1, 13):
                    y = rng.integers(0, 256, (N, H, W)).astype(np.uint8)
                    y.reshape(-1)[:256] = np.resize(np.arange(256, dtype=np.uint8), min(256, y.size))      # every code where it fits
                    fmt = FMTS[(H + W + N + pad) % 2]
                    hc, wc = VO.chroma_size(H, W)
                    src = Laid(fmt, N, H, W, pads=(pad, pad), gap=7 if N > 1 else 0).fill(
                        {"y": y, "cb": np.zeros((N, hc, wc), np.uint8), "cr": np.zeros((N, hc, wc), np.uint8)})
                    d = src.s.desc()
                    d.c0 = d.c1 = None                                             # chroma is not looked at
                    q0 = torch.full((N, 1, H, W), 0x5A, dtype=torch.int8, device=device()) if want_q else None
                    x = torch.full((N, 1, H, W), float("nan"), device=device()) if want_f else None
                    before = video.instances()
                    import ctypes as C
                    rc = video.lib().sesrq_video_decode(h, C.byref(d), q0.data_ptr() if want_q else None, x.data_ptr() if want_f else None,
                                                        N, H, W, stream_ptr())
                    assert rc == 0, video.last_error()
                    torch.cuda.synchronize()
                    after = video.instances()
                    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}
                    wq, wx = VO.decode(y, s0, z0, ed)
                    what = f"decode {outs} {N}x{H}x{W} pad {pad} domain {(s0, z0, ed)}"
                    if want_q:
                        same(what + " q0", q0, wq)
                    if want_f:
                        same(what + " x", x, wx)
                    same(what + " src untouched", src.s.y, y)
                    assert src.padding_intact()
    # through the python entry, with an Engine-less domain: a Bundle is not needed for x alone
    fr = VO.random_frames(rng, 2, 5, 9)
    s = Laid("i420", 2, 5, 9, pads=(3, 1)).fill(fr).s
    if want_f and not want_q:
        _, xf = video.decode(None, s, want_q=False, want_f=True)
        same("decode(None)", xf, VO.decode(fr["y"])[1])


# ------------------------------------------------------------------------------------------------------------------- geometry
def _sizes(r):
    """Every W from 1 to two tiles and two at H = 5, every H likewise at W = 7, in the LR tile of factor r."""
    tw, th = VO.tile(r)
    ws, hs = list(range(1, 2 * tw + 3)), list(range(1, 2 * th + 3))
    assert (tw * r, th * r) == VO.header_tile() and ws[0] == hs[0] == 1
    return [(5, w) for w in ws] + [(h, 7) for h in hs]


@pytest.mark.parametrize("dtype", ["i8", "f32"])
@pytest.mark.parametrize("r", [2, 4])
def test_geometry_every_width_and_height_across_the_tile_seams(r, dtype):
    tw, th = VO.tile(r)
    sizes = _sizes(r)
    assert {1, 2, 3, tw - 1, tw, tw + 1, 2 * tw, 2 * tw + 1} <= {w for _, w in sizes}
    assert {1, 2, 3, th - 1, th, th + 1, 2 * th, 2 * th + 1} <= {h for h, _ in sizes}
    assert any((r * w) % 32 for _, w in sizes) and any((r * w) % 32 == 0 for _, w in sizes)      # both store paths, of luma and chroma
    rng = np.random.default_rng(100 * r + len(dtype))
    seen = {"low": False, "high": False, "negative": False}      # what the {0, 255} planes must reach
    used, i = set(), 0
    for N in (1, 3):
        for kind in ("random", "extreme"):
            for H, W in sizes:
                lr = VO.random_frames(rng, N, H, W, kind)
                y = _luma(rng, (N, 1, r * H, r * W), dtype)
                pair, padded = PAIRS[i % 4], (i // 4) % 2 == 1
                i += 1
                got, want = _export(y, lr, r, pair, pads=(5, 3) if padded else (0, 0), gap=11 if padded and N > 1 else 0)
                _same_frames(f"r={r} {dtype} N={N} {kind} {H}x{W} {pair} padded={padded}", got, want)
                used.add((pair, padded))
                if kind == "extreme":
                    for k in ("cb", "cr"):
                        v, h = VO.chroma_q6(lr[k], r, keep=True)
                        v = v[..., :r * H // 2, :r * W // 2]
                        seen["low"] |= bool(((v + 32) >> 6 < 0).any())
                        seen["high"] |= bool(((v + 32) >> 6 > 255).any())
                        seen["negative"] |= bool((h < 0).any())
    assert used == {(p, b) for p in PAIRS for b in (False, True)}
    assert all(seen.values()), f"the {{0, 255}} planes did not reach: {[k for k, v in seen.items() if not v]}"


@pytest.mark.parametrize("r", [2, 4])
def test_odd_sizes_round_the_chroma_planes_up_and_crop_the_upscaled_plane(r):
    rng = np.random.default_rng(r + 7)
    i = 0
    for H in (1, 3, 5):
        for W in (1, 3, 5):
            for dtype in ("i8", "f32"):
                lr = VO.random_frames(rng, 2, H, W)
                assert lr["cb"].shape == (2, (H + 1) // 2, (W + 1) // 2)
                y = _luma(rng, (2, 1, r * H, r * W), dtype)
                got, want = _export(y, lr, r, PAIRS[i % 4], pads=(1, 1) if i % 3 == 0 else (0, 0))
                i += 1
                assert want["cb"].shape == (2, r * H // 2, r * W // 2) and r * ((W + 1) // 2) > r * W // 2
                _same_frames(f"odd r={r} {H}x{W} {dtype}", got, want)


def test_batch_frames_do_not_leak_into_their_neighbours():
    """Frames of opposite extremes side by side (all 0 and all 255, luma and chroma alike): a constant plane upscales to itself, so
    each output frame must equal the export of that frame alone and its chroma must be its own constant."""
    rng = np.random.default_rng(17)
    i = 0
    for r in (2, 4):
        tw, th = VO.tile(r)
        for H, W in ((3, 5), (th + 1, tw + 1), (1, 1)):
            N = 5
            hc, wc = VO.chroma_size(H, W)
            lr = {"y": np.zeros((N, H, W), np.uint8), "cb": np.zeros((N, hc, wc), np.uint8), "cr": np.zeros((N, hc, wc), np.uint8)}
            for n in range(N):
                lr["cb"][n], lr["cr"][n] = (0, 255) if n % 2 else (255, 0)
            y = _luma(rng, (N, 1, r * H, r * W), "i8")
            got, want = _export(y, lr, r, PAIRS[i % 4], pads=(0, 0), gap=3)
            i += 1
            _same_frames(f"batch r={r} {H}x{W}", got, want)
            for n in range(N):
                assert (got["cb"][n] == lr["cb"][n, 0, 0]).all() and (got["cr"][n] == lr["cr"][n, 0, 0]).all(), (r, H, W, n)
                alone = VO.export(y[n:n + 1], {k: v[n:n + 1] for k, v in lr.items()}, r, scale=DOMAIN[0], zero=DOMAIN[1])
                assert all(np.array_equal(got[k][n:n + 1], alone[k]) for k in alone)


# ------------------------------------------------------------------------------------------------------------------- luma
def _fixture_domain():
    meta = json.loads(str(np.load(os.path.join(IMG, "sesr_x4.npz"), allow_pickle=False)["meta"]))
    L = len(meta["scale"]) - 1
    return float(np.float32(meta["scale"][L])), int(meta["zero"][L])


@pytest.mark.parametrize("r", [2, 4])
def test_every_int8_code_under_three_output_domains(r):
    s_fix, z_fix = _fixture_domain()
    rng = np.random.default_rng(r)
    H = W = 16 // r
    lr = VO.random_frames(rng, 3, H, W)
    codes = np.arange(-128, 128).astype(np.int8)
    y = np.stack([codes, codes[::-1], rng.permutation(codes)]).reshape(3, 1, 16, 16)
    for i, (scale, zero) in enumerate(((s_fix, z_fix), (s_fix, -128), (s_fix, 127), (1.0, 0), (3e38, -128))):
        got, want = _export(y, lr, r, PAIRS[i % 4], scale=scale, zero=zero)
        _same_frames(f"codes r={r} scale={scale} zero={zero}", got, want)
    assert len(np.unique(_export(y, lr, r, scale=s_fix, zero=z_fix)[0]["y"])) > 100


@pytest.mark.parametrize("r", [2, 4])
def test_fp32_luma_specials_and_truncation_steps(r):
    special = np.array([0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000000,
                        0x00000001, 0x80000001, 0x3f800000, 0x3f800001, 0x3f7fffff, 0xbf800000, 0x7f7fffff, 0xff7fffff],
                       np.uint32).view(F32)
    steps = (np.arange(256, dtype=np.float64) / 255).astype(F32)                  # on the steps, one ulp below and one above
    around = np.concatenate([steps, np.nextafter(steps, F32(-1)), np.nextafter(steps, F32(2))])
    vals = np.concatenate([special, np.array([-0.25, 1.5, 16 / 255, 235 / 255, 0.5], F32), around])
    n = 32 * 32
    assert len(vals) <= n
    y = np.resize(vals, n).astype(F32).reshape(1, 1, 32, 32)
    y = np.concatenate([y, y[:, :, ::-1, ::-1]]).copy()
    lr = VO.random_frames(np.random.default_rng(r + 40), 2, 32 // r, 32 // r)
    for pair in (PAIRS[0], PAIRS[3]):
        got, want = _export(y, lr, r, pair)
        _same_frames(f"fp32 specials r={r}", got, want)
    flat = got["y"][0].reshape(-1)
    assert flat[:8].tolist() == [0, 0, 0, 0, 255, 0, 0, 0]                         # NaNs as 0.0, +inf, -inf, -0.0, 0.0
    byte = flat[len(special) + 5:len(special) + 5 + 3 * 256].reshape(3, 256).astype(int)
    assert np.abs(byte[0] - np.arange(256)).max() <= 1 and (byte[1] <= byte[0]).all() and (byte[0] <= byte[2]).all()
    assert (byte[1] < byte[2]).any()                                               # the steps do separate neighbours


# ------------------------------------------------------------------------------------------------------------------- buffers
I8_OFFS = (0, 1, 2, 3, 7)
F32_OFFS = (0, 4, 8, 12)
ROUNDS = ((0x5A, bytes([0x7F])), (0xA5, bytes([0x80])))


@pytest.mark.parametrize("dtype", ["i8", "f32"])
@pytest.mark.parametrize("r", [2, 4])
def test_export_in_hostile_surroundings(r, dtype):
    """Every plane of lr and out and the luma at every address class, in arenas whose every other byte is a canary: the bytes equal the
    oracle's, nothing beside the buffers changes, no padding byte of a row or between frames is written.  W = 8 gives whole 16-byte
    runs (the 16-byte path when the addresses allow: offset 0, pitches that keep rows aligned), W = 7 only the per-element path."""
    import ctypes as C
    import torch
    from sesrq import video
    rng = np.random.default_rng(31 * r + len(dtype))
    y_offs = I8_OFFS if dtype == "i8" else F32_OFFS
    seen = {"lr": set(), "out": set(), "y": set()}
    i = 0
    for H, W in ((3, 8), (5, 7)):
        N = 2
        lr_fr = VO.random_frames(rng, N, H, W)
        y = _luma(rng, (N, 1, r * H, r * W), dtype)
        want = VO.export(y, lr_fr, r, scale=DOMAIN[0], zero=DOMAIN[1])
        places = [(0, 0, 0, 0)] + [(I8_OFFS[(k + 1) % 5], I8_OFFS[(k + 2) % 5], y_offs[k % len(y_offs)], 1 + k) for k in range(5)] + \
                 [(0, 0, y_offs[1], 0), (0, 1, 0, 16), (1, 0, 0, 0)]
        for lo, oo, yo, pad in places:
            for rnd, (canary, around) in enumerate(ROUNDS):
                pair = PAIRS[i % 4]
                i += 1
                name = f"video_export<{dtype},r{r},{pair[1]}>"
                what = f"{name} {H}x{W} lr({pair[0]})@{lo} out@{oo} y@{yo} pad {pad} run {rnd + 1}"
                before = video.instances()
                room_in = [(N * (rows + 1) * (nb + 8) + 64) for rows, nb in video.plane_shapes(pair[0], H, W)]
                ain = Arena(device(), Arena.room(y.nbytes, *room_in), around if dtype == "i8" else np.array([np.nan], F32).tobytes())
                lr = Laid(pair[0], N, H, W, pads=(2, 1), gap=3, offs=(lo, (lo + 1) % 8, (lo + 5) % 8), arena=ain).fill(lr_fr)
                dy = ain.place(y.shape, torch.int8 if dtype == "i8" else torch.float32, yo, fill=y, name="y")
                room_out = [(N * (rows + 1) * (nb + pad + 8) + 64) for rows, nb in video.plane_shapes(pair[1], r * H, r * W)]
                aout = Arena(device(), Arena.room(*room_out), canary)
                out = Laid(pair[1], N, r * H, r * W, pads=(pad, pad), gap=pad, offs=(oo, (oo + 3) % 8, (oo + 6) % 8), arena=aout,
                           canary=canary)
                dl, do = lr.s.desc(), out.s.desc()
                dl.y = None                                                        # the LR luma is not looked at
                rc = video.lib().sesrq_video_export(dy.data_ptr(), video.Y_I8 if dtype == "i8" else video.Y_F32, DOMAIN[0], DOMAIN[1],
                                                    C.byref(dl), r, C.byref(do), N, H, W, stream_ptr())
                assert rc == 0, (what, video.last_error())
                torch.cuda.synchronize()
                for a in (ain, aout):
                    stray = a.check()
                    assert not stray, f"{what}: bytes outside the caller's buffers changed: {stray[:6]}"
                assert out.padding_intact(), f"{what}: a padding byte of out was written"
                _same_frames(what, out.frames(), want)
                _same_frames(what + " lr untouched", lr.frames(), lr_fr)
                same(what + " y untouched", dy, y)
                after = video.instances()
                assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}, what
                seen["lr"].add(lo), seen["out"].add(oo), seen["y"].add(yo)
    assert seen["lr"] == seen["out"] == set(I8_OFFS) and seen["y"] == set(y_offs), seen


def test_decode_in_hostile_surroundings():
    import ctypes as C
    import torch
    from sesrq import video
    rng = np.random.default_rng(9)
    s0, z0, ed = _domains()[0]
    h = video._so.context(device(), s0, z0, ed)
    for H, W in ((3, 32), (5, 7)):
        fr = VO.random_frames(rng, 2, H, W)
        wq, wx = VO.decode(fr["y"], s0, z0, ed)
        for so, qo, xo, pad in ((0, 0, 0, 0), (1, 2, 4, 1), (2, 6, 8, 16), (3, 14, 12, 5), (7, 10, 0, 0)):
            for canary, around in ROUNDS:
                room_in = [(2 * (rows + 1) * (nb + pad + 8) + 64) for rows, nb in video.plane_shapes("nv12", H, W)]
                ain = Arena(device(), Arena.room(*room_in), around)
                src = Laid("nv12", 2, H, W, pads=(pad, 0), gap=pad, offs=(so, 0, 0), arena=ain, canary=around[0]).fill(fr)
                aout = Arena(device(), Arena.room(wq.nbytes, wx.nbytes), canary)
                q0 = aout.place(wq.shape, torch.int8, qo, name="q0")
                x = aout.place(wx.shape, torch.float32, xo, name="x")
                d = src.s.desc()
                assert video.lib().sesrq_video_decode(h, C.byref(d), q0.data_ptr(), x.data_ptr(), 2, H, W, stream_ptr()) == 0, video.last_error()
                torch.cuda.synchronize()
                assert not ain.check() and not aout.check(), (so, qo, xo, pad)
                same(f"decode src@{so} q0@{qo}", q0, wq)
                same(f"decode src@{so} x@{xo}", x, wx)
                _same_frames("decode src untouched", src.frames(), fr)
                assert src.padding_intact()


@pytest.mark.parametrize("dtype", ["i8", "f32"])
def test_exported_luma_equals_the_image_librarys_grey_export(dtype):
    """The sibling library on the same luma, on the device: the Y plane of an exported frame is the grey export byte for byte."""
    import torch
    from sesrq import image, video
    rng = np.random.default_rng(77)
    r, N, H, W = 4, 2, 9, 37
    y = _t(_luma(rng, (N, 1, r * H, r * W), dtype))
    lr = Laid("nv12", N, H, W).fill(VO.random_frames(rng, N, H, W))
    dom = dict(scale=DOMAIN[0], zero=DOMAIN[1]) if dtype == "i8" else {}
    out = video.export(y, lr.s, r, fmt="i420", **dom)
    grey = image.export(y, **dom)
    torch.cuda.synchronize()
    assert out.fmt_name == "i420" and out.N == N
    assert torch.equal(out.y, grey[..., 0]), "the exported Y plane differs from sesrq.image.export at C = 1"


# ------------------------------------------------------------------------------------------------------------------- large
def test_output_surface_crossing_four_gib():
    """One batch of identical frames whose output surface (one buffer, frame after frame) crosses 2^32 bytes: every frame is compared
    on the device with frame 0, and frame 0 with the oracle."""
    import torch
    from sesrq import video
    r, H, W = 4, 64, 96
    per = video.frame_bytes("nv12", r * H, r * W)
    N = (1 << 32) // per + 2
    assert N * per > 1 << 32 and (N - 1) * per > 1 << 32          # the last frame lies wholly behind 2^32
    rng = np.random.default_rng(4096)
    lr1 = VO.random_frames(rng, 1, H, W)
    y1 = _luma(rng, (1, 1, r * H, r * W), "i8")
    want = VO.export(y1, lr1, r, scale=DOMAIN[0], zero=DOMAIN[1])
    y = _t(y1).expand(N, 1, r * H, r * W).contiguous()
    one = Laid("i420", 1, H, W).fill(lr1).s
    lr = video.Surface("i420", H, W, *[p.expand(N, *p.shape[1:]) for p in one.planes()])      # frame stride 0: one frame, N times
    out = video.Surface.alloc("nv12", N, r * H, r * W, device())
    assert out.buf.numel() == N * per and out.frame_y == per
    out.buf.fill_(CANARY)
    got = video.export(y, lr, r, scale=DOMAIN[0], zero=DOMAIN[1], out=out)
    torch.cuda.synchronize()
    assert got is out
    for p in out.planes():
        assert bool((p == p[:1]).all()), "a frame differs from frame 0"
    same("frame 0 y", out.y[0], want["y"][0])
    c = out.c0[0].cpu().numpy()
    same("frame 0 cb", np.ascontiguousarray(c[:, 0::2]), want["cb"][0])
    same("frame 0 cr", np.ascontiguousarray(c[:, 1::2]), want["cr"][0])
    same("last frame y", out.y[N - 1], want["y"][0])


# ------------------------------------------------------------------------------------------------------------------- engine
def _engine(net="sesr_x4", **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(os.path.join(IMG, net + ".npz")), device(), **kw)


def _golden_lr():
    """The golden SESR-x4 LR frames' luma as bytes: the Y plane of video frames (a) 16 x 16 x ..., with chroma drawn at random."""
    F = np.load(os.path.join(IMG, "frames.npz"), allow_pickle=False)
    lr = F["lr_a"]                                              # (H, W, 3) uint8: every code in every channel
    rng = np.random.default_rng(5)
    H, W = lr.shape[:2]
    fr = VO.random_frames(rng, 3, H, W)
    for n in range(3):
        fr["y"][n] = lr[..., n]
    return fr


def test_forward_video_equals_forward_on_the_decoded_q0_and_export():
    import torch
    from sesrq import video
    e = _engine()
    b = e.bundle
    scale, zero = b.scale[b.L], b.zero[b.L]
    fr = _golden_lr()
    N, H, W = fr["y"].shape
    side = torch.cuda.Stream(device=device())
    for i, (fi, fo) in enumerate(PAIRS):
        src = Laid(fi, N, H, W, pads=(3, 1) if i % 2 else (0, 0)).fill(fr).s
        q0, _ = video.decode(e, src)
        same("q0", q0, VO.decode(fr["y"], b.scale[0], b.zero[0], e.exact_div)[0])
        q, _ = e.forward(q0, want_q=True, want_f=False)
        torch.cuda.synchronize()
        want = VO.export(q.cpu().numpy(), fr, 4, scale=np.float32(scale), zero=zero)
        got, luma = e.forward_video(src, want_q=True)
        torch.cuda.synchronize()
        assert got.fmt_name == fi and (got.N, got.H, got.W) == (N, 4 * H, 4 * W) and torch.equal(luma, q)
        _same_frames(f"forward_video {fi}", VO.unpack(got.tobytes(), fi, 4 * H, 4 * W), want)
        # into a caller's out of the other format, behind pitches; on a side stream
        out = Laid(fo, N, 4 * H, 4 * W, pads=(16, 2), gap=9)
        assert e.forward_video(src, out=out.s) is out.s
        torch.cuda.synchronize()
        _same_frames(f"forward_video {fi} -> caller's {fo}", out.frames(), want)
        assert out.padding_intact()
        moved = video.Surface(fi, H, W, *[(p.to(torch.int32) * 1).to(torch.uint8) for p in src.planes()])      # produced on the current stream
        got_side = e.forward_video(moved, stream=side, slot=1)
        side.synchronize()
        _same_frames(f"forward_video {fi} side stream", VO.unpack(got_side.tobytes(), fi, 4 * H, 4 * W), want)
    assert (want["cb"] != want["cr"]).any() and len(np.unique(want["y"])) > 50


def test_forward_video_takes_the_fp32_frame_and_output_on_an_anchored_engine():
    """The fp32 branch: an anchor_add engine decodes the Y plane into the fp32 frame, runs the fp32 forward and exports its fp32
    output -- equal to forward() on the decoded frame followed by the export, and launched as the fp32 instantiations."""
    import torch
    from sesrq import video
    e = _engine(anchor_add=True)
    assert e.anchor_add
    fr = _golden_lr()
    N, H, W = fr["y"].shape
    x = VO.decode(fr["y"])[1]
    _, y = e.forward(_t(x), want_q=False, want_f=True)
    torch.cuda.synchronize()
    want = VO.export(y.cpu().numpy(), fr, 4)
    _, plain = _engine().forward(_t(x), want_q=False, want_f=True)
    assert not torch.equal(plain, y), "the anchored output is the plain one: the case would not tell the branches apart"
    for fi, fo in (("nv12", "i420"), ("i420", "nv12")):
        src = Laid(fi, N, H, W, pads=(1, 1)).fill(fr).s
        out = Laid(fo, N, 4 * H, 4 * W, pads=(3, 5), gap=2)
        before = video.instances()
        got, luma = e.forward_video(src, out=out.s, want_q=True)
        torch.cuda.synchronize()
        after = video.instances()
        assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {"video_decode<x>": 1, f"video_export<f32,r4,{fo}>": 1}
        assert got is out.s and luma.dtype == torch.float32 and torch.equal(luma, y)
        _same_frames(f"forward_video anchored {fi} -> {fo}", out.frames(), want)
        assert out.padding_intact()


def test_forward_video_refusals():
    import torch
    from sesrq import _lib, video
    fr = _golden_lr()
    N, H, W = fr["y"].shape
    src = Laid("nv12", N, H, W).fill(fr).s
    e = _engine()
    e6 = _engine("sesr_x2_rand", anchor_add=True)
    torch.cuda.synchronize()
    launches = sum(video.instances().values()) + sum(_lib.instances().values())
    for name, bad in (("short", Laid("nv12", N, 4 * H - 1, 4 * W).s), ("frames", Laid("nv12", N + 1, 4 * H, 4 * W).s),
                      ("host", video.Surface.alloc("nv12", N, 4 * H, 4 * W)), ("tensor", torch.empty((N, 4 * H, 4 * W), dtype=torch.uint8, device=device()))):
        with pytest.raises(ValueError, match="out must be a Surface"):
            e.forward_video(src, out=bad)
    with pytest.raises(ValueError, match="Surface"):
        e.forward_video(src.y)
    with pytest.raises(ValueError, match="HIP device"):
        e.forward_video(src.cpu())
    with pytest.raises(ValueError, match="luma net"):
        e6.forward_video(src)
    y = torch.zeros((N, 1, 4 * H, 4 * W), device=device())
    with pytest.raises(ValueError, match="2 or 4"):
        video.export(y, src, 3)
    with pytest.raises(ValueError, match="luma is a"):
        video.export(y[:, :, 1:], src, 4)
    with pytest.raises(ValueError, match="scale and zero"):
        video.export(y.to(torch.int8), src, 4)
    with pytest.raises(ValueError, match="float32 or int8"):
        video.export(y.to(torch.float16), src, 4)
    with pytest.raises(ValueError, match="out must be a Surface"):
        video.export(y, src, 4, fmt="i420", out=Laid("nv12", N, 4 * H, 4 * W).s)
    with pytest.raises(ValueError, match="pixel format"):
        video.export(y, src, 4, fmt="yuyv")
    with pytest.raises(ValueError, match="1 channel in"):
        video.decode(e6, src)
    torch.cuda.synchronize()
    assert sum(video.instances().values()) + sum(_lib.instances().values()) == launches, "a refused call launched a kernel"


def test_evaluate_video_equals_score_on_the_frames_made_by_hand():
    import torch
    from sesrq import quality, video
    e = _engine()
    b = e.bundle
    rng = np.random.default_rng(21)
    fr = _golden_lr()
    N, H, W = fr["y"].shape
    hr = VO.random_frames(rng, N, 4 * H, 4 * W)
    lrs = [video.Surface.views(np.frombuffer(bytearray(VO.pack({k: v[n:n + 1] for k, v in fr.items()}, "nv12")), np.uint8), "nv12", 1, H, W) for n in range(N)]
    hrs = [video.Surface.views(np.frombuffer(bytearray(VO.pack({k: v[n:n + 1] for k, v in hr.items()}, "i420")), np.uint8), "i420", 1, 4 * H, 4 * W)
           for n in range(N)]
    got = quality.evaluate_video(e, lrs, hrs)
    x = VO.decode(fr["y"])[1]
    gt = VO.decode(hr["y"])[1]
    rows = []
    for n in range(N):
        q, _ = e.forward(_t(x[n:n + 1]), want_q=True, want_f=False)
        rows.append(quality.score(q, _t(gt[n:n + 1]), 5, scale=float(b.scale[b.L]), zero=int(b.zero[b.L])))
    torch.cuda.synchronize()
    want = torch.cat(rows).cpu().numpy()
    assert got.shape == (N, 3) and got.dtype == np.float64 and np.array_equal(got, want)
    with pytest.raises(ValueError, match="MFLAG 6"):
        quality.evaluate_video(e, lrs, hrs, mflag=6)


def test_sim_yuv_save_yuv(capsys, tmp_path, monkeypatch):
    import sim
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "sesr_x4.params.npz")
    rng = np.random.default_rng(33)
    H, W = 9, 13
    fr = VO.random_frames(rng, 2, H, W)
    hr = VO.random_frames(rng, 2, 4 * H, 4 * W)
    with open(tmp_path / "lr.yuv", "wb") as f:
        f.write(VO.pack(fr, "nv12"))
    with open(tmp_path / "hr.yuv", "wb") as f:
        f.write(VO.pack(hr, "nv12"))
    STORE.clear()
    y = sim.main(["--mflag", "5", "--params", params, "--yuv", str(tmp_path / "lr.yuv"), "--size", f"{W}x{H}", "--pix-fmt", "nv12",
                  "--save-yuv", str(tmp_path / "sr.yuv"), "--out-pix-fmt", "i420", "--gt-yuv", str(tmp_path / "hr.yuv")])
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[-1].startswith("yuv:") and "mean psnr is" in lines[-2] and float(lines[-3]) > 0 and float(lines[-4]) > 0
    assert tuple(y.shape) == (2, 1, 4 * H, 4 * W)
    want = VO.export(y.cpu().numpy(), fr, 4)
    assert open(tmp_path / "sr.yuv", "rb").read() == VO.pack(want, "i420"), "the written file differs from the oracle's bytes"
    STORE.clear()
    sim.main(["--mflag", "5", "--params", params, "--yuv", str(tmp_path / "lr.yuv"), "--size", f"{W}x{H}", "--pix-fmt", "nv12",
              "--frames", "1:2", "--save-yuv", str(tmp_path / "one.yuv")])
    capsys.readouterr()
    assert open(tmp_path / "one.yuv", "rb").read() == VO.pack({k: v[1:] for k, v in want.items()}, "nv12")
    # from the command line nothing is returned and no output is kept: the same file
    STORE.clear()
    monkeypatch.setattr(sys, "argv", ["sim.py", "--mflag", "5", "--params", params, "--yuv", str(tmp_path / "lr.yuv"), "--size", f"{W}x{H}",
                                      "--pix-fmt", "nv12", "--save-yuv", str(tmp_path / "cli.yuv"), "--save", str(tmp_path / "cli.npy")])
    assert sim.main() is None
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[-1].startswith("yuv:") and f"output: (2, 1, {4 * H}, {4 * W})" in "\n".join(lines)
    assert open(tmp_path / "cli.yuv", "rb").read() == VO.pack(want, "nv12")
    assert np.array_equal(np.load(str(tmp_path / "cli.npy")), y.cpu().numpy())
    for bad in (["--size", f"{W}x{H}"], ["--yuv", str(tmp_path / "lr.yuv"), "--pix-fmt", "nv12"],
                ["--yuv", str(tmp_path / "lr.yuv"), "--size", f"{W}x{H}", "--pix-fmt", "nv12", "--input", str(tmp_path / "lr.yuv")]):
        STORE.clear()
        with pytest.raises(SystemExit, match="--yuv"):
            sim.main(["--mflag", "5", "--params", params] + bad)


def test_zz_every_video_instance_ran():
    """LAST in this file: every kernel instantiation libsesrq_video.so can launch was launched by a checked case above, by name."""
    from sesrq import video
    k = video.instances()
    names = [f"video_decode<{o}>" for o in ("q0", "x", "q0,x")] + \
        [f"video_export<{d},r{r},{f}>" for d in ("i8", "f32") for r in (2, 4) for f in FMTS]
    assert sorted(k) == sorted(names), k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
