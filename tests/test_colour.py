"""The colour export on the device (sesrq.colour, libsesrq_colour.so, Engine.forward_colour, sim.py --colour) against the numpy
restatement of include/sesrq_colour.h (tests/colour_oracle.py; tests/test_colour_oracle.py anchors it outside itself).  Every
comparison is exact and covers every byte; frames are small.

  chroma           all 2^24 triples, both byte orders
  geometry         every W from 1 to 2 TILE_W + 2 at H = 5, every H from 1 to 2 TILE_H + 2 at W = 7; r = 2 and 4, int8 and fp32 Y,
                   N = 1 and 3; random images and images drawn from {0, 255} (both clamps of step 4, negative sums of step 2)
  batch            neighbouring frames of opposite extremes: nothing of a frame reaches its neighbour
  luma extremes    every int8 code under three output domains; fp32 specials and values on rounding ties of step 4
  caller buffers   every buffer at odd addresses in a canary-filled arena: the same bytes, no canary touched
  large output     one batch whose output crosses 2^32 bytes
  sweeps           (tests/test_resampler_sweep_device.py) every 4-tuple of the cube corners and mid-grey as the taps of each pass
  strips           (tests/test_resampler_limits.py) one LR row and one LR column, one and two wide, of 2^22 + 5 pixels, r = 2 and 4
  forward_colour   on the golden LR frames, a side stream, a caller's out, the refusals; sim.py --colour --save-png
  instances        LAST: every instantiation was launched by a checked case"""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import Arena, device, same, sha256, stream_ptr

import colour_oracle as CO
from colour_oracle import header_tile

pytestmark = pytest.mark.gpu

F32 = np.float32
IMG = os.path.join(GOLDEN, "image")
DOMAIN = (0.0047, -119)                       # an int8 output domain for the cases that need no particular one


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


def _bgr(img):
    return np.ascontiguousarray(img[..., ::-1])


def _luma(rng, shape, dtype):
    """A random luma of `shape`: int8 codes, or fp32 values around and outside [0, 1]."""
    if dtype == "i8":
        return rng.integers(-128, 128, shape).astype(np.int8)
    return (rng.random(shape) * 1.3 - 0.15).astype(F32)


def _export(y, img, r, order="rgb", **kw):
    import torch
    from sesrq import colour
    dom = dict(scale=DOMAIN[0], zero=DOMAIN[1]) if y.dtype == np.int8 else {}
    dom.update(kw)
    got = colour.export(_t(y), _t(img), r, order=order, **dom)
    torch.cuda.synchronize()
    return got.cpu().numpy(), CO.export(y, img, r, order, scale=dom.get("scale"), zero=dom.get("zero"))


def _all_triples():
    """Every (R, G, B) triple once: a 4096 x 4096 x 3 uint8 image."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], 1).astype(np.uint8).reshape(1, 4096, 4096, 3)


def test_chroma_exhaustive_every_triple():
    import torch
    from sesrq import colour
    img = _all_triples()
    want = CO.chroma(img)
    assert want.dtype == np.int16 and want.min() == 1024 and want.max() == 15360
    for order, src in (("rgb", img), ("bgr", _bgr(img))):
        got = colour.chroma(_t(src), order=order)
        torch.cuda.synchronize()
        same(f"chroma {order}", got, want)
    # a batch of small odd frames: the plane layout (N, 2, H, W)
    rng = np.random.default_rng(5)
    small = rng.integers(0, 256, (3, 7, 13, 3)).astype(np.uint8)
    same("chroma batch", colour.chroma(_t(small)), CO.chroma(small))
    same("chroma one frame", colour.chroma(_t(small[0])), CO.chroma(small[:1]))


# ------------------------------------------------------------------------------------------------------------------- geometry
def _sizes(r):
    """Every W from 1 to two tiles and two at H = 5, every H likewise at W = 7, in the LR tile of factor r (at r = 2 twice the
    exported TILE_W / TILE_H: the sweep goes further than 2 TILE + 2, never less far)."""
    tw, th = CO.tile(r)
    ws, hs = list(range(1, 2 * tw + 3)), list(range(1, 2 * th + 3))
    assert ws[-1] >= 2 * header_tile()[0] + 2 and hs[-1] >= 2 * header_tile()[1] + 2 and ws[0] == hs[0] == 1
    assert CO.tile(4) == header_tile()
    return [(5, w) for w in ws] + [(h, 7) for h in hs]


@pytest.mark.parametrize("dtype", ["i8", "f32"])
@pytest.mark.parametrize("r", [2, 4])
def test_geometry_every_width_and_height_across_the_tile_seams(r, dtype):
    tw, th = CO.tile(r)
    sizes = _sizes(r)
    assert {1, 2, 3, tw - 1, tw, tw + 1, 2 * tw, 2 * tw + 1} <= {w for _, w in sizes}
    assert {1, 2, 3, th - 1, th, th + 1, 2 * th, 2 * th + 1} <= {h for h, _ in sizes}
    assert any((r * w) % 16 for _, w in sizes) and any((r * w) % 16 == 0 for _, w in sizes)      # both store paths
    rng = np.random.default_rng(100 * r + len(dtype))
    seen = {"low": False, "high": False, "negative": False}      # what the {0, 255} images must reach
    for N in (1, 3):
        for kind in ("random", "extreme"):
            for H, W in sizes:
                img = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8) if kind == "random" else \
                    (rng.integers(0, 2, (N, H, W, 3)) * 255).astype(np.uint8)
                y = _luma(rng, (N, 1, r * H, r * W), dtype)
                order = ("rgb", "bgr")[(H + W) % 2]
                got, want = _export(y, img, r, order)
                same(f"r={r} {dtype} N={N} {kind} {H}x{W} {order}", got, want)
                if kind == "extreme":
                    up, h = CO.upscale(CO.chroma(img, order), r, keep=True)
                    p = CO.dequant(y, *DOMAIN) if dtype == "i8" else y
                    f = np.stack(CO.colour_f32(CO.luma(p)[:, 0], up[:, 0], up[:, 1]))
                    seen["low"] |= bool((f < -0.5).any())
                    seen["high"] |= bool((f > 255.5).any())
                    seen["negative"] |= bool((h < 0).any())
    assert all(seen.values()), f"the {{0, 255}} images did not reach: {[k for k, v in seen.items() if not v]}"


def test_batch_frames_do_not_leak_into_their_neighbours():
    """Frames of opposite extremes side by side: all-0 and all-255 (the luma line's extremes; both are neutral in chroma), and
    saturated blue and yellow (the chroma extremes, where an edge clamp that crossed into the next frame would show).  A constant frame
    gives a constant chroma plane, so each output frame must equal the export of that frame alone."""
    rng = np.random.default_rng(17)
    for r in (2, 4):
        tw, th = CO.tile(r)
        for H, W in ((3, 5), (th + 1, tw + 1), (1, 1)):
            for pair in (((0, 0, 0), (255, 255, 255)), ((0, 0, 255), (255, 255, 0))):
                N = 5
                img = np.empty((N, H, W, 3), np.uint8)
                for n in range(N):
                    img[n] = pair[n % 2]
                y = _luma(rng, (N, 1, r * H, r * W), "i8")
                got, want = _export(y, img, r)
                same(f"batch r={r} {H}x{W} {pair}", got, want)
                c = CO.chroma(img)
                for n in range(N):
                    alone = CO.export(y[n:n + 1], img[n:n + 1], r, scale=DOMAIN[0], zero=DOMAIN[1])
                    assert np.array_equal(got[n:n + 1], alone), (r, H, W, pair, n)
                    up = CO.upscale(c[n], r)
                    assert (up[0] == c[n, 0, 0, 0]).all() and (up[1] == c[n, 1, 0, 0]).all()
                assert (c[0] != c[1]).any() or pair[0] == (0, 0, 0)


# ------------------------------------------------------------------------------------------------------------------- luma
def _fixture_domain():
    z = np.load(os.path.join(IMG, "sesr_x4.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    L = len(meta["scale"]) - 1
    return float(np.float32(meta["scale"][L])), int(meta["zero"][L])


@pytest.mark.parametrize("r", [2, 4])
def test_every_int8_code_under_three_output_domains(r):
    s_fix, z_fix = _fixture_domain()
    rng = np.random.default_rng(r)
    H = W = 16 // r
    img = rng.integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    img[1] = 128                                             # a grey frame: the luma alone decides the bytes
    codes = np.arange(-128, 128).astype(np.int8)
    y = np.stack([codes, codes[::-1], rng.permutation(codes)]).reshape(3, 1, 16, 16)
    for scale, zero in ((s_fix, z_fix), (s_fix, -128), (s_fix, 127), (1.0, 0), (3e38, -128)):
        got, want = _export(y, img, r, scale=scale, zero=zero)
        same(f"codes r={r} scale={scale} zero={zero}", got, want)
    assert len(np.unique(got[1])) <= 2 and len(np.unique(_export(y, img, r, scale=s_fix, zero=z_fix)[0][1])) > 100


def _tie_lumas():
    """fp32 predictions p whose a = 1.16438356 (255 p - 16) is exactly k + 1/2: with neutral chroma all three bytes sit on a tie."""
    out = []
    for k in range(255):
        p0 = F32((16 + (k + 0.5) / 1.16438356) / 255)
        p = (p0.view(np.uint32).astype(np.int64) + np.arange(-200, 201)).astype(np.uint32).view(F32)
        a = F32(1.16438356) * (p * F32(255.0) - F32(16.0))
        out += [(float(v), k) for v in p[a == F32(k + 0.5)]]
    return out


@pytest.mark.parametrize("r", [2, 4])
def test_fp32_luma_specials_and_rounding_ties(r):
    ties = _tie_lumas()
    assert len(ties) >= 100 and {k % 2 for _, k in ties} == {0, 1}          # ties towards the even byte below and above
    special = np.array([0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000000,
                        0x00000001, 0x80000001, 0x3f800000, 0x3f800001, 0x3f7fffff, 0xbf800000, 0x7f7fffff, 0xff7fffff],
                       np.uint32).view(F32)
    vals = np.concatenate([special, np.array([-0.25, 1.5, 16 / 255, 235 / 255, 0.5], F32), np.array([v for v, _ in ties], F32)])
    n = 16 * 32
    assert len(vals) <= n
    y = np.resize(vals, n).astype(F32).reshape(1, 1, 16, 32)
    y = np.concatenate([y, y[:, :, ::-1, ::-1]]).copy()
    H, W = 16 // r, 32 // r
    rng = np.random.default_rng(r + 40)
    img = np.stack([np.full((H, W, 3), 77, np.uint8), rng.integers(0, 256, (H, W, 3)).astype(np.uint8)])
    got, want = _export(y, img, r)
    same(f"fp32 specials r={r}", got, want)
    # the grey frame: neutral chroma, so a tie of a is a tie of every byte, resolved to even
    assert (CO.chroma(img[:1]) == 8192).all()
    flat = got[0].reshape(-1, 3)
    for i, (v, k) in enumerate(ties):
        assert tuple(flat[len(special) + 5 + i]) == (k + (k % 2),) * 3, (v, k, flat[len(special) + 5 + i])
    assert tuple(flat[0]) == tuple(flat[1]) == tuple(flat[2]) == tuple(flat[3]) == tuple(flat[7]) == (0, 0, 0)      # NaN as 0.0


# ------------------------------------------------------------------------------------------------------------------- buffers
I8_OFFS = (0, 1, 2, 3, 7)
F32_OFFS = (0, 4, 8, 12)
ROUNDS = ((0x5A, bytes([0x7F])), (0xA5, bytes([0x80])))


@pytest.mark.parametrize("dtype", ["i8", "f32"])
@pytest.mark.parametrize("r", [2, 4])
def test_export_in_hostile_surroundings(r, dtype):
    """img, out and y at every address class, in arenas whose every other byte is a canary: the bytes equal the oracle's, nothing
    beside the buffers changes.  W = 8 gives whole 16-pixel runs (the 16-byte path when the addresses allow: offset 0), W = 7 only
    the per-element path; both are launches of the same instantiation."""
    import torch
    from sesrq import colour
    name = f"colour_export<{dtype},r{r}>"
    rng = np.random.default_rng(31 * r + len(dtype))
    y_offs = I8_OFFS if dtype == "i8" else F32_OFFS
    seen = {"img": set(), "out": set(), "y": set()}
    for H, W in ((3, 8), (5, 7)):
        N = 2
        img = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
        y = _luma(rng, (N, 1, r * H, r * W), dtype)
        want = CO.export(y, img, r, "rgb", scale=DOMAIN[0], zero=DOMAIN[1])
        places = [(0, 0, 0)] + [(I8_OFFS[(i + 1) % 5], I8_OFFS[(i + 2) % 5], y_offs[i % len(y_offs)]) for i in range(5)] + \
                 [(0, 0, y_offs[1]), (0, 1, 0), (1, 0, 0)]
        for io, oo, yo in places:
            for rnd, (canary, around) in enumerate(ROUNDS):
                what = f"{name} {H}x{W} img@{io} out@{oo} y@{yo} run {rnd + 1}"
                before = colour.instances()
                ain = Arena(device(), Arena.room(img.nbytes, y.nbytes), around if dtype == "i8" else np.array([np.nan], F32).tobytes())
                dimg = ain.place(img.shape, torch.uint8, io, fill=img, name="img")
                dy = ain.place(y.shape, torch.int8 if dtype == "i8" else torch.float32, yo, fill=y, name="y")
                aout = Arena(device(), Arena.room(want.nbytes), canary)
                out = aout.place(want.shape, torch.uint8, oo, name="out")
                rc = colour.lib().sesrq_colour_export(dy.data_ptr(), colour.Y_I8 if dtype == "i8" else colour.Y_F32, DOMAIN[0], DOMAIN[1],
                                                      dimg.data_ptr(), 0, r, out.data_ptr(), N, H, W, stream_ptr())
                assert rc == 0, (what, colour.last_error())
                torch.cuda.synchronize()
                for a in (ain, aout):
                    stray = a.check()
                    assert not stray, f"{what}: bytes outside the caller's buffers changed: {stray[:6]}"
                same(what, out, want)
                same(what + " img untouched", dimg, img)
                same(what + " y untouched", dy, y)
                after = colour.instances()
                assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}, what
                seen["img"].add(io), seen["out"].add(oo), seen["y"].add(yo)
    assert seen["img"] == seen["out"] == set(I8_OFFS) and seen["y"] == set(y_offs), seen


def test_chroma_in_hostile_surroundings():
    import torch
    from sesrq import colour
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (2, 5, 7, 3)).astype(np.uint8)
    want = CO.chroma(img)
    for io, co in ((0, 0), (1, 2), (2, 6), (3, 14), (7, 10)):
        for canary, around in ROUNDS:
            ain = Arena(device(), Arena.room(img.nbytes), around)
            dimg = ain.place(img.shape, torch.uint8, io, fill=img, name="img")
            aout = Arena(device(), Arena.room(want.nbytes), canary)
            out = aout.place(want.shape, torch.int16, co, name="cbcr")
            assert colour.lib().sesrq_colour_chroma(dimg.data_ptr(), 0, out.data_ptr(), 2, 5, 7, stream_ptr()) == 0, colour.last_error()
            torch.cuda.synchronize()
            assert not ain.check() and not aout.check(), (io, co)
            same(f"chroma img@{io} cbcr@{co}", out, want)


# ------------------------------------------------------------------------------------------------------------------- large
def test_output_crossing_four_gib():
    """One batch whose output crosses 2^32 bytes: the frames are copies of three distinct small frames (two tiles by eight at r = 4), compared
    on the device against the oracle of those three."""
    import torch
    from sesrq import colour
    r, H, W = 4, 64, 64
    per = r * H * r * W * 3
    N = (1 << 32) // per + 2
    assert N * per > 1 << 32 and (N - 1) * per > 1 << 32          # the last frame lies wholly behind 2^32
    rng = np.random.default_rng(4096)
    img3 = rng.integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    y3 = _luma(rng, (3, 1, r * H, r * W), "i8")
    want3 = _t(CO.export(y3, img3, r, scale=DOMAIN[0], zero=DOMAIN[1]))
    idx = torch.arange(N, device=device()) % 3
    img, y = _t(img3)[idx], _t(y3)[idx]
    out = torch.full((N, r * H, r * W, 3), 0x5A, dtype=torch.uint8, device=device())
    got = colour.export(y, img, r, scale=DOMAIN[0], zero=DOMAIN[1], out=out)
    torch.cuda.synchronize()
    assert got is out
    for k in range(3):
        assert bool((out[k::3] == want3[k]).all()), f"frames {k} mod 3 differ"
    same("last frame", out[N - 1], want3[(N - 1) % 3])


# ------------------------------------------------------------------------------------------------------------------- engine
def _lr(f):
    """The LR frame f of tests/golden/image/frames.npz: (a) is stored, (b) and (c) are regenerated and checked against its SHA-256."""
    F = np.load(os.path.join(IMG, "frames.npz"), allow_pickle=False)
    if f == "a":
        lr = F["lr_a"]
    else:
        sys.path.insert(0, GOLDEN)
        from make_image_golden import NATURAL
        from natural import natural_frame
        h, w, seed = NATURAL[f]
        lr = np.rint(natural_frame(3, h, w, seed)[0].astype(np.float64) * 255).astype(np.uint8).transpose(1, 2, 0).copy()
    assert sha256(lr) == json.loads(str(F["meta"]))["sha"][f"lr_{f}"], f"frame {f} differs from the one the reference ran on"
    return lr


def _engine(net="sesr_x4", **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(os.path.join(IMG, net + ".npz")), device(), **kw)


def test_forward_colour_equals_the_oracle_on_forward_images_output():
    import torch
    e = _engine()
    b = e.bundle
    scale, zero = b.scale[b.L], b.zero[b.L]
    side = torch.cuda.Stream(device=device())
    for f in ("a", "b", "c"):
        lr = _lr(f)
        wants = {}
        for order in ("rgb", "bgr"):
            src = _bgr(lr) if order == "bgr" else lr
            d = _t(src)
            q, _ = e.forward_image(d, order=order, want_f=False)
            got = e.forward_colour(d, order=order)
            torch.cuda.synchronize()
            assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 4 * lr.shape[0], 4 * lr.shape[1], 3)
            wants[order] = CO.export(q.cpu().numpy(), src[None], 4, order, scale=np.float32(scale), zero=zero)
            same(f"forward_colour {f} {order}", got, wants[order])
        want = wants["rgb"]
        assert np.array_equal(wants["bgr"], want[..., ::-1]) and (want[..., 0] != want[..., 2]).any()
        # the same bytes on a side stream, into a caller's out, and for a batch
        x = (_t(lr.astype(np.int32)) * 1).to(torch.uint8)          # produced on the current stream just before the call
        got_side = e.forward_colour(x, stream=side, slot=1)
        side.synchronize()
        same(f"forward_colour {f} side stream", got_side, want)
        out = torch.full(tuple(got.shape), 0x5A, dtype=torch.uint8, device=device())
        assert e.forward_colour(_t(lr), out=out) is out
        torch.cuda.synchronize()
        same(f"forward_colour {f} caller out", out, want)
    two = np.stack([_lr("c"), _lr("c")[::-1, ::-1]])
    got2 = e.forward_colour(_t(two))
    q2, _ = e.forward_image(_t(two), want_f=False)
    torch.cuda.synchronize()
    same("forward_colour batch", got2, CO.export(q2.cpu().numpy(), two, 4, scale=np.float32(scale), zero=zero))


def test_forward_colour_refusals():
    import torch
    from sesrq import _lib, colour
    lr = _t(_lr("c"))
    e = _engine()
    e6 = _engine("sesr_x2_rand", anchor_add=True)
    torch.cuda.synchronize()
    launches = sum(colour.instances().values()) + sum(_lib.instances().values())
    shp = (1, 4 * lr.shape[0], 4 * lr.shape[1], 3)
    for name, bad in (("short", torch.empty((1, shp[1] - 1, shp[2], 3), dtype=torch.uint8, device=device())),
                      ("planar", torch.empty((1, 3, shp[1], shp[2]), dtype=torch.uint8, device=device())),
                      ("int8", torch.empty(shp, dtype=torch.int8, device=device())),
                      ("strided", torch.empty((1, shp[1], 2 * shp[2], 3), dtype=torch.uint8, device=device())[:, :, ::2]),
                      ("host", torch.empty(shp, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="out must be a contiguous uint8 tensor of the output shape"):
            e.forward_colour(lr, out=bad)
    with pytest.raises(ValueError, match="order"):
        e.forward_colour(lr, order="rbg")
    with pytest.raises(ValueError, match="uint8"):
        e.forward_colour(lr.to(torch.int16))
    with pytest.raises(ValueError, match="interleaved"):
        e.forward_colour(lr.permute(2, 0, 1).contiguous())
    with pytest.raises(ValueError, match="image.export"):
        e6.forward_colour(lr)
    y = torch.zeros((1, 1, shp[1], shp[2]), device=device())
    with pytest.raises(ValueError, match="2 or 4"):
        colour.export(y, lr, 3)
    with pytest.raises(ValueError, match="luma is a"):
        colour.export(y[:, :, 1:], lr, 4)
    with pytest.raises(ValueError, match="scale and zero"):
        colour.export(y.to(torch.int8), lr, 4)
    with pytest.raises(ValueError, match="float32 or int8"):
        colour.export(y.to(torch.float16), lr, 4)
    torch.cuda.synchronize()
    assert sum(colour.instances().values()) + sum(_lib.instances().values()) == launches, "a refused call launched a kernel"


def test_sim_colour_save_png(capsys, tmp_path):
    pytest.importorskip("PIL")
    import sim
    from sesrq import image
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "sesr_x4.params.npz")
    lr = _lr("c")
    image.save_png(str(tmp_path / "lr.png"), lr)
    np.save(str(tmp_path / "lr_bgr.npy"), _bgr(lr))
    STORE.clear()
    y = sim.main(["--mflag", "5", "--params", params, "--input", str(tmp_path / "lr.png"), "--colour", "--save-png", str(tmp_path / "sr.png")])
    assert capsys.readouterr().out.strip().split("\n")[-1].startswith("png:")
    STORE.clear()
    sim.main(["--mflag", "5", "--params", params, "--input", str(tmp_path / "lr_bgr.npy"), "--image", "--order", "bgr", "--colour",
              "--save-png", str(tmp_path / "sr_bgr.png")])
    STORE.clear()
    sim.main(["--mflag", "5", "--params", params, "--input", str(tmp_path / "lr.png"), "--save-png", str(tmp_path / "grey.png")])
    capsys.readouterr()
    want = CO.export(y.cpu().numpy(), lr[None], 4)[0]
    got = image.load_image(str(tmp_path / "sr.png"))
    from PIL import Image
    with Image.open(str(tmp_path / "sr.png")) as im:
        assert im.mode == "RGB"
    with Image.open(str(tmp_path / "grey.png")) as im:
        assert im.mode == "L"                                  # without the flag everything is as before
    assert got.shape == (4 * lr.shape[0], 4 * lr.shape[1], 3) and np.array_equal(got, want)
    assert np.array_equal(image.load_image(str(tmp_path / "sr_bgr.png")), want)
    assert (got[..., 0] != got[..., 1]).any()                  # colour, not grey
    # --colour without a luma net's image route to finish: not an image input, no --save-png
    for bad in (["--input", str(tmp_path / "lr_bgr.npy"), "--save-png", str(tmp_path / "no.png")],
                ["--input", str(tmp_path / "lr.png")]):
        STORE.clear()
        with pytest.raises(SystemExit, match="--colour"):
            sim.main(["--mflag", "5", "--params", params, "--colour"] + bad)
    assert not os.path.exists(str(tmp_path / "no.png"))


def test_zz_every_colour_instance_ran():
    """LAST in this file: every kernel instantiation libsesrq_colour.so can launch was launched by a checked case above."""
    from sesrq import colour
    k = colour.instances()
    assert len(k) == 5, k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
