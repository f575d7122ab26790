"""The bicubic downscale and its fused decode on the device (sesrq.downscale, libsesrq_downscale.so, Engine.forward_hr,
quality.evaluate_hr, Calibrator.enqueue_hr, sim.py --hr) against the numpy restatement of include/sesrq_downscale.h
(tests/downscale_oracle.py; tests/test_downscale_oracle.py anchors it outside itself).  Every comparison is exact and covers every
byte and every fp32 word; frames are small.

  geometry         every LR width from 1 to 2 tiles + 2 at LR height 5, every LR height likewise at LR width 7; r = 2 and 4, forms Y
                   and RGB, orders RGB and BGR, N = 1 and 3, random and {0, 255} images, each output subset (lr, q0, x, all three)
  clamps           the patterns that fire both clamps of each pass, and the 256 constants
  composition      fused q0 / x == image.decode of the kernel's own LR image, under exact_div 0 and 2 and the golden input domains
  batch            neighbouring frames of opposite extremes: nothing of a frame reaches its neighbour
  caller buffers   every buffer at odd addresses in canary arenas, twice in hostile surroundings
  large input      one batch whose HR input crosses 2^32 bytes
  engine           forward_hr == forward_image of the oracle's LR image; evaluate_hr == evaluate_image(oracle LR, HR);
                   Calibrator.enqueue_hr == enqueue_image on the oracle LR; sim.py --hr and --save-lr
  refusals         the C ABI's, on pointers that are never dereferenced
  sweeps           (tests/test_resampler_sweep_device.py) every reachable sum of the vertical and of the horizontal pass, r = 2 and 4
  strips           (tests/test_resampler_limits.py) one LR row and one LR column, one and two wide, of 2^22 + 5 pixels, r = 2 and 4
  instances        LAST: every instantiation was launched by a checked case"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import Arena, calib_params, device, same, stream_ptr

import downscale_oracle as DO
import image_oracle as IO
from test_downscale_oracle import c_abi_refusals

pytestmark = pytest.mark.gpu

F32 = np.float32
IMG = os.path.join(GOLDEN, "image")
DOMAIN = (0.0039, -128)                       # an input domain for the cases that need no particular one
FORMS = ("y", "rgb")
SUBSETS = (("lr",), ("q0",), ("x",), ("lr", "q0", "x"))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


def _bgr(img):
    return np.ascontiguousarray(img[..., ::-1])


def _image(rng, shape, kind):
    return rng.integers(0, 256, shape, dtype=np.uint8) if kind == "random" else (rng.integers(0, 2, shape) * 255).astype(np.uint8)


def _run(img_d, r, form, order, subset, domain=DOMAIN, exact_div=0, canary=0x5A):
    """One launch into canary-filled outputs of the subset: {name: tensor}."""
    import torch
    from sesrq import downscale
    N, H, W, _ = img_d.shape
    Ch = 1 if form == "y" else 3
    out = {"lr": torch.full((N, H // r, W // r, 3), canary, dtype=torch.uint8, device=device()) if "lr" in subset else None,
           "q0": torch.full((N, Ch, H // r, W // r), canary, dtype=torch.int8, device=device()) if "q0" in subset else None,
           "x": torch.full((N, Ch, H // r, W // r), float("nan"), dtype=torch.float32, device=device()) if "x" in subset else None}
    downscale.launch(device(), domain[0], domain[1], exact_div, img_d, order, r, form, out["lr"], out["q0"], out["x"],
                     torch.cuda.current_stream(device()))
    return {k: v for k, v in out.items() if v is not None}


def _wants(img, r, domain=DOMAIN, exact_div=0):
    """{(form, order): {name: device tensor}} of an RGB-order image and of its BGR twin, from one oracle run of the LR image."""
    lr = DO.downscale(img, r)
    res = {}
    for form in FORMS:
        x = np.ascontiguousarray(IO.decode(lr, form))
        q = np.ascontiguousarray(IO.q0(x, domain[0], domain[1], exact_div)).astype(np.int8)
        xd, qd = _t(x), _t(q)
        res[form, "rgb"] = {"lr": _t(lr), "q0": qd, "x": xd}
        res[form, "bgr"] = {"lr": _t(_bgr(lr)), "q0": qd, "x": xd}
    return res


def _mismatches(got, want):
    """Device count of differing elements; fp32 compared as words."""
    import torch
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == torch.float32:
        got, want = got.view(torch.int32), want.view(torch.int32)
    return (got != want).sum()


def _sizes(r):
    tw, th = DO.tile(r)
    ws, hs = list(range(1, 2 * tw + 3)), list(range(1, 2 * th + 3))
    (hw, hh), _ = DO.header_tile()
    assert ws[-1] >= 2 * hw + 2 and hs[-1] >= 2 * hh + 2 and ws[0] == hs[0] == 1 and DO.tile(4) == (hw, hh)
    return [(5, w) for w in ws] + [(h, 7) for h in hs]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("r", [2, 4])
def test_geometry_every_width_and_height_across_the_tile_seams(r, N):
    import torch
    tw, th = DO.tile(r)
    sizes = _sizes(r)
    assert {1, 2, 3, tw - 1, tw, tw + 1, 2 * tw, 2 * tw + 1} <= {w for _, w in sizes}
    assert {1, 2, 3, th - 1, th, th + 1, 2 * th, 2 * th + 1} <= {h for h, _ in sizes}
    rng = np.random.default_rng(100 * r + N)
    seen = {"low": False, "high": False}
    for kind in ("random", "extreme"):
        for h, w in sizes:
            img = _image(rng, (N, r * h, r * w, 3), kind)
            wants = _wants(img, r)
            src = {"rgb": _t(img), "bgr": _t(_bgr(img))}
            names, bad = [], []
            for form in FORMS:
                for order in ("rgb", "bgr"):
                    for subset in SUBSETS:
                        for k, v in _run(src[order], r, form, order, subset).items():
                            names.append(f"r={r} N={N} {kind} LR {h}x{w} {form} {order} {'+'.join(subset)}: {k}")
                            bad.append(_mismatches(v, wants[form, order][k]))
            counts = torch.stack(bad).cpu().numpy()
            wrong = [(n, int(c)) for n, c in zip(names, counts) if c]
            assert not wrong, f"{len(wrong)} outputs differ from the oracle, first: {wrong[:4]}"
            if kind == "extreme":
                s = DO.one_pass(img, r, 1, sums=True)
                seen["low"] |= bool((s < -DO.D[r] // 2).any())
                seen["high"] |= bool((s > 255 * DO.D[r] + DO.D[r] // 2).any())
    assert all(seen.values()), f"the {{0, 255}} images did not reach the clamps: {seen}"


@pytest.mark.parametrize("r", [2, 4])
def test_clamp_patterns_and_the_256_constants(r):
    import torch
    n, d = 12 * r, 5
    frames = []
    for high in (True, False):
        line = DO.clamp_pattern(n, r, d, high)
        frames += [np.broadcast_to(line[:, None, None], (n, n, 3)), np.broadcast_to(line[None, :, None], (n, n, 3))]
    img = np.ascontiguousarray(np.stack(frames))
    want, v = DO.downscale(img, r, keep=True)
    assert (want[0, d] == 255).all() and (want[1, :, d] == 255).all() and (want[2, d] == 0).all() and (want[3, :, d] == 0).all()
    assert (v[0, d] == 255).all() and (v[2, d] == 0).all()                               # the vertical pass's own clamps
    got = _run(_t(img), r, "rgb", "rgb", ("lr", "q0", "x"))
    torch.cuda.synchronize()
    same(f"clamp patterns r={r}", got["lr"], want)
    same(f"clamp patterns r={r} x", got["x"], IO.decode(want, "rgb"))
    for H, W in ((r, r), (3 * r, 5 * r), (2 * DO.HR_TILE[1] + r, DO.HR_TILE[0] + r)):
        const = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, H, W, 3)))
        assert np.array_equal(DO.downscale(const, r), const[:, :H // r, :W // r])
        same(f"constants r={r} {H}x{W}", _run(_t(const), r, "y", "rgb", ("lr",))["lr"], const[:, :H // r, :W // r])


def _golden_domain(net):
    meta = json.loads(str(np.load(os.path.join(IMG, net + ".npz"), allow_pickle=False)["meta"]))
    return float(np.float32(meta["scale"][0])), int(meta["zero"][0])


@pytest.mark.parametrize("r", [2, 4])
def test_composition_fused_decode_equals_image_decode_of_the_kernels_own_lr(r):
    """The composition law: q0 / x of the fused kernel are libsesrq_image.so's decode of the LR image the same kernel writes, bit for
    bit -- under the true quotient and the reciprocal form, a plain domain and the golden nets' natural-frame input domains."""
    import torch
    from sesrq import image
    rng = np.random.default_rng(r)
    tw, th = DO.tile(r)
    img = _image(rng, (2, r * (th + 3), r * (tw + 5), 3), "random")
    img[1] = _image(rng, img.shape[1:], "extreme")
    d = _t(img)
    st = torch.cuda.current_stream(device())
    for domain in (DOMAIN, _golden_domain("sesr_x4"), _golden_domain("sesr_x2_rand")):
        for exact_div in (0, 2):
            for form in FORMS:
                for order in ("rgb", "bgr"):
                    got = _run(d, r, form, order, ("lr", "q0", "x"), domain, exact_div)
                    q = torch.full_like(got["q0"], 0x5A)
                    x = torch.full_like(got["x"], float("nan"))
                    image.launch(device(), domain[0], domain[1], exact_div, got["lr"], form, order, q, x, st)
                    torch.cuda.synchronize()
                    what = f"r={r} {form} {order} domain={domain} exact_div={exact_div}"
                    same(what + " q0", got["q0"], q)
                    same(what + " x", got["x"], x)
                    lr = DO.downscale(img, r)                  # the same bytes in both orders: the order only names the channels
                    same(what + " lr", got["lr"], lr)
                    same(what + " q0 oracle", got["q0"], IO.q0(IO.decode(lr, form, order), domain[0], domain[1], exact_div), cast=np.int8)
    assert len(np.unique(got["q0"].cpu().numpy())) > 50


def test_batch_frames_do_not_leak_into_their_neighbours():
    """Frames of opposite extremes side by side: a constant frame downscales to itself, whatever its neighbours hold; an index that
    mirrored into the next frame of the batch would show at the borders."""
    import torch
    for r in (2, 4):
        tw, th = DO.tile(r)
        for h, w in ((1, 1), (3, 5), (th + 1, tw + 1)):
            N = 5
            img = np.empty((N, r * h, r * w, 3), np.uint8)
            img[0::2], img[1::2] = 0, 255
            got = _run(_t(img), r, "rgb", "rgb", ("lr", "x"))
            torch.cuda.synchronize()
            same(f"batch r={r} {h}x{w}", got["lr"], img[:, :h, :w])
            same(f"batch r={r} {h}x{w} x", got["x"], IO.decode(img[:, :h, :w], "rgb"))
            same(f"batch r={r} {h}x{w} oracle", got["lr"], DO.downscale(img, r))


# ------------------------------------------------------------------------------------------------------------------- buffers
OFFS = (0, 1, 2, 3, 7)
X_OFFS = (0, 4, 8, 12)
ROUNDS = ((0x5A, bytes([0x7F])), (0xA5, bytes([0x80])))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("r", [2, 4])
def test_run_in_hostile_surroundings(r, form):
    """img, lr, q0 and x at every address class, in arenas whose every other byte is a canary, twice with different surroundings: the
    bytes equal the oracle's and nothing beside the buffers changes."""
    import torch
    from sesrq import downscale
    name = f"downscale<r{r},{'Y' if form == 'y' else 'RGB'}>"
    rng = np.random.default_rng(31 * r + len(form))
    h_ctx = downscale._so.context(device(), DOMAIN[0], DOMAIN[1], 0)
    seen = {"img": set(), "lr": set(), "q0": set(), "x": set()}
    Ch = 1 if form == "y" else 3
    for h, w in ((3, 8), (5, 7)):
        N = 2
        img = _image(rng, (N, r * h, r * w, 3), "random")
        lr, x, q = DO.decode(img, r, form, "rgb", *DOMAIN)
        places = [(0, 0, 0, 0)] + [(OFFS[(i + 1) % 5], OFFS[(i + 2) % 5], OFFS[(i + 3) % 5], X_OFFS[i % 4]) for i in range(5)] + \
                 [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 4)]
        for io, lo, qo, xo in places:
            for rnd, (canary, around) in enumerate(ROUNDS):
                what = f"{name} LR {h}x{w} img@{io} lr@{lo} q0@{qo} x@{xo} run {rnd + 1}"
                before = downscale.instances()
                ain = Arena(device(), Arena.room(img.nbytes), around)
                dimg = ain.place(img.shape, torch.uint8, io, fill=img, name="img")
                aout = Arena(device(), Arena.room(lr.nbytes, q.nbytes, x.nbytes), canary)
                dlr = aout.place(lr.shape, torch.uint8, lo, name="lr")
                dq = aout.place(q.shape, torch.int8, qo, name="q0")
                dx = aout.place(x.shape, torch.float32, xo, name="x")
                rc = downscale.lib().sesrq_downscale_run(h_ctx, dimg.data_ptr(), 0, r, 0 if form == "y" else 1, dlr.data_ptr(),
                                                         dq.data_ptr(), dx.data_ptr(), N, r * h, r * w, stream_ptr())
                assert rc == 0, (what, downscale.last_error())
                torch.cuda.synchronize()
                for a in (ain, aout):
                    stray = a.check()
                    assert not stray, f"{what}: bytes outside the caller's buffers changed: {stray[:6]}"
                same(what + " lr", dlr, lr)
                same(what + " q0", dq, q)
                same(what + " x", dx, x)
                same(what + " img untouched", dimg, img)
                after = downscale.instances()
                assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}, what
                seen["img"].add(io), seen["lr"].add(lo), seen["q0"].add(qo), seen["x"].add(xo)
    assert seen["img"] == seen["lr"] == seen["q0"] == set(OFFS) and seen["x"] == set(X_OFFS), seen
    assert Ch == x.shape[1]


# ------------------------------------------------------------------------------------------------------------------- large
def test_hr_input_crossing_four_gib():
    """One batch whose HR input crosses 2^32 bytes: the frames are tiled on the device from three distinct small frames (four tiles by
    sixteen), every output compared on the device against a gather of the oracle's run of those three."""
    import torch
    r, H, W = 4, 512, 512
    per = H * W * 3
    N = (1 << 32) // per + 2
    assert N * per > 1 << 32 and (N - 1) * per > 1 << 32          # the last frame lies wholly behind 2^32
    rng = np.random.default_rng(4096)
    img3 = _image(rng, (3, H, W, 3), "random")
    lr3, x3, q3 = DO.decode(img3, r, "y", "rgb", *DOMAIN)
    img = torch.empty((N, H, W, 3), dtype=torch.uint8, device=device())
    for k in range(3):
        img[k::3] = _t(img3[k])
    assert img.numel() > 1 << 32
    got = _run(img, r, "y", "rgb", ("lr", "q0", "x"))
    torch.cuda.synchronize()
    for k in range(3):
        assert bool((got["lr"][k::3] == _t(lr3[k])).all()), f"lr frames {k} mod 3 differ"
        assert bool((got["q0"][k::3] == _t(q3[k])).all()), f"q0 frames {k} mod 3 differ"
        assert bool((got["x"][k::3].view(torch.int32) == _t(x3[k]).view(torch.int32)).all()), f"x frames {k} mod 3 differ"
    same("last frame", got["lr"][N - 1], lr3[(N - 1) % 3])


# ------------------------------------------------------------------------------------------------------------------- engine
def _engine(net="sesr_x4", **kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(os.path.join(IMG, net + ".npz")), device(), **kw)


def _hr(seed, H, W):
    """A smooth-plus-noise HR image: structure for the net to work on."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([127 + 100 * np.sin(xx / 7. + yy / 11.), 127 + 100 * np.cos(xx / 5. - yy / 9.), (xx + yy) / (H + W) * 255], -1)
    return (base + rng.normal(0, 12, base.shape)).clip(0, 255).astype(np.uint8)


@pytest.mark.parametrize("net,kw", [("sesr_x4", {}), ("sesr_x2_rand", {"anchor_add": True}), ("sesr_x2_rand", {}),
                                    ("sesr_x4", {"reciprocal_division": True})])
def test_forward_hr_equals_forward_image_of_the_oracles_lr(net, kw):
    import torch
    e = _engine(net, **kw)
    r = e.bundle.pixel_shuffle
    side = torch.cuda.Stream(device=device())
    for order in ("rgb", "bgr"):
        hr = np.stack([_hr(1, 96, 144), _hr(2, 96, 144)])
        lr = DO.downscale(hr, r)
        q_w, y_w = e.forward_image(_t(lr), order=order)
        q, y = e.forward_hr(_t(hr), order=order)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (2, e.bundle.out_channels, 96, 144)
        same(f"forward_hr {net} {kw} {order} q", q, q_w)
        same(f"forward_hr {net} {kw} {order} y", y, y_w)
        out_q, out_f = torch.full_like(q, 0x5A), torch.full_like(y, float("nan"))
        x = (_t(hr[0].astype(np.int32)) * 1).to(torch.uint8)      # produced on the current stream just before the call
        q1, y1 = e.forward_hr(x, order=order, out_q=out_q[:1], out_f=out_f[:1], stream=side, slot=1)
        side.synchronize()
        assert q1.data_ptr() == out_q.data_ptr() and y1.data_ptr() == out_f.data_ptr()
        same("side stream, caller outputs q", q1, q_w[:1])
        same("side stream, caller outputs y", y1, y_w[:1])
        only_q = e.forward_hr(_t(hr), order=order, want_f=False)
        assert only_q[1] is None
        same("int8 alone", only_q[0], q_w)


def test_forward_hr_refusals():
    import torch
    from sesrq import _lib, downscale
    e = _engine()
    hr = _t(_hr(3, 48, 64))
    torch.cuda.synchronize()
    launches = sum(downscale.instances().values()) + sum(_lib.instances().values())
    shp = (1, 1, 48, 64)
    for bad in (torch.empty((1, 1, 47, 64), dtype=torch.int8, device=device()), torch.empty(shp, dtype=torch.uint8, device=device()),
                torch.empty((1, 1, 48, 128), dtype=torch.int8, device=device())[..., ::2], torch.empty(shp, dtype=torch.int8)):
        with pytest.raises(ValueError, match="every int8 output must be a contiguous tensor"):
            e.forward_hr(hr, out_q=bad)
    with pytest.raises(ValueError, match="every fp32 output must be a contiguous tensor"):
        e.forward_hr(hr, out_f=torch.empty(shp, dtype=torch.float64, device=device()))
    with pytest.raises(ValueError, match="modcrop"):
        e.forward_hr(hr[:46])
    with pytest.raises(ValueError, match="order"):
        e.forward_hr(hr, order="rbg")
    with pytest.raises(ValueError, match="uint8"):
        e.forward_hr(hr.to(torch.int16))
    with pytest.raises(ValueError, match="expected"):
        e.forward_hr(hr.cpu())
    with pytest.raises(ValueError, match="int8 output, the fp32 output or both"):
        e.forward_hr(hr, want_q=False, want_f=False)
    with pytest.raises(ValueError, match="2 or 4"):
        downscale.downscale(hr, 3)
    with pytest.raises(ValueError, match="out must be a contiguous uint8 tensor of the output shape"):
        downscale.downscale(hr, 4, out=torch.empty((1, 12, 16, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="takes 1"):
        downscale.decode(e, hr, 4, "rgb")
    torch.cuda.synchronize()
    assert sum(downscale.instances().values()) + sum(_lib.instances().values()) == launches, "a refused call launched a kernel"
    out = torch.full((1, 12, 16, 3), 0x5A, dtype=torch.uint8, device=device())
    assert downscale.downscale(hr, 4, out=out) is out
    same("downscale into a caller's out", out, DO.downscale(hr.cpu().numpy(), 4))
    q0, x = downscale.decode(e, hr, 4, "y", want_f=True)
    _, xw, qw = DO.decode(hr.cpu().numpy(), 4, "y", "rgb", e.bundle.scale[0], e.bundle.zero[0])
    same("decode q0", q0, qw)
    same("decode x", x, xw)


@pytest.mark.parametrize("mflag,net,kw", [(5, "sesr_x4", {}), (6, "sesr_x2_rand", {"anchor_add": True})])
def test_evaluate_hr_equals_evaluate_image_of_the_oracles_lr(mflag, net, kw):
    from sesrq import quality
    e = _engine(net, **kw)
    r = e.bundle.pixel_shuffle
    hrs = [_hr(10 + k, 96, 120 + 24 * k) for k in range(3)]
    for order in ("rgb", "bgr"):
        got = quality.evaluate_hr(e, hrs, mflag, order=order)
        want = quality.evaluate_image(e, [DO.downscale(h, r)[0] for h in hrs], hrs, mflag, order=order)
        assert got.shape == (3, 3) and np.array_equal(got, want), (got, want)
    assert np.isfinite(got).all() and (got[:, 1] > 5).all()
    with pytest.raises(ValueError, match="upscales by"):
        quality.evaluate_hr(e, hrs, 11 - mflag)


@pytest.mark.parametrize("case", ["sesr_x4", "sesr_x2_rand"])
def test_enqueue_hr_gives_the_records_of_enqueue_image_on_the_oracles_lr(case):
    import torch
    from sesrq.calibrate import Calibrator
    Wf, bf, r = calib_params(case)
    a, b = Calibrator(Wf, bf, r, device()), Calibrator(Wf, bf, r, device())
    for k in range(3):
        hr = _hr(20 + k, 48, 72)
        order = ("rgb", "bgr")[k % 2]
        src = hr if order == "rgb" else _bgr(hr)
        ya = a.enqueue_hr(_t(src), order=order)
        xa = a.last_input.clone()
        yb = b.enqueue_image(_t(DO.downscale(src, r)[0]), order=order)
        torch.cuda.synchronize()
        same(f"{case} frame {k} input", xa, b.last_input)
        same(f"{case} frame {k} mode-0 output", ya, yb)
    a.sync(), b.sync()
    assert a.run_min == b.run_min and a.run_max == b.run_max and a.last_scale == b.last_scale and a.last_zero == b.last_zero
    assert a.finalize() == b.finalize()
    with pytest.raises(ValueError, match="modcrop"):
        a.enqueue_hr(_t(_hr(1, 48, 72))[:, :71])


def test_sim_hr_line_and_save_lr(capsys, tmp_path):
    pytest.importorskip("PIL")
    import sim
    from sesrq import image
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "sesr_x4.params.npz")
    hr = _hr(5, 50, 64)                                        # no multiple of 12: --modcrop keeps 48 x 60
    crop = np.ascontiguousarray(hr[:48, :60])
    lr = DO.downscale(crop, 4)[0]
    image.save_png(str(tmp_path / "hr.png"), hr)
    image.save_png(str(tmp_path / "crop.png"), crop)
    image.save_png(str(tmp_path / "lr.png"), lr)
    STORE.clear()
    y = sim.main(["--mflag", "5", "--params", params, "--hr", str(tmp_path / "hr.png"), "--save-lr", str(tmp_path / "made.png"),
                  "--colour", "--save-png", str(tmp_path / "sr.png")])
    lines = capsys.readouterr().out.strip().split("\n")
    STORE.clear()
    y_w = sim.main(["--mflag", "5", "--params", params, "--input", str(tmp_path / "lr.png"), "--gt", str(tmp_path / "crop.png"),
                    "--colour", "--save-png", str(tmp_path / "sr_w.png")])
    lines_w = capsys.readouterr().out.strip().split("\n")
    same("sim.py --hr output", y, y_w)
    mean = [l for l in lines if "mean psnr is" in l]
    assert len(mean) == 1 and mean == [l for l in lines_w if "mean psnr is" in l], (lines, lines_w)
    assert any(l.startswith("lr:") for l in lines) and not any(l.startswith("lr:") for l in lines_w)
    assert np.array_equal(image.load_image(str(tmp_path / "made.png")), lr)
    assert np.array_equal(image.load_image(str(tmp_path / "sr.png")), image.load_image(str(tmp_path / "sr_w.png")))
    for bad, msg in ((["--hr", str(tmp_path / "hr.png"), "--no-modcrop"], "modcrop"),
                     (["--hr", str(tmp_path / "hr.png"), "--input", str(tmp_path / "lr.png")], "neither --input nor --gt"),
                     (["--input", str(tmp_path / "lr.png"), "--save-lr", str(tmp_path / "no.png")], "--save-lr")):
        STORE.clear()
        with pytest.raises(SystemExit, match=msg):
            sim.main(["--mflag", "5", "--params", params] + bad)
    with pytest.raises(SystemExit, match="--mflag 5 or 6"):
        sim.main(["--mflag", "3", "--params", params, "--hr", str(tmp_path / "hr.png")])
    assert not os.path.exists(str(tmp_path / "no.png"))


def test_test_py_hr_equals_input_and_gt_of_the_oracles_lr(capsys, tmp_path):
    """test.py --hr: the lines and the calibrated domains of test.py --input <oracle LR> --gt <cropped HR>."""
    pytest.importorskip("PIL")
    from calib_cases import load_test_py
    from sesrq import image
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "sesr_x4.params.npz")
    hrs, crops, lrs = [], [], []
    for k in range(2):
        hr = _hr(30 + k, 50 + 12 * k, 64)
        crop = np.ascontiguousarray(hr[:48 + 12 * k, :60])
        for name, a, to in (("hr", hr, hrs), ("crop", crop, crops), ("lr", DO.downscale(crop, 4)[0], lrs)):
            image.save_png(str(tmp_path / f"{name}{k}.png"), a)
            to.append(str(tmp_path / f"{name}{k}.png"))
    mod = load_test_py()
    STORE.clear()
    got = mod.main(["--mflag", "5", "--params", params, "--hr", *hrs])
    lines = capsys.readouterr().out
    STORE.clear()
    want = mod.main(["--mflag", "5", "--params", params, "--input", *lrs, "--gt", *crops])
    assert got == want and lines == capsys.readouterr().out and "mean psnr is" in lines
    STORE.clear()


def test_size_refusals_through_the_c_abi():
    c_abi_refusals()


def test_zz_every_downscale_instance_ran():
    """LAST in this file: every kernel instantiation libsesrq_downscale.so can launch was launched by a checked case above."""
    from sesrq import downscale
    k = downscale.instances()
    assert sorted(k) == sorted(f"downscale<r{r},{f}>" for r in (2, 4) for f in ("lr", "Y", "RGB")), k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
