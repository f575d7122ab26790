"""SR video inputs from the HR clip alone (sesrq.video_hr, libsesrq_video_hr.so, Engine.forward_video_hr / forward_video_rgb_hr,
quality.evaluate_video_hr, sim.py --hr-yuv) against tests/video_hr_oracle.py, which only slices planes into downscale_oracle and
video_oracle.  Every byte and every fp32 word is compared for equality; frames are small and sit on the kernel's tile seams."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import Arena, device, same, stream_ptr

import downscale_oracle as DO
import video_hr_oracle as HO
import video_oracle as VO
from test_video import CANARY, FMTS, PAIRS, Laid, _domains, _engine, _same_frames

gpu = pytest.mark.gpu
LUMA = {(False, False): "none", (True, False): "q0", (False, True): "x", (True, True): "q0,x"}


# ------------------------------------------------------------------------------------------------------------------- no device
@pytest.mark.parametrize("r", [2, 4])
def test_oracle_is_the_image_oracle_per_plane_and_the_video_decode(r):
    rng = np.random.default_rng(r)
    hr = VO.random_frames(rng, 2, 6 * r, 10 * r)
    s0, z0, ed = 0.0047, -119, 0
    lr, q0, x = HO.run(hr, r, s0, z0, ed)
    same("luma", lr["y"], DO.downscale(np.repeat(hr["y"][..., None], 3, -1), r)[..., 1])
    assert lr["cb"].shape == (2, 3, 5) and np.array_equal(lr["cr"], HO.plane(hr["cr"], r))
    wq, wx = VO.decode(lr["y"], s0, z0, ed)
    same("q0", q0, wq)
    same("x", x, wx)


def test_weights_are_the_downscale_librarys():
    from sesrq import downscale, video_hr
    for r in (2, 4):
        (w, D), (dw, dD) = video_hr.weights(r), downscale.weights(r)
        assert D == dD == DO.D[r] and np.array_equal(w, dw) and tuple(w) == DO.WEIGHTS[r]
    with pytest.raises(ValueError, match="r = 3"):
        video_hr.weights(3)


def test_refusals_through_the_c_abi_without_a_device():
    """Pointers that are never dereferenced: every refusal comes before any HIP call."""
    from sesrq import video, video_hr
    fake = 4096

    def surf(fmt, W, H, N=1, **kw):
        hc, cb = H // 2, (W if fmt == video.NV12 else W // 2)
        d = dict(format=fmt, y=fake, c0=fake, c1=fake, pitch_y=W, pitch_c=cb, frame_y=H * W, frame_c=hc * cb)
        d.update(kw)
        return video.SurfaceDesc(*[d[k] for k, _ in video.SurfaceDesc._fields_])

    def call(r=4, H=4, W=8, N=1, hr=None, lr=None, want_lr=True, x=None):
        hr = hr or surf(video.NV12, r * W, r * H, N)
        lr = lr or surf(video.I420, W, H, N)
        return video_hr.lib().sesrq_video_hr_run(None, C.byref(hr), r, C.byref(lr) if want_lr else None, None, x, N, H, W, None)

    for kw, msg in ((dict(H=5), "modcrop"), (dict(W=7), "modcrop"), (dict(r=2, H=3), "modcrop"),
                    (dict(hr=surf(video.NV12, 32, 16, pitch_y=31)), "pitch_y 31 of hr"), (dict(lr=surf(video.I420, 8, 4, pitch_c=3)), "pitch_c 3 of lr"),
                    (dict(hr=surf(video.NV12, 32, 16, pitch_c=30)), "pitch_c 30 of hr"), (dict(want_lr=False), "none of lr, q0 and x"),
                    (dict(want_lr=False, x=fake), "ctx is NULL"), (dict(N=2, lr=surf(video.I420, 8, 4, 2, frame_y=31)), "below its plane's extent"),
                    (dict(N=2, lr=surf(video.NV12, 8, 4, 2, frame_c=15)), "below its plane's extent"), (dict(r=3), "r = 3"),
                    (dict(hr=surf(7, 32, 16)), "hr format 7"), (dict(lr=surf(video.I420, 8, 4, c1=None)), "chroma plane of lr")):
        assert call(**kw) != 0 and msg in video_hr.last_error(), (kw, msg, video_hr.last_error())
    with pytest.raises(ValueError, match="modcrop"):
        video_hr.lr_size(video.Surface.alloc("nv12", 1, 20, 16), 4)
    host = video.Surface.alloc("i420", 2, 21, 19)
    crop = video_hr.modcrop(host, 4)
    assert (crop.N, crop.H, crop.W) == (2, 16, 16) and crop.c1.shape == (2, 8, 8) and video_hr.modcrop((21, 19), 2) == (20, 16)


# ------------------------------------------------------------------------------------------------------------------- device
def _run(hr_fr, r, pair, q=True, f=True, lr_y=True, want_lr=True, padded=False, domain=None, arena=None, offs=(0, 0, 0), qx=(0, 0)):
    """One launch through the C ABI -> nothing; every output, every padding byte and the launched instantiation are checked."""
    import torch
    from sesrq import video_hr
    N, HH, WW = hr_fr["y"].shape
    H, W = HH // r, WW // r
    s0, z0, ed = domain or _domains()[0]
    lr_w, wq, wx = HO.run(hr_fr, r, s0, z0, ed)
    ain, aout = arena or (None, None)
    hr = Laid(pair[0], N, HH, WW, pads=(3, 1) if padded else (0, 0), gap=5 if padded else 0, arena=ain, offs=offs).fill(hr_fr)
    lr = Laid(pair[1], N, H, W, pads=(5, 3) if padded else (0, 0), gap=11 if padded and N > 1 else 0, arena=aout,
              offs=offs[::-1]) if want_lr else None
    mk = (lambda dt, o, v: aout.place((N, 1, H, W), dt, o)) if arena else (lambda dt, o, v: torch.full((N, 1, H, W), v, dtype=dt, device=device()))
    q0 = mk(torch.int8, qx[0], 0x5A) if q else None
    x = mk(torch.float32, qx[1], float("nan")) if f else None
    dh, dl = hr.s.desc(), lr.s.desc() if lr else None
    if lr and not lr_y:
        dl.y = None
    h = video_hr._so.context(device(), s0, z0, ed) if q or f else None
    before = video_hr.instances()
    rc = video_hr.lib().sesrq_video_hr_run(h, C.byref(dh), r, C.byref(dl) if lr else None, q0.data_ptr() if q else None,
                                           x.data_ptr() if f else None, N, H, W, stream_ptr())
    assert rc == 0, video_hr.last_error()
    torch.cuda.synchronize()
    after = video_hr.instances()
    name = f"video_hr<r{r},{pair[0]}->{pair[1] if lr else 'none'},{LUMA[(q, f)]}>"
    what = f"{name} N={N} {H}x{W} padded={padded} lr_y={lr_y}"
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}, what
    if lr:
        got = lr.frames()
        if not lr_y:
            assert bool((lr.flat[0] == CANARY).all()), what + ": an absent lr->y was written"
            got["y"] = lr_w["y"]
        _same_frames(what, got, lr_w)
        assert lr.padding_intact(), what + ": a padding byte of lr was written"
    if q:
        same(what + " q0", q0, wq)
    if f:
        same(what + " x", x, wx)
    _same_frames(what + " hr untouched", hr.frames(), hr_fr)
    assert hr.padding_intact()
    for a in arena or ():
        assert not a.check(), f"{what}: bytes outside the caller's buffers changed: {a.check()[:4]}"


def _sizes(r):
    """Per axis: the smallest legal LR size, one tile, one tile -+ 2 and two tiles + 2, the other axis small."""
    tw, th = HO.tile(r)
    return [(4, w) for w in (2, tw - 2, tw, tw + 2, 2 * tw + 2)] + [(h, 6) for h in (2, th - 2, th, th + 2, 2 * th + 2)] + [(2, 2)]


@gpu
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("r", [2, 4])
def test_sizes_on_the_tile_seams_through_exact_and_padded_pitches(r, pair):
    rng = np.random.default_rng(10 * r + PAIRS.index(pair))
    for i, (H, W) in enumerate(_sizes(r)):
        for N in (1, 3):
            _run(VO.random_frames(rng, N, r * H, r * W), r, pair, padded=(i + N) % 2 == 0, domain=_domains()[i % 3])


@gpu
@pytest.mark.parametrize("r", [2, 4])
def test_every_output_set_launches_its_instantiation(r):
    rng = np.random.default_rng(r + 50)
    tw, th = HO.tile(r)
    hr = VO.random_frames(rng, 2, r * (th + 2), r * (tw + 2))
    for i, (q, f, want_lr, lr_y) in enumerate(((True, False, False, True), (False, True, False, True), (False, False, True, True),
                                               (False, False, True, False), (True, False, True, False), (False, True, True, False),
                                               (True, True, True, True), (True, True, False, True))):
        for pair in (PAIRS[i % 4], PAIRS[(i + 1) % 4]):
            _run(hr, r, pair, q=q, f=f, want_lr=want_lr, lr_y=lr_y, padded=i % 2 == 1)


def _fires(p, r):
    """Both clamps of both passes fire somewhere in the planes p (N, H, W)."""
    sv, v = DO.one_pass(p, r, 1, sums=True), DO.one_pass(p, r, 1)
    for s in (sv, DO.one_pass(v, r, 2, sums=True)):
        u = (s + DO.D[r] // 2) // DO.D[r]
        if not ((u < 0).any() and (u > 255).any()):
            return False
    return True


@gpu
@pytest.mark.parametrize("r", [2, 4])
def test_both_clamps_of_both_passes_fire_in_every_plane(r):
    rng = np.random.default_rng(r + 60)
    H = W = 16
    fr = VO.random_frames(rng, 3, r * H, r * W, "extreme")
    for k, p in fr.items():
        n = p.shape[1]
        hi, lo = DO.clamp_pattern(n, r, 2, True), DO.clamp_pattern(n, r, 2, False)
        p[0, :, :n // 2], p[0, :, n // 2:] = hi[:, None], lo[:, None]            # rows: the vertical pass
        p[1, :n // 2], p[1, n // 2:] = hi[None, :], lo[None, :]                  # columns: the horizontal pass
        assert _fires(p[:2], r), k
    for pair in PAIRS:
        _run(fr, r, pair)


@gpu
@pytest.mark.parametrize("r", [2, 4])
def test_neighbouring_tiles_of_opposite_extremes(r):
    tw, th = HO.tile(r)
    H, W = 2 * th, 2 * tw + 2
    fr = {}
    for k, (hh, ww, tth, ttw) in {"y": (r * H, r * W, r * th, r * tw), "cb": (r * H // 2, r * W // 2, r * th // 2, r * tw // 2)}.items():
        yy, xx = np.meshgrid(np.arange(hh) // tth, np.arange(ww) // ttw, indexing="ij")
        fr[k] = np.stack([((yy + xx + n) % 2 * 255).astype(np.uint8) for n in range(2)])
    fr["cr"] = 255 - fr["cb"]
    for pair in (PAIRS[1], PAIRS[2]):
        _run(fr, r, pair, padded=True)


@gpu
@pytest.mark.parametrize("r", [2, 4])
def test_caller_buffers_at_odd_addresses_in_canary_arenas(r):
    """Every plane and q0 at odd addresses, x at 4 mod 16, every other byte of the arenas a canary.  W = 32 has whole 16-byte runs
    (taken as such only at offset 0), W = 14 none."""
    from sesrq import video
    rng = np.random.default_rng(r + 70)
    for i, (H, W) in enumerate(((4, 32), (6, 14))):
        hr = VO.random_frames(rng, 2, r * H, r * W)
        for j, (offs, qx) in enumerate((((0, 0, 0), (0, 0)), ((1, 3, 5), (7, 4)), ((3, 1, 7), (1, 20)), ((2, 6, 9), (13, 12)))):
            pair = PAIRS[(i + j) % 4]
            room = lambda fmt, h, w: [2 * (rows + 1) * (nb + 16) + 64 for rows, nb in video.plane_shapes(fmt, h, w)]
            ain = Arena(device(), Arena.room(*room(pair[0], r * H, r * W)), CANARY)
            aout = Arena(device(), Arena.room(*room(pair[1], H, W), 2 * H * W, 8 * H * W), CANARY)
            _run(hr, r, pair, padded=True, arena=(ain, aout), offs=offs, qx=qx)


# ------------------------------------------------------------------------------------------------------------------- routes
def _hr_surfaces(r, fmt, N=2, H=8, W=12, seed=5):
    from sesrq import video
    fr = VO.random_frames(np.random.default_rng(seed), N, r * H, r * W)
    lr = HO.downscale(fr, r)
    host = lambda f, h, w: video.Surface.views(np.frombuffer(bytearray(VO.pack(f, fmt)), np.uint8), fmt, N, h, w)
    return host(fr, r * H, r * W), host(lr, H, W)


@gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_forward_video_hr_equals_forward_video_on_the_oracles_lr_surface(fmt):
    import torch
    from sesrq import video
    hr, lr = (video.to_device(s, device()) for s in _hr_surfaces(4, fmt))
    for e in (_engine(), _engine(anchor_add=True)):
        want, wl = e.forward_video(lr, want_q=True)
        got, gl = e.forward_video_hr(hr, want_q=True)
        torch.cuda.synchronize()
        assert (got.N, got.H, got.W) == (hr.N, hr.H, hr.W) and torch.equal(gl, wl) and got.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="modcrop"):
        e.forward_video_hr(video.to_device(video.Surface.alloc(fmt, 1, 36, 32), device()))
    with pytest.raises(ValueError, match="luma net"):
        _engine("sesr_x2_rand", anchor_add=True).forward_video_hr(hr)


@gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_forward_video_rgb_hr_equals_forward_video_rgb_on_the_oracles_lr_surface(fmt):
    import torch
    from sesrq import video
    hr, lr = (video.to_device(s, device()) for s in _hr_surfaces(2, fmt))
    e = _engine("sesr_x2_rand", anchor_add=True)
    want, wp = e.forward_video_rgb(lr, want_q=True)
    got, gp = e.forward_video_rgb_hr(hr, want_q=True)
    torch.cuda.synchronize()
    assert torch.equal(gp, wp) and got.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="RGB net"):
        _engine().forward_video_rgb_hr(hr)


@gpu
def test_evaluate_video_hr_equals_the_siblings_on_the_pair():
    from sesrq import quality
    for mflag, r, e in ((5, 4, _engine()), (6, 2, _engine("sesr_x2_rand", anchor_add=True))):
        hr, lr = _hr_surfaces(r, FMTS[mflag % 2], N=3)
        hrs, lrs = [hr[n:n + 1] for n in range(3)], [lr[n:n + 1] for n in range(3)]
        want = (quality.evaluate_video if mflag == 5 else quality.evaluate_video_rgb)(e, lrs, hrs)
        got = quality.evaluate_video_hr(e, hrs, mflag)
        assert got.shape == (3, 3) and np.array_equal(got, want), mflag
    with pytest.raises(ValueError, match="MFLAG 3"):
        quality.evaluate_video_hr(e, hrs, 3)


@gpu
def test_sim_hr_yuv_writes_the_oracles_lr_file_and_prints_the_pairs_scores(capsys, tmp_path):
    import sim
    from sesrq.store import STORE
    hr, lr = _hr_surfaces(4, "nv12", N=2, H=6, W=10, seed=9)
    (tmp_path / "hr.yuv").write_bytes(hr.tobytes())
    (tmp_path / "lr.yuv").write_bytes(lr.tobytes())
    base = ["--mflag", "5", "--params", os.path.join(GOLDEN, "sesr_x4.params.npz"), "--pix-fmt", "nv12"]
    STORE.clear()
    y = sim.main(base + ["--hr-yuv", str(tmp_path / "hr.yuv"), "--size", "40x24", "--save-lr-yuv", str(tmp_path / "made.yuv")])
    got = [l for l in capsys.readouterr().out.strip().split("\n") if "psnr" in l or l.replace(".", "").isdigit()]
    assert (tmp_path / "made.yuv").read_bytes() == lr.tobytes(), "the written LR file differs from the oracle's bytes"
    STORE.clear()
    y2 = sim.main(base + ["--yuv", str(tmp_path / "lr.yuv"), "--size", "10x6", "--gt-yuv", str(tmp_path / "hr.yuv")])
    want = [l for l in capsys.readouterr().out.strip().split("\n") if "psnr" in l or l.replace(".", "").isdigit()]
    assert len(got) == 3 and got == want and np.array_equal(y.cpu().numpy(), y2.cpu().numpy())
    for beside in (["--yuv", str(tmp_path / "lr.yuv")], ["--gt-yuv", str(tmp_path / "hr.yuv")], ["--input", "x.npy"], ["--hr", "x.png"]):
        STORE.clear()
        with pytest.raises(SystemExit, match="--hr-yuv"):
            sim.main(base + ["--hr-yuv", str(tmp_path / "hr.yuv"), "--size", "40x24"] + beside)
