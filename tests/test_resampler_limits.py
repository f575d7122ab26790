"""The three bicubic resamplers at their frame limits: video_decode's grid-stride loop beyond its second trip, and downscale<r,form>,
colour_export<yd,r> and video_export<yd,r,fmt> on strip frames -- one row or one column of four million pixels, where tiles_x or
tiles_y is in the hundreds of thousands and n, tx, ty come out of blockIdx.x by division.  Every comparison is exact and covers
every byte and every fp32 word.

  loop             video_decode<q0 | x | q0,x> on frames of more than two rounds of items (a round is compute units x 16 x 128, read
                   from the device) at W = 33: two whole runs and a one-pixel run a row, three runs a row against a stride that is no
                   multiple of 3, so a lane's successive items change between the 16-byte and the per-pixel path; N = 1 and 3,
                   Y pitches 33 and 48; every element against VO.decode.  A batch that wraps equals its single frames, none of which
                   wraps.
  strips           r = 2 and 4; one LR row of 2^22 + 5 pixels (the last tile and the last 16-byte run are partial), one LR column of
                   2^22 + 5 rows one and two pixels wide; the downscale's HR strip is r times that.  The frames are periodic
                   (tests/geometry.py, P = 61 on the LR axis -- for video on the chroma axis, which is half the luma axis --, r P
                   on the HR axis); the oracle runs on the small_len axis and every output element is compared on the device through
                   the map.  The map holds: the upscalers reach 2 LR samples with clamped edges, the downscale under 3 LR pixels with
                   mirrored edges, both inside geometry.R = 7.  Video's luma is pointwise (tiled).  Colour and video take int8 luma on
                   the row and the two-pixel column and fp32 luma on the one-pixel column; video writes NV12 on the row and I420 on
                   the columns (from the other format).

Every case asserts its own precondition, checks the launch counters, and prints one "RESAMPLER|" line with its shape and seconds:
profiles/resampler_limits.txt is made of them.  No size refusal is added: the existing files cover them."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import colour_oracle as CO
import downscale_oracle as DO
import geometry as G
import video_oracle as VO
from helpers import device, stream_ptr

F32 = np.float32
P = G.P
BIG = (1 << 22) + 5
STRIPS = {"row": (1, BIG), "column": (BIG, 1), "column2": (BIG, 2)}          # LR (H, W)
IN_DOMAIN = (0.0039, -128)
OUT_DOMAIN = (0.0047, -119)
CANARY = 0x5A
SEG = 16


def _report(what, **kw):
    print("RESAMPLER| " + what + " | " + " | ".join(f"{k}={v}" for k, v in kw.items()), flush=True)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


def _room(need):
    import torch
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(device())[0]
    if free < need:
        pytest.skip(f"{need / 2 ** 20:.0f} MiB of device memory needed, {free / 2 ** 20:.0f} MiB free")


def _assert_same(what, got, expect):
    bad, first = G.compare_all(got, expect)
    assert bad == 0, f"{what}: {bad} of {got.numel()} differ, first at (n, c, y, x) = {first[0]}: got {first[1]} want {first[2]}"


def _delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _small(pat, hs, ws):
    """The periodic frame of hs x ws on the host from a (F, C, PY, PX) tile."""
    return np.ascontiguousarray(pat[:, :, np.arange(hs) % pat.shape[2]][:, :, :, np.arange(ws) % pat.shape[3]])


def _nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def _nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def _luma_tile(rng, dtype, side):
    if dtype == "i8":
        return rng.integers(-128, 128, (1, 1, side, side)).astype(np.int8)
    return (rng.random((1, 1, side, side)) * 1.3 - 0.15).astype(F32)


def _strip_facts(H, W, r, tile):
    """(tiles, the strip's long axis in LR pixels): asserts that the grid is a strip of many tiles whose last one is partial."""
    tw, th = tile
    tx, ty = -(-W // tw), -(-H // th)
    long, t = (W, tw) if W > H else (H, th)
    assert min(tx, ty) == 1 and tx * ty > 60000 and long % t != 0 and long > 1 << 22
    return tx * ty


# ===================================================================================================================== the loop
@pytest.mark.gpu
@pytest.mark.parametrize("pitch", [33, 48])
@pytest.mark.parametrize("N", [1, 3])
def test_video_decode_loop_takes_a_third_trip(N, pitch):
    import torch
    from sesrq import video
    t0 = time.time()
    W, segs = 33, 3
    cus = torch.cuda.get_device_properties(device()).multi_processor_count
    round_ = cus * 16 * 128                                                  # items of one trip of the whole grid
    H = (26 * round_ // (10 * segs * N)) | 1                                 # 2.6 rounds; a frame of three is 0.87 of one
    items = N * H * segs
    assert 2 * round_ + round_ // 2 < items < 3 * round_                    # a third trip of more than half the grid, and a partial one
    assert H * segs < round_ or N == 1                                       # a single frame of the batch does not wrap
    assert math.gcd(segs, round_) == 1                                       # a lane's successive items are different runs of a row
    assert W % SEG == 1 and pitch >= W
    _room(N * H * (pitch + 2 * W + 8 * W) + (1 << 28))
    s0, z0 = IN_DOMAIN
    y = np.random.default_rng(pitch + N).integers(0, 256, (N, H, W)).astype(np.uint8)
    y[0, 0, :] = np.arange(W)
    y.reshape(-1)[W:W + 256] = np.arange(256)                                # every code
    wq, wx = VO.decode(y, s0, z0, 0)
    wq, wx = _t(np.asarray(wq).astype(np.int8)), _t(wx).view(torch.int32)
    flat = torch.full((N * H * pitch + 16,), CANARY, dtype=torch.uint8, device=device())
    assert flat.data_ptr() % 16 == 0
    src = flat.as_strided((N, H, W), (H * pitch, pitch, 1))
    src.copy_(_t(y))
    h = video._so.context(device(), s0, z0, 0)

    def run(outs, n0, n1):
        q0 = torch.full((n1 - n0, 1, H, W), CANARY, dtype=torch.int8, device=device()) if "q0" in outs else None
        x = torch.full((n1 - n0, 1, H, W), float("nan"), device=device()) if "x" in outs else None
        d = video.SurfaceDesc(video.NV12, src[n0:n1].data_ptr(), None, None, pitch, 0, H * pitch, 0)      # chroma is not looked at
        before = video.instances()
        rc = video.lib().sesrq_video_decode(h, C.byref(d), q0.data_ptr() if q0 is not None else None,
                                            x.data_ptr() if x is not None else None, n1 - n0, H, W, stream_ptr())
        assert rc == 0, video.last_error()
        torch.cuda.synchronize()
        assert _delta(before, video.instances()) == {f"video_decode<{outs}>": 1}
        return q0, x

    for outs in ("q0", "x", "q0,x"):
        q0, x = run(outs, 0, N)
        if q0 is not None:
            bad = int(torch.count_nonzero(q0 != wq))
            assert bad == 0, f"video_decode<{outs}> N={N} pitch {pitch}: {bad} of {q0.numel()} q0 differ from the oracle"
        if x is not None:
            bad = int(torch.count_nonzero(x.view(torch.int32) != wx))
            assert bad == 0, f"video_decode<{outs}> N={N} pitch {pitch}: {bad} of {x.numel()} x differ from the oracle"
    if N > 1:                                                                # q0, x: the batch that wraps against its frames, which do not
        for n in range(N):
            q1, x1 = run("q0,x", n, n + 1)
            assert torch.equal(q1[0], q0[n]) and torch.equal(x1[0].view(torch.int32), x[n].view(torch.int32)), n
    assert bool((flat.as_strided((N * H, pitch - W), (pitch, 1), W) == CANARY).all()) or pitch == W, "the source's padding was written"
    _report("video_decode loop", shape=f"{N}x{H}x{W}", pitch=pitch, items=items, round=round_, trips=f"{items / round_:.3f}",
            launches=3 + (N if N > 1 else 0), seconds=f"{time.time() - t0:.2f}")


# ===================================================================================================================== strips
def test_the_strip_maps_hold_on_the_oracles():
    """No device: on an axis long enough to take the map (over 4 P) the oracle's output of the periodic frame is the gather of its output
    of the small frame -- for the downscale (mirrored edges, HR period r P), for the upscale of colour and video (clamped edges), and
    for video's chroma planes cropped to r D / 2 of an odd luma size D."""
    rng = np.random.default_rng(7)
    D = 5 * P + 17
    Ds = G.small_len(D)
    assert D > 4 * P and Ds < D
    for r in (2, 4):
        pat = rng.integers(0, 256, (1, 3, r * P, r * P)).astype(np.uint8)
        for H, W in ((1, D), (D, 2)):
            hs, ws = G.small_len(H), G.small_len(W)
            big = DO.downscale(_nhwc(_small(pat, r * H, r * W)), r)
            small = DO.downscale(_nhwc(_small(pat, r * hs, r * ws)), r)
            assert np.array_equal(big, small[:, G.out_map(H, 1)][:, :, G.out_map(W, 1)]), (r, H, W)
            cpat, ypat = pat[:, :, :P, :P], _luma_tile(rng, "i8", r * P)
            big = CO.export(_small(ypat, r * H, r * W), _nhwc(_small(cpat, H, W)), r, scale=OUT_DOMAIN[0], zero=OUT_DOMAIN[1])
            small = CO.export(_small(ypat, r * hs, r * ws), _nhwc(_small(cpat, hs, ws)), r, scale=OUT_DOMAIN[0], zero=OUT_DOMAIN[1])
            assert np.array_equal(big, small[:, G.out_map(H, r)][:, :, G.out_map(W, r)]), (r, H, W)
            Hl, Wl = (1, 2 * D - 1) if H == 1 else (2 * D - 1, 2 * W)            # a luma size whose chroma planes are H x W, odd on the long axis
            assert VO.chroma_size(Hl, Wl) == (H, W)
            big = VO.chroma(_small(cpat[:, :2], H, W)[0], r, Hl, Wl)
            small = VO.chroma_bytes(VO.chroma_q6(_small(cpat[:, :2], hs, ws)[0], r))
            my, mx = G.out_map(H, r)[:r * Hl // 2], G.out_map(W, r)[:r * Wl // 2]
            assert big.shape[1:] == (len(my), len(mx)) and np.array_equal(big, small[:, my][:, :, mx]), (r, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("strip", list(STRIPS))
@pytest.mark.parametrize("r", [2, 4])
def test_downscale_on_a_strip(r, strip):
    import torch
    from sesrq import downscale
    t0 = time.time()
    H, W = STRIPS[strip]
    tiles = _strip_facts(H, W, r, DO.tile(r))
    form = "y" if strip == "row" else "rgb"
    order = "bgr" if strip == "column2" else "rgb"
    Ch = 1 if form == "y" else 3
    hr_bytes = 3 * r * r * H * W
    assert hr_bytes > (1 << 22) * 3 * r * r
    _room(2 * hr_bytes + H * W * (3 + 5 * Ch) * 2 + (1 << 28))
    pat = np.random.default_rng(300 + r).integers(0, 256, (1, 3, r * P, r * P)).astype(np.uint8)      # the HR tile: period r P
    hs, ws = G.small_len(H), G.small_len(W)
    lr_s, x_s, q_s = DO.decode(_nhwc(_small(pat, r * hs, r * ws)), r, form, order, *IN_DOMAIN)
    assert lr_s.shape == (1, hs, ws, 3) and len(np.unique(lr_s)) > 50
    img = G.device_frame(pat, 1, r * H, r * W, device()).permute(0, 2, 3, 1).contiguous()
    lr = torch.full((1, H, W, 3), CANARY, dtype=torch.uint8, device=device())
    q0 = torch.full((1, Ch, H, W), CANARY, dtype=torch.int8, device=device())
    x = torch.full((1, Ch, H, W), float("nan"), dtype=torch.float32, device=device())
    before = downscale.instances()
    downscale.launch(device(), IN_DOMAIN[0], IN_DOMAIN[1], 0, img, order, r, form, lr, q0, x, torch.cuda.current_stream(device()))
    torch.cuda.synchronize()
    name = f"downscale<r{r},{'Y' if form == 'y' else 'RGB'}>"
    assert _delta(before, downscale.instances()) == {name: 1}
    what = f"{name} {order} {strip} LR {H}x{W}"
    _assert_same(what + " lr", lr.permute(0, 3, 1, 2), G.Expect(_nchw(lr_s), H, W, 1, device()))
    _assert_same(what + " q0", q0, G.Expect(q_s, H, W, 1, device()))
    _assert_same(what + " x", x, G.Expect(x_s, H, W, 1, device()))
    del img, lr, q0, x
    torch.cuda.empty_cache()
    _report(f"downscale strip r={r} {strip}", op=f"{form}/{order}", hr=f"1x{r * H}x{r * W}x3", lr=f"{H}x{W}", tiles=tiles,
            hr_bytes=hr_bytes, seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("strip", list(STRIPS))
@pytest.mark.parametrize("r", [2, 4])
def test_colour_export_on_a_strip(r, strip):
    import torch
    from sesrq import colour
    t0 = time.time()
    H, W = STRIPS[strip]
    tiles = _strip_facts(H, W, r, CO.tile(r))
    dtype = "f32" if strip == "column" else "i8"
    order = "bgr" if strip == "column2" else "rgb"
    assert strip != "row" or (r * W) % SEG != 0                              # the last 16-pixel run of the row is partial
    out_bytes = 3 * r * r * H * W
    assert out_bytes > (1 << 22) * 3 * r * r
    _room(out_bytes * 2 + r * r * H * W * (5 if dtype == "f32" else 2) + 6 * H * W + (1 << 28))
    rng = np.random.default_rng(400 + r)
    pat = rng.integers(0, 256, (1, 3, P, P)).astype(np.uint8)
    ypat = _luma_tile(rng, dtype, r * P)
    hs, ws = G.small_len(H), G.small_len(W)
    dom = dict(scale=OUT_DOMAIN[0], zero=OUT_DOMAIN[1]) if dtype == "i8" else {}
    want = CO.export(_small(ypat, r * hs, r * ws), _nhwc(_small(pat, hs, ws)), r, order, scale=dom.get("scale"), zero=dom.get("zero"))
    assert want.shape == (1, r * hs, r * ws, 3) and len(np.unique(want)) > 50
    img = G.device_frame(pat, 1, H, W, device()).permute(0, 2, 3, 1).contiguous()
    y = G.device_frame(ypat, 1, r * H, r * W, device())
    before = colour.instances()
    got = colour.export(y, img, r, order=order, **dom)
    torch.cuda.synchronize()
    name = f"colour_export<{dtype},r{r}>"
    assert _delta(before, colour.instances()) == {name: 1} and tuple(got.shape) == (1, r * H, r * W, 3)
    _assert_same(f"{name} {order} {strip} LR {H}x{W}", got.permute(0, 3, 1, 2), G.Expect(_nchw(want), H, W, r, device()))
    del img, y, got
    torch.cuda.empty_cache()
    _report(f"colour strip r={r} {strip}", op=f"{dtype}/{order}", lr=f"1x{H}x{W}x3", out=f"{r * H}x{r * W}", tiles=tiles,
            out_bytes=out_bytes, seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("strip", list(STRIPS))
@pytest.mark.parametrize("r", [2, 4])
def test_video_export_on_a_strip(r, strip):
    import torch
    from sesrq import video
    t0 = time.time()
    H, W = STRIPS[strip]                                                     # the LR luma; the chroma planes are half of it, rounded up
    tiles = _strip_facts(H, W, r, VO.tile(r))
    dtype = "f32" if strip == "column" else "i8"
    fi, fo = ("i420", "nv12") if strip == "row" else ("nv12", "i420")
    Hc, Wc = VO.chroma_size(H, W)
    cH, cW = r * H // 2, r * W // 2                                          # the HR chroma planes: the top left of r Hc x r Wc
    assert cH >= 1 and cW >= 1 and (cH < r * Hc or cW < r * Wc)              # an odd size: the upscaled plane is cropped
    assert strip != "row" or ((r * W) % SEG != 0 and cW % SEG != 0 and (2 * cW) % SEG != 0)      # partial last runs, luma and chroma
    out_bytes = r * r * H * W + 2 * cH * cW
    _room(out_bytes * 2 + r * r * H * W * (5 if dtype == "f32" else 2) + (1 << 28))
    rng = np.random.default_rng(500 + r)
    cpat = rng.integers(0, 256, (1, 2, P, P)).astype(np.uint8)               # Cb and Cr: period P on the chroma axes
    ypat = _luma_tile(rng, dtype, P)                                         # the luma is pointwise: any period
    dom = dict(scale=OUT_DOMAIN[0], zero=OUT_DOMAIN[1]) if dtype == "i8" else {}
    want_y = VO.luma(ypat, dom.get("scale"), dom.get("zero"))[:, None]       # (1, 1, P, P)
    want_c = VO.chroma_bytes(VO.chroma_q6(_small(cpat, G.small_len(Hc), G.small_len(Wc)), r))        # (1, 2, r Hcs, r Wcs)
    assert len(np.unique(want_c)) > 50 and len(np.unique(want_y)) > 50
    my, mx = G.out_map(Hc, r)[:cH], G.out_map(Wc, r)[:cW]

    chroma = G.device_frame(cpat, 1, Hc, Wc, device())
    lr = video.Surface.alloc(fi, 1, H, W, device())
    lr.buf.fill_(CANARY)
    if fi == "nv12":
        lr.c0.unflatten(2, (Wc, 2)).copy_(chroma.permute(0, 2, 3, 1))
    else:
        lr.c0.copy_(chroma[:, 0])
        lr.c1.copy_(chroma[:, 1])
    y = G.device_frame(ypat, 1, r * H, r * W, device())
    out = video.Surface.alloc(fo, 1, r * H, r * W, device())
    out.buf.fill_(CANARY)
    assert out.buf.numel() == out_bytes
    before = video.instances()
    assert video.export(y, lr, r, out=out, **dom) is out
    torch.cuda.synchronize()
    name = f"video_export<{dtype},r{r},{fo}>"
    assert _delta(before, video.instances()) == {name: 1}
    what = f"{name} from {fi}, {strip} LR {H}x{W}"
    _assert_same(what + " y", out.y[:, None], G.Expect(want_y, r * H, r * W, 1, device(), tiled=True))
    if fo == "nv12":
        _assert_same(what + " cbcr", out.c0.unflatten(2, (cW, 2)).permute(0, 3, 1, 2), G.Expect(want_c, Hc, Wc, r, device(), my=my, mx=mx))
    else:
        _assert_same(what + " cb", out.c0[:, None], G.Expect(want_c[:, :1], Hc, Wc, r, device(), my=my, mx=mx))
        _assert_same(what + " cr", out.c1[:, None], G.Expect(want_c[:, 1:], Hc, Wc, r, device(), my=my, mx=mx))
    del chroma, lr, y, out
    torch.cuda.empty_cache()
    _report(f"video strip r={r} {strip}", op=f"{dtype}/{fi}->{fo}", lr=f"1x{H}x{W}", chroma=f"{Hc}x{Wc}", out=f"{r * H}x{r * W}",
            tiles=tiles, out_bytes=out_bytes, seconds=f"{time.time() - t0:.2f}")
