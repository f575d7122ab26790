"""Every sum of each pass of the three bicubic resamplers on the device: downscale<r,form> (libsesrq_downscale.so),
video_export<yd,r,fmt> (libsesrq_video.so) and colour_export<yd,r> (libsesrq_colour.so) on the sweep frames of
tests/resampler_sweep.py, against tests/downscale_oracle.py, tests/video_oracle.py and tests/colour_oracle.py.  Every comparison is
exact and covers every byte and every fp32 word.  tests/test_resampler_sweep.py proves on the CPU what the frames rely on: a frame of
constant rows (columns) leaves the horizontal (vertical) pass an identity, so the swept pass's result reaches the output as it is, and
the targets sit in tap windows that do not overlap.

  downscale        r = 2, 4 x the vertical and the horizontal pass: one frame whose sweep positions take every reachable sum
                   T = sum w b (77 465 at r = 2, 1 223 839 at r = 4: every integer from below -D / 2 to above 256 D among them), two
                   LR pixels across; lr, q0 and x of one launch in the RGB form; the r = 2 frames again in the Y form and in BGR
                   order.  Zero omission: the sums of the frame (DO.one_pass(..., sums=True)) are the reachable set, exactly.
                   Expected bytes: at r = 2 the whole-frame oracle DO.downscale, which the line's own pass must equal; at r = 4 the
                   whole-frame oracle takes 12 s and 5 GB on the host, so the expected frame is DO.one_pass of the line along the
                   swept axis (2.4 s, once for both passes) -- exact by the identity the CPU test proves, and cross-checked at r = 2.
  video export     r = 2, 4 x the two passes: chroma planes whose sweep positions take, at every phase, the lowest and the highest
                   reachable T of every Q6 value the phase reaches; NV12 -> I420 and I420 -> NV12; random int8 luma.  Zero omission:
                   the Q6 values of the swept pass at each phase (VO.chroma_q6(..., keep=True)) are the phase's reachable set.
                   Negative horizontal-pass values in even and odd columns and at every phase, final Q6 below -32 and above
                   255 * 64 + 31 are asserted from the oracle's intermediates.
  colour export    r = 2, 4 x the two passes: every 4-tuple of the eight cube corners and mid-grey as the four taps of every phase,
                   int8 luma at both ends of its range and in the middle, both byte orders; Q6 chroma below 16 * 64 and above
                   240 * 64 in the swept pass.

Every case checks the launch counters (exactly the named instantiation ran, once a launch) and prints one "RESAMPLER|" line with its
shape and seconds: profiles/resampler_limits.txt is made of them."""
import functools
import time

import numpy as np
import pytest

import colour_oracle as CO
import downscale_oracle as DO
import image_oracle as IO
import resampler_sweep as RS
import video_oracle as VO
from helpers import device

pytestmark = pytest.mark.gpu

SWEPT = ("vertical", "horizontal")
IN_DOMAIN = (0.0039, -128)                    # the input domain of the downscale's fused decode
OUT_DOMAIN = (0.0047, -119)                   # the int8 output domain of the exports' luma
CANARY = 0x5A


def _report(what, **kw):
    print("RESAMPLER| " + what + " | " + " | ".join(f"{k}={v}" for k, v in kw.items()), flush=True)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(device())          # a copy: shared oracle results are read-only


def _bgr(a):
    return np.ascontiguousarray(a[..., ::-1])


def _differ(got, want):
    """How many elements of a device tensor differ from the array `want`, which may be 1 long where `got` repeats: fp32 as words."""
    import torch
    w = _t(want)
    assert got.dtype == w.dtype and got.dim() == w.dim() and all(b in (1, a) for a, b in zip(got.shape, w.shape)), (got.shape, w.shape)
    if got.dtype == torch.float32:
        got, w = got.view(torch.int32), w.view(torch.int32)
    return int(torch.count_nonzero(got != w.expand(got.shape)))


def _delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


# ------------------------------------------------------------------------------------------------------------------- downscale
@functools.lru_cache(maxsize=None)
def _downscale_line(r):
    """(line (L, 3), its LR line (L / r, 3) by the oracle's pass, the number of targets): shared by both passes, read-only.  Asserts
    the zero-omission condition: the sums of the line are the reachable set."""
    line, rows, T = RS.downscale_line(r)
    R = RS.downscale_reach(r)
    sums = DO.one_pass(line, r, 0, sums=True)
    assert np.array_equal(sums[rows], T)
    seen = np.zeros(R.hi - R.lo + 1, bool)
    seen[sums.reshape(-1) - R.lo] = True
    assert np.array_equal(seen, R.reach), f"{int((seen != R.reach).sum())} reachable sums are not in the sweep frame"
    D = DO.D[r]
    assert seen[-D // 2 - 2 - R.lo:256 * D + D // 2 + 2 - R.lo].all()      # every integer across both clamp thresholds
    lr = DO.one_pass(line, r, 0)
    for a in (line, lr):
        a.setflags(write=False)
    return line, lr, int(R.reach.sum())


@pytest.mark.parametrize("swept", SWEPT)
@pytest.mark.parametrize("r", [2, 4])
def test_downscale_every_reachable_sum_of_one_pass(r, swept):
    import torch
    from sesrq import downscale
    t0 = time.time()
    line, lr_line, targets = _downscale_line(r)
    img = RS.frame_of(line, swept, RS.ACROSS * r)
    whole = r == 2                                                           # the whole-frame oracle (module docstring)
    if whole:
        lr = DO.downscale(img, r)
        assert np.array_equal(lr, RS.frame_of(lr_line, swept, RS.ACROSS)), "the line's pass is not the frame's: no identity"
    else:
        lr = RS.frame_of(lr_line, swept, 1)                                  # one LR pixel across: the device repeats it
    N, H, W, _ = img.shape
    runs = [("rgb", "rgb")] + ([("y", "rgb"), ("rgb", "bgr"), ("y", "bgr")] if r == 2 else [])
    st = torch.cuda.current_stream(device())
    for form, order in runs:
        src, lr_o = (img, lr) if order == "rgb" else (_bgr(img), _bgr(lr))
        x = np.ascontiguousarray(IO.decode(lr_o, form, order))
        q = np.ascontiguousarray(IO.q0(x, IN_DOMAIN[0], IN_DOMAIN[1], 0)).astype(np.int8)
        Ch = 1 if form == "y" else 3
        got_lr = torch.full((N, H // r, W // r, 3), CANARY, dtype=torch.uint8, device=device())
        got_q = torch.full((N, Ch, H // r, W // r), CANARY, dtype=torch.int8, device=device())
        got_x = torch.full((N, Ch, H // r, W // r), float("nan"), dtype=torch.float32, device=device())
        before = downscale.instances()
        downscale.launch(device(), IN_DOMAIN[0], IN_DOMAIN[1], 0, _t(src), order, r, form, got_lr, got_q, got_x, st)
        torch.cuda.synchronize()
        name = f"downscale<r{r},{'Y' if form == 'y' else 'RGB'}>"
        assert _delta(before, downscale.instances()) == {name: 1}
        bad = {"lr": _differ(got_lr, lr_o), "q0": _differ(got_q, q), "x": _differ(got_x, x)}
        assert not any(bad.values()), f"{name} {order}, the {swept} pass swept: elements that differ from the oracle: {bad}"
        assert len(np.unique(lr)) == 256
    _report(f"downscale sweep r={r} {swept}", hr=f"{N}x{H}x{W}x3", targets=targets, launches=len(runs),
            expected="DO.downscale" if whole else "DO.one_pass of the line", seconds=f"{time.time() - t0:.2f}")


# ------------------------------------------------------------------------------------------------------------------- video
def _surface(fmt, fr):
    """A dict of planes as a contiguous device Surface in `fmt`."""
    from sesrq import video
    N, H, W = fr["y"].shape
    s = video.Surface.alloc(fmt, N, H, W, device())
    s.buf.fill_(CANARY)
    s.y.copy_(_t(fr["y"]))
    if fmt == "nv12":
        s.c0.copy_(_t(np.stack([fr["cb"], fr["cr"]], -1).reshape(s.c0.shape)))
    else:
        s.c0.copy_(_t(fr["cb"]))
        s.c1.copy_(_t(fr["cr"]))
    return s


def _differ_frames(s, want):
    """Differing bytes of each plane of a device Surface against the oracle's dict of planes."""
    if s.fmt_name == "nv12":
        return {"y": _differ(s.y, want["y"]), "cbcr": _differ(s.c0, np.stack([want["cb"], want["cr"]], -1).reshape(s.c0.shape))}
    return {"y": _differ(s.y, want["y"]), "cb": _differ(s.c0, want["cb"]), "cr": _differ(s.c1, want["cr"])}


@functools.lru_cache(maxsize=None)
def _upscale_lines(r):
    lines, out, phi, T = RS.upscale_lines(r)
    lines.setflags(write=False)
    return lines, int(np.unique(np.stack([phi.reshape(-1), T.reshape(-1)]), axis=1).shape[1])


@pytest.mark.parametrize("swept", SWEPT)
@pytest.mark.parametrize("r", [2, 4])
def test_video_export_every_q6_value_of_one_pass(r, swept):
    import torch
    from sesrq import video
    t0 = time.time()
    lines, targets = _upscale_lines(r)
    fr = {"cb": RS.frame_of(lines[0], swept, RS.ACROSS), "cr": RS.frame_of(lines[1], swept, RS.ACROSS)}
    _, Hc, Wc = fr["cb"].shape
    H, W = 2 * Hc, 2 * Wc
    fr["y"] = np.zeros((1, H, W), np.uint8)                                  # the LR luma is not looked at
    y = np.random.default_rng(50 + r).integers(-128, 128, (1, 1, r * H, r * W)).astype(np.int8)
    want = VO.export(y, fr, r, scale=OUT_DOMAIN[0], zero=OUT_DOMAIN[1])
    assert want["cb"].shape == (1, r * Hc, r * Wc)                           # even sizes: nothing of the upscaled plane is cropped

    # zero omission and the values the issue names, from the oracle's own intermediates
    v, h = zip(*[VO.chroma_q6(fr[k][0], r, keep=True) for k in ("cb", "cr")])
    v, h = np.stack(v), np.stack(h)                                          # (2, r Hc, r Wc), (2, Hc, r Wc)
    sw = v[:, :, 0] if swept == "vertical" else h[:, 0, :]                   # the swept pass's results along the swept axis
    for phi in range(r):
        got = np.unique(sw[:, phi::r])
        assert np.array_equal(got, RS.upscale_q6(r, phi)), f"phase {phi}: {RS.upscale_q6(r, phi).size - got.size} Q6 values are not in the frame"
    assert (v < -32).any() and (v > 255 * 64 + 31).any()
    assert want["cb"].min() == 0 and want["cb"].max() == 255 and len(np.unique(want["cr"])) == 256
    if swept == "horizontal":
        neg = (h < 0).any((0, 1))                                            # output columns that hold a negative value
        assert all(neg[phi::r].any() for phi in range(r)) and neg[0::2].any() and neg[1::2].any()
        assert h.min() == min(RS.upscale_range(r, phi)[0] for phi in range(r)) and v.shape[1] >= r      # ... read at every vertical phase
    else:
        assert (h >= 0).all()                                                # constant rows: the vertical pass reads 64 b

    yd = _t(y)
    for fi, fo in (("nv12", "i420"), ("i420", "nv12")):
        lr = _surface(fi, fr)
        out = video.Surface.alloc(fo, 1, r * H, r * W, device())
        out.buf.fill_(CANARY)
        before = video.instances()
        assert video.export(yd, lr, r, scale=OUT_DOMAIN[0], zero=OUT_DOMAIN[1], out=out) is out
        torch.cuda.synchronize()
        name = f"video_export<i8,r{r},{fo}>"
        assert _delta(before, video.instances()) == {name: 1}
        bad = _differ_frames(out, want)
        assert not any(bad.values()), f"{name} from {fi}, the {swept} pass swept: bytes that differ from the oracle: {bad}"
        assert not any(_differ_frames(lr, fr).values()), "the LR surface was written"
    _report(f"video sweep r={r} {swept}", lr=f"1x{H}x{W}", chroma=f"{Hc}x{Wc}", targets=targets, launches=2,
            q6=f"{int(sw.min())}..{int(sw.max())}", seconds=f"{time.time() - t0:.2f}")


# ------------------------------------------------------------------------------------------------------------------- colour
@pytest.mark.parametrize("swept", SWEPT)
@pytest.mark.parametrize("r", [2, 4])
def test_colour_export_every_four_tuple_of_the_palette_in_one_pass(r, swept):
    import torch
    from sesrq import colour
    t0 = time.time()
    line, idx = RS.palette_line()
    one = RS.frame_of(line, swept, RS.ACROSS)                                # (1, H, W, 3)
    assert len(idx) == 6561 and line.shape[0] == 4 * len(idx)                # every 4-tuple, a window each (the CPU test: of every phase)
    _, H, W, _ = one.shape
    mid = int(round(OUT_DOMAIN[1] + 0.5 / OUT_DOMAIN[0]))
    codes = (-128, mid, 127)                                                 # both ends of the int8 range and the middle of [0, 1]
    assert -128 < mid < 127
    img = np.ascontiguousarray(np.repeat(one, len(codes), 0))
    y = np.ascontiguousarray(np.broadcast_to(np.asarray(codes, np.int8)[:, None, None, None], (len(codes), 1, r * H, r * W)))
    up, h = CO.upscale(CO.chroma(one), r, keep=True)
    sw = up if swept == "vertical" else h
    assert (sw < 16 * 64).any() and (sw > 240 * 64).any()                     # beyond both ends of the studio chroma range
    yd = _t(y)
    for order in ("rgb", "bgr"):
        src = img if order == "rgb" else _bgr(img)
        want = CO.export(y, src, r, order, scale=OUT_DOMAIN[0], zero=OUT_DOMAIN[1])
        before = colour.instances()
        got = colour.export(yd, _t(src), r, order=order, scale=OUT_DOMAIN[0], zero=OUT_DOMAIN[1])
        torch.cuda.synchronize()
        name = f"colour_export<i8,r{r}>"
        assert _delta(before, colour.instances()) == {name: 1}
        bad = _differ(got, want)
        assert bad == 0, f"{name} {order}, the {swept} pass swept: {bad} bytes differ from the oracle"
        assert want.min() == 0 and want.max() == 255
    _report(f"colour sweep r={r} {swept}", lr=f"{len(codes)}x{H}x{W}x3", windows=len(idx), launches=2,
            q6=f"{int(sw.min())}..{int(sw.max())}", seconds=f"{time.time() - t0:.2f}")
