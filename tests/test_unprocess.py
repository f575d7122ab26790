"""The fused unprocess on the device (sesrq.unprocess, Engine.forward_srgb, quality.evaluate_srgb) against tests/unprocess_oracle.py:
every byte and fp32 word equal, no tolerance; every case names the instantiation it expects from the launch counters."""
import itertools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import Arena, calib_params, device, same, stream_ptr, to_device

import unprocess_oracle as UO

pytestmark = pytest.mark.gpu

SEG, THREADS, BLOCKS_PER_CU = 16, 256, 8      # csrc/sesrq_unprocess.hip
OUTS = ("raw", "gt", "q0", "spread")
SETS = [tuple(k for i, k in enumerate(OUTS) if m >> i & 1) for m in range(1, 16)]


_t = to_device
_dtype = lambda k: getattr(__import__("torch"), dict(raw="uint16", gt="float32", q0="int8", spread="float32")[k])
_shape = lambda k, N, H, W: (N, H, W) if k == "raw" else (N, 3, H, W)


def _profile(highlight=True):
    from sesrq import unprocess
    return unprocess.Profile(UO.RGB2CAM, UO.INV_GAINS, "paper", highlight)


def _name(wants, fmt):
    home = (", lds" if fmt.white - fmt.black < 4096 else ", global") if "q0" in wants else ""
    return f"unprocess<{'+'.join(k for k in OUTS if k in wants)}{home}>"


def _oracle(img, p, fmt, order="rgb"):
    return UO.run(img, p.curve, p.rgb2cam, p.inv_gains, p.highlight, order, fmt.cfa, fmt.black, fmt.white)


def _launch(what, dimg, p, fmt, order, wants):      # one launch into fresh tensors; exactly the expected instantiation ran
    import torch
    from sesrq import unprocess
    N, H, W, _ = dimg.shape
    out = {k: torch.empty(_shape(k, N, H, W), dtype=_dtype(k), device=device()) for k in wants}
    before = unprocess.instances()
    unprocess.launch(p, fmt, *UO.DOMAIN, 0, dimg, order, *(out.get(k) for k in OUTS), torch.cuda.current_stream(device()))
    torch.cuda.synchronize()
    after = unprocess.instances()
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {_name(wants, fmt): 1}, what
    return out


def _check(what, img, p, fmt, order, *sets):
    want, dimg = _oracle(img, p, fmt, order), _t(img)
    for wants in sets:
        out = _launch(what, dimg, p, fmt, order, wants)
        for k in wants:
            same(f"{what} {wants} {k}", out[k], want[k])
    return out


@pytest.mark.parametrize("white", [4095 + 64, 65535])
@pytest.mark.parametrize("highlight", [True, False])
@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("cfa", UO.CFAS)
def test_all_codes_at_every_bayer_phase(cfa, order, highlight, white):
    from sesrq import sensor
    fmt = sensor.Format(cfa, 64 if white < 65535 else 0, white)
    img = UO.all_codes()
    _check(f"{cfa} {order} {highlight} {white}", img, _profile(highlight), fmt, order, OUTS)


@pytest.mark.parametrize("N", [1, 3])
def test_every_width_across_the_segment_seams(N):
    from sesrq import sensor
    rng = np.random.default_rng(7 + N)
    """Every (H, W) under each single-output set and the full set, the ten others taking turns; highlight, format and order drawn per frame."""
    fmts = (sensor.Format("grbg", 16, 1023), sensor.Format("gbrg", 0, 65535))
    always = [s for s in SETS if len(s) in (1, 4)]
    turns = itertools.cycle(s for s in SETS if s not in always)
    for H in (1, 2, 3):
        for W in range(1, 2 * SEG + 3):
            img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
            hl, f, o = rng.integers(0, 2, 3)
            _check(f"N={N} {H}x{W}", img, _profile(bool(hl)), fmts[f], ("rgb", "bgr")[o], *always, next(turns))


OFFSETS = (0, 1, 2, 3, 7)
ROUNDS = ((0x5A, bytes([0x7F])), (0xA5, bytes([0x80])))


@pytest.mark.parametrize("shape", [(2, 3, 32), (2, 5, 7)])       # whole segments; narrow forms only
def test_buffers_in_hostile_surroundings(shape):
    import torch
    from sesrq import sensor, unprocess
    N, H, W = shape
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    p, fmt = _profile(), sensor.Format("bggr", 0, 4095)
    h = unprocess.context(p, fmt, *UO.DOMAIN, 0, device())
    aligned = _check(f"aligned {shape}", img, p, fmt, "rgb", OUTS)
    esz = dict(img=1, raw=2, gt=4, q0=1, spread=4)
    for i, (canary, around) in itertools.product(range(len(OFFSETS)), ROUNDS):
        off = {k: -(-OFFSETS[(i + j) % 5] // e) * e for j, (k, e) in enumerate(esz.items())}
        what = f"{shape} {off} canary {canary:#x}"
        ain = Arena(device(), Arena.room(img.nbytes), around)
        dimg = ain.place(img.shape, torch.uint8, off["img"], fill=img, name="img")
        aout = Arena(device(), Arena.room(*(int(np.prod(_shape(k, N, H, W))) * esz[k] for k in OUTS)), canary)
        out = {k: aout.place(_shape(k, N, H, W), _dtype(k), off[k], name=k) for k in OUTS}
        rc = unprocess.lib().sesrq_unprocess_run(h, dimg.data_ptr(), 0, *(out[k].data_ptr() for k in OUTS), N, H, W, stream_ptr())
        assert rc == 0, (what, unprocess.last_error())
        torch.cuda.synchronize()
        for a in (ain, aout):
            stray = a.check()
            assert not stray, f"{what}: bytes outside the caller's buffers changed: {stray[:6]}"
        for k in OUTS:
            same(f"{what} {k}", out[k], aligned[k])
        same(what + " img untouched", dimg, img)


@pytest.mark.parametrize("trips,W", [(1, 1024), (2, 1030)])
def test_frames_just_above_one_and_two_trips_of_the_grid(trips, W):
    import torch
    import geometry as G
    from sesrq import sensor, unprocess
    PY, PX = 6, 122                         # the block the frame is tiled from: even sides keep the Bayer phase
    segs = -(-W // SEG)
    trip = torch.cuda.get_device_properties(device()).multi_processor_count * BLOCKS_PER_CU * THREADS      # items of one round
    H = trips * trip // segs + 2
    block = np.random.default_rng(trips).integers(0, 256, (1, PY, PX, 3), dtype=np.uint8)
    p, fmt = _profile(), sensor.Format("grbg", 0, 4095)
    small = _oracle(block, p, fmt)
    yy, xx = torch.arange(H, device=device()) % PY, torch.arange(W, device=device()) % PX
    img = _t(block)[:, yy][:, :, xx].contiguous()
    out = _launch(f"{trips} trips", img, p, fmt, "rgb", OUTS)
    for k in OUTS:
        got, want = (out[k].to(torch.int32)[:, None], small[k].astype(np.int32)[:, None]) if k == "raw" else (out[k], small[k])
        bad, first = G.compare_all(got, G.Expect(want, H, W, 1, device(), tiled=True))
        assert bad == 0, (k, bad, first)


def _engine(**kw):
    import sesrq
    from sesrq.bundle import Bundle
    return sesrq.Engine(Bundle.load(os.path.join(GOLDEN, "raw", "nrdm_3.npz")), device(), **kw)


@pytest.mark.parametrize("fmt_args", [None, ("grbg", 64, 1023)])
def test_forward_srgb_is_forward_raw_on_the_oracles_frame(fmt_args):
    import torch
    from sesrq import noise, quality, sensor, unprocess
    from sesrq.calibrate import Calibrator
    e = _engine()
    b = e.bundle
    fmt = None if fmt_args is None else sensor.Format(*fmt_args)
    f = sensor.REFERENCE if fmt is None else fmt
    p = unprocess.from_colormatrix([[1.0234, -0.2969, -0.2266], [-0.5625, 1.6328, -0.0469], [-0.0703, 0.2188, 0.6406]], 2.1, 1.6)
    img = np.random.default_rng(3).integers(0, 256, (2, 48, 66, 3), dtype=np.uint8)
    img[:, 8:16] |= 0xE0                                                # highlights
    k = UO.codes(img, p.curve, p.rgb2cam, p.inv_gains, True, "bgr", f.white - f.black)
    want = UO.outputs(k, f.cfa, f.black, f.white, b.scale[0], b.zero[0], e.exact_div)
    raw = _t(want["raw"])
    got = unprocess.run(_t(img), p, fmt, e, order="bgr", want_q=True, want_spread=True)
    for name in OUTS:
        same(f"run {name}", got[name], want[name])
    q0, sp = sensor.unpack(e, raw, f, want_q=True, want_spread=True)
    same("sensor.unpack(raw) q0", q0, got["q0"])
    same("sensor.unpack(raw) spread", sp, got["spread"])
    model = noise.NoiseModel(0.004, 1e-4, seed=1)
    for kw in ({}, dict(noise=model)):
        q, y = e.forward_raw(raw, fmt=fmt, **kw)
        q2, y2, gt = e.forward_srgb(_t(img), p, order="bgr", fmt=fmt, want_gt=True, **kw)
        torch.cuda.synchronize()
        same(f"forward_srgb q {kw}", q2, q)
        same(f"forward_srgb y {kw}", y2, y)
        same(f"forward_srgb gt {kw}", gt, want["gt"])
        gts = [(f.black + k[n]).astype(np.uint16) for n in range(2)]
        a = quality.evaluate_raw(e, [want["raw"][n] for n in range(2)], gts, 3, fmt=fmt, **kw)
        s = quality.evaluate_srgb(e, [img[n] for n in range(2)], p, 3, order="bgr", fmt=fmt, **kw)
        assert np.array_equal(a, s) and a.shape == (2, 3) and np.isfinite(a).all(), (a, s)
        cals = [Calibrator(*calib_params("nrdm_3"), device(), quan_bits=8) for _ in range(2)]
        same(f"enqueue_srgb {kw}", cals[0].enqueue_srgb(_t(img), p, order="bgr", fmt=fmt, **kw), cals[1].enqueue_raw(raw, fmt=fmt, **kw))


def test_run_refuses_before_any_launch_and_every_instance_ran():
    import torch
    from sesrq import sensor, unprocess
    p, fmt = _profile(), sensor.Format()
    h = unprocess.context(p, fmt, *UO.DOMAIN, 0, device())
    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=device())
    raw = torch.zeros((1, 4, 5), dtype=torch.uint16, device=device())
    gt = torch.zeros((1, 3, 4, 5), dtype=torch.float32, device=device())
    launches = sum(unprocess.instances().values())
    run = unprocess.lib().sesrq_unprocess_run
    I, R, G = img.data_ptr(), raw.data_ptr(), gt.data_ptr()
    for args, word in (((h, I, 0, None, None, None, None, 1, 4, 4), "none of raw"), ((None, I, 0, R, None, None, None, 1, 4, 4), "ctx is NULL"),
                       ((h, None, 0, R, None, None, None, 1, 4, 4), "img is NULL"), ((h, I, 2, R, None, None, None, 1, 4, 4), "order 2"),
                       ((h, I, 0, R, None, None, None, 1, 0, 4), "empty frame"), ((h, I, 0, R + 1, None, None, None, 1, 4, 4), "2-byte"),
                       ((h, I, 0, None, G + 2, None, None, 1, 4, 4), "4-byte"),
                       ((h, I, 0, R, None, None, None, 65536, 65536, 16), "too large")):
        assert run(*args, stream_ptr()) != 0 and word in unprocess.last_error(), (word, unprocess.last_error())
    from sesrq import noise
    noisy = dict(noise=noise.NoiseModel(0.004, 1e-4, seed=1), out_q=torch.empty(3, dtype=torch.int8, device=device()))
    for a, kw, word in (((img, "paper"), {}, "Profile"), ((img.float(), p), {}, "torch.uint8"), ((img, p), dict(fmt=sensor.Format(packing="raw12")),
                        "16-bit containers"), ((img, p), noisy, "output shape")):      # the last: forward_raw's, before the noise route's launch
        with pytest.raises(ValueError, match=word):
            _engine().forward_srgb(*a, **kw)
    torch.cuda.synchronize()
    assert sum(unprocess.instances().values()) == launches, "a refused call launched a kernel"
    k = unprocess.instances()              # the LAST test of the file: every instantiation was launched by a checked case above
    assert len(k) == 7 + 2 * 8 and all(k.values()), sorted(n for n, c in k.items() if c == 0)
