"""The MFLAG 1 (nr) metric on the device (sesrq.quality.score(pred, gt, 1), libsesrq_mosaic.so, include/sesrq_mosaic.h): PSNR / SSIM of
the Bayer mosaics of the prediction and the ground truth, against the reference-run mosaics of tests/golden/quality/mosaic.npz and the
float64 oracle (tests/mosaic_oracle.py), and bit for bit against the shipped single-channel form (MFLAG 5) on mono frames gathered
with torch.

Tolerances.  PSNR 1e-5 dB and SSIM 1e-6 are tests/test_quality.py's (_check, TOL_SSIM).  mse: bit for bit where every value is a
multiple of 1/256 (every squared difference is a multiple of 2^-16 and the sums stay far below 2^53: any summation order is exact);
otherwise the relative tolerance that 1e-5 dB of the RGB PSNR is, 10^(1e-5 / 10) - 1 = 2.3e-6.

Shapes are the smallest at which each mechanism is live: the tile seams of tests/test_quality_seams.py (W 254 / 255 and 502 / 503: nbx
steps and the last tile owns one SSIM column; H 38 / 39 and 70 / 71 likewise for rows), 7x7 / 7x8 / 8x7 (one window, both parities of
the last row and column), and W % 4 == 0 beside W % 4 != 0 (the 16-byte and the per-element loads)."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import Arena, OW, PAD, RH, device, nbx, nby, score, stream_ptr, to_device as _dev
import image_oracle as IO
import mosaic_oracle as M
import quality_oracle as Q
from test_quality import _check
from test_quality_seams import DY_SCALE, SCALE, TOL_SSIM, ZERO, _offset_view, frames

F32 = np.float32
HEADER = os.path.join(ROOT, "include", "sesrq_mosaic.h")
MSE_RTOL = 10.0 ** (1e-5 / 10.0) - 1.0
KERNELS = ("mosaic_tile<f32>", "mosaic_tile<i8>", "mosaic_finish")

SEAM_SHAPES = sorted({(H, W) for W in (254, 255, 502, 503) for H in (7, 39)} | {(H, W) for H in (38, 39, 70, 71) for W in (9, 255)})
SMALL_SHAPES = [(7, 7), (7, 8), (8, 7)]
CROSS_SHAPES = SMALL_SHAPES + SEAM_SHAPES


def mosaic_fixture():
    z = np.load(os.path.join(GOLDEN, "quality", "mosaic.npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_oracle_three2one_is_the_reference_run_mosaic():
    """mosaic_oracle.three2one on the clipped prediction and on the ground truth equals the mosaics the reference's own three2one gave,
    bit for bit; its metrics are the stored restated values; the int8 frames dequantise to the stored fp32 predictions."""
    z, meta = mosaic_fixture()
    assert sorted(meta["cases"]) == ["mosaic_67x101", "mosaic_7x7", "mosaic_8x9", "mosaic_9x8", "mosaic_same"]
    shapes = set()
    for name, c in meta["cases"].items():
        pred, gt = z[name + ".pred"], z[name + ".gt"]
        assert pred.dtype == F32 and gt.dtype == F32 and pred.shape == gt.shape and pred.shape[1] == 3
        shapes.add(pred.shape[2:])
        mp = M.three2one(np.clip(pred, 0, 1)).astype(np.float64)
        mg = M.three2one(gt).astype(np.float64)
        assert mp.tobytes() == z[name + ".mosaic_pred_ref"].tobytes(), name
        assert mg.tobytes() == z[name + ".mosaic_gt_ref"].tobytes(), name
        got = M.metrics(pred, gt)
        for col, key in enumerate(("mse_restated", "psnr_restated", "ssim_restated")):
            assert got[:, col].tobytes() == z[name + "." + key].tobytes(), (name, key)
        assert np.array_equal(IO.dequant(z[name + ".q"], meta["scale"], meta["zero"]), pred), name
        if c["identical"]:
            assert (got[:, 0] == 0).all() and np.isposinf(got[:, 1]).all() and (got[:, 2] == 1.0).all()
        else:
            assert (pred > 1).any() and (pred < 0).any(), name          # the clip fires
    assert shapes == {(67, 101), (7, 7), (9, 12), (8, 9), (9, 8)}


def test_oracle_selects_channel_by_row_and_column_parity():
    """three2one against the definition written out: R at (even, even), G where exactly one is odd, B at (odd, odd); the mosaic's
    metric is the single-channel form of tests/quality_oracle.py on the gathered frames, in data_range 1."""
    rng = np.random.default_rng(1)
    t = rng.random((2, 3, 9, 8)).astype(F32)
    m = M.three2one(t)
    assert m.dtype == F32 and m.shape == (2, 9, 8)
    for r in range(9):
        for c in range(8):
            assert (m[:, r, c] == t[:, (r & 1) + (c & 1), r, c]).all()
    assert M.selected(9, 8).sum() == 72 and (M.selected(9, 8).sum(axis=0) == 1).all()
    g = rng.random((2, 3, 9, 8)).astype(F32)
    got = M.metrics(t, g)
    mono = Q.metrics(m[:, None], M.three2one(g)[:, None], 5)
    assert np.array_equal(got[:, 2], mono[:, 2]) and np.allclose(mono[:, 0], 65025.0 * got[:, 0], rtol=1e-12, atol=0)


def test_mosaic_library_exports_every_declared_symbol():
    from sesrq import quality
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_mosaic[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 6, names
    assert sorted(quality.MOSAIC_SYMBOLS) == names, "python binding and header disagree"
    lib = quality.mosaic_lib()
    for n in names:
        assert getattr(lib, n) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", quality.MOSAIC_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sesrq_\w+)", nm))
    assert set(names) == exported, "libsesrq_mosaic.so exports exactly what its header declares"
    assert [lib.sesrq_mosaic_kernel_name(i).decode() for i in range(lib.sesrq_mosaic_kernel_count())] == list(KERNELS)
    assert lib.sesrq_mosaic_kernel_name(3) is None and lib.sesrq_mosaic_kernel_launches(-1) == -1


def test_mosaic_argument_checks_without_a_device():
    from sesrq import quality
    lib = quality.mosaic_lib()
    fake = C.c_void_p(4096)                       # never dereferenced: every check runs before any HIP call
    ws = lib.sesrq_mosaic_workspace_bytes(2, 67, 101)
    assert ws == 2 * nbx(101) * nby(67) * 16 and lib.sesrq_mosaic_workspace_bytes(1, 67, 101) * 2 == ws
    assert lib.sesrq_mosaic_workspace_bytes(2, 6, 101) == 0 and lib.sesrq_mosaic_workspace_bytes(2, 67, 6) == 0
    assert lib.sesrq_mosaic_workspace_bytes(0, 67, 101) == 0
    for H, W in CROSS_SHAPES:                     # one wave per tile, two doubles per tile: a third of the RGB form's slab
        assert lib.sesrq_mosaic_workspace_bytes(3, H, W) == 3 * nbx(W) * nby(H) * 16
        assert 3 * lib.sesrq_mosaic_workspace_bytes(3, H, W) == quality.lib().sesrq_eval_workspace_bytes(3, 3, H, W)

    def call(dtype=0, scale=0.5, zero=0, N=2, H=67, W=101, pred=fake, gt=fake, out=fake, work=fake, nbytes=ws, desc=True):
        d = quality.MosaicDesc(pred_dtype=dtype, pred_scale=scale, pred_zero=zero)
        rc = lib.sesrq_mosaic_score(C.byref(d) if desc else None, pred, gt, N, H, W, out, work, nbytes, None)
        return rc, quality.mosaic_last_error()

    cases = {
        "H < 7": dict(H=6),
        "W < 7": dict(W=6),
        "N < 1": dict(N=0),
        "N too large": dict(N=65536),
        "workspace too small": dict(nbytes=ws - 1),
        "NULL pred": dict(pred=None),
        "NULL gt": dict(gt=None),
        "NULL out": dict(out=None),
        "NULL workspace": dict(work=None),
        "NULL desc": dict(desc=False),
        "unknown dtype": dict(dtype=5),
        "int8 scale 0": dict(dtype=quality.PRED_I8, scale=0.0),
        "int8 scale nan": dict(dtype=quality.PRED_I8, scale=float("nan")),
        "int8 scale inf": dict(dtype=quality.PRED_I8, scale=float("inf")),
        "int8 zero": dict(dtype=quality.PRED_I8, zero=128),
    }
    for what, kw in cases.items():
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("sesrq_mosaic"), (what, rc, msg)


def test_score_mflag_1_refusals_on_the_host():
    torch = pytest.importorskip("torch")
    from sesrq import quality
    assert quality.FORMS[1] == quality.FORM_MOSAIC and quality.FORMS[2] == quality.FORM_RGB
    assert quality.form_of(1) == quality.FORM_MOSAIC and quality.CHANNELS[quality.FORM_MOSAIC] == 3
    a = torch.zeros(1, 3, 8, 8)
    for bad in ((torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8)),      # channels
                (a, torch.zeros(1, 3, 8, 9)),                            # shape
                (torch.zeros(1, 3, 6, 8), torch.zeros(1, 3, 6, 8)),      # smaller than the window
                (torch.zeros(0, 3, 8, 8), torch.zeros(0, 3, 8, 8)),      # no frames
                (a, a),                                                  # not on a device
                (a.numpy(), a.numpy())):                                 # not tensors
        with pytest.raises(ValueError):
            quality.score(bad[0], bad[1], 1)
    with pytest.raises(ValueError, match="MFLAG 7"):
        quality.form_of(7)
    with pytest.raises(ValueError, match="super-resolution"):           # images feed the SR nets only
        quality.evaluate_image(None, [], [], 1)
    with pytest.raises(ValueError, match="super-resolution"):
        quality.evaluate_image(None, [], [], 2)


# ------------------------------------------------------------------------------------------------------------------------ GPU
_score = functools.partial(score, mflag=1)


def _gathered(pred, gt, **kw):
    """The only route without the mosaic form: two torch gathers into mono frames, scored in the single-channel form (MFLAG 5), whose
    kernel clips the prediction (a clip commutes with a gather)."""
    import torch
    from sesrq import quality
    p, g = _dev(pred), _dev(gt)
    N, _, H, W = p.shape
    idx = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(M.channel_map(H, W), (N, 1, H, W)))).to(device())
    res = quality.score(torch.gather(p, 1, idx).contiguous(), torch.gather(g, 1, idx).contiguous(), 5, **kw)
    torch.cuda.synchronize()
    return res.cpu().numpy()


def _launches():
    from sesrq import quality
    return quality.mosaic_kernels()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "i8"])
def test_every_fixture_case(dtype):
    z, meta = mosaic_fixture()
    for name, c in meta["cases"].items():
        pred = z[name + ".q"] if dtype == "i8" else z[name + ".pred"]
        kw = dict(scale=meta["scale"], zero=meta["zero"]) if dtype == "i8" else {}
        got = _score(pred, z[name + ".gt"], **kw)
        for n in range(len(got)):
            print(name, dtype, n, "mse", got[n, 0], z[name + ".mse_restated"][n], "psnr", got[n, 1], z[name + ".psnr_restated"][n],
                  "ssim", got[n, 2], z[name + ".ssim_restated"][n])
        _check(got, z[name + ".psnr_restated"], z[name + ".ssim_restated"], name)
        np.testing.assert_allclose(got[:, 0], z[name + ".mse_restated"], rtol=MSE_RTOL, atol=0, err_msg=name)
        if c["identical"]:
            assert (got[:, 0] == 0.0).all() and np.isposinf(got[:, 1]).all() and (got[:, 2] == 1.0).all(), (name, got)


def _exact_mse(gk, pk):
    """mse of k/256 frames from the integer sum of squared differences over the selected sites, by mosaic_finish's expression."""
    H, W = gk.shape[-2:]
    sse_k = ((M.three2one(gk) - M.three2one(pk)) ** 2).reshape(gk.shape[0], -1).sum(axis=1)
    assert sse_k.dtype == np.int64
    return (sse_k.astype(np.float64) / 65536.0) / (float(H) * W)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "i8"])
def test_cross_check_against_the_single_channel_form(dtype):
    """On independent noise at every seam: SSIM has the bits the shipped Y255 form gives on the gathered mono frames and
    mse_y255 == 65025.0 * mse_mosaic exactly; against the oracle at the file's tolerances; on the k/256 frames mse equals the integer
    sum bit for bit.  Launches are counted by the new kernels' names."""
    tile = KERNELS[0] if dtype == "f32" else KERNELS[1]
    before = _launches()
    for H, W in CROSS_SHAPES:
        f = frames(H, W)
        for dyadic in (False, True):
            gt = f.dgt if dyadic else f.gt
            if dtype == "i8":
                q, scale = (f.dq, DY_SCALE) if dyadic else (f.q, SCALE)
                pred, seen, kw = q, IO.dequant(q, scale, ZERO), dict(scale=scale, zero=ZERO)
            else:
                pred = seen = f.dpred if dyadic else f.pred
                kw = {}
            what = (dtype, H, W, "k/256" if dyadic else "noise")
            got = _score(pred, gt, **kw)
            mono = _gathered(pred, gt, **kw)
            assert got[:, 2].tobytes() == mono[:, 2].tobytes(), (what, got[:, 2], mono[:, 2])
            assert mono[:, 0].tobytes() == (65025.0 * got[:, 0]).tobytes(), (what, mono[:, 0], got[:, 0])
            want = M.metrics(seen, gt)
            _check(got, want[:, 1], want[:, 2], what)
            np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=MSE_RTOL, atol=0, err_msg=str(what))
            if dyadic:
                exact = _exact_mse(f.dgt_k, f.dq_k if dtype == "i8" else f.dpred_k)
                assert got[:, 0].tobytes() == exact.tobytes(), (what, got[:, 0], exact)
    after = _launches()
    assert after[tile] - before[tile] == 2 * len(CROSS_SHAPES) == after[KERNELS[2]] - before[KERNELS[2]]
    other = KERNELS[1] if dtype == "f32" else KERNELS[0]
    assert after[other] == before[other]
    assert {nbx(W) for _, W in CROSS_SHAPES} == {1, 2, 3} and {nby(H) for H, _ in CROSS_SHAPES} == {1, 2, 3}
    for W in (255, 503):                          # single-column and single-row tile tails
        assert (W - 2 * PAD) - (nbx(W) - 1) * OW == 1
    for H in (39, 71):
        assert (H - 2 * PAD) - (nby(H) - 1) * RH == 1


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(7, 9), (39, 255), (40, 256)])
def test_poison_only_selected_samples_count(H, W):
    """NaN at every unselected (pixel, channel) of pred and gt: the scores keep the bits of the clean frames.  One NaN at a selected
    position of frame 1 (pred, then gt): frame 1's scores are NaN, frames 0 and 2 keep their bits.  (40, 256): the 16-byte loads.)"""
    f = frames(H, W)
    three = lambda a: np.concatenate([a, a[:1]])
    pred, gt, q = three(f.pred), three(f.gt), three(f.q)
    sel = np.broadcast_to(M.selected(H, W), pred.shape)
    clean = _score(pred, gt)
    clean_q = _score(q, gt, scale=SCALE, zero=ZERO)
    assert np.isfinite(clean).all() and np.isfinite(clean_q).all()
    pp, pg = np.where(sel, pred, F32(np.nan)), np.where(sel, gt, F32(np.nan))
    assert np.isnan(pp).sum() == 2 * pred.size // 3 == np.isnan(pg).sum()
    assert _score(pp, pg).tobytes() == clean.tobytes()
    assert _score(q, pg, scale=SCALE, zero=ZERO).tobytes() == clean_q.tobytes()
    for r, c in ((0, 0), (H - 1, W - 1), (H // 2, W // 2 + 1)):
        ch = (r & 1) + (c & 1)
        for where in ("pred", "gt"):
            p2, g2 = pp.copy(), pg.copy()
            (p2 if where == "pred" else g2)[1, ch, r, c] = np.nan
            got = _score(p2, g2)
            assert np.isnan(got[1]).all(), (where, r, c, got)
            assert got[[0, 2]].tobytes() == clean[[0, 2]].tobytes(), (where, r, c, got, clean)
        g2 = pg.copy()
        g2[1, ch, r, c] = np.nan
        got = _score(q, g2, scale=SCALE, zero=ZERO)
        assert np.isnan(got[1]).all() and got[[0, 2]].tobytes() == clean_q[[0, 2]].tobytes(), ("i8", r, c, got)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (9, 9)])
def test_distinct_planes_closed_form(H, W):
    """Constant planes pred = (0.25, 0.5, 0.75), gt = (0.5, 0.5, 0.5): every R and every B site contributes 0.0625, the G sites
    nothing.  A swapped parity (R <-> B keeps the count; G <-> R / B does not) or a wrong plane changes the count."""
    pred = np.empty((2, 3, H, W), F32)
    pred[:, 0], pred[:, 1], pred[:, 2] = 0.25, 0.5, 0.75
    gt = np.full((2, 3, H, W), 0.5, F32)
    cm = M.channel_map(H, W)
    rb = int((cm != 1).sum())
    assert rb == ((H + 1) // 2) * ((W + 1) // 2) + (H // 2) * (W // 2)
    want = (rb * 0.0625) / (float(H) * W)
    got = _score(pred, gt)
    assert (got[:, 0] == want).all(), (got[:, 0], want)
    assert abs(got[0, 1] - 10 * np.log10(1 / want)) <= 1e-9
    # planes that differ in gt instead, R and B apart: a mosaic that swapped them would score another mse
    gt2 = np.empty((2, 3, H, W), F32)
    gt2[:, 0], gt2[:, 1], gt2[:, 2] = 0.25, 0.5, 1.0
    want2 = (int((cm == 2).sum()) * 0.0625) / (float(H) * W)
    got2 = _score(pred, gt2)
    assert (got2[:, 0] == want2).all(), (got2[:, 0], want2)
    ref = M.metrics(pred, gt2)
    _check(got2, ref[:, 1], ref[:, 2], ("planes", H, W))


@pytest.mark.gpu
@pytest.mark.parametrize("W", [12, 252, 256, 255, 9])
def test_both_load_paths_give_the_same_bits(W):
    """include/sesrq_mosaic.h, "Caller buffers": aligned frames (the 16-byte loads where W % 4 == 0) and frames 4 bytes off (an int8
    pred 1 byte off: the per-element loads) score the same data to the same bits; W % 4 != 0 takes the per-element loads at any
    address."""
    import torch
    from sesrq import quality
    H = 39
    f = frames(H, W)
    for pred, poff, kw in ((f.pred, 4, {}), (f.q, 1, dict(scale=SCALE, zero=ZERO))):
        base = quality.score(_offset_view(pred, 0, torch), _offset_view(f.gt, 0, torch), 1, **kw)
        for po, go in ((poff, 0), (0, 4), (poff, 4)):
            got = quality.score(_offset_view(pred, po, torch), _offset_view(f.gt, go, torch), 1, **kw)
            torch.cuda.synchronize()
            assert torch.equal(got, base), (W, pred.dtype, po, go, got, base)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(7, 7), (9, 12)])
def test_300_one_tile_frames_score_as_each_alone(H, W):
    import torch
    from sesrq import quality
    N = 300
    rng = np.random.default_rng([N, H, W, 1])
    gt = rng.random((N, 3, H, W), dtype=F32)
    pred = (rng.random((N, 3, H, W), dtype=F32) * F32(1.2) - F32(0.1)).astype(F32)
    q = rng.integers(-128, 128, (N, 3, H, W)).astype(np.int8)
    for p, kw in ((pred, {}), (q, dict(scale=SCALE, zero=ZERO))):
        pt, g = _dev(p), _dev(gt)
        batch = quality.score(pt, g, 1, **kw)
        alone = torch.cat([quality.score(pt[n:n + 1], g[n:n + 1], 1, **kw) for n in range(N)])
        torch.cuda.synchronize()
        assert torch.equal(batch, alone), (p.dtype, H, W, (batch != alone).nonzero()[:4])
        assert len(torch.unique(batch[:, 2])) > N // 2
        k = [0, 1, 150, 299]
        seen = IO.dequant(q[k], SCALE, ZERO) if kw else pred[k]
        want = M.metrics(seen, gt[k])
        _check(batch[k].cpu().numpy(), want[:, 1], want[:, 2], (str(p.dtype), H, W))


ROUNDS = ((0x5A, np.array([np.nan], F32).tobytes(), bytes([0x7F]), 0x00), (0xA5, np.array([-3e38], F32).tobytes(), bytes([0x80]), 0xFF))
PLACES = ((0, 0), (4, 0), (0, 4), (8, 12), (12, 8))
PLACES_I8 = (0, 1, 2, 3, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "i8"])
@pytest.mark.parametrize("H,W", [(7, 8), (7, 7), (9, 12)])
def test_score_in_hostile_surroundings(H, W, dtype):
    """sesrq_mosaic_score with pred, gt, out and the workspace placed in canary arenas at every address class (tests/helpers.py Arena,
    as tests/test_caller_buffers.py places sesrq_eval's): nothing outside out and the workspace is written, what surrounds the frames
    (NaN, -3e38, int8 extremes) does not reach the scores, and a workspace pre-filled with 0x00 or 0xFF gives the same bits."""
    import torch
    from sesrq import quality
    scale, zero = 0.0051, -117
    rng = np.random.default_rng(H * W + 3)
    gt = rng.random((2, 3, H, W)).astype(F32)
    if dtype == "i8":
        pred = rng.integers(-128, 128, (2, 3, H, W)).astype(np.int8)
        seen = IO.dequant(pred, scale, zero)
    else:
        pred = (gt + rng.normal(0, 0.05, gt.shape)).astype(F32)
        pred[0, 0, 0, 0], pred[1, 2, -1 - H % 2, -1 - W % 2] = 1.3, -0.2      # selected sites, clipped
        seen = pred
    want = M.metrics(seen, gt)
    lib = quality.mosaic_lib()
    ws_bytes = lib.sesrq_mosaic_workspace_bytes(2, H, W)
    assert ws_bytes == 32
    desc = quality.MosaicDesc(pred_dtype=quality.PRED_I8 if dtype == "i8" else quality.PRED_F32, pred_scale=scale if dtype == "i8" else 0.0,
                              pred_zero=zero if dtype == "i8" else 0)
    bits = set()
    tt = {np.dtype(np.int8): torch.int8, np.dtype(F32): torch.float32}
    for i, (po, go) in enumerate(PLACES):
        po = PLACES_I8[i] if dtype == "i8" else po
        for r, (canary, around_f32, around_i8, ws_fill) in enumerate(ROUNDS):
            what = f"mosaic {dtype} {H}x{W} at ({po}, {go}) run {r + 1}"
            af = Arena(device(), Arena.room(gt.nbytes, gt.nbytes), around_f32)
            g = af.place(gt.shape, torch.float32, go, fill=gt.copy(), name="gt")
            a8 = Arena(device(), Arena.room(gt.nbytes), around_i8)
            p = (a8 if dtype == "i8" else af).place(pred.shape, tt[pred.dtype], po, fill=pred.copy(), name="pred")
            aout = Arena(device(), Arena.room(48, ws_bytes), canary)
            out = aout.place((2, 3), torch.float64, 8 + 16 * (i % 2), name="out")
            ws = aout.place(ws_bytes, torch.uint8, 8 + 16 * ((i + 1) % 2), fill=ws_fill, name="workspace")
            rc = lib.sesrq_mosaic_score(C.byref(desc), p.data_ptr(), g.data_ptr(), 2, H, W, out.data_ptr(), ws.data_ptr(), ws_bytes,
                                        stream_ptr())
            assert rc == 0, (what, quality.mosaic_last_error())
            torch.cuda.synchronize()
            for a in (af, a8, aout):
                stray = a.check()
                assert not stray, f"{what}: bytes outside the caller's buffers changed: {stray[:6]}"
            got = out.cpu().numpy()
            assert np.isfinite(got).all(), (what, got)
            _check(got, want[:, 1], want[:, 2], what)
            bits.add(got.tobytes())
    assert len(bits) == 1, "the scores depend on the buffers' addresses, their surroundings or the workspace's prior contents"


@pytest.mark.gpu
def test_zz_every_mosaic_kernel_ran():
    """LAST in this file: every kernel instantiation libsesrq_mosaic.so can launch was launched by a checked case above."""
    k = _launches()
    assert sorted(k) == sorted(KERNELS), k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
