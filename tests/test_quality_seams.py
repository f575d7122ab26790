"""libsesrq_eval.so (csrc/sesrq_eval.hip) at its tile seams and conditioning edges, against the float64 oracle (tests/quality_oracle.py)
at the tolerances of tests/test_quality.py (_check: 1e-5 dB, 1e-6 SSIM).

eval_tile cuts a frame into tiles of OW = 248 SSIM columns x RH = 32 SSIM rows with carried fp64 window sums, lane-shuffled halo columns,
a masked last band and a separate rule that gives every squared error to exactly one tile.  An off-by-one in any bound moves SSIM by one
row or column of one tile; the shapes here are the smallest at which that is 1/249 .. 1/498 of a one-row map:

  1  seam geometry: every tile kernel (and sesrq_eval_anchored) at the widths where nbx steps and the heights where nby steps, on
     independent uniform noise (neighbouring SSIM values differ by ~0.1); the squared-error partition bit for bit on k/256 frames.
     CPU: the oracle against scipy's uniform_filter on the same frames, and the sweep has teeth -- every tile boundary's column / row,
     dropped or counted twice, moves the oracle's mean by >= 10x the tolerance on every noisy case.
  2  the 16-byte and the scalar load path give the same bits (include/sesrq_eval.h, "Caller buffers").
  3  conditioning: constant, nearly flat bright / dark, checkerboard, fully clipped, wide gt, int8 zero points at the int8 limits, mse == 0.
     CPU: the fp32 final quotient the kernel documents, restated on fp64 moments, stays within the tolerance on every case.
  4  N = 300 one-tile frames: a row of a batch has the bits of that frame scored alone.
  5  a NaN inside a frame makes that frame's three scores NaN and leaves the other frames' bits alone (include/sesrq_eval.h)."""
import functools
import types

import numpy as np
import pytest

import image_oracle as IO
import quality_oracle as Q
from helpers import OW, PAD, RH, device, nbx, nby, score as _score, score_anchored as _score_anchored, to_device as _dev
from test_quality import _check, _ssim_scipy

F32 = np.float32
TOL_SSIM = 1e-6                             # test_quality._check
SCALE, ZERO = float(F32(1.0 / 220.0)), -110  # the int8 output domain of tests/golden/quality (make_quality_golden.py:24)
DY_SCALE = 1.0 / 256.0                      # int8 domain of the k/256 frames: (q + 110) / 256 is on the grid

WS = (7, 8, 9, 12, 250, 252, 253, 254, 255, 256, 258, 502, 503, 504)
HS = (7, 8, 13, 14, 38, 39, 40, 70, 71)
SHAPES = sorted({(H, W) for W in WS for H in (7, 39)} | {(H, W) for H in HS for W in (9, 255)})
# sesrq_eval_anchored scores twice an LR frame: the even members of both lists and H = 72, each crossed with the even neighbours of the
# sweep's fixed sides (H 7 -> 8, 39 -> 40; W 9 -> 10, 255 -> 256), which keep their tile counts
A_SHAPES = sorted({(H, W) for W in WS if W % 2 == 0 for H in (8, 40)} | {(H, W) for H in HS + (72,) if H % 2 == 0 for W in (10, 256)})

# mflag, channels, kernel instance (sesrq.quality.kernels())
FORMS = {"rgb-f32": (3, 3, "eval_tile<f32,rgb>"), "rgb-i8": (3, 3, "eval_tile<i8,rgb>"), "y255-f32": (5, 1, "eval_tile<f32,y255>"),
         "y255-i8": (5, 1, "eval_tile<i8,y255>"), "x2-f32": (6, 3, "eval_tile<f32,x2>")}

# Frames are seeded by (SEEDS.get((H, W), 0), H, W).  A shape is listed where seed 0 gave a frame on which some seam column / row of
# some noisy case sums to nearly nothing (test_seam_mutants_move_the_oracle): the smallest seed without such a frame.
SEEDS = {(7, 256): 2, (7, 258): 2, (7, 503): 8, (7, 504): 1, (39, 253): 1, (39, 255): 7, (39, 258): 1, (39, 502): 2, (39, 503): 64,
         (39, 504): 8,
         (40, 255): 1, (70, 255): 2, (71, 255): 23}
A_SEEDS = {(8, 504): 5, (38, 256): 1, (40, 258): 1, (40, 504): 1}


def _ro(**kw):
    for a in kw.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return types.SimpleNamespace(**kw)


def make_frames(H, W, seed):
    """Two different frames of one shape.  Noisy: gt and pred independent U[0, 1), ~2 % of pred outside [0, 1]; q an int8 prediction over
    the whole int8 range in the fixture's domain ([-0.08, 1.08]).  Dyadic: gt and clip(pred) on the grid k/256."""
    rng = np.random.default_rng([seed, H, W])
    shape = (2, 3, H, W)
    gt = rng.random(shape, dtype=F32)
    pred = rng.random(shape, dtype=F32)
    u = rng.random(shape)
    pred[u < 0.01], pred[u > 0.99] = F32(1.25), F32(-0.25)
    pred[:, :, 0, 0], pred[:, :, -1, -1] = F32(1.25), F32(-0.25)       # in the smallest frames too
    q = rng.integers(-128, 128, shape).astype(np.int8)
    dg = rng.integers(0, 257, shape)
    dp = rng.integers(-20, 277, shape)
    dq = rng.integers(-128, 128, shape).astype(np.int8)
    return _ro(gt=gt, pred=pred, q=q, dgt=(dg / 256.0).astype(F32), dpred=(dp / 256.0).astype(F32), dq=dq,
               dgt_k=dg, dpred_k=np.clip(dp, 0, 256), dq_k=np.clip(dq.astype(np.int64) - ZERO, 0, 256))


@functools.lru_cache(maxsize=None)
def frames(H, W):
    return make_frames(H, W, SEEDS.get((H, W), 0))


def make_anchored(H, W, seed):
    """pred U[-0.1, 0.8) and a random LR frame U[0, 0.5): fl32(pred + up2(lr)) spans [-0.1, 1.3)."""
    rng = np.random.default_rng([seed, H, W, 2])
    gt = rng.random((2, 3, H, W), dtype=F32)
    pred = (rng.random((2, 3, H, W), dtype=F32) * F32(0.9) - F32(0.1)).astype(F32)
    lr = (rng.random((2, 3, H // 2, W // 2), dtype=F32) * F32(0.5)).astype(F32)
    seen = (pred + IO.upsample2(lr)).astype(F32)
    assert seen.dtype == F32 and seen.max() > 1.0 and seen.min() < 0.0
    return _ro(gt=gt, pred=pred, lr=lr, seen=seen)


@functools.lru_cache(maxsize=None)
def anchored_frames(H, W):
    return make_anchored(H, W, A_SEEDS.get((H, W), 0))


def case_of(form, H, W, dyadic=False):
    """(what the device is handed, the fp32 frame it must score, gt, score() keywords) of one form on the shape's shared frames."""
    f = frames(H, W)
    kind, dt = form.split("-")
    Ch = FORMS[form][1]
    gt = (f.dgt if dyadic else f.gt)[:, :Ch]
    if dt == "i8":
        q, scale = (f.dq, DY_SCALE) if dyadic else (f.q, SCALE)
        return q[:, :Ch], IO.dequant(q[:, :Ch], scale, ZERO), gt, dict(scale=scale, zero=ZERO)
    pred = (f.dpred if dyadic else f.pred)[:, :Ch]
    return pred, pred, gt, {}


@functools.lru_cache(maxsize=None)
def want_of(form, H, W, dyadic=False):
    _, seen, gt, _ = case_of(form, H, W, dyadic)
    return Q.metrics(seen, gt, FORMS[form][0])


def exact_mse(form, H, W):
    """mse of the dyadic frames from the integer sum of squared differences (every term a multiple of 2^-16: any order is exact),
    by the expressions of eval_finish (csrc/sesrq_eval.hip: sse / (C * px) and 65025.0 * (sse / px))."""
    f = frames(H, W)
    Ch = FORMS[form][1]
    pk = (f.dq_k if form.endswith("i8") else f.dpred_k)[:, :Ch]
    sse_k = ((f.dgt_k[:, :Ch] - pk) ** 2).reshape(2, -1).sum(axis=1)
    assert sse_k.dtype == np.int64 and (sse_k < 2 ** 53).all()
    sse = sse_k.astype(np.float64) / 65536.0
    px = float(H) * W
    return sse / (Ch * px) if Ch == 3 else 65025.0 * (sse / px)


def ssim_maps(seen, gt):
    """Per frame, the map whose mean is the frame's SSIM: the mean over channels of the oracle's per-channel maps, (N, H - 6, W - 6)."""
    return np.array([np.mean([Q.ssim_map(gt[n, c], np.clip(seen[n, c].astype(np.float64), 0, 1)) for c in range(gt.shape[1])], axis=0)
                     for n in range(gt.shape[0])])


def seam_mutants(H, W):
    """[(name, axis, index into the SSIM map)]: the last column / row of a tile and the first of its neighbour, at every tile boundary.
    Tile (by, bx) owns map rows [by RH, (by + 1) RH) and map columns [bx OW, (bx + 1) OW) (o0 / o1 and s_c0 / s_c1 less PAD)."""
    out = []
    for b in range(1, nbx(W)):
        out += [(f"last column of tile column {b - 1}", 1, b * OW - 1), (f"first column of tile column {b}", 1, b * OW)]
    for b in range(1, nby(H)):
        out += [(f"last row of tile row {b - 1}", 0, b * RH - 1), (f"first row of tile row {b}", 0, b * RH)]
    return out


def noisy_maps(H, W):
    """name -> (2, H - 6, W - 6) SSIM maps of every noisy case the GPU sweep scores at this shape."""
    out = {}
    if (H, W) in SHAPES:
        for form in ("rgb-f32", "rgb-i8", "y255-f32", "y255-i8"):           # x2-f32 scores the frames (and SSIM) of rgb-f32
            _, seen, gt, _ = case_of(form, H, W)
            out[form] = ssim_maps(seen, gt)
    if (H, W) in A_SHAPES:
        a = anchored_frames(H, W)
        out["x2-anchored"] = ssim_maps(a.seen, a.gt)
    return out


def weakest_mutant(H, W, maps=None):
    """(smallest move of a frame's SSIM over every noisy case, frame and seam mutant of the shape, which one).  Dropping a column from
    the sum and counting it twice move the mean by the same amount with opposite signs: |sum of the column| / size of the map."""
    worst = (np.inf, None)
    for name, m in (maps or noisy_maps(H, W)).items():
        for what, axis, i in seam_mutants(H, W):
            line = np.take(m, i, axis=axis + 1)
            for n in range(m.shape[0]):
                base = m[n].mean(dtype=np.float64)
                dropped = (m[n].sum(dtype=np.float64) - line[n].sum(dtype=np.float64)) / m[n].size
                doubled = (m[n].sum(dtype=np.float64) + line[n].sum(dtype=np.float64)) / m[n].size
                move = min(abs(dropped - base), abs(doubled - base))
                if move < worst[0]:
                    worst = (move, (name, n, what))
    return worst


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_shape_lists_cross_every_seam():
    """The restated geometry is the library's (its workspace is 16 bytes per (frame, tile, channel)), the sweep has frames on both
    sides of every step of nbx and nby, last tiles that own exactly one SSIM column / row, and partly filled last lanes at W % 4 == 0."""
    from sesrq import quality
    lib = quality.lib()
    for H, W in SHAPES + A_SHAPES:
        for Ch in (1, 3):
            assert lib.sesrq_eval_workspace_bytes(2, Ch, H, W) == 2 * nbx(W) * nby(H) * Ch * 16, (H, W)
    assert len(SHAPES) == 2 * len(WS) + 2 * len(HS) - 4
    assert [nbx(W) for W in (254, 255, 502, 503)] == [1, 2, 2, 3] and [nby(H) for H in (38, 39, 70, 71)] == [1, 2, 2, 3]
    for W in (255, 503):
        assert (W - 2 * PAD) - (nbx(W) - 1) * OW == 1 and (7, W) in SHAPES and (39, W) in SHAPES
    for H in (39, 71):
        assert (H - 2 * PAD) - (nby(H) - 1) * RH == 1 and (H, 9) in SHAPES and (H, 255) in SHAPES
    assert {(H, W) for H, W in A_SHAPES if nbx(W) >= 2} and {(H, W) for H, W in A_SHAPES if nby(H) >= 2}
    assert all(H % 2 == 0 and W % 2 == 0 for H, W in A_SHAPES) and (72, 256) in A_SHAPES and nby(72) == 3
    for H, W in SHAPES:
        f = frames(H, W)
        assert not np.array_equal(f.gt[0], f.gt[1]) and ((f.pred > 1).any() and (f.pred < 0).any())
        d = IO.dequant(f.q, SCALE, ZERO)
        assert d.max() > 1 and d.min() < 0
        # the dyadic frames are on the grid, as fp32 frames and as the int8 frames' dequantised values
        assert np.array_equal(f.dgt.astype(np.float64) * 256, f.dgt_k)
        assert np.array_equal(np.clip(f.dpred.astype(np.float64), 0, 1) * 256, f.dpred_k)
        assert np.array_equal(np.clip(IO.dequant(f.dq, DY_SCALE, ZERO).astype(np.float64), 0, 1) * 256, f.dq_k)


def test_oracle_matches_scipy_on_the_seam_shapes():
    pytest.importorskip("scipy")
    for H, W in SHAPES:
        f = frames(H, W)
        p = np.clip(f.pred.astype(np.float64), 0, 1)
        for n in range(2):
            for c in range(3):
                got, want = Q.ssim_channel(f.gt[n, c], p[n, c]), _ssim_scipy(f.gt[n, c], p[n, c])
                assert abs(got - want) <= 1e-9, (H, W, n, c, got, want)


def test_seam_mutants_move_the_oracle():
    """The sweep has teeth: on every shape with a tile boundary and every noisy case it scores, the oracle's SSIM with one seam column
    (row) left out of the sum, or counted twice, under the unchanged divisor is >= 10x the tolerance away from the oracle's SSIM --
    a kernel with that off-by-one cannot pass.  A frame that fails this is a bad input: give the shape another seed (SEEDS)."""
    seen = 0
    for H, W in sorted(set(SHAPES + A_SHAPES)):
        if not seam_mutants(H, W):
            continue
        move, which = weakest_mutant(H, W)
        assert move >= 10 * TOL_SSIM, (H, W, move, which)
        seen += 1
    assert seen == sum(1 for H, W in set(SHAPES + A_SHAPES) if nbx(W) >= 2 or nby(H) >= 2) >= 30


# -------------------------------------------------------------------------------------------- conditioning cases (39 x 255: 2 x 2 tiles)
CH, CW = 39, 255


def _fp32_quotient_ssim(seen, gt):
    """The kernel's documented rounding and nothing else: fp64 moments, the five inputs of the quotient and the quotient in fp32
    (csrc/sesrq_eval.hip, `if (emit)`), the map summed in fp64."""
    out = []
    for n in range(gt.shape[0]):
        acc = []
        for c in range(gt.shape[1]):
            ux, uy, vx, vy, vxy = (m.astype(F32) for m in Q.window_moments(np.clip(seen[n, c].astype(np.float64), 0, 1), gt[n, c]))
            C1, C2 = F32(0.01) * F32(0.01), F32(0.03) * F32(0.03)
            A1, A2 = F32(2) * ux * uy + C1, F32(2) * vxy + C2
            B1, B2 = ux * ux + uy * uy + C1, vx + vy + C2
            s = (A1 * A2) / (B1 * B2)
            assert s.dtype == F32
            acc.append(s.mean(dtype=np.float64))
        out.append(np.mean(acc))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def conditioning_cases():
    """name -> (pred as handed to the device, the fp32 frame scored, gt, score() keywords); all (2, 3, 39, 255), two different frames."""
    rng = np.random.default_rng(39255)
    shape = (2, 3, CH, CW)
    noise = lambda lo, hi: (lo + (hi - lo) * rng.random(shape)).astype(F32)
    const = lambda a, b: np.concatenate([np.full((1,) + shape[1:], a, F32), np.full((1,) + shape[1:], b, F32)])
    yy, xx = np.meshgrid(np.arange(CH), np.arange(CW), indexing="ij")
    board = np.broadcast_to(((yy + xx) & 1).astype(F32), shape).copy()
    cases = {}

    def f32(name, pred, gt):
        cases[name] = (pred, pred, gt, {})

    def i8(name, q, gt, scale=SCALE, zero=ZERO):
        q = q.astype(np.int8)
        cases[name] = (q, IO.dequant(q, scale, zero), gt, dict(scale=scale, zero=zero))

    f32("constant, pred == gt", const(0.5, 0.25), const(0.5, 0.25))
    f32("constant, pred != gt", const(0.7, 0.1), const(0.3, 0.9))
    i8("constant, pred != gt, int8", np.concatenate([np.full((1,) + shape[1:], 44), np.full((1,) + shape[1:], -88)]), const(0.3, 0.9))
    f32("bright and nearly flat", noise(0.9989, 0.9991), noise(0.9989, 0.9991))
    f32("dark and nearly flat", noise(0.0009, 0.0011), noise(0.0009, 0.0011))
    i8("dark and nearly flat, int8", rng.integers(-110, -108, shape), noise(0.0009, 0.0011))
    f32("checkerboard against its inverse and against noise", np.concatenate([1 - board[:1], noise(0, 1)[:1]]), board)
    i8("checkerboard, int8", np.where(np.concatenate([1 - board[:1], board[:1]]) > 0, 110, -110), board)
    f32("pred > 1 everywhere", noise(1.01, 2.0), noise(0, 1))
    i8("pred > 1 everywhere, int8", rng.integers(111, 128, shape), noise(0, 1))
    f32("pred < 0 everywhere", noise(-2.0, -0.01), noise(0, 1))
    i8("pred < 0 everywhere, int8", rng.integers(-128, -110, shape), noise(0, 1))
    f32("gt far outside [0, 1]", noise(-0.1, 1.1), noise(-1.0, 2.5))
    for zero in (-128, 127):
        q = rng.integers(-128, 128, shape)
        q[:, :, 0, 0], q[:, :, -1, -1] = -128, 127
        i8(f"int8 zero point {zero}", q, noise(0, 1), zero=zero)
    same = noise(0, 1)
    f32("mse == 0 on noise", same, same.copy())
    q = rng.integers(-128, 128, shape).astype(np.int8)
    i8("mse == 0 on noise, int8", q, np.clip(IO.dequant(q, SCALE, ZERO), 0, 1).astype(F32))
    for v in cases.values():
        for a in v[:3]:
            a.setflags(write=False)
    return cases


def _closed_form(x, y):
    """SSIM of two constant frames: the variances are exactly 0."""
    x, y = float(np.clip(F32(x), 0, 1)), float(F32(y))
    return (2 * x * y + 1e-4) / (x * x + y * y + 1e-4)


CLOSED = {"constant, pred == gt": ((0.5, 0.5), (0.25, 0.25)), "constant, pred != gt": ((0.7, 0.3), (0.1, 0.9)),
          "constant, pred != gt, int8": ((F32(154) * F32(SCALE), 0.3), (F32(22) * F32(SCALE), 0.9))}
MSE_ZERO = ("constant, pred == gt", "mse == 0 on noise", "mse == 0 on noise, int8")
EPS_PSNR = 10.0 * np.log10(255.0 ** 2 / 1e-8)


def test_conditioning_cases_are_what_they_say():
    cases = conditioning_cases()
    assert len(cases) == 17
    for name, (pred, seen, gt, kw) in cases.items():
        assert seen.dtype == F32 and gt.dtype == F32 and seen.shape == gt.shape == (2, 3, CH, CW), name
        assert (pred.dtype == np.int8) == bool(kw) == ("int8" in name), name
        assert not np.array_equal(seen[0], seen[1]) or not np.array_equal(gt[0], gt[1]), name
    seen = lambda n: cases[n][1]
    assert (seen("pred > 1 everywhere") > 1).all() and (seen("pred > 1 everywhere, int8") > 1).all()
    assert (seen("pred < 0 everywhere") < 0).all() and (seen("pred < 0 everywhere, int8") < 0).all()
    g = cases["gt far outside [0, 1]"][2]
    assert g.min() < -0.99 and g.max() > 2.49
    for n in ("bright and nearly flat", "dark and nearly flat", "dark and nearly flat, int8"):
        c = 0.999 if "bright" in n else 0.001
        assert np.abs(cases[n][2].astype(np.float64) - c).max() <= 1e-4 + 2.0 ** -24 and np.ptp(cases[n][2]) > 1.9e-4, n
        assert np.ptp(seen(n)) > 0 and (seen(n) >= 0).all() and (seen(n) <= 1).all(), n
    for zero in (-128, 127):
        q = cases[f"int8 zero point {zero}"][0]
        assert q.min() == -128 and q.max() == 127
    for n in MSE_ZERO:
        assert np.array_equal(np.clip(seen(n), 0, 1), cases[n][2]), n
    for n, pairs in CLOSED.items():
        for k, (x, y) in enumerate(pairs):
            assert (seen(n)[k] == F32(x)).all() and (cases[n][2][k] == F32(y)).all(), (n, k)
            assert abs(Q.metrics(seen(n), cases[n][2], 3)[k, 2] - _closed_form(x, y)) <= 1e-9, (n, k)


def test_fp32_quotient_stays_within_tolerance_on_the_conditioning_cases():
    """What the design promises (csrc/sesrq_eval.hip header: fp64 moments, only the final quotient fp32) holds the tolerance on every
    conditioning case, for the three-channel forms and for channel 0 alone (Y255)."""
    for name, (_, seen, gt, _) in conditioning_cases().items():
        for Ch in (3, 1):
            got = _fp32_quotient_ssim(seen[:, :Ch], gt[:, :Ch])
            want = Q.metrics(seen[:, :Ch], gt[:, :Ch], 3 if Ch == 3 else 5)[:, 2]
            assert np.abs(got - want).max() <= TOL_SSIM, (name, Ch, got, want)


def test_oracle_propagates_nan_like_np_clip():
    f = frames(39, 255)
    for where in ("pred", "gt"):
        p, g = np.concatenate([f.pred, f.pred[:1]]), np.concatenate([f.gt, f.gt[:1]])
        (p if where == "pred" else g)[1, 2, 0, 0] = np.nan
        for mflag in (3, 6):
            m = Q.metrics(p, g, mflag)
            assert np.isnan(m[1]).all() and np.isfinite(m[[0, 2]]).all(), (where, mflag, m)


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _crossed_both_seams(ran):
    assert any(nbx(W) >= 2 for _, W in ran) and any(nby(H) >= 2 for H, _ in ran) and any(nbx(W) >= 3 for _, W in ran) \
        and any(nby(H) >= 3 for H, _ in ran), ran


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_seam_sweep(form):
    """One tile kernel over every seam shape: noise frames against the oracle; k/256 frames against the oracle and, for RGB and Y255,
    mse against the exact integer sum, bit for bit."""
    from sesrq import quality
    mflag, Ch, kernel = FORMS[form]
    before = quality.kernels()[kernel]
    ran = []
    for H, W in SHAPES:
        pred, _, gt, kw = case_of(form, H, W)
        want = want_of(form, H, W)
        _check(_score(pred, gt, mflag, **kw), want[:, 1], want[:, 2], (form, H, W))
        pred, _, gt, kw = case_of(form, H, W, dyadic=True)
        want = want_of(form, H, W, True)
        got = _score(pred, gt, mflag, **kw)
        _check(got, want[:, 1], want[:, 2], (form, H, W, "k/256"))
        if mflag != 6:
            exact = exact_mse(form, H, W)
            assert got[:, 0].tobytes() == exact.tobytes(), (form, H, W, got[:, 0], exact)
        ran.append((H, W))
    assert quality.kernels()[kernel] - before == 2 * len(SHAPES) and ran == SHAPES
    _crossed_both_seams(ran)


@pytest.mark.gpu
def test_seam_sweep_anchored():
    from sesrq import quality
    before = quality.kernels()["eval_tile<f32,x2>"]
    ran = []
    for H, W in A_SHAPES:
        a = anchored_frames(H, W)
        want = Q.metrics(a.seen, a.gt, 6)
        got = _score_anchored(a.pred, a.lr, a.gt)
        _check(got, want[:, 1], want[:, 2], ("anchored", H, W))
        assert np.array_equal(got, _score(a.seen, a.gt, 6)), ("anchored vs the frame formed beforehand", H, W)
        ran.append((H, W))
    assert quality.kernels()["eval_tile<f32,x2>"] - before == 2 * len(A_SHAPES)
    _crossed_both_seams(ran)


def _offset_view(a, off, torch):
    """The array on the device at data_ptr() % 16 == off: a view into a larger tensor."""
    t = torch.from_numpy(np.array(a, order="C", copy=True))
    big = torch.empty(t.numel() + 16, dtype=t.dtype, device=device())
    lead = ((off - big.data_ptr()) % 16) // t.element_size()
    v = big[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off and v.is_contiguous()
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("W", [12, 252, 256])
def test_both_load_paths_give_the_same_bits(W):
    """include/sesrq_eval.h, "Caller buffers": the 16-byte loads (W % 4 == 0, pred and gt aligned) and the scalar loads (either one
    4 bytes off; an int8 pred 1 byte off) score the same data to the same bits."""
    import torch
    from sesrq import quality
    H = 39
    for form, (mflag, Ch, _) in FORMS.items():
        pred, _, gt, kw = case_of(form, H, W)
        poff = 1 if pred.dtype == np.int8 else 4
        base = quality.score(_offset_view(pred, 0, torch), _offset_view(gt, 0, torch), mflag, **kw)
        for po, go in ((poff, 0), (0, 4), (poff, 4)):
            p, g = _offset_view(pred, po, torch), _offset_view(gt, go, torch)
            got = quality.score(p, g, mflag, **kw)
            torch.cuda.synchronize()
            assert torch.equal(got, base), (form, W, po, go, got, base)
    H = 40
    a = anchored_frames(H, W)
    base = quality.score_anchored(_offset_view(a.pred, 0, torch), _offset_view(a.lr, 0, torch), _offset_view(a.gt, 0, torch))
    for po, lo, go in ((4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 4, 4)):
        got = quality.score_anchored(_offset_view(a.pred, po, torch), _offset_view(a.lr, lo, torch), _offset_view(a.gt, go, torch))
        torch.cuda.synchronize()
        assert torch.equal(got, base), ("anchored", W, po, lo, go, got, base)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(conditioning_cases()))
def test_conditioning(name):
    pred, seen, gt, kw = conditioning_cases()[name]
    forms = ((3, 3), (5, 1)) if kw else ((3, 3), (5, 1), (6, 3))
    for mflag, Ch in forms:
        want = Q.metrics(seen[:, :Ch], gt[:, :Ch], mflag)
        got = _score(pred[:, :Ch], gt[:, :Ch], mflag, **kw)
        assert np.isfinite(got[:, [0, 2]]).all(), (name, mflag, got)
        _check(got, want[:, 1], want[:, 2], (name, mflag))
        if name in CLOSED:
            for k, (x, y) in enumerate(CLOSED[name]):
                assert abs(got[k, 2] - _closed_form(x, y)) <= TOL_SSIM, (name, mflag, k, got[k, 2])
        if name in MSE_ZERO:
            assert (got[:, 0] == 0.0).all() and (got[:, 2] == 1.0).all(), (name, mflag, got)
            if mflag == 3:
                assert np.isposinf(got[:, 1]).all(), (name, got)
            else:
                assert np.allclose(got[:, 1], EPS_PSNR, rtol=0, atol=1e-9), (name, mflag, got)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(7, 7), (9, 12)])
def test_300_one_tile_frames_score_as_each_alone(H, W):
    """One tile per frame: eval_finish has fewer partials (1 or 3) than threads.  Every row of the batch has the bits of its frame alone."""
    import torch
    from sesrq import quality
    N = 300
    rng = np.random.default_rng([N, H, W])
    gt = rng.random((N, 3, H, W), dtype=F32)
    pred = (rng.random((N, 3, H, W), dtype=F32) * F32(1.2) - F32(0.1)).astype(F32)
    q = rng.integers(-128, 128, (N, 3, H, W)).astype(np.int8)
    assert len({gt[n].tobytes() for n in range(N)}) == N and len({pred[n].tobytes() for n in range(N)}) == N
    for form, (mflag, Ch, _) in FORMS.items():
        p, kw = (q, dict(scale=SCALE, zero=ZERO)) if form.endswith("i8") else (pred, {})
        p, g = _dev(p[:, :Ch]), _dev(gt[:, :Ch])
        batch = quality.score(p, g, mflag, **kw)
        alone = torch.cat([quality.score(p[n:n + 1], g[n:n + 1], mflag, **kw) for n in range(N)])
        torch.cuda.synchronize()
        assert torch.equal(batch, alone), (form, H, W, (batch != alone).nonzero()[:4])
        assert len(torch.unique(batch[:, 2])) > N // 2
        k = [0, 1, 150, 299]
        seen = IO.dequant(q[k][:, :Ch], SCALE, ZERO) if form.endswith("i8") else pred[k][:, :Ch]
        want = Q.metrics(seen, gt[k][:, :Ch], mflag)
        _check(batch[k].cpu().numpy(), want[:, 1], want[:, 2], (form, H, W))


NAN_PLACES = {"corner": (7, 9, 0, 0), "seam": (CH, CW, 20, OW + PAD)}      # (H, W, row, column): column 251 is tile column 1's first SSIM column


@pytest.mark.gpu
@pytest.mark.parametrize("place", list(NAN_PLACES))
@pytest.mark.parametrize("where", ["pred", "gt"])
def test_nan_in_a_frame_is_that_frames_score(where, place):
    """include/sesrq_eval.h: a NaN in pred (fp32) or in gt makes that frame's mse, psnr and ssim NaN, as the reference's np.clip does;
    the other frames of the batch keep their bits.  The anchored entry too, with the NaN in pred or in the LR frame."""
    H, W, r, c = NAN_PLACES[place]
    f = frames(H, W)
    three = lambda a: np.concatenate([a, a[:1]])
    for form, (mflag, Ch, _) in FORMS.items():
        if where == "pred" and form.endswith("i8"):
            continue
        pred, _, gt, kw = case_of(form, H, W)
        pred, gt = three(pred), three(gt)
        clean = _score(pred, gt, mflag, **kw)
        assert np.isfinite(clean).all()
        (pred if where == "pred" else gt)[1, Ch - 1, r, c] = np.nan
        got = _score(pred, gt, mflag, **kw)
        assert np.isnan(got[1]).all(), (form, where, place, got)
        assert got[[0, 2]].tobytes() == clean[[0, 2]].tobytes(), (form, where, place, got, clean)
    H, W = H + 1, W + 1
    a = anchored_frames(H, W)
    clean = _score_anchored(three(a.pred), three(a.lr), three(a.gt))
    assert np.isfinite(clean).all()
    for target in (("pred", "lr") if where == "pred" else ("gt",)):
        t = {"pred": three(a.pred), "lr": three(a.lr), "gt": three(a.gt)}
        t[target][1, 2, r // 2 if target == "lr" else r, c // 2 if target == "lr" else c] = np.nan
        got = _score_anchored(t["pred"], t["lr"], t["gt"])
        assert np.isnan(got[1]).all(), ("anchored", target, place, got)
        assert got[[0, 2]].tobytes() == clean[[0, 2]].tobytes(), ("anchored", target, place, got, clean)
