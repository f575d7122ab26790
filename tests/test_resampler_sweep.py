"""tests/resampler_sweep.py on the CPU: the reachable sets of every weight vector of the three bicubic resamplers, the builder that
realises a sum, and -- on the oracles -- that a sweep frame isolates one pass and that its targets do not touch each other.

  reach            the DP against brute force on short vectors; the counts of unreachable sums of the downscale (56 of 77 521 at
                   r = 2, 162 of 1 224 001 at r = 4, all within 2000 of the ends) and of the upscale phases (r = 2: only multiples
                   of 8; r = 4: 3192 in phases 0 and 3, 352 of them further than 2000 from both ends, 552 in phases 1 and 2)
  Q6 values        the upscale sweeps are defined on floor((T + 8) / 16): every integer between a phase's minimum and maximum is
                   reached but 9 (r = 2) or 7 (r = 4, phases 0 and 3) values, all within 13 of an end; both edges of each bin
  builder          sum w b == T for every target of every weight vector
  frames           a frame of constant rows (columns) is its own horizontal (vertical) pass in tests/downscale_oracle.py and in
                   tests/colour_oracle.py's upscale; the sums at the sweep positions are the targets whatever the neighbouring
                   windows hold, and rewriting one window changes no other sweep position
  palette          every 4-tuple of the nine colours is the four taps of every phase once"""
import itertools

import numpy as np
import pytest

import colour_oracle as CO
import downscale_oracle as DO
import resampler_sweep as RS
import video_oracle as VO

PHASES = [(r, phi) for r in (2, 4) for phi in range(r)]


@pytest.mark.parametrize("w", [(3,), (-5,), (3, -5), (-24, 232), (7, 7), (-2, 6, 255)])
def test_reach_equals_brute_force(w):
    R = RS.Reach(w)
    want = np.zeros(1, np.int64)
    for k in w:                                                              # every sum, tap by tap, as a set
        want = np.unique(want[:, None] + k * np.arange(256)[None, :])
    assert np.array_equal(R.values(), want)
    assert R.lo == want[0] and R.hi == want[-1] and R.unreachable().size == R.hi - R.lo + 1 - want.size
    taps = R.taps_for(want)
    assert taps.dtype == np.uint8 and np.array_equal(taps.astype(np.int64) @ np.asarray(w), want)
    assert not R.has([R.lo - 1, R.hi + 1]).any() and R.has([R.lo, R.hi]).all()


@pytest.mark.parametrize("r,span,lo,hi,missing", [(2, 77521, -6120, 71400, 56), (4, 1224001, -89760, 1134240, 162)])
def test_downscale_reachable_sets(r, span, lo, hi, missing):
    R = RS.downscale_reach(r)
    assert R.w == DO.WEIGHTS[r] and sum(R.w) == DO.D[r]
    assert (R.lo, R.hi, R.hi - R.lo + 1) == (lo, hi, span)
    u = R.unreachable()
    assert u.size == missing and np.minimum(u - R.lo, R.hi - u).max() < 2000
    D = DO.D[r]
    assert R.lo + 2000 < -D // 2 and 256 * D + D // 2 < R.hi - 2000          # both clamp thresholds lie in the dense part
    assert R.has(np.arange(R.lo + 2000, R.hi - 2000 + 1)).all()
    v = RS.downscale_targets(r)
    assert v.size == span - missing
    taps = R.taps_for(v)                                                     # the builder, for every target
    assert np.array_equal(taps.astype(np.int64) @ np.asarray(R.w), v)


@pytest.mark.parametrize("r,phi", PHASES)
def test_upscale_reachable_sets_and_their_q6_values(r, phi):
    R = RS.upscale_reach(r, phi)
    assert R.w == CO.WEIGHTS[r][phi] and sum(R.w) == 1024
    u = R.unreachable()
    edge = np.minimum(u - R.lo, R.hi - u)
    if r == 2:
        assert all(w % 8 == 0 for w in R.w) and (R.values() % 8 == 0).all()
        on = u % 8 == 0                                                      # of the multiples of 8 ...
        assert on.sum() == 56 and edge[on].max() < 2000                      # ... 56 are unreachable, all near the ends
    else:
        assert (u.size, int((edge > 2000).sum())) == {0: (3192, 352), 1: (552, 0), 2: (552, 0), 3: (3192, 352)}[phi]
    lo, hi = RS.upscale_range(r, phi)
    assert (lo, hi) == {2: (-1530, 17850), 4: ((-1912, 18233) if phi in (0, 3) else (-892, 17213))}[r]
    q = RS.upscale_q6(r, phi)
    miss = np.setdiff1d(np.arange(lo, hi + 1), q)
    assert miss.size == (9 if r == 2 else 7 if phi in (0, 3) else 0)
    assert miss.size == 0 or np.minimum(miss - lo, hi - miss).max() <= 13
    assert q[0] == lo and q[-1] == hi and lo < -32 and hi > 255 * 64 + 31    # beyond both clamps of the chroma byte

    t = RS.upscale_targets(r, phi)
    v = R.values()
    assert R.has(t).all() and np.array_equal(np.unique(RS.q6_of(t)), q)
    qv = RS.q6_of(v)
    for q_at in (lo, -33, -32, -1, 0, 1, 8191, 255 * 64 + 31, 255 * 64 + 32, hi):     # the edges of a bin are the bin's own extremes
        inside = v[qv == q_at]
        mine = t[RS.q6_of(t) == q_at]
        assert inside.size and mine[0] == inside[0] and mine[-1] == inside[-1]
    far = (q > lo + 256) & (q < hi - 256) if r == 2 else np.ones(q.size, bool)
    lows = np.array([t[RS.q6_of(t) == k][0] for k in q[far][::97]])
    highs = np.array([t[RS.q6_of(t) == k][-1] for k in q[far][::97]])
    if r == 2:
        assert np.array_equal(lows, 16 * q[far][::97] - 8) and np.array_equal(highs, 16 * q[far][::97])
    else:
        dense = np.minimum(q[far][::97] - lo, hi - q[far][::97]) > 3200 // 16 + 1
        assert np.array_equal(lows[dense] % 16, np.full(dense.sum(), 8)) and np.array_equal(highs[dense] % 16, np.full(dense.sum(), 7))
    taps = R.taps_for(t)                                                     # the builder, for every target and for every reachable T
    assert np.array_equal(taps.astype(np.int64) @ np.asarray(R.w), t)
    assert np.array_equal(R.taps_for(v).astype(np.int64) @ np.asarray(R.w), v)


def _some(values, around, rng, n=40):
    """A few targets: both ends, those next to each of `around`, and random ones, shuffled."""
    near = np.concatenate([values[np.abs(values - a) <= 2] for a in around])
    return rng.permutation(np.unique(np.r_[values[:3], values[-3:], near, rng.choice(values, n, replace=False)]))


@pytest.mark.parametrize("swept", ["vertical", "horizontal"])
@pytest.mark.parametrize("r", [2, 4])
def test_downscale_frames_isolate_one_pass_and_their_windows_are_independent(r, swept):
    rng = np.random.default_rng(r)
    D = DO.D[r]
    t = _some(RS.downscale_targets(r), (-D // 2, D // 2, 256 * D - D // 2, 255 * D + D // 2), rng)
    line, rows, T = RS.downscale_line(r, t)
    assert rows.tolist() == list(range(2, 4 * T.shape[0], 4)) and set(T.reshape(-1).tolist()) == set(t.tolist())
    img = RS.frame_of(line, swept, RS.ACROSS * r)
    assert img.shape == ((1, line.shape[0], 2 * r, 3) if swept == "vertical" else (1, 2 * r, line.shape[0], 3))
    lr, v = DO.downscale(img, r, keep=True)
    want = np.clip((T + D // 2) // D, 0, 255)
    # the identity of the other pass
    if swept == "vertical":
        assert np.array_equal(lr, v[:, :, ::r])                              # constant rows: the horizontal pass changes nothing
        sums = DO.one_pass(img, r, 1, sums=True)
    else:
        assert np.array_equal(v, img[:, :2])                                 # constant columns: the vertical pass changes nothing
        sums = DO.one_pass(v, r, 2, sums=True)
    s, out = RS.along(sums, swept), RS.along(lr, swept)
    for x in range(RS.ACROSS):
        assert np.array_equal(s[rows, x * (r if swept == "vertical" else 1)], T)     # the sums are the targets ...
        assert np.array_equal(out[rows, x], want)                            # ... and the LR bytes their rounding, unattenuated
    assert np.array_equal(DO.one_pass(line, r, 0), out[:, 0])                # the line alone predicts the frame
    assert want.min() == 0 and want.max() == 255 and (T < -D // 2).any() and (T >= 256 * D - D // 2).any()
    # independence: other bytes in window 3 change no other sweep row
    other = line.copy()
    other[r // 2 + 4 * r * 3:r // 2 + 4 * r * 4] = rng.integers(0, 256, (4 * r, 3))
    d = DO.one_pass(other, r, 0, sums=True) != DO.one_pass(line, r, 0, sums=True)
    assert d[rows[3]].any() and not np.delete(d[rows], 3, 0).any()


@pytest.mark.parametrize("swept", ["vertical", "horizontal"])
@pytest.mark.parametrize("r", [2, 4])
def test_upscale_frames_isolate_one_pass_and_their_windows_are_independent(r, swept):
    rng = np.random.default_rng(10 + r)
    phis, ts = [], []
    for phi in range(r):
        t = RS.upscale_targets(r, phi)
        t = _some(t, (-33 * 16, 0, (255 * 64 + 32) * 16), rng, 12)
        phis.append(np.full(t.size, phi)), ts.append(t)
    order = rng.permutation(sum(t.size for t in ts))
    lines, out, phi, T = RS.upscale_lines(r, (np.concatenate(phis)[order], np.concatenate(ts)[order]))
    n = T.shape[1]
    assert lines.shape == (2, RS.STEP * n) and np.array_equal(out, r * (RS.STEP * np.arange(n) + 2) + phi)
    assert not np.array_equal(T[0], T[1])                                    # Cb and Cr carry different targets
    want = RS.q6_of(T)
    for p in range(2):
        plane = RS.frame_of(lines[p], swept, RS.ACROSS)[0]
        v, h = VO.chroma_q6(plane, r, keep=True)
        if swept == "vertical":
            assert np.array_equal(h, np.repeat(64 * plane.astype(np.int64), r, 1))       # constant rows: the horizontal pass is 64 b
            assert all(np.array_equal(v[out[p], x], want[p]) for x in range(r * RS.ACROSS))
        else:
            assert np.array_equal(v, np.repeat(h[:1], r * RS.ACROSS, 0))      # constant columns: the vertical pass changes nothing
            assert np.array_equal(h[0, out[p]], want[p])
        assert np.array_equal(CO.upscale_axis(64 * lines[p].astype(np.int64), r, 0), RS.along(v[None], swept)[:, 0])
    assert want.min() < -32 and want.max() > 255 * 64 + 31
    # independence: other bytes in window 2 change no other sweep position
    other = lines[0].copy()
    other[RS.STEP * 2:RS.STEP * 3] = rng.integers(0, 256, RS.STEP)
    d = CO.upscale_axis(64 * other.astype(np.int64), r, 0) != CO.upscale_axis(64 * lines[0].astype(np.int64), r, 0)
    assert not np.delete(d[out[0]], 2).any()


def test_the_full_lines_hold_every_target_once():
    """The sizes the device tests run at: every target is in the line, no sweep position is spent twice but for the padding."""
    for r in (2, 4):
        phi, t = RS.upscale_pairs(r)
        assert t.size == sum(RS.upscale_targets(r, p).size for p in range(r))
        lines, out, ph, T = RS.upscale_lines(r)
        assert T.size in (t.size, t.size + 1) and lines.shape[1] == RS.STEP * T.shape[1]
        got = set(zip(ph.reshape(-1).tolist(), T.reshape(-1).tolist()))
        assert got == set(zip(phi.tolist(), t.tolist()))
    line, rows, T = RS.downscale_line(2)
    assert np.array_equal(np.unique(T), RS.downscale_targets(2)) and line.shape[0] == 8 * (rows.size + 1)
    assert np.array_equal(DO.one_pass(line, 2, 0, sums=True)[rows], T)


def test_the_palette_line_gives_every_phase_every_four_tuple():
    line, idx = RS.palette_line()
    n = len(RS.PALETTE)
    assert n == 9 and idx.shape == (n ** 4, 4) and len(set(map(tuple, idx.tolist()))) == 6561 and line.shape == (4 * 6561, 3)
    assert set(itertools.product(range(n), repeat=4)) == set(map(tuple, idx.tolist()))
    assert np.array_equal(line.reshape(6561, 4, 3), np.asarray(RS.PALETTE, np.uint8)[idx])
    for r in (2, 4):
        for phi in range(r):
            j = 4 * np.arange(6561) + (2 if CO.FIRST[r][phi] == -2 else 1)  # the LR index whose taps are window m exactly
            assert np.array_equal((j + CO.FIRST[r][phi])[:, None] + np.arange(4), 4 * np.arange(6561)[:, None] + np.arange(4))
    c = CO.chroma(line[None, None])[0, :, 0]                                 # Q6 chroma of the line: both extremes are in it
    assert c.min() == 1024 and c.max() == 15360
