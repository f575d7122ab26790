"""Sweep frames for the three bicubic resamplers (downscale, colour export, video export) -- TEST INFRASTRUCTURE.
tests/test_resampler_sweep.py checks it on the CPU, tests/test_resampler_sweep_device.py runs the frames on the device.

A pass of a resampler rounds a sum T = sum w_k b_k of tap bytes b_k in 0 .. 255.  Random frames put T near the middle of its range
and {0, 255} frames far outside both clamps; the sums next to a clamp threshold or a byte boundary are met by chance only.  Here:

  Reach            the set of T a weight vector reaches (a boolean DP over the range of the sum, one layer a tap, O(range) a layer:
                   along each residue class mod |w| the nearest reachable predecessor), and taps_for(T): tap bytes that give T exactly
  downscale        every reachable T of the 4 r taps is a target
  upscale          T is not dense (the r = 2 weights are multiples of 8), so the targets are defined on the result
                   q = (512 + 64 T) >> 10 = floor((T + 8) / 16): for every q a phase reaches (every integer between its minimum and
                   maximum but a few within 13 of either end) the lowest and the highest reachable T of its bin, both edges of the floor

A sweep frame makes the other pass an identity: a line that is constant along an axis is its own pass along that axis (downscale:
D / 2 + D v rounds to v; upscale: (512 + 1024 h) >> 10 = h), so a frame whose rows are constant sweeps the vertical pass and one whose
columns are constant the horizontal pass, and an error of the swept pass reaches the output as it is.  Targets sit in tap windows that
do not overlap:

  downscale        LR index 4 i + 2 takes HR indices 4 r i + r / 2 .. 4 r i + r / 2 + 4 r - 1; the three channels carry three targets
  upscale          window m is LR samples 5 m .. 5 m + 4; its target of phase phi is output index r (5 m + 2) + phi, whose taps are
                   5 m .. 5 m + 3 (first tap -2) or 5 m + 1 .. 5 m + 4 (first tap -1); Cb and Cr carry different targets
  colour           chroma comes from RGB triples and cannot be set freely: every 4-tuple of a palette, window m = LR pixels
                   4 m .. 4 m + 3, which output index r (4 m + 2) + phi (first tap -2) or r (4 m + 1) + phi (first tap -1) takes whole
"""
import functools

import numpy as np

import colour_oracle as CO
import downscale_oracle as DO

TOP = 255
FILL = 128                          # bytes of a line outside every window
PALETTE = ((0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (255, 255, 255),
           (128, 128, 128))         # the eight cube corners and mid-grey
ACROSS = 2                          # LR pixels (chroma samples) across the axis that is not swept
STEP = 5                            # LR samples a window of the upscalers


class Reach:
    """The sums T = sum w[k] b[k] with every b[k] in 0 .. 255 of one weight vector, and tap bytes for each of them."""

    def __init__(self, weights):
        self.w = tuple(int(v) for v in weights)
        assert self.w and all(self.w)
        lo, reach, self.layers = 0, np.ones(1, bool), []
        for w in self.w:
            nlo = lo + min(0, w * TOP)
            prev = np.zeros(reach.size + abs(w) * TOP, bool)              # the sums so far, laid into the new range
            prev[lo - nlo:lo - nlo + reach.size] = reach
            if w < 0:
                prev = prev[::-1]                                         # a predecessor t - w s lies above t: mirror the axis
            a = abs(w)
            rows = -(-prev.size // a)
            grid = np.zeros(rows * a, bool)
            grid[:prev.size] = prev
            grid = grid.reshape(rows, a)                                  # a column is a residue class mod |w|: predecessors lie above
            row = np.arange(rows, dtype=np.int32)[:, None]
            near = np.maximum.accumulate(np.where(grid, row, np.int32(-TOP - 2)), axis=0)
            s = (row - near).reshape(-1)[:prev.size]                      # the smallest tap byte that reaches a sum, if any does
            choice = np.where(s <= TOP, s, -1).astype(np.int16)
            if w < 0:
                choice = choice[::-1]
            lo, reach = nlo, choice >= 0
            self.layers.append((lo, np.ascontiguousarray(choice)))
        self.lo, self.hi = lo, lo + reach.size - 1
        self.reach = reach
        self.reach.setflags(write=False)
        assert self.lo == TOP * sum(v for v in self.w if v < 0) and self.hi == TOP * sum(v for v in self.w if v > 0)
        assert reach[0] and reach[-1]

    def values(self):
        """Every reachable T, ascending."""
        return self.lo + np.flatnonzero(self.reach).astype(np.int64)

    def unreachable(self):
        """Every integer of [lo, hi] that no tap bytes give, ascending."""
        return self.lo + np.flatnonzero(~self.reach).astype(np.int64)

    def has(self, T):
        T = np.asarray(T, np.int64)
        ok = (T >= self.lo) & (T <= self.hi)
        return ok & self.reach[np.where(ok, T - self.lo, 0)]

    def taps_for(self, T):
        """Tap bytes (..., len(w)) uint8 with sum w[k] b[..., k] == T, for reachable T."""
        T = np.asarray(T, np.int64)
        assert self.has(T).all(), "a target no tap bytes reach"
        t = T.reshape(-1).copy()
        out = np.empty((t.size, len(self.w)), np.uint8)
        for k in range(len(self.w) - 1, -1, -1):
            lo, choice = self.layers[k]
            s = choice[t - lo].astype(np.int64)
            assert (s >= 0).all()
            out[:, k] = s
            t -= self.w[k] * s
        assert not t.any()
        return out.reshape(T.shape + (len(self.w),))


@functools.lru_cache(maxsize=None)
def downscale_reach(r):
    return Reach(DO.WEIGHTS[r])


@functools.lru_cache(maxsize=None)
def upscale_reach(r, phi):
    return Reach(CO.WEIGHTS[r][phi])


def q6_of(T):
    """The upscalers' pass on bytes of Q6 64 b: (512 + 64 T) >> 10."""
    return (512 + 64 * np.asarray(T, np.int64)) >> 10


def downscale_targets(r):
    """Every reachable T of the downscale at factor r."""
    return downscale_reach(r).values()


def upscale_range(r, phi):
    """(lowest, highest) Q6 result of phase phi."""
    R = upscale_reach(r, phi)
    return int(q6_of(R.lo)), int(q6_of(R.hi))


def upscale_q6(r, phi):
    """Every Q6 result phase phi reaches, ascending.  Not quite every integer of upscale_range: a few values within 13 of either end
    have no reachable T (9 at r = 2, 7 in phases 0 and 3 of r = 4, none in phases 1 and 2; tests/test_resampler_sweep.py counts)."""
    return np.unique(q6_of(upscale_reach(r, phi).values()))


def upscale_targets(r, phi):
    """The lowest and the highest reachable T of every bin floor((T + 8) / 16) = q that holds one: (T ascending, without repeats)."""
    v = upscale_reach(r, phi).values()
    q = q6_of(v)
    first = np.flatnonzero(np.r_[True, q[1:] != q[:-1]])
    last = np.r_[first[1:] - 1, q.size - 1]
    return np.unique(np.r_[v[first], v[last]])


# ------------------------------------------------------------------------------------------------------------------ lines
def downscale_line(r, targets=None):
    """(line (L, 3) uint8, rows (n,), T (n, 3)): LR index rows[i] = 4 i + 2 of the line has the sums T[i] in its three channels.  The
    targets (default: every reachable T) are dealt to the channels in turn, the last one repeated to fill a row of three."""
    R = downscale_reach(r)
    t = np.asarray(downscale_targets(r) if targets is None else targets, np.int64).reshape(-1)
    t = np.r_[t, np.repeat(t[-1:], -t.size % 3)].reshape(-1, 3)
    n, K = t.shape[0], 4 * r
    line = np.full((K * (n + 1), 3), FILL, np.uint8)
    line[r // 2:r // 2 + K * n] = R.taps_for(t).transpose(0, 2, 1).reshape(n * K, 3)
    return line, 4 * np.arange(n, dtype=np.int64) + 2, t


def upscale_pairs(r):
    """Every (phase, T) target of the upscale at factor r: (phi (M,), T (M,))."""
    ts = [upscale_targets(r, phi) for phi in range(r)]
    return np.concatenate([np.full(t.size, phi, np.int64) for phi, t in enumerate(ts)]), np.concatenate(ts)


def upscale_lines(r, pairs=None):
    """(lines (2, L) uint8, out (2, n), phi (2, n), T (2, n)): output index out[p, m] = r (5 m + 2) + phi[p, m] of plane p's line has the
    sum T[p, m].  The targets (default: every one of upscale_pairs) are dealt to Cb and Cr in turn, the last one repeated."""
    phi, t = upscale_pairs(r) if pairs is None else (np.asarray(pairs[0], np.int64), np.asarray(pairs[1], np.int64))
    pad = -t.size % 2
    phi, t = np.r_[phi, np.repeat(phi[-1:], pad)].reshape(-1, 2).T, np.r_[t, np.repeat(t[-1:], pad)].reshape(-1, 2).T
    n = t.shape[1]
    lines = np.full((2, STEP * n), FILL, np.uint8)
    at = STEP * np.arange(n, dtype=np.int64)
    for ph in range(r):
        first = CO.FIRST[r][ph] + 2                                       # 0 or 1: where in the window tap 0 sits
        for p in range(2):
            m = np.flatnonzero(phi[p] == ph)
            lines[p, (at[m] + first)[:, None] + np.arange(4)[None, :]] = upscale_reach(r, ph).taps_for(t[p, m])
    return lines, r * (at[None, :] + 2) + phi, phi, t


def palette_line():
    """((L, 3) uint8, idx (6561, 4)): every 4-tuple of the palette, window m = pixels 4 m .. 4 m + 3."""
    n = len(PALETTE)
    idx = np.stack(np.unravel_index(np.arange(n ** 4), (n,) * 4), 1)
    return np.asarray(PALETTE, np.uint8)[idx.reshape(-1)], idx


# ------------------------------------------------------------------------------------------------------------------ frames
def frame_of(line, swept, across):
    """A line (L, ...) as a frame: swept = "vertical" -> (1, L, across, ...), every row constant; "horizontal" -> (1, across, L, ...),
    every column constant."""
    line = np.asarray(line)
    if swept == "vertical":
        return np.ascontiguousarray(np.broadcast_to(line[None, :, None], (1, line.shape[0], across) + line.shape[1:]))
    assert swept == "horizontal"
    return np.ascontiguousarray(np.broadcast_to(line[None, None], (1, across) + line.shape))


def along(a, swept):
    """The swept axis of a frame (N, H, W, ...) made by frame_of moved to the front of (L, across, ...), frame 0."""
    return a[0] if swept == "vertical" else np.swapaxes(a[0], 0, 1)
