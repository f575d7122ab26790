"""Periodic frames at the geometric limits of the library, and the small oracle run that predicts every byte of them -- TEST
INFRASTRUCTURE.  tests/test_geometry_limits.py runs these.

The C oracle on 16 M pixels takes tens of seconds and a few crops would miss an offset that is wrong only far out.  So a huge frame is
built periodic: x[n, ch, y, c] = pattern[n mod F, ch, y mod P, c mod P].  All five convolutions pad with a constant and the receptive
field is R = 7 pixels on each side (2 + 1 + 1 + 1 + 2), so pixel c of an axis of length D sees what pixel m(c) of the same construction
at length Ds = 3 P + (D mod P) sees:

    m(c) = c                    c < R                (the left / top border)
    m(c) = Ds - (D - c)         c >= D - R           (the right / bottom border; Ds = D mod P keeps the phase)
    m(c) = P + (c mod P)        otherwise            (the interior: R pixels of the same phase on both sides)

An axis of at most 4 P pixels is its own small frame (m = identity).  With PixelShuffle r, output pixel c r + j is output pixel
m(c) r + j of the small frame.  P = 61 is prime: every strip, tile and step of 8, 16, 32, 60 or 64 sees every phase.  Frame n of a batch
is base frame n mod F, F coprime to 8.

The device side brings back mismatch counts and the first mismatching index only: every byte (every fp32 word) is compared, in
slices of the batch so that the expected tensor never exists whole.
"""
import functools

import numpy as np

from oracle import c_oracle as CO
from oracle import sesrq_oracle as O

P = 61
R = 7                      # receptive field of the five convolutions on each side


def small_len(D, period=P):
    """Length of the small axis that predicts an axis of length D."""
    return D if D <= 4 * period else 3 * period + D % period


def gather_map(D, period=P):
    """m: (D,) int64, index into the small axis of small_len(D) pixels."""
    Ds = small_len(D, period)
    c = np.arange(D, dtype=np.int64)
    if Ds == D:
        return c
    m = period + c % period
    m[:R] = c[:R]
    m[D - R:] = Ds - (D - c[D - R:])
    return m


def out_map(D, r, period=P):
    """The same map on the pixel-shuffled axis: output pixel c r + j -> m(c) r + j."""
    m = gather_map(D, period)
    return (m[:, None] * r + np.arange(r, dtype=np.int64)[None, :]).reshape(-1)


def pattern(cin, F, seed):
    """(F, cin, P, P) fp32 in [0, 1): the one random tile a case is made of."""
    return np.random.default_rng(seed).random((F, cin, P, P), dtype=np.float32)


def tile_frame(pat, N, H, W):
    """The periodic frame on the host (small sizes only): (N, cin, H, W)."""
    F = pat.shape[0]
    return np.ascontiguousarray(pat[np.arange(N) % F][:, :, np.arange(H) % P][:, :, :, np.arange(W) % P])


@functools.lru_cache(maxsize=None)
def _small_cached(net_key, net_fn, cin, F, seed, H, W):
    net = net_fn(*net_key)
    pat = pattern(cin, F, seed)
    xs = tile_frame(pat, F, small_len(H), small_len(W))
    res = CO.forward(net, xs)
    q0 = O.quantize_input(pat, net.scale[0], net.zero[0], quan_bits=net.quan_bits).astype(np.int8)
    out = dict(pattern=pat, q0_pattern=q0, x=xs, q_out=res["q_out"], y=res["y"])
    for v in out.values():
        v.setflags(write=False)
    return out


def small_run(net_fn, net_key, cin, F, seed, H, W):
    """The oracle's outputs of the F base frames at the small size of (H, W): computed once per case, shared, read-only."""
    return _small_cached(net_key, net_fn, cin, F, seed, H, W)


def gathered(small_out, N, H, W, r):
    """The expected big output on the host, by the map (small sizes only: the CPU test of the map)."""
    F = small_out.shape[0]
    return small_out[np.arange(N) % F][:, :, out_map(H, r)][:, :, :, out_map(W, r)]


def liveness(small_q, N, H, W, r):
    """(distinct bytes, share of the most frequent one) of the big int8 output, exactly, from the small output and the multiplicity
    of every small pixel under the map."""
    F = small_q.shape[0]
    wn = np.bincount(np.arange(N) % F, minlength=F).astype(np.float64)
    wy = np.bincount(out_map(H, r), minlength=small_q.shape[2]).astype(np.float64)
    wx = np.bincount(out_map(W, r), minlength=small_q.shape[3]).astype(np.float64)
    w = wn[:, None, None, None] * wy[None, None, :, None] * wx[None, None, None, :]
    w = np.broadcast_to(w, small_q.shape)
    counts = np.bincount(small_q.astype(np.int64).ravel() + 128, weights=w.ravel(), minlength=256)
    return int((counts > 0).sum()), float(counts.max() / counts.sum())


# ---------------------------------------------------------------------------------------------------- device side
# The largest single torch gather these helpers issue, in elements.  One index_select producing 2^28 + 80 four-byte elements returned
# wrong rows on the device (see compare_all); every gather up to 2^28 elements has agreed with its banded form.  Asserted at each site,
# so that a future case cannot silently be compared with a corrupted expectation.
GATHER_MAX = 1 << 28


def _gather(t, rows, cols):
    """t[:, :, rows][:, :, :, cols], the axis first that keeps the intermediate small (a frame two pixels wide takes its two columns of
    the tile before its 2^24 rows); the result and the intermediate stay within GATHER_MAX."""
    cols_first = cols.numel() * t.shape[2] <= rows.numel() * t.shape[3]
    mid = t.shape[0] * t.shape[1] * (cols.numel() * t.shape[2] if cols_first else rows.numel() * t.shape[3])
    n = t.shape[0] * t.shape[1] * rows.numel() * cols.numel()
    assert max(n, mid) <= GATHER_MAX, f"one gather of {max(n, mid)} elements: band it"
    return t.index_select(3, cols).index_select(2, rows) if cols_first else t.index_select(2, rows).index_select(3, cols)


def device_frame(pat, N, H, W, dev):
    """The periodic frame on the device from a (F, C, PY, PX) tile of any dtype torch gathers: (N, C, H, W), contiguous,
    out[n, c, y, x] = tile[n mod F, c, y mod PY, x mod PX]; built in bands of rows of at most GATHER_MAX / 2 elements."""
    import torch
    t = torch.from_numpy(np.array(pat, copy=True)).to(dev)
    F, C, PY, PX = t.shape
    nx = torch.arange(W, device=dev) % PX
    out = torch.empty((N, C, H, W), dtype=t.dtype, device=dev)
    full = N // F
    rows = max(1, (GATHER_MAX // 2) // (F * C * W))
    for r0 in range(0, H, rows):
        r1 = min(H, r0 + rows)
        band = _gather(t, torch.arange(r0, r1, device=dev) % PY, nx)             # (F, C, r1 - r0, W)
        if full:
            out[:full * F].view(full, F, C, H, W)[:, :, :, r0:r1].copy_(band.unsqueeze(0).expand(full, *band.shape))
        if N % F:
            out[full * F:, :, r0:r1].copy_(band[:N % F])
        del band
    return out


class Expect:
    """The expected output of a case on the device: the small oracle output and the index vectors of both axes; pieces are gathered
    on demand.  tiled=False: the gather map of the convolution nets (out_map).  tiled=True: a pointwise operation on a frame tiled from
    a (PY, PX) block -- output pixel (y, x) is pixel (y mod PY, x mod PX) of the small output, whose own size is the period (the row
    indices are formed band by band: the frame may have 2^31 rows).  my, mx: the index vectors of the output's rows and columns into
    the small output, given outright (an operation whose output axes are not H r and W r long: a plane cropped from the upscaled one);
    H, W and r are then not looked at."""

    def __init__(self, small, H, W, r, dev, words=True, tiled=False, my=None, mx=None):
        import torch
        self.small = torch.from_numpy(np.array(small, copy=True)).to(dev)
        self.words = words
        if self.small.dtype == torch.float32 and words:
            self.small = self.small.view(torch.int32)            # fp32 is compared as words (words=False: as values, -0.0 == 0.0)
        self.Hr, self.Wr = H * r, W * r
        if my is not None or mx is not None:
            assert my is not None and mx is not None and not tiled
            assert int(np.max(my)) < self.small.shape[2] and int(np.max(mx)) < self.small.shape[3]
            self.Hr, self.Wr = len(my), len(mx)
            ty = torch.from_numpy(np.asarray(my, np.int64)).to(dev)
            self.rows = lambda r0, r1: ty[r0:r1]
            self.mx = torch.from_numpy(np.asarray(mx, np.int64)).to(dev)
        elif tiled:
            PY, PX = self.small.shape[2], self.small.shape[3]
            self.rows = lambda r0, r1: torch.arange(r0, r1, device=dev) % PY
            self.mx = torch.arange(self.Wr, device=dev) % PX
        else:
            my = torch.from_numpy(out_map(H, r)).to(dev)
            self.rows = lambda r0, r1: my[r0:r1]
            self.mx = torch.from_numpy(out_map(W, r)).to(dev)
        self.base = None
        self.F = small.shape[0]

    def frames(self, n0, n1, r0=0, r1=None):
        """Expected frames n0 .. n1 - 1, output rows r0 .. r1 - 1: (n1 - n0, C, r1 - r0, W r)."""
        import torch
        idx = torch.arange(n0, n1, device=self.small.device) % self.F
        if r1 is not None and (r0, r1) != (0, self.Hr):          # a band of one huge frame: gathered on its own
            return _gather(self.small.index_select(0, idx), self.rows(r0, r1), self.mx)
        if self.base is None:
            self.base = _gather(self.small, self.rows(0, self.Hr), self.mx)      # the F base frames
        if n1 - n0 == self.F and n0 % self.F == 0:
            return self.base
        assert (n1 - n0) * self.base[0].numel() <= GATHER_MAX
        return self.base.index_select(0, idx)


def compare_all(got, expect, slice_bytes=1 << 28):
    """(mismatches, first mismatching (n, c, y, x) or None, got there, wanted there): every element of `got` against the gathered
    oracle output, in pieces of at most 256 MiB of `got` -- whole frames of a batch, or bands of rows of a frame larger than that (the
    expected piece and the mismatch mask are the compare's own device memory, and no tensor op runs on more than 2^28 bytes); only
    these scalars leave the device.  (The bands are not only thrift: one torch index_select that gathers more than 2^28 four-byte
    elements returned wrong rows on the device -- 2^28 of 2^28 + 80 words of a one-column frame of 2^24 + 5 rows -- while the
    library's output equalled (q - zero) * scale everywhere and the banded gather.)"""
    import torch
    g = got.view(torch.int32) if got.dtype == torch.float32 and expect.words else got
    N, C, Hr, Wr = g.shape
    assert (Hr, Wr) == (expect.Hr, expect.Wr), (tuple(g.shape), expect.Hr, expect.Wr)
    per = g[0].numel() * g.element_size()
    step = max(1, min(N, slice_bytes // max(per, 1)))
    if step >= expect.F:
        step -= step % expect.F                  # whole periods: the base frames are reused as they are
    rows = Hr if per <= slice_bytes else max(1, slice_bytes // (C * Wr * g.element_size()))
    bad, first = 0, None
    for n0 in range(0, N, step):
        n1 = min(N, n0 + step)
        for r0 in range(0, Hr, rows):
            r1 = min(Hr, r0 + rows)
            want = expect.frames(n0, n1, r0, r1)
            ne = g[n0:n1, :, r0:r1] != want
            k = int(torch.count_nonzero(ne))
            if k and first is None:
                flat = int(ne.reshape(-1).to(torch.uint8).argmax())
                idx = np.unravel_index(flat, tuple(ne.shape))
                at = (int(idx[0]) + n0, int(idx[1]), int(idx[2]) + r0, int(idx[3]))
                first = (at, g[at].item(), want[tuple(int(i) for i in idx)].item())
            bad += k
            del ne, want
    return bad, first
