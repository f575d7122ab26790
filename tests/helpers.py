"""Shared test helpers (oracle <-> product glue).  The oracle is imported here and only here /
in tests: the product package never sees it."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

from conftest import GOLDEN, load_fixture, fixture_input
from oracle import sesrq_oracle as O
import sesrq
from sesrq.bundle import Bundle, LayerParams


def bundle_from_oracle(net: O.Net) -> Bundle:
    return Bundle(layers=[LayerParams(wq=l.wq, add_const=l.add_const, M=l.M, n=l.n, relu=l.relu, M_oc=getattr(l, 'M_oc', None),
                                      n_oc=getattr(l, 'n_oc', None)) for l in net.layers],
                  scale=list(net.scale), zero=list(net.zero), M_res=net.M_res, n_res=net.n_res,
                  pixel_shuffle=net.pixel_shuffle, pe_num=net.pe, pe_acc_bits=net.acc_bits, pe_add_bits=net.add_bits,
                  name=net.name, quan_bits=getattr(net, "quan_bits", 8))


def fixture_case(path):
    fx, meta = load_fixture(path)
    return fx, meta, O.net_from_fixture(fx), fixture_input(fx, meta)


def rand_frame(shape, seed):
    """U[0,1) float32 frames from a seeded CPU generator."""
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32).numpy()


# ---------------------------------------------------------------------------------------------------- device, tensors, hashing
PIXEL_SHUFFLE = {3: 1, 5: 4, 6: 2}       # the reference's mflag -> PixelShuffle factor of the net


def device():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def to_device(a):
    """A fresh contiguous copy of the array on the device: shared oracle results are read-only arrays."""
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(device())


def stream_ptr():
    """The current stream as the C ABI takes it."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device()).cuda_stream)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def full_input(meta):
    """The reference's shared 80 x 960 random frame of a fixture's net."""
    return np.load(os.path.join(GOLDEN, "rand_SR_Input_80x960.npy" if meta["mflag"] == 5 else "rand_DM_Input_80x960.npy"))


def calib_params(case):
    """(float weights, float biases, PixelShuffle) of a .params fixture, by golden case name or by path: what a Calibrator is made of."""
    p, pm = load_fixture(case if case.endswith(".npz") else os.path.join(GOLDEN, f"{case}.params.npz"))
    return [p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], PIXEL_SHUFFLE[pm["mflag"]]


def pass_equals(what, cal, want):
    """A Calibrator after its pass against calib_oracle.Pass: running extrema and the last batch's (scale, zero)."""
    assert cal.run_min == want.run_min, (what, cal.run_min, want.run_min)
    assert cal.run_max == want.run_max, (what, cal.run_max, want.run_max)
    assert cal.last_scale == want.last_scale and cal.last_zero == want.last_zero, (what, cal.last_zero, want.last_zero)


# ---------------------------------------------------------------------------------------------------- the PSNR / SSIM scorers
OW, RH, PAD = 248, 32, 3                    # csrc/sesrq_eval_tile.h (SSIM columns / rows of a tile, window radius)


def nbx(W):
    return -(-(W - 2 * PAD) // OW)          # csrc/sesrq_eval_tile.h geometry()


def nby(H):
    return -(-(H - 2 * PAD) // RH)


def score(pred, gt, mflag, **kw):
    """sesrq.quality.score of fresh device copies of the frames (the shared ones are read-only), as a host array."""
    import torch
    from sesrq import quality
    res = quality.score(to_device(pred), to_device(gt), mflag, **kw)
    torch.cuda.synchronize()
    return res.cpu().numpy()


def score_anchored(pred, lr, gt):
    import torch
    from sesrq import quality
    res = quality.score_anchored(to_device(pred), to_device(lr), to_device(gt))
    torch.cuda.synchronize()
    return res.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- 12-bit RGGB raw frames
def raw_frames():
    return np.load(os.path.join(GOLDEN, "raw", "frames.npz"), allow_pickle=False)


def sites(H, W):
    """Site channel of every pixel: (0,0) R, (0,1) / (1,0) G, (1,1) B."""
    yy, xx = np.meshgrid(np.arange(H) & 1, np.arange(W) & 1, indexing="ij")
    return yy + xx


def spread_like(raw, per_code, fill):
    """(H, W) codes -> (3, H, W): per_code[min(code, 4095)] at the site channel, `fill` elsewhere."""
    H, W = raw.shape
    out = np.full((3, H, W), fill, per_code.dtype)
    np.put_along_axis(out, sites(H, W)[None], per_code[np.minimum(raw, 4095)][None], 0)
    return out


def reference_levels():
    """x(code) for every code 0 .. 4095 as the reference formed it in inp (read off frame (a), which holds every code at every phase)."""
    return raw_frames()["levels_inp"]


def raw_frames_sha():
    return json.loads(str(raw_frames()["meta"]))["sha"]


def raw_frame(f):
    """(raw (H, W) uint16, ground truth (1, 3, H, W) uint16 RGB) of frame f, the bytes the reference ran on: frame (a) is stored,
    (b) and (c) are regenerated (make_raw_golden.natural_raw)."""
    if f == "a":
        F = raw_frames()
        raw, gt16 = F["raw_a"], F["gt16_a"]
    else:
        sys.path.insert(0, GOLDEN)
        from make_raw_golden import natural_raw
        raw, gt16 = natural_raw(f)
        gt16 = gt16[None]
    s = raw_frames_sha()
    assert sha256(raw) == s[f"raw_{f}"] and sha256(gt16) == s[f"gt16_{f}"], f"frame {f} differs from the one the reference ran on"
    return raw, gt16


def ref_inp(f):
    """The reference's fp32 input frame (1, 3, H, W) of frame f, rebuilt from its per-code values and checked against its SHA-256."""
    x = spread_like(raw_frame(f)[0], reference_levels(), np.float32(0))[None]
    assert sha256(x) == raw_frames_sha()[f"inp_{f}"], f
    return x


def ref_gt(f):
    """The reference's fp32 ground truth (1, 3, H, W) of frame f, rebuilt the same way."""
    g = raw_frames()["levels_gt"][np.minimum(raw_frame(f)[1], 4095)]
    assert sha256(g) == raw_frames_sha()[f"gt_{f}"], f
    return g


# ---------------------------------------------------------------------------------------------------- the comparator
def same(name, got, want, *, reshape=False, values=False, cast=None):
    """Raise AssertionError unless `got` (a tensor or an array) IS `want`: identical shape, identical dtype, identical bits (floats are
    compared as unsigned words: -0.0 is not +0.0, a NaN equals only its own payload).  A call site names each relaxation it needs:
    reshape=True accepts equal size and compares in want's shape; values=True compares with != on values, not on words;
    cast=dtype converts `want` first."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = want.cpu().numpy() if hasattr(want, "cpu") else np.asarray(want)
    if cast is not None:
        want = want.astype(cast)
    if reshape:
        assert got.size == want.size, f"{name}: {got.size} elements {got.shape} != {want.size} elements {want.shape}"
        got = got.reshape(want.shape)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {got.dtype} {got.shape} != {want.dtype} {want.shape}"
    g, w = got, want
    if not values and got.dtype.kind == "f":
        words = np.dtype(f"u{got.dtype.itemsize}")
        g, w = np.ascontiguousarray(got).view(words), np.ascontiguousarray(want).view(words)
    bad = np.argwhere(g != w)
    if len(bad):
        i = tuple(int(j) for j in bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {got.size} differ, first at {i}: got {got[i]} want {want[i]}")


# ---------------------------------------------------------------------------------------------------- caller buffers under watch
class Stray(tuple):
    """One run of arena bytes outside every placement that no longer holds the canary: (name, side, offset, length, first bytes).
    side "before": offset -1 is the byte just in front of placement `name`; side "behind": offset 1 is the first byte after it."""
    __slots__ = ()
    name, side, offset, length, data = (property(lambda s, i=i: s[i]) for i in range(5))

    def __repr__(self):
        return f"{self.length} B {self.side} {self.name} at {self.offset:+d}: {bytes(self.data).hex()}"


class Arena:
    """One uint8 tensor with a 256-byte aligned base, filled with a canary, in which a test places the buffers it hands to a kernel.

    The canary is one byte or a short byte pattern whose length divides 256 (laid from the aligned base, so a 4-byte pattern reads as
    one fp32 value at every element-aligned address): what surrounds a placement is then both hostile to a kernel that reads beside
    its input and a witness of a kernel that writes beside its output.  Every placement has at least GAP canary bytes of its own in front and behind."""
    ALIGN = 256
    GAP = 256

    @staticmethod
    def room(*nbytes):
        """Arena bytes that hold placements of these sizes at any offset_mod."""
        return Arena.GAP + sum(Arena.ALIGN + 2 * Arena.GAP + -(-int(n) // Arena.ALIGN) * Arena.ALIGN for n in nbytes)

    def __init__(self, device, nbytes, canary=0x5A):
        import torch
        self.nbytes = int(nbytes)
        raw = torch.empty(self.nbytes + self.ALIGN, dtype=torch.uint8, device=device)
        off = -raw.data_ptr() % self.ALIGN
        self.buf = raw[off:off + self.nbytes]
        assert self.buf.data_ptr() % self.ALIGN == 0
        self.spans = []                       # (start, end, name) in placement order
        self.repaint(canary)

    def _pattern(self, canary):
        import torch
        pat = bytes([canary]) if isinstance(canary, int) else bytes(canary)
        if not pat or self.ALIGN % len(pat):
            raise ValueError("the canary is one byte or a pattern whose length divides 256")
        reps = -(-self.nbytes // len(pat))
        return torch.frombuffer(bytearray(pat), dtype=torch.uint8).repeat(reps)[:self.nbytes].to(self.buf.device)

    def repaint(self, canary):
        """Refill everything outside the placements with `canary` (their contents stay)."""
        self.expect = self._pattern(canary)
        keep = [self.buf[s:e].clone() for s, e, _ in self.spans]
        self.buf.copy_(self.expect)
        for (s, e, _), k in zip(self.spans, keep):
            self.buf[s:e].copy_(k)

    def place(self, shape, dtype, offset_mod=0, fill=None, name=None):
        """A contiguous view of `shape` and `dtype` whose data_ptr() is congruent to offset_mod modulo 256, at least GAP bytes behind the
        previous placement.  fill: a scalar, or an array / tensor of the shape (copied in); None leaves the canary in it."""
        import numpy as np
        import torch
        esz = torch.empty((), dtype=dtype).element_size()
        if not 0 <= offset_mod < self.ALIGN or offset_mod % esz:
            raise ValueError(f"offset_mod {offset_mod} is not a multiple of the element size {esz} below {self.ALIGN}")
        shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape, dtype=np.int64)) * esz
        # two gaps between neighbours: a byte up to GAP - 1 behind a placement is nearer to it than to the next one
        last = self.spans[-1][1] + self.GAP if self.spans else 0
        start = -(-(last + self.GAP) // self.ALIGN) * self.ALIGN + offset_mod
        end = start + n
        if end + self.GAP > self.nbytes:
            raise ValueError(f"arena of {self.nbytes} bytes cannot hold {n} more bytes at {start}")
        if isinstance(fill, np.ndarray):
            fill = torch.from_numpy(np.ascontiguousarray(fill))
        if isinstance(fill, torch.Tensor) and (tuple(fill.shape) != shape or fill.dtype != dtype):
            raise ValueError(f"fill is {fill.dtype} {tuple(fill.shape)}, the placement {dtype} {shape}")
        self.spans.append((start, end, name if name is not None else f"#{len(self.spans)}"))
        view = self.buf[start:end].view(dtype).reshape(shape)
        assert view.data_ptr() % self.ALIGN == offset_mod and view.is_contiguous()
        if isinstance(fill, torch.Tensor):
            view.copy_(fill)
        elif fill is not None:
            view.fill_(fill)
        return view

    def check(self):
        """[Stray] for every run of bytes outside all placements that differs from the canary, relative to the nearest placement
        (to the arena's base, name None, when nothing is placed).  Empty when nobody wrote beside a placement."""
        bad = self.buf != self.expect
        for s, e, _ in self.spans:
            bad[s:e] = False
        idx = bad.nonzero().flatten().cpu().numpy()
        if not len(idx):
            return []
        import numpy as np
        cuts = np.flatnonzero(np.diff(idx) != 1) + 1
        host = None
        out = []
        for run in np.split(idx, cuts):
            p, n = int(run[0]), len(run)
            if host is None:
                host = self.buf.cpu().numpy()
            data = host[p:p + min(n, 16)].tobytes()
            if not self.spans:
                out.append(Stray((None, "behind", p + 1, n, data)))
                continue
            s, e, name = min(self.spans, key=lambda sp: sp[0] - p if p < sp[0] else p - sp[1] + 1)
            out.append(Stray((name, "before", p - s, n, data)) if p < s else Stray((name, "behind", p - e + 1, n, data)))
        return out
