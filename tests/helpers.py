"""Shared test helpers (oracle <-> product glue).  The oracle is imported here and only here /
in tests: the product package never sees it."""
import json
import os

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
