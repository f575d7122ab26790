"""Threshold tables of the fp32 input quantiser -- TEST INFRASTRUCTURE (not collected).

q0 = clamp_b(rint(fl(fl(x / s0) + z0)))  (myQL/quan_func.py:218-225; reciprocal: fl(x * fl(1 / s0)) for the quotient) is a non-decreasing
step function of x for s0 > 0: every operation of the chain is monotone.  Over the total order of sign-magnitude bit patterns from -inf to
+inf (key() below: -0.0 sits directly below +0.0, both quantise alike) it is therefore completely described by 2^b - 1 thresholds:
threshold c is the smallest key whose code is >= qlo + 1 + c.  table() finds them by bisection over keys on
oracle.sesrq_oracle.quantize_input -- numpy's fp32 division is IEEE-exact on the CPU -- and the code of any x is then

    searchsorted(thresholds, key(x), 'right') + qlo            (a NaN: qlo, include/sesrq.h)

which is integer compares only: torch evaluates it on the device for a whole frame with no float arithmetic of its own.
tests/test_input_sweep.py proves the tables against both oracles on the CPU and sweeps the kernels with them on the device.
"""
import functools
from typing import NamedTuple

import numpy as np

from oracle import sesrq_oracle as O

F32 = np.float32
KEY_NINF, KEY_PINF = 0x007FFFFF, 0xFF800000          # key(-inf), key(+inf): every key between them is a number, everything outside a NaN
NKEYS = 1 << 32
MARGIN = 4096                                        # the windowed sweep reaches pred^4096(xlo) .. succ^4096(xhi)


class Domain(NamedTuple):
    s0: float
    z0: int
    b: int = 8
    reciprocal: bool = False

    @property
    def qlo(self):
        return -(1 << (self.b - 1))

    @property
    def qhi(self):
        return (1 << (self.b - 1)) - 1

    @property
    def id(self):
        return f"s{float(F32(self.s0))!r}-z{self.z0}-b{self.b}" + ("-recip" if self.reciprocal else "")


def key(bits):
    """uint32 bit patterns -> int64 keys whose integer order is the total order of the floats (sign-magnitude): negative patterns
    mirrored below 2^31, positive ones shifted above."""
    u = np.asarray(bits).astype(np.int64) & 0xFFFFFFFF
    return np.where(u >> 31 != 0, 0xFFFFFFFF - u, u + (1 << 31))


def unkey(k):
    k = np.asarray(k, np.int64)
    return np.where(k >> 31 != 0, k - (1 << 31), 0xFFFFFFFF - k).astype(np.uint32)


def as_float(bits):
    return np.ascontiguousarray(np.atleast_1d(bits), np.uint32).view(F32)


def as_bits(x):
    return np.ascontiguousarray(np.atleast_1d(x), F32).view(np.uint32)


def is_nan(bits):
    return (np.asarray(bits).astype(np.int64) & 0x7FFFFFFF) > 0x7F800000


def oracle_codes(dom, bits):
    """The numpy oracle's codes of the patterns (no NaN among them: the reference leaves nan.to(int8) undefined)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return O.quantize_input(as_float(bits), dom.s0, dom.z0, dom.reciprocal, dom.b).astype(np.int64)


@functools.lru_cache(maxsize=None)
def table(dom):
    """int64[2^b - 1]: thresholds[c] = the smallest key in [key(-inf), key(+inf)] whose code is >= qlo + 1 + c.  All thresholds are
    bisected at once: 33 oracle calls on 2^b - 1 values."""
    want = np.arange(dom.qlo + 1, dom.qhi + 1, dtype=np.int64)
    lo = np.full(want.shape, KEY_NINF, np.int64)           # code(lo) < want <= code(hi) throughout
    hi = np.full(want.shape, KEY_PINF, np.int64)
    assert oracle_codes(dom, unkey(lo[:1]))[0] == dom.qlo and oracle_codes(dom, unkey(hi[:1]))[0] == dom.qhi, dom
    while (hi - lo > 1).any():
        mid = (lo + hi) >> 1
        up = oracle_codes(dom, unkey(mid)) >= want
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    hi.setflags(write=False)
    return hi


def codes(dom, bits):
    """The expected code of every pattern from the table alone; a NaN gives the lowest code."""
    c = np.searchsorted(table(dom), key(bits), "right") + dom.qlo
    return np.where(is_nan(bits), dom.qlo, c)


def clamp_ends(dom):
    """(key(xlo), key(xhi)) of the range the MFMA staging code clamps x to: fl((-128 - z0) s0), fl((127 - z0) s0)
    (csrc/sesrq_verify.hip)."""
    xlo, xhi = F32((-128.0 - dom.z0) * float(F32(dom.s0))), F32((127.0 - dom.z0) * float(F32(dom.s0)))
    return int(key(as_bits(xlo))[0]), int(key(as_bits(xhi))[0])


def window(dom):
    """[first key, last key] of the windowed sweep: MARGIN patterns beyond the clamp range on either side, within the numbers."""
    a, b = clamp_ends(dom)
    return max(KEY_NINF, a - MARGIN), min(KEY_PINF, b + MARGIN)


def specials():
    """uint32 patterns every sweep carries whatever its window: +-0, +-denormal min and max, +-FLT_MIN, +-FLT_MAX, +-inf."""
    pos = np.array([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000], np.uint32)
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def nans():
    """Quiet and signalling NaNs, both signs, several payloads (quiet bit 22 set / clear; payload ends and a middle)."""
    pay = np.array([0x000001, 0x000002, 0x155555, 0x2AAAAA, 0x3FFFFF, 0x400000, 0x400001, 0x555555, 0x7FFFFF], np.uint32)
    pos = np.uint32(0x7F800000) | pay
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def stride_sample():
    """One pattern of every 2^24: 256 patterns that cross every exponent byte, offset so that none is a special."""
    return (np.arange(256, dtype=np.uint32) << np.uint32(24)) | np.uint32(0x00A5C3E1)
