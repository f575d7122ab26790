"""Every fp32 bit pattern through every first-layer input quantiser form.

q0 = clamp_b(rint(fl(fl(x / s0) + z0))) (myQL/quan_func.py:218-225) is what every fp32 frame goes through first, and the one map of the
library whose domain is all 2^32 float patterns.  The MFMA first-layer kernels do not divide (csrc/sesrq_mfma_common.h: x clamped to
[xlo, xhi], the quotient in three instructions, the rounding by a magic add, no clamp of the result), allowed by a device proof
(csrc/sesrq_verify.hip) of a RESTATEMENT of that code against the device's own division.  Here the staging code of the kernels that run
is compared with an independent division: tests/input_sweep.py turns numpy's IEEE division into a threshold table per input domain
(s0, z0, b, reciprocal); a carrier net (tests/constructions.py Carrier: centre taps only) shows the code of every pixel of a frame at
the output; frames are made on the device from consecutive bit patterns, and the output is compared on the device with
LUT[bucketize(key(x))].  Only mismatch counts and the first offending (bit pattern, got, want) come back.

CPU part: every table the device part uses has 2^b - 1 strictly increasing thresholds, equals the numpy oracle and (true division) the
C oracle on +-256 patterns around every threshold, on 2^22 seeded patterns and on the specials; its ends are the steps at xlo / xhi and
lie inside the windowed sweep's range; the true and the reciprocal tables differ at s0 = 0.0039 and not at 1 / 255; every carrier's LUT
is injective on both oracles.

Device part, which domain got which sweep:
  FULL (all 2^32 patterns, NaN payloads and both infinities included) on EVERY site -- every registered first-layer instantiation that
      stages fp32: merged, hybrid, the sparse hybrid by risky register, GEN_STD / GEN_ANY, residual tensor on and off, 1, 2, 3 and 4
      channels, the width-aware forms, dot4 under ENGINE_DOT4 and under exact_division -- for two domains: (0.00392155787524055, -128)
      and the natural-frame (0.003686274624630517, -136); the exact_div = 2 sites against the reciprocal tables of (0.0039, -128) and
      the same natural scale.  One section more runs the full sweep at H x W = 4097 x 4095 (2^24 - 1 pixels, the largest frame the MFMA
      kernels take) on the SESR-x2 shape, fused and per layer, int8 / fp32 / both outputs in turn: every byte of every forward is
      checked there.
  WINDOW (every pattern of [pred^4096(xlo), succ^4096(xhi)], plus the specials, NaNs and one pattern of every 2^24 at every channel
      position) for every other domain -- the remaining reference-calibrated and natural ones, z0 = 127 (xlo < xhi = 0; sesrq_create
      takes none above), z0 = 0 (xlo < 0 < xhi), s0 = 2.5, s0 = 1e-20, (0.0039, -128) under true division -- on three sites (merged
      MFMA, per-PE MFMA, dot4), and on every other site for one of them in turn.  NOT the cross product of sites and domains (92 x 10
      more sweeps): beyond the window x is clamped, and what remains there -- the specials, the NaN classes, the stride sample -- rides
      on every sweep, FULL ones too.
  The int8 hand-off (an upstream net's output re-quantised while staged): all 256 codes, three upstream domains, on every 8-bit
      instantiation of the MFMA and dot4 first layers.
  The debug forward's tap kernels: +-256 patterns around every threshold and the specials (their frames carry PE dumps: small ones).
  The proof's rejecting branch: scales with an all-ones mantissa around 2^-8 and their neighbours, 2e-37 and the denormal 1e-39;
      every refused scale must run layer 0 on the dot4 kernel and pass the windowed sweep there.

A NaN element quantises to the lowest code (include/sesrq.h): quiet and signalling, both signs, several payloads, every channel.
"""
import functools
import itertools

import numpy as np
import pytest

import input_sweep as IS
from constructions import Carrier
from helpers import bundle_from_oracle, device
from input_sweep import Domain
from oracle import sesrq_oracle as O
from planner import expected_plan_and_engines
import sesrq
from sesrq import _lib

F32 = np.float32

# ------------------------------------------------------------------------------------------------ domains
SYN = (1.0 / 255.0, -128)                                   # the synthetic nets'; 0.00392156862745098 of the reference's is the same float
REF = [(0.00392155787524055, -128), (0.003921552265391631, -128)]
NAT = [(0.003686274624630517, -136), (0.003643347951127034, -139), (0.003274281936533311, -169), (0.003226687160192751, -174)]
# the proof enumerates each sign on its own.  z0 = 127, the largest zero point sesrq_create takes: xlo < xhi = 0; z0 = 0: xlo < 0 < xhi
SIGNS = [(1.0 / 255.0, 127), (1.0 / 255.0, 0)]
SCALES = [(2.5, -128), (1e-20, -128)]
RECIP = [(0.0039, -128), NAT[0]]                            # exact_div = 2 against the reciprocal table
FULL = [REF[0], NAT[0]]
ALL8 = [SYN] + REF + NAT + SIGNS + SCALES + RECIP[:1]      # (0.0039, -128) under TRUE division too: where a reciprocal form would show
TINY = [(1e-39, -128), (2e-37, -128)]                       # the rejecting-branch candidates far from 1 / 255
ONES = [(float(np.ldexp(F32(2.0) - F32(2.0 ** -23), e)), -128) for e in (-10, -9, -8, -7, -6)]       # mantissa all ones


def neighbours(s):
    b = int(IS.as_bits(F32(s))[0])
    return [float(IS.as_float(np.uint32(b + d))[0]) for d in (-1, 1)]


CANDIDATES = ONES + [(n, -128) for s, _ in ONES for n in neighbours(s)] + [(ONES[2][0], z) for z in (-136, 0)] + TINY


# ------------------------------------------------------------------------------------------------ sites
class Site:
    """One way to run the first layer: the carrier's shape, the engine's options, and the registry name of the kernel that must run."""

    def __init__(self, sid, kernel, cin=3, rc=False, risky=(), bits=(18, 20), b=8, recip=False, **kw):
        self.id, self.kernel, self.cin, self.rc, self.risky, self.bits, self.b, self.recip, self.kw = sid, kernel, cin, rc, tuple(risky), bits, b, recip, kw
        if recip:
            self.kw["reciprocal_division"] = True

    def carrier(self, s0, z0, **shape):
        return Carrier(self.cin, s0, z0, b=self.b, rc=self.rc, risky=self.risky, bits=self.bits, **shape)

    def domain(self, s0, z0):
        return Domain(s0, z0, self.b, self.recip)


def tf(v):
    return "true" if v else "false"


def nch(cin):
    return cin if cin in (1, 3) else 4


def mfma_sites(cin, rc, src=1, recip=False):
    """Every 8-bit MFMA first-layer instantiation of (channels, residual tensor, source form src: 1 = fp32, 3 = upstream int8)."""
    n, tag, out = nch(cin), f"c{cin}-rc{int(rc)}" + ("-recip" if recip else ""), []
    kw = dict(cin=cin, rc=rc, recip=recip)
    out.append(Site(f"w4-merged-{tag}", f"mfma_f5_kernel_w4<0, {src}, {tf(rc)}, {n}, 4>", **kw))
    if cin == 3:      # the sparse hybrid, by the accumulator register that holds the risky rows (two registers: all four)
        for rr, rows in enumerate([(3,), (7,), (11,), (15,), (7, 15)]):
            out.append(Site(f"w4-hybs{rr}-{tag}", f"mfma_f5_kernel_w4<5, {src}, {tf(rc)}, 3, {rr}>", risky=rows, **kw))
    else:
        out.append(Site(f"w4-hybrid-{tag}", f"mfma_f5_kernel_w4<3, {src}, {tf(rc)}, {n}, 4>", risky=(15,), **kw))
    out.append(Site(f"f5-genstd-{tag}", f"mfma_f5_kernel<1, {src}, {tf(rc)}, {n}>", force_general=True, **kw))
    out.append(Site(f"f5-genany-{tag}", f"mfma_f5_kernel<2, {src}, {tf(rc)}, {n}>", bits=(19, 21), force_general=True, **kw))
    return out


def dot4_sites(cin, rc, src=1, b=8, recip=False):
    tag = f"c{cin}-rc{int(rc)}-b{b}" + ("-recip" if recip else "")
    kw = dict(cin=cin, rc=rc, b=b, recip=recip, engine=_lib.ENGINE_DOT4)
    return [Site(f"dot4-merged-{tag}", f"conv_dot4_kernel<5, 1, false, 0, 16, {src}>", **kw),
            Site(f"dot4-general-{tag}", f"conv_dot4_kernel<5, 1, true, 0, 16, {src}>", force_general=True, **kw)]


def narrow_sites(cin, rc, b):
    tag, n = f"c{cin}-rc{int(rc)}-b{b}", nch(cin)
    kw = dict(cin=cin, rc=rc, b=b, engine=_lib.ENGINE_MFMA_Q)
    return [Site(f"w4q-{tag}", f"mfma_f5_kernel_w4_q<1, {tf(rc)}, {n}>", **kw),
            Site(f"f5q-{tag}", f"mfma_f5_kernel_q<1, {tf(rc)}, {n}>", force_general=True, **kw)]


def all_f32_sites():
    out = []
    for cin, rc in itertools.product((1, 2, 3, 4), (False, True)):
        out += mfma_sites(cin, rc)
        if cin in (1, 3):
            out += dot4_sites(cin, rc)
    for b in (4, 2):
        for cin, rc in itertools.product((1, 3, 4), (False, True)):
            out += narrow_sites(cin, rc, b)
    for b in (3, 5, 6, 7):
        out += narrow_sites(3, b % 2 == 1, b)[:1] + dot4_sites(3, False, b=b)[:1]
    out += dot4_sites(3, False, b=4) + dot4_sites(1, True, b=2)
    # exact_division=True under the default engine selection: layer 0 alone goes to the dot4 kernel, and divides
    out.append(Site("dot4-exactdiv-c3-rc0", "conv_dot4_kernel<5, 1, false, 0, 16, 1>", cin=3, exact_division=True))
    # ... and at b = 4 and 2 under the width-aware engine, which is where a narrow net has an MFMA first layer to leave
    for b in (4, 2):
        out.append(Site(f"dot4-exactdiv-c3-rc0-b{b}", "conv_dot4_kernel<5, 1, false, 0, 16, 1>", cin=3, b=b, exact_division=True,
                        engine=_lib.ENGINE_MFMA_Q))
    # exact_div = 2 on the f5 kernels (r2 == 0 on the proven form's instructions) and on dot4 (x * fl(1 / s0))
    out += mfma_sites(3, False, recip=True)[:1] + mfma_sites(4, True, recip=True)[2:] + dot4_sites(3, False, recip=True)[:1]
    out.append(Site("w4q-c3-rc0-b4-recip", "mfma_f5_kernel_w4_q<1, false, 3>", cin=3, b=4, recip=True, engine=_lib.ENGINE_MFMA_Q))
    return out


SITES = {s.id: s for s in all_f32_sites()}
assert len(SITES) == len(all_f32_sites())
DOMAIN_SITES = ["w4-merged-c3-rc0", "f5-genstd-c3-rc1", "dot4-merged-c3-rc0-b8"]
ROUND8 = [SYN] + REF[1:] + NAT[1:] + SIGNS + SCALES + RECIP[:1]      # what goes round the 8-bit instantiations beside their full sweeps
ROUNDQ = [NAT[1], SYN, NAT[3]]                                        # ... and the narrow ones

# every site gets the full sweep on both FULL domains (z0 = -128 and a natural one), the exact_div = 2 sites on the RECIP pair
FULL_CASES = [(sid, d) for sid, s in SITES.items() for d in (RECIP if s.recip else FULL)]
WINDOW_CASES = [(s, d) for d in ALL8 if d not in FULL for s in DOMAIN_SITES]
_round8, _roundq = itertools.cycle(ROUND8), itertools.cycle(ROUNDQ)
WINDOW_CASES += [(sid, next(_round8 if s.b == 8 else _roundq)) for sid, s in SITES.items() if sid not in DOMAIN_SITES and not s.recip]
I8D_UPSTREAM = [(0.0053741, 127), (0.00392156862745098, -128), (0.0071, -3)]      # (s_prev, z_prev): z_prev = 127 and -128 among them


def case_id(c):
    return f"{c[0]}-s{c[1][0]!r}-z{c[1][1]}"


def table_domains():
    """Every (s0, z0, b, reciprocal) the device part compares with: the CPU part proves each table."""
    out = {SITES[s].domain(*d) for s, d in FULL_CASES + WINDOW_CASES}
    out |= {Domain(s, z, 8, False) for s, z in CANDIDATES + ALL8} | {Domain(s, z, 8, True) for s, z in RECIP + [SYN, SCALES[1]]}
    return sorted(out, key=lambda d: (d.b, d.reciprocal, d.z0, d.s0))


DOMAINS = table_domains()


# ------------------------------------------------------------------------------------------------ CPU part
@functools.lru_cache(maxsize=None)
def _micro_net(dom):
    """The smallest net the C oracle runs (three 1x1 layers): its input0 tap is the C oracle's q0."""
    lay = [O.Layer(wq=np.ones((1, 1, 1, 1), np.int8), add_const=np.zeros(1, np.int32), M=1 << 15, n=15, relu=(k != 2)) for k in range(3)]
    half = 1 << (dom.b - 1)
    return O.Net(layers=lay, scale=[dom.s0, 1.0, 1.0, 1.0], zero=[dom.z0, -half, -half, -half], M_res=1 << 15, n_res=16, quan_bits=dom.b)


def c_codes(dom, bits):
    from oracle import c_oracle as CO
    x = IS.as_float(bits)
    rows = 64 if len(x) >= 4096 else 1                     # the C oracle's threads share a frame by rows
    x = np.concatenate([x, np.zeros(-len(x) % rows, F32)]).reshape(1, 1, rows, -1)
    return CO.forward(_micro_net(dom), x, keep=True, want_f=False)["input0"].reshape(-1)[:len(bits)].astype(np.int64)


@functools.lru_cache(maxsize=1)
def seeded_sample():
    """2^22 and a few seeded patterns without the NaNs, shared by every table's test."""
    sample = np.random.default_rng(20261019).integers(0, 1 << 32, (1 << 22) + (1 << 16), dtype=np.uint64).astype(np.uint32)
    sample = sample[~IS.is_nan(sample)]
    assert len(sample) >= 1 << 22
    sample.setflags(write=False)
    return sample


@functools.lru_cache(maxsize=1)
def seeded_keys():
    return IS.key(seeded_sample())


def assert_table(dom, bits, what, keys=None):
    """The table against the numpy oracle, and against the C oracle where it exists (true division); no NaN among the patterns."""
    bits = np.asarray(bits, np.uint32)
    if keys is None:
        assert not IS.is_nan(bits).any()
        keys = IS.key(bits)
    want = np.searchsorted(IS.table(dom), keys, "right") + dom.qlo
    for name, got in (("numpy", IS.oracle_codes(dom, bits)),) + ((("C", c_codes(dom, bits)),) if not dom.reciprocal else ()):
        bad = np.nonzero(got != want)[0]
        assert not len(bad), f"{dom.id} {what}: {len(bad)} differ from the {name} oracle, first 0x{bits[bad[0]]:08x}: table {want[bad[0]]}, oracle {got[bad[0]]}"


@pytest.mark.parametrize("dom", DOMAINS, ids=[d.id for d in DOMAINS])
def test_table_is_the_oracles_quantiser(dom):
    """2^b - 1 strictly increasing thresholds, each a step of exactly one code; the table equals both oracles on +-256 patterns around
    every threshold, on 2^22 seeded patterns and on the specials."""
    thr = IS.table(dom)
    assert thr.shape == ((1 << dom.b) - 1,) and (np.diff(thr) > 0).all(), dom
    assert thr[0] > IS.KEY_NINF and thr[-1] <= IS.KEY_PINF
    at, below = IS.oracle_codes(dom, IS.unkey(thr)), IS.oracle_codes(dom, IS.unkey(thr - 1))
    assert np.array_equal(at, np.arange(dom.qlo + 1, dom.qhi + 1)) and np.array_equal(below, np.arange(dom.qlo, dom.qhi)), dom
    near = np.clip(thr[:, None] + np.arange(-256, 257)[None, :], IS.KEY_NINF, IS.KEY_PINF).reshape(-1)
    assert_table(dom, IS.unkey(near), "around the thresholds")
    assert_table(dom, seeded_sample(), "seeded sample", seeded_keys())
    assert_table(dom, IS.specials(), "specials")
    assert IS.codes(dom, IS.nans()).tolist() == [dom.qlo] * len(IS.nans())


@pytest.mark.parametrize("dom", DOMAINS, ids=[d.id for d in DOMAINS])
def test_table_ends_are_the_clamp_steps(dom):
    """The first and the last threshold are the steps next to xlo and xhi: they sit where (qlo + 0.5 - z0) s0 and (qhi - 0.5 - z0) s0
    round to, strictly inside the range [xlo, xhi] the MFMA staging code clamps x to, so the windowed sweep holds every threshold."""
    thr, s = IS.table(dom), float(F32(dom.s0))
    for t, ideal in ((thr[0], (dom.qlo + 0.5 - dom.z0) * s), (thr[-1], (dom.qhi - 0.5 - dom.z0) * s)):
        v = float(IS.as_float(IS.unkey(t))[0])
        assert abs(v - ideal) <= 4 * 2.0 ** -24 * max(abs(ideal), abs(dom.z0) * s, s), (dom, v, ideal)
    klo, khi = IS.clamp_ends(dom)
    assert klo < thr[0] and thr[-1] <= khi, (dom, klo, thr[0], thr[-1], khi)
    w = IS.window(dom)
    assert w[0] <= klo and khi <= w[1] and (w[0] == IS.KEY_NINF or w[0] == klo - IS.MARGIN) and w[1] == khi + IS.MARGIN


def test_true_and_reciprocal_tables_differ_where_they_should():
    """x * fl(1 / s0) rounds some ties differently from the quotient: at s0 = 0.0039 most thresholds move, each by one pattern, so a
    kernel that takes the wrong form fails the sweep of (0.0039, -128) and fails it next to thresholds only.  At the synthetic 1 / 255
    (fl(1 / s0) = 255 - 2^-16) a single threshold moves, the last one: random frames of that domain cannot tell the forms apart."""
    d = IS.table(Domain(0.0039, -128, 8, True)) - IS.table(Domain(0.0039, -128, 8, False))
    assert np.count_nonzero(d) > 128 and np.abs(d).max() == 1, d[d != 0]
    d = IS.table(Domain(*SYN, 8, True)) - IS.table(Domain(*SYN, 8, False))
    assert np.flatnonzero(d).tolist() == [254] and d[254] == 1, d[d != 0]
    for b in (4, 2):      # the narrow tables are the 8-bit one's middle: clamp_b o clamp8 == clamp_b
        t8, tb = IS.table(Domain(*NAT[0], 8, False)), IS.table(Domain(*NAT[0], b, False))
        assert np.array_equal(tb, t8[128 - (1 << (b - 1)):127 + (1 << (b - 1))])


def carriers():
    seen = {}
    for s in SITES.values():
        seen.setdefault((s.cin, s.rc, s.risky, s.bits, s.b), s)
    return seen


CARRIERS = carriers()


@pytest.mark.parametrize("key", list(CARRIERS), ids=[f"c{k[0]}-rc{int(k[1])}-risky{len(k[2])}-acc{k[3][0]}-b{k[4]}" for k in CARRIERS])
def test_carrier_lut_is_injective_on_both_oracles(key):
    """Every output channel of every carrier shows every code of its input channel as a byte of its own, on the numpy and on the C
    oracle, and a code in one channel moves no other channel: the device sweep can tell any two codes apart at any pixel."""
    from oracle import c_oracle as CO
    site = CARRIERS[key]
    for shape in (dict(), dict(cout=4 * site.cin, ps=2)):
        car = site.carrier(*NAT[0], **shape)
        lut = car.lut(O.forward)
        assert lut.shape == (car.cout, 1 << car.b) and all(len(set(row.tolist())) == 1 << car.b for row in lut), car.net.name
        # the C oracle takes fp32 frames: the same net behind a unit input domain, where x = q0 quantises to itself
        unit = site.carrier(1.0, 0, **shape)
        q0 = car.all_codes()
        st = CO.forward(unit.net, q0.astype(F32), keep=True)
        assert np.array_equal(st["input0"], q0)
        for o in range(car.cout):
            assert np.array_equal(np.roll(car.unshuffle(st["q_out"])[o, 0], -(o % car.cin)), lut[o]), (car.net.name, o)
    # own pixel, own channel only: a frame of one code with one other code in it differs at that pixel's bytes alone
    car = site.carrier(*NAT[0])
    base = np.full((1, car.cin, 9, 11), -1, np.int8)
    one = base.copy()
    one[0, car.cin - 1, 4, 5] = car.net.qlo
    a, b = (car.unshuffle(O.forward(car.net, x)["q_out"]) for x in (base, one))
    diff = np.argwhere(a != b)
    assert len(diff) and all(o % car.cin == car.cin - 1 and (y, x) == (4, 5) for o, y, x in diff), diff


# ------------------------------------------------------------------------------------------------ device part
LAUNCHED = set()       # every first-layer instantiation a checked sweep launched AND named
RAN = set()            # the sweeps that ran: the closure test needs the whole module


def _counters():
    return {**_lib.instances(), **_lib.narrow_instances()}


class Sweeper:
    """One engine on a carrier of one site and domain, and the device-side comparison of its output with the table."""

    def __init__(self, site, s0, z0, shape=None, upstream=None, plan_kw=None):
        import torch
        self.t = torch
        self.site, self.dom, self.dev = site, site.domain(s0, z0), device()
        self.car = site.carrier(s0, z0, **(shape or {}))
        kw = dict(site.kw, **(plan_kw or {}))
        self.e = sesrq.Engine(bundle_from_oracle(self.car.net), self.dev, upstream=upstream, **kw)
        self.tag = f"{site.id} {self.dom.id} {kw}"
        proven = self.e.fast_division_proven()
        pk = {k: v for k, v in kw.items() if k in ("engine", "force_general", "fuse_hidden")}
        plan, names = expected_plan_and_engines(self.car.net, fast_division=proven and not kw.get("exact_division"), **pk)
        assert self.e.layer_engines() == names and self.e.launch_plan() == plan, f"{self.tag}: {self.e.layer_engines()} {self.e.launch_plan()}, expected {names} {plan}"
        self.thr = torch.from_numpy(np.array(IS.table(self.dom))).to(self.dev)
        self.lut = torch.from_numpy(self.car.lut(O.forward)).to(self.dev)
        self.before = _counters()
        self.counts = []
        self.zout = float(self.car.net.zero[5])

    # -- frames from patterns, expected bytes from keys: integer work only
    def frame(self, bits, H, W):
        t = self.t
        signed = bits - ((bits >> 31) << 32)                       # the pattern as a two's complement int32
        return signed.to(t.int32).view(t.float32).view(1, self.car.cin, H, W)

    def index(self, bits):
        """LUT index (code - qlo) of every pattern: bucketize of the key in the table; a NaN takes the lowest code."""
        t = self.t
        keys = t.where(bits >> 31 != 0, 0xFFFFFFFF - bits, bits + (1 << 31))
        idx = t.bucketize(keys, self.thr, right=True)
        return t.where((bits & 0x7FFFFFFF) > 0x7F800000, t.zeros_like(idx), idx)

    def mismatches(self, bits, H, W, want_q=True, want_f=False, debug=False):
        """(device count of wrong bytes and values, [rows of them]) of one forward on the frame of these patterns."""
        t, car = self.t, self.car
        x = self.frame(bits, H, W)
        if debug:
            res = self.e.forward_debug(x, pe=True, acts=False)
            q, y = res["q_out"], res["y"]
        else:
            q, y = self.e.forward(x, want_q=want_q, want_f=want_f)
        idx = self.index(bits).view(car.cin, H * W)
        qs = car.unshuffle(q).reshape(car.cout, H * W) if q is not None else None
        ys = car.unshuffle(y).reshape(car.cout, H * W) if y is not None else None
        n, rows = t.zeros((), dtype=t.int64, device=self.dev), []
        for o in range(car.cout):
            want = self.lut[o][idx[o % car.cin]]
            bad = t.zeros(H * W, dtype=t.bool, device=self.dev)
            if qs is not None:
                bad |= qs[o] != want
            if ys is not None:
                bad |= ys[o] != (want.to(t.float32) - self.zout)
            n += bad.sum()
            rows.append((bad, want))
        return n, rows, qs, ys

    def check(self, make, H, W, **kw):
        """Enqueue one checked forward on the patterns make() gives; nothing comes back to the host until finish()."""
        n, *_ = self.mismatches(make(), H, W, **kw)
        self.counts.append((n, make, H, W, kw))

    def key_range(self, s, n):
        t = self.t
        keys = t.arange(s, s + n, dtype=t.int64, device=self.dev)
        return t.where(keys >> 31 != 0, keys - (1 << 31), 0xFFFFFFFF - keys)

    def sweep(self, k0, k1, H=2048, W=None, kinds=((True, False),)):
        """Every key of [k0, k1] in frames of cin * H * W consecutive keys (the last one moved back inside the 2^32 keys); by default
        2^22 pixels a forward, 2^23 of one or two channels: a frame of 2^24 pixels is beyond the MFMA kernels' 32-bit offsets."""
        W = W or (4096 if self.car.cin <= 2 else 2048)
        n = self.car.cin * H * W
        assert 0 <= k0 <= k1 < IS.NKEYS and n <= IS.NKEYS
        for i, s in enumerate(range(k0, k1 + 1, n)):
            wq, wf = kinds[i % len(kinds)]
            self.check(functools.partial(self.key_range, min(s, IS.NKEYS - n), n), H, W, want_q=wq, want_f=wf)
            if len(self.counts) >= 64:
                self.finish(final=False)

    def specials(self, extra=(), **kw):
        """The specials, the NaNs and the stride sample (and `extra` patterns) at every channel position of one small frame."""
        v = np.concatenate([IS.specials(), IS.nans(), IS.stride_sample(), np.asarray(extra, np.uint32)]).astype(np.int64)
        W = 64
        H = -(-len(v) // W)
        v = np.concatenate([v, np.zeros(H * W - len(v), np.int64)])
        planes = np.stack([np.roll(v, 97 * c + c) for c in range(self.car.cin)])
        bits = self.t.from_numpy(planes.reshape(-1)).to(self.dev)
        self.check(lambda: bits, H, W, **kw)

    def finish(self, final=True):
        """One host round trip for everything enqueued; a difference is reported by its bit patterns.  final: the kernel named by the
        site was launched (registry counters), and is recorded for the closure test."""
        t = self.t
        if self.counts:
            tot = t.stack([c[0] for c in self.counts]).cpu().numpy()
            for (_, make, H, W, kw), nb in zip(self.counts, tot):
                if nb:
                    bits = make()
                    _, rows, qs, ys = self.mismatches(bits, H, W, **kw)
                    lines = []
                    for o, (bad, want) in enumerate(rows):
                        for p in bad.nonzero().flatten()[:4].tolist():
                            pat = int(bits.view(self.car.cin, H * W)[o % self.car.cin, p])
                            got = int(qs[o, p]) if qs is not None else float(ys[o, p])
                            lines.append(f"0x{pat:08x} ({IS.as_float(np.uint32(pat))[0]!r}) channel {o}: got {got} want {int(want[p])}")
                    raise AssertionError(f"{self.tag} {kw}: {int(nb)} of {self.car.cout * H * W} differ; " + "; ".join(lines[:12]))
            self.counts = []
        if final:
            t.cuda.synchronize()
            hit = {k for k, v in _counters().items() if v > self.before.get(k, 0)}
            assert self.site.kernel in hit, f"{self.tag}: {self.site.kernel} was not launched: {sorted(h for h in hit if 'f5' in h or 'dot4_kernel<5, 1' in h)}"
            LAUNCHED.add(self.site.kernel)
            self.e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", FULL_CASES, ids=[case_id(c) for c in FULL_CASES])
def test_full_sweep(case):
    """All 2^32 patterns through the site's first-layer kernel: 256 forwards of a 2- or 4-channel frame (2^24
    patterns each), 342 of a 3-channel 2048 x 2048 one, 512 of a 1-channel 2048 x 4096 one."""
    sw = Sweeper(SITES[case[0]], *case[1])
    sw.specials()
    sw.sweep(0, IS.NKEYS - 1)
    sw.finish()
    RAN.add(("full", case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", WINDOW_CASES, ids=[case_id(c) for c in WINDOW_CASES])
def test_window_sweep(case):
    """Every pattern of [pred^4096(xlo), succ^4096(xhi)], the specials, the NaNs and the stride sample."""
    sw = Sweeper(SITES[case[0]], *case[1])
    sw.specials()
    sw.sweep(*IS.window(sw.dom))
    sw.finish()
    RAN.add(("window", case))


BIG = (4097, 4095)        # 2^24 - 1 pixels: the largest frame frame_fits_32bit_offsets accepts
BIG_PLANS = {"fused": dict(), "per-layer": dict(fuse_hidden=0)}
BIG_PARTS = list(range(4))


@pytest.mark.gpu
@pytest.mark.parametrize("plan", list(BIG_PLANS))
@pytest.mark.parametrize("part", BIG_PARTS)
def test_full_sweep_at_the_largest_frame(plan, part):
    """The full sweep on the SESR-x2 shape (3 -> 12 channels, PixelShuffle 2) at 4097 x 4095: 86 forwards in four parts, int8-only,
    fp32-only and both outputs in turn, every byte and every value of every forward checked -- the upper half of the 32-bit offset
    range of the first layer, the fused trio or the per-layer hidden kernels, and the last layer's three store forms."""
    H, W = BIG
    sw = Sweeper(SITES["w4-merged-c3-rc0"], *FULL[list(BIG_PLANS).index(plan)], shape=dict(cout=12, ps=2), plan_kw=BIG_PLANS[plan])
    n = 3 * H * W
    total = -(-IS.NKEYS // n)
    per = -(-total // len(BIG_PARTS))
    k0, k1 = part * per * n, min(IS.NKEYS, (part + 1) * per * n) - 1
    sw.sweep(k0, k1, H, W, kinds=((True, False), (False, True), (True, True)))
    sw.finish()
    RAN.add(("big", plan, part))


@pytest.mark.gpu
def test_a_zero_point_above_127_is_no_input_domain():
    """z0 > 127 would put both ends of [xlo, xhi] below zero; sesrq_create refuses it, so z0 = 127 is the edge the sweeps run."""
    with pytest.raises(ValueError, match="zero point out of range"):
        sesrq.Engine(bundle_from_oracle(SITES["w4-merged-c3-rc0"].carrier(1.0 / 255.0, 128).net), device())


def i8d_sites(cin):
    out = []
    for rc in (False, True):
        out += mfma_sites(cin, rc, src=3)
        if cin in (1, 3):
            out += dot4_sites(cin, rc, src=3)
    if cin == 3:
        out += mfma_sites(3, False, src=3, recip=True)[:1] + dot4_sites(3, False, src=3, recip=True)[:1]
    return out


I8D_CINS = [1, 2, 3, 4]


@pytest.mark.gpu
@pytest.mark.parametrize("cin", I8D_CINS)
def test_int8_hand_off(cin):
    """An upstream net's int8 output re-quantised while the first layer stages it: q0 = quantize_input(fl((q - z_prev) s_prev)) for all
    256 codes in every channel, three upstream domains, on every 8-bit first-layer instantiation that takes such a frame."""
    import torch
    doms = itertools.cycle(ROUND8[:8])
    for site in i8d_sites(cin):
        for s_prev, z_prev in I8D_UPSTREAM:
            s0, z0 = RECIP[0] if site.recip else next(doms)
            up = site.carrier(s0, z0)
            up.net.scale[5], up.net.zero[5] = s_prev, z_prev
            sw = Sweeper(site, s0, z0, upstream=bundle_from_oracle(up.net))
            q = sw.car.all_codes()
            x = (q.astype(F32) - F32(z_prev)) * F32(s_prev)
            want_q0 = O.quantize_input(x, s0, z0, site.recip).astype(np.int64)
            assert np.array_equal(want_q0, IS.codes(sw.dom, IS.as_bits(x.reshape(-1))).reshape(x.shape))       # the table agrees
            lut = sw.car.lut(O.forward)
            got = sw.e.forward(torch.from_numpy(q).to(sw.dev), want_f=False)[0].cpu().numpy()[0, :, 0, :]
            for o in range(sw.car.cout):
                want = lut[o][want_q0[0, o % cin, 0] + 128]
                bad = np.nonzero(got[o] != want)[0]
                assert not len(bad), f"{sw.tag} upstream ({s_prev}, {z_prev}): code {q[0, o % cin, 0, bad[0]]} channel {o}: got {got[o][bad[0]]} want {want[bad[0]]}"
            sw.finish()
    RAN.add(("i8d", cin))


def near_thresholds(dom):
    thr = IS.table(dom)
    return IS.unkey(np.clip(thr[:, None] + np.arange(-256, 257)[None, :], IS.KEY_NINF, IS.KEY_PINF).reshape(-1))


TAP_RCS = [False, True]


@pytest.mark.gpu
@pytest.mark.parametrize("rc", TAP_RCS)
def test_debug_forward_tap_kernels(rc):
    """The PE-tap kernels of sesrq_forward_debug stage the frame with the same code: +-256 patterns around every threshold, the
    specials and the NaNs, fp32 frames and the int8 hand-off."""
    import torch
    site = Site(f"f5-tap-rc{int(rc)}", f"mfma_f5_kernel<4, 1, {tf(rc)}, 4>", cin=3, rc=rc)
    sw = Sweeper(site, *NAT[1])
    sw.specials(extra=near_thresholds(sw.dom), debug=True)
    sw.finish()
    s_prev, z_prev = I8D_UPSTREAM[0]
    site = Site(f"f5-tap-i8d-rc{int(rc)}", f"mfma_f5_kernel<4, 3, {tf(rc)}, 4>", cin=3, rc=rc)
    up = site.carrier(*REF[1])
    up.net.scale[5], up.net.zero[5] = s_prev, z_prev
    sw = Sweeper(site, *REF[1], upstream=bundle_from_oracle(up.net))
    q = sw.car.all_codes()
    want_q0 = O.quantize_input((q.astype(F32) - F32(z_prev)) * F32(s_prev), *REF[1]).astype(np.int64)
    got = sw.e.forward_debug(torch.from_numpy(q).to(sw.dev), pe=True, acts=False)["q_out"].cpu().numpy()[0, :, 0, :]
    lut = sw.car.lut(O.forward)
    for o in range(sw.car.cout):
        assert np.array_equal(got[o], lut[o][want_q0[0, o % 3, 0] + 128]), (sw.tag, o)
    sw.finish()
    RAN.add(("tap", rc))


@pytest.mark.gpu
@pytest.mark.parametrize("cand", CANDIDATES, ids=[f"s{float(F32(s))!r}-z{z}" for s, z in CANDIDATES])
def test_refused_scales_divide_on_dot4_and_pass_the_sweep(cand):
    """The proof's rejecting branch: every candidate scale is asked; a refused one must run layer 0 on the dot4 kernel (which divides)
    and pass the windowed sweep there, an accepted one passes it on the MFMA kernel.  The denormal scale 1e-39 (fl(1 / s0) = inf) must
    be refused.  The verdict is printed (pytest -s; profiles/input_sweep.txt keeps them)."""
    s0, z0 = cand
    probe = sesrq.Engine(bundle_from_oracle(SITES["w4-merged-c3-rc0"].carrier(s0, z0).net), device())
    proven = probe.fast_division_proven()
    probe.close()
    print(f"fast division at s0 = {float(F32(s0))!r} (0x{IS.as_bits(F32(s0))[0]:08x}), z0 = {z0}: {'proven' if proven else 'REFUSED'}")
    site = SITES["w4-merged-c3-rc0"] if proven else Site("dot4-refused", "conv_dot4_kernel<5, 1, false, 0, 16, 1>", cin=3)
    sw = Sweeper(site, s0, z0)
    assert sw.e.layer_engines()[0].startswith("mfma-f5" if proven else "dot4"), (s0, z0, sw.e.layer_engines())
    sw.specials()
    sw.sweep(*IS.window(sw.dom))
    sw.finish()
    if cand == TINY[0]:
        assert not proven, "the denormal scale must be refused"
    RAN.add(("refused", cand))


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(fuse_hidden=0), dict(engine=_lib.ENGINE_DOT4), dict(exact_division=True),
                                dict(reciprocal_division=True), dict(force_general=True), dict(anchor_add=True),
                                dict(anchor_add=True, engine=_lib.ENGINE_DOT4)], ids=str)
def test_a_nan_moves_only_its_own_pixels(kw):
    """An ordinary net (synth_net: full 5x5 and 3x3 weights) on a frame with NaNs and infinities in it gives exactly the oracle's output
    on the frame with those elements replaced by values that quantise to the same codes (NaN, -inf: the lowest; +inf: the highest): a
    NaN reaches nothing but the code of its own element, under every engine and division form alike.  With anchor_add the fp32 output
    adds the frame itself, nearest-upsampled: the int8 output is still the oracle's, and the fp32 output is NaN / +-inf in the 2 x 2
    block of such an element and the oracle's value plus the frame's everywhere else."""
    import torch
    net = O.synth_net("sesr_x2", 3)
    net.scale[0], net.zero[0] = NAT[2]
    rng = np.random.default_rng(7)
    x = rng.random((1, 3, 37, 70), dtype=F32)
    spots = [(0, 0, 0), (1, 0, 69), (2, 36, 0), (0, 36, 69), (1, 17, 33), (2, 17, 34), (0, 12, 63), (1, 12, 64), (2, 5, 5)]
    infs = [((0, 20, 20), 0x7F800000, F32(1e30), 127), ((2, 36, 69), 0xFF800000, F32(-1e30), -128), ((1, 9, 64), 0x7F800000, F32(1e30), 127)]
    clean, dirty = x.copy(), x.copy().view(np.uint32)
    for (c, yy, xx), pat in zip(spots, IS.nans()[[0, 2, 4, 5, 8, 9, 11, 14, 17]]):
        dirty[0, c, yy, xx] = pat
        clean[0, c, yy, xx] = F32(-1e30)
    for (c, yy, xx), pat, val, _ in infs:
        dirty[0, c, yy, xx] = pat
        clean[0, c, yy, xx] = val
    dirty = dirty.view(F32)
    recip = bool(kw.get("reciprocal_division"))
    q0 = O.quantize_input(clean, *NAT[2], recip)
    assert (q0[0][tuple(zip(*spots))] == -128).all() and [int(q0[0][i[0]]) for i in infs] == [i[3] for i in infs]
    st = O.forward(net, q0)
    e = sesrq.Engine(bundle_from_oracle(net), device(), **kw)
    q, y = e.forward(torch.from_numpy(dirty).to(device()))
    want_y = st["y"]
    if kw.get("anchor_add"):
        with np.errstate(invalid="ignore"):
            want_y = st["y"] + np.repeat(np.repeat(dirty, 2, axis=2), 2, axis=3)
        assert np.isnan(want_y).sum() == 4 * len(spots) and np.isinf(want_y).sum() == 4 * len(infs)
    assert np.array_equal(q.cpu().numpy(), st["q_out"]), kw
    assert np.array_equal(y.cpu().numpy(), want_y, equal_nan=True), kw
    e.close()


def required_instances():
    """Every registered first-layer instantiation that stages fp32 (source form 1) or an upstream int8 frame (3), by registry name."""
    out = []
    for name in _counters():
        if "<" not in name:
            continue
        args = [a.strip() for a in name[name.index("<") + 1:-1].split(",")]
        if name.startswith("mfma_f5_kernel_w4<") or name.startswith("mfma_f5_kernel<"):
            src = args[1]
        elif name.startswith("mfma_f5_kernel"):         # the width-aware ones: <SRC, RC, NCH>
            src = args[0]
        elif name.startswith("conv_dot4_kernel<5, 1, "):
            src = args[5]
        else:
            continue
        if src in ("1", "3"):
            out.append(name)
    return out


def test_sites_name_every_registered_instantiation():
    """CPU: the sites of the device part, the hand-off's and the tap kernels' together name every registered first-layer instantiation
    that stages fp32 or an upstream int8 frame, and nothing that is not registered."""
    named = {s.kernel for s in SITES.values()} | {s.kernel for cin in I8D_CINS for s in i8d_sites(cin)}
    named |= {f"mfma_f5_kernel<4, {src}, {tf(rc)}, 4>" for src in (1, 3) for rc in (False, True)}
    req = set(required_instances())
    assert len(req) >= 84 and named == req, (sorted(req - named), sorted(named - req))


@pytest.mark.gpu
def test_every_staging_instantiation_was_swept():
    """The closure: every registered first-layer instantiation that stages fp32 or an upstream int8 frame was launched by a checked sweep
    above that named it.  Needs the whole module."""
    expected = len(FULL_CASES) + len(WINDOW_CASES) + len(BIG_PLANS) * len(BIG_PARTS) + len(I8D_CINS) + len(TAP_RCS) + len(CANDIDATES)
    if len(RAN) != expected:
        pytest.skip(f"only {len(RAN)} of the module's {expected} sweeps ran in this session")
    print("\n".join(sorted(LAUNCHED)))
    missing = [n for n in required_instances() if n not in LAUNCHED]
    assert not missing, f"never launched by a sweep that named it: {missing}"
