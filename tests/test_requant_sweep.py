"""Every accumulator value through every requant epilogue form.

The reduced epilogues (the one-fma form, the single-rounding output form, the cvt_pk_u8 stores, the fused trio's 511-entry merge table,
the biased MAGIC + s accumulator) are allowed per layer by a load-time proof over every accumulator value s whose result is not
saturated (csrc/sesrq_verify.hip); tests/test_one_fma.py pins that proof to numpy.  Random and natural frames put a few thousand sums per
layer into ranges of 1e5 .. 4e6 values, of which one or a handful can tell the forms apart.  Here the sums are SWEPT: a ramp row
(tests/constructions.py) takes 65 536 consecutive sums in one 272 x 272 frame, sixteen rows 2^20 of them in one forward, and every byte
the device writes is compared with the C oracle's.

What is swept, per (M, n): the proof's own range s in [floor(-2 / scale), ceil(258 / scale)], clipped to the biased limit +-(2^22 - 1);
for a target zero point z != -128 also the window in which clamp8(t' + z) is not saturated, where both fit one forward.  The pairs:
form 1 holds over a long range (65535, 26), (32768, 26), (60000, 25), (60000, 24); form 1 fails and form 2 holds (32865, 24), first at
s = 11486; both fail (34059, 24) at s = 6650, (33041, 26) at s = 90383 (form 2 at 323957); the smallest accepted scale (65024, 32), both fail at
s = 99078 (form 2 at 1486171), over the whole biased range; the analytic cases (2^15, 15) and (45000, 16); the largest scale (65535, 8); the smallest multiplier (1, 0).
The construction reaches every sum of the biased range: wide rows up to 4 194 046 (and down to -(2^22 - 1)), narrow rows (weight -1 on
the a ramp, static worst sum 128) the 257 sums above, 2^22 - 1 included.  No sum below 2^22 - 1 stays unreached.

CPU part: exact_byte (the requant in exact integer arithmetic, both fp32 roundings by hand) against the oracle's fp32 path over every
swept range; for every forward of every sweep the coverage (the set of sums at interior pixels IS the intended interval) and the C
oracle's output bytes against exact_byte through the whole net; the numpy oracle as second witness on one forward per site; for every
pair whose proof rejects a form, that the first differing s lies in the swept set and the rejected form's numpy model gives another byte.
GPU part: every sweep under every plan that changes which epilogue runs, the kernel and form asserted by name (layer_engines,
one_fma_layers, launch_plan through tests/planner.py, the launched instantiation through the registry counters), selected with
sesrq_options only.  A difference is reported by its sums.  No mismatch was found in the library; that the sweep can fail was shown
once on a side build whose prove_direct_requant accepts (32865, 24) unwalked: every sweep of that pair that takes form 1 (first layer,
trio positions a, b, c, h5 last layers, the anchored fp32 store) failed with "1 bytes differ ... differs at s = 11486: got -105 want
-106", and nothing else failed (profiles/requant_sweep.txt).

The width-aware engine (SESRQ_ENGINE_MFMA_Q) runs the same construction at b = 4 and b = 2 (ramps over the width's range, 4^b sums per
row, a (2^b + 16)^2 frame) on (65535, 26) over every s whose t' lies in [-2, 2^b + 2], at the hidden, merging and last positions.
"""
import functools

import numpy as np
import pytest

import test_one_fma as T
from constructions import BIASED_LIMIT, MARGIN, ONE, HALF, Ramp, exact_byte, ramp, ramp_cover, ramp_interval
from helpers import bundle_from_oracle, device, same
from instances import RF_ALL, RF_MASKS, Track
from oracle import sesrq_oracle as O
from planner import expected_plan_and_engines, verdicts
import sesrq
from sesrq import _lib

F32 = np.float32
LIM = BIASED_LIMIT - 1

LONG = [(65535, 26), (32768, 26), (60000, 25), (60000, 24)]      # form 1 holds
F2 = (32865, 24)                                                  # form 1 fails at s = 11486, form 2 holds
BOTH = [(34059, 24), (33041, 26)]                                 # both fail, first at s = 6650 / 90383
TINY = (65024, 32)                                                # the smallest accepted scale; both fail, first at s = 99078
ANALYTIC = [(1 << 15, 15), (45000, 16)]                           # n <= 17 can never fail
BIG, UNIT = (65535, 8), (1, 0)                                    # two or three sums wide; the smallest multiplier
PAIRS = LONG + [F2] + BOTH + [TINY] + ANALYTIC + [BIG, UNIT]
# (M, n) -> the first sum at which (form 1, form 2) leaves the reference's bytes, by the numpy models below
FIRST_DIFF = {(32865, 24): (11486, None), (34059, 24): (6650, 6650), (33041, 26): (90383, 323957), (65024, 32): (99078, 1486171)}
ZEROS = [-127, -129, -100, 0, 127, -200, -32768]                  # target domains beside -128: the general round_pack path
WIDE_PAIR = (30000, 30)                                           # +-2^22 lands on +-117: the unbiased flavour's sums move the byte


def pid(Mn):
    return f"{Mn[0]}-{Mn[1]}"


# ------------------------------------------------------------------------------------------------ ranges and numpy models of the forms
def proof_range(Mn):
    """prove_direct_requant's own: every s whose t' lies in [-2, 258], clipped to the biased limit."""
    scale = Mn[0] * 2.0 ** -Mn[1]
    return max(-LIM, int(np.floor(-2.0 / scale))), min(LIM, int(np.ceil(258.0 / scale)))


def narrow_range(Mn, b):
    """The same at a width b < 8: the clamp saturates beyond t' = 2^b."""
    scale = Mn[0] * 2.0 ** -Mn[1]
    return int(np.floor(-2.0 / scale)), int(np.ceil(((1 << b) + 2.0) / scale))


def sweep_range(Mn, z=-128):
    """The proof's range, widened by the window in which clamp8(t' + z) is not saturated where the whole stays within eight rows."""
    lo, hi = proof_range(Mn)
    scale = Mn[0] * 2.0 ** -Mn[1]
    wlo, whi = max(-LIM, int(np.floor((-130.0 - z) / scale))), min(LIM, int(np.ceil((130.0 - z) / scale)))
    if max(hi, whi) - min(lo, wlo) < 8 * 65536:
        lo, hi = min(lo, wlo), max(hi, whi)
    return lo, hi


def form_bytes(s, Mn, form):
    """The numpy models of the three forms (tests/test_one_fma.py) as bytes: 0 = the reference's two roundings, 1 = the one-fma form,
    2 = the single-rounding form."""
    M, n = Mn
    s = np.asarray(s, np.int64)
    tp = (s * M).astype(F32) * F32(2.0 ** -n)
    if form == 0:
        return np.clip(np.rint(tp + F32(-128.0)), -128, 127)
    if form == 1:
        return np.clip(np.rint(tp), 0, 255) - 128
    exact = (s * M).astype(np.float64) * 2.0 ** -n - 128.0
    return np.clip(np.rint(exact.astype(F32) + F32(128.0)), 0, 255) - 128


@functools.lru_cache(maxsize=None)
def first_difference(Mn, form):
    lo, hi = proof_range(Mn)
    s = np.arange(lo, hi + 1, dtype=np.int64)
    bad = np.nonzero(form_bytes(s, Mn, 0) != form_bytes(s, Mn, form))[0]
    return int(s[bad[0]]) if len(bad) else None


@functools.lru_cache(maxsize=None)
def proofs(Mn):
    """(form 1 proven, form 2 proven) by the host proof sesrq_create runs; tests/test_one_fma.py pins it to numpy.  sesrq_requant_form
    answers for form 2 only where form 1 fails; where it holds, form 2 is the numpy restatement and the proof's own precondition: the
    fma's addend Cs = Cd - 128 must be exact in fp32 (prove_single_requant; e.g. (65535, 8): Cd = -3.2e9, form 2 refused)."""
    f1 = sesrq.requant_form(*Mn) == 1
    if not f1:
        return f1, sesrq.requant_form(*Mn, output_layer=True) == 2
    Cd = -(F32(12582912.0) * F32(Mn[0])) * F32(2.0 ** -Mn[1])
    exact_addend = float(F32(Cd - F32(128.0))) == float(Cd) - 128.0
    return f1, bool(exact_addend and T.single_rounding_verdict(*Mn))


# ------------------------------------------------------------------------------------------------ the sweeps
class Sweep:
    """Forwards (fw: callables that build a Ramp net) that share a site, and the plans they run under on the device."""

    def __init__(self, sid, site, fw, plans, ins=("i8",), outs=((True, True),), witness=False, anchor=False):
        self.id, self.site, self.fw, self.plans, self.ins, self.outs, self.witness, self.anchor = sid, site, list(fw), plans, ins, outs, witness, anchor


CAP = {0: 16, 1: 8, 2: 8, 3: 8}
PER_TEST = 3            # forwards per test: each is a C-oracle forward (well under a second) and a dozen device forwards


def forwards(t, Mn, lo, hi, biased=True, **kw):
    """[lambda -> Ramp] covering [lo, hi] at site t: wide rows in groups of the site's capacity, narrow rows in forwards of their own."""
    cap = kw.get("cout", 16) if t == 4 else 8 if kw.get("split") else CAP[t]
    wide, narrow = ramp_cover(lo, hi, biased, kw.get("b", 8))
    out = []
    for rows in (wide, narrow):
        for i in range(0, len(rows), cap):
            out.append(functools.partial(Ramp, t, Mn, rows[i:i + cap], **kw))
    return out


def add_sweeps(reg, sid, site, fw, plans, **kw):
    """Register the forwards in tests of at most PER_TEST; the first part carries the numpy witness flag."""
    witness, per = kw.pop("witness", False), kw.pop("per", PER_TEST)
    parts = [fw[i:i + per] for i in range(0, len(fw), per)]
    for j, part in enumerate(parts):
        name = sid if len(parts) == 1 else f"{sid}-part{j}"
        reg.append(Sweep(name, site, part, plans, witness=witness and j == 0, **kw))


DOT4 = dict(engine=_lib.ENGINE_DOT4)
DOT4_PE = dict(engine=_lib.ENGINE_DOT4, force_general=True)
PE = dict(force_general=True)
PER_LAYER = dict(fuse_hidden=0)
FIRST_PLANS = [dict(), dict(reduced_forms=RF_ALL & ~2), PE, DOT4, DOT4_PE]
TRIO_PLANS = [dict(reduced_forms=m) for m in RF_MASKS] + [PER_LAYER, dict(fuse_hidden=0, reduced_forms=1 | 8), PE, DOT4, DOT4_PE]
LAST_PLANS = [dict(), dict(reduced_forms=RF_ALL & ~16), dict(reduced_forms=RF_ALL & ~16 & ~32), PE, DOT4, DOT4_PE]
LAST_OUTS = ((True, False), (False, True), (True, True))
LAST_SHAPES = {"h5-12-ps2": dict(cout=12, ps=2), "h5-16-ps4": dict(cout=16, ps=4), "h5p-4-ps2": dict(cout=4, ps=2),
               "dot4-3x3-12-ps2": dict(cout=12, ps=2, klast=3)}
MFMA_Q = dict(engine=_lib.ENGINE_MFMA_Q)
NARROW_PLANS = [MFMA_Q, dict(fuse_hidden=0, **MFMA_Q), dict(force_general=True, **MFMA_Q), dict()]
MERGE_RES = [HALF, ONE, O.qconst(0.3141), O.qconst(0.8765), (65535, 32), (1, 0)]
MERGE_ZEROS = [-128, -100, 0, 127]


def build_sweeps():
    reg = []
    for Mn in PAIRS:
        lo, hi = proof_range(Mn)
        # first layer (mfma-f5), 4 channels, int8 and fp32 frames; forms on and off (bit 2)
        add_sweeps(reg, f"first-{pid(Mn)}", 0, forwards(0, Mn, lo, hi), FIRST_PLANS, ins=("i8", "f32"), witness=Mn == F2)
        # the fused trio's three positions, the per-layer kernels (epi_mid, epi_preres), their per-PE flavours, dot4
        for t, pos in ((1, "a"), (2, "b"), (3, "c")):
            add_sweeps(reg, f"hidden-{pos}-{pid(Mn)}", t, forwards(t, Mn, lo, hi), TRIO_PLANS, witness=Mn == F2)
        # last layer: h5 (12 / ps 2, 16 / ps 4), h5p, 3x3 (dot4); forms 1 / 2 / none; int8, fp32, both
        for tag, shape in LAST_SHAPES.items():
            if Mn == TINY and tag != "h5-16-ps4":
                continue                                   # the whole biased range once per site: the 16-row shape
            add_sweeps(reg, f"last-{tag}-{pid(Mn)}", 4, forwards(4, Mn, lo, hi, **shape), LAST_PLANS, outs=LAST_OUTS,
                       witness=Mn == F2 and tag == "h5-12-ps2")
    Mn = LONG[0]
    for z in ZEROS:
        lo, hi = sweep_range(Mn, z)
        # zero[1] != -128: layer 0 writes a separate residual tensor; the output shows rc and q side by side
        add_sweeps(reg, f"first-z{z}", 0, forwards(0, Mn, lo, hi, split=True, z=z), FIRST_PLANS, ins=("i8", "f32"), witness=z == -100)
        for t, pos in ((1, "a"), (2, "b")):
            add_sweeps(reg, f"hidden-{pos}-z{z}", t, forwards(t, Mn, lo, hi, z=z), TRIO_PLANS)
        # position c requantises into the fixed -128 domain of ic; zero[L - 1] belongs to the merge's second requant
        add_sweeps(reg, f"hidden-c-zmerge{z}", 3, forwards(3, Mn, *proof_range(Mn), zmerge=z), TRIO_PLANS, witness=z == -100)
        for tag in ("h5-12-ps2", "h5-16-ps4"):
            add_sweeps(reg, f"last-{tag}-z{z}", 4, forwards(4, Mn, lo, hi, z=z, **LAST_SHAPES[tag]), LAST_PLANS, outs=LAST_OUTS)
    # fp32 output with the x2 anchor add: a three-channel frame, 12 channels at PixelShuffle 2
    for Mn in (LONG[0], F2, BOTH[0]):
        add_sweeps(reg, f"last-anchor-{pid(Mn)}", 4, forwards(4, Mn, *proof_range(Mn), cout=12, ps=2, cin=3),
                   [dict(anchor_add=True, **kw) for kw in LAST_PLANS[:4]], ins=("f32",), outs=((False, True), (True, True)), anchor=True)
    # the unbiased flavour: add constants that put reach beyond 2^22, swept past +-2^22
    for t, site in ((0, "first"), (1, "hidden-a"), (3, "hidden-c"), (4, "last")):
        kw = dict(cout=16, ps=4, z=0) if t == 4 else {}
        fw = forwards(t, WIDE_PAIR, BIASED_LIMIT - 100000, BIASED_LIMIT + 100000, biased=False, **kw)
        fw += forwards(t, WIDE_PAIR, -BIASED_LIMIT - 100000, -BIASED_LIMIT + 100000, biased=False, **kw)
        plans = {0: FIRST_PLANS[:1] + FIRST_PLANS[2:], 4: LAST_PLANS[:1] + LAST_PLANS[3:]}.get(t, [dict(), PER_LAYER, PE, DOT4, DOT4_PE])
        add_sweeps(reg, f"unbiased-{site}", t, fw, plans, ins=("i8", "f32") if t == 0 else ("i8",), outs=LAST_OUTS if t == 4 else ((True, True),),
                   witness=t == 3)
    # the merge's second requant alone: u = rc + ic + 256 takes all 511 values
    for res in MERGE_RES:
        fw = [functools.partial(Ramp, "m", ONE, [ramp(0)], res=res, zmerge=z) for z in MERGE_ZEROS]
        add_sweeps(reg, f"merge-{pid(res)}", "m", fw, [dict(), PER_LAYER, PE, DOT4], witness=res == MERGE_RES[2])
    # the width-aware engine: b = 4 and b = 2 on one long-range pair at the hidden, merging and last positions (epi_*_q)
    for b in (4, 2):
        lo, hi = narrow_range(LONG[0], b)
        per = 4 if b == 4 else 24                          # frames of 32 x 32 and 20 x 20 pixels: a forward takes a millisecond
        for t, pos in ((2, "hidden-b"), (3, "hidden-c")):
            add_sweeps(reg, f"narrow-q{b}-{pos}", t, forwards(t, LONG[0], lo, hi, b=b), NARROW_PLANS, per=per, witness=True)
        for tag in ("h5-12-ps2", "h5-16-ps4"):
            add_sweeps(reg, f"narrow-q{b}-last-{tag}", 4, forwards(4, LONG[0], lo, hi, b=b, **LAST_SHAPES[tag]), NARROW_PLANS, outs=LAST_OUTS,
                       per=per, witness=tag == "h5-12-ps2")
        fw = [functools.partial(Ramp, "m", ONE, [ramp(0)], res=res, b=b) for res in MERGE_RES]
        add_sweeps(reg, f"narrow-q{b}-merge", "m", fw, NARROW_PLANS, per=6)
    return reg


SWEEPS = build_sweeps()
SWEEP_IDS = [s.id for s in SWEEPS]


def unshuffle(a, r):
    """The inverse of O.pixel_shuffle: (N, C, H r, W r) -> (N, C r r, H, W)."""
    N, c, H, W = a.shape
    return a.reshape(N, c, H // r, r, W // r, r).transpose(0, 1, 3, 5, 2, 4).reshape(N, c * r * r, H // r, W // r)


@functools.lru_cache(maxsize=8)
def _want(key, make):
    from oracle import c_oracle as CO
    r = make()
    st = CO.forward(r.net, r.x, keep=True)
    assert np.array_equal(st["input0"], r.q0)
    S = r.assert_covered(st)
    return r, dict(q_out=st["q_out"], y=st["y"]), S


def want(sweep, i, make):
    """(the Ramp, the C oracle's q_out and y, the sums per row) of forward i of a sweep, after the proof that the sums are covered."""
    return _want((sweep.id, i), make)


def interior_rows(r, q):
    m = MARGIN
    return unshuffle(q, r.net.pixel_shuffle)[0, :, m:-m, m:-m]


# ------------------------------------------------------------------------------------------------ CPU part
def swept_ranges():
    """{(M, n), z, relu, b}: -> [lo, hi] of everything the sweeps put through a requant."""
    out = {}
    for b in (4, 2):
        for relu in (True, False):
            out[(LONG[0], -(1 << (b - 1)), relu, b)] = narrow_range(LONG[0], b)
    for Mn in PAIRS:
        for relu in (True, False):
            out[(Mn, -128, relu, 8)] = proof_range(Mn)
    for z in ZEROS:
        for relu in (True, False):
            out[(LONG[0], z, relu, 8)] = sweep_range(LONG[0], z)
    for relu, z in ((True, -128), (False, 0)):
        out[(WIDE_PAIR, z, relu, 8)] = (-BIASED_LIMIT - 100000, BIASED_LIMIT + 100000)
    return out


def oracle_byte(s, M, n, z, relu, b=8):
    t = O.requant(np.asarray(s, np.int64), M, n)
    if relu:
        t = np.maximum(t, F32(0))
    return O._qb(t + F32(z), b).astype(np.int8)


def test_exact_integer_restatement_equals_the_oracle():
    """exact_byte (integer arithmetic, both roundings by hand) against O.requant + O._qb over every swept range of every case, and the
    merge's u -> q4 over all 511 values for every (M_res, n_res, zero[L - 1]) of the merge cases.  exact_byte is the independent
    reference; the oracle's fp32 path is the subject, outside the (M, n, z) of its fixtures."""
    n = 0
    for (Mn, z, relu, b), (lo, hi) in swept_ranges().items():
        for a in range(lo, hi + 1, 1 << 20):
            s = np.arange(a, min(hi + 1, a + (1 << 20)), dtype=np.int64)
            got, ref = exact_byte(s, Mn[0], Mn[1], z, relu, b), oracle_byte(s, Mn[0], Mn[1], z, relu, b)
            bad = np.nonzero(got != ref)[0]
            assert not len(bad), f"(M, n) = {Mn}, z = {z}, relu = {relu}, b = {b}: s = {s[bad[0]]}: exact {got[bad[0]]}, oracle {ref[bad[0]]}"
            n += len(s)
    u = np.arange(511, dtype=np.int64)
    for res in MERGE_RES:
        for z in MERGE_ZEROS + ZEROS:
            v = (u.astype(F32) * F32(res[0])) * F32(2.0 ** -res[1])
            assert np.array_equal(exact_byte(u, res[0], res[1], z, relu=False), O._qb(v + F32(z)).astype(np.int8)), (res, z)
        for b in (4, 2):
            ub = np.arange((2 << b) - 1, dtype=np.int64)
            v = (ub.astype(F32) * F32(res[0])) * F32(2.0 ** -res[1]) + F32(-(1 << (b - 1)))
            assert np.array_equal(exact_byte(ub, res[0], res[1], -(1 << (b - 1)), relu=False, b=b), O._qb(v, b).astype(np.int8)), (res, b)
    assert n > 30 * (1 << 20)
    # the restatement has teeth: a tie that fp32 rounds to even, and the double rounding that separates the forms at (32865, 24)
    assert exact_byte([3], 1 << 15, 16, 0, False).tolist() == [2] and exact_byte([5], 1 << 15, 16, 0, False).tolist() == [2]
    s = FIRST_DIFF[F2][0]
    assert int(exact_byte([s], *F2, -128, True)[0]) == int(form_bytes([s], F2, 0)[0]) != int(form_bytes([s], F2, 1)[0])


def test_pairs_are_what_the_table_says():
    """The proof's verdict for every pair, and for every rejected form: the first differing sum is the one the kernels' source and the
    sweep's docstring name, it lies in the swept range, and the rejected form's numpy model gives another byte there -- which is what
    lets the device sweep fail."""
    for Mn in LONG + ANALYTIC + [BIG, UNIT]:
        assert proofs(Mn)[0] and T.one_fma_verdict(*Mn) == (True, None), Mn
    assert proofs(F2) == (False, True) and [proofs(Mn) for Mn in BOTH + [TINY]] == [(False, False)] * 3
    for Mn in LONG:
        lo, hi = proof_range(Mn)
        assert Mn[1] in (24, 25, 26) and hi - lo > 65536, Mn
    assert proof_range(TINY) == (int(np.floor(-2.0 / (65024 * 2.0 ** -32))), LIM) and proof_range(BIG)[1] - proof_range(BIG)[0] <= 3
    for Mn, (d1, d2) in FIRST_DIFF.items():
        lo, hi = proof_range(Mn)
        assert T.one_fma_verdict(*Mn) == (False, d1) and first_difference(Mn, 1) == d1, (Mn, T.one_fma_verdict(*Mn))
        assert first_difference(Mn, 2) == d2 and T.single_rounding_verdict(*Mn) == (d2 is None), (Mn, first_difference(Mn, 2))
        for form, d in ((1, d1), (2, d2)):
            if d is None:
                continue
            assert lo <= d <= hi
            ref, other = int(form_bytes([d], Mn, 0)[0]), int(form_bytes([d], Mn, form)[0])
            assert ref != other and ref == int(exact_byte([d], *Mn, -128, True)[0]), (Mn, form, d, ref, other)
            rows = sum(ramp_cover(lo, hi), [])               # ... and the rows every site sweeps carry it
            assert any(a <= d <= b for a, b in map(ramp_interval, rows)), (Mn, d)


@pytest.mark.parametrize("sid", SWEEP_IDS)
def test_sweep_covers_its_range_and_the_oracle_is_the_restatement(sid):
    """Every forward of the sweep: the sums attained at interior pixels ARE the rows' intervals (Ramp.assert_covered; a case that misses
    its range fails), the intervals contain the intended range without a gap, and the C oracle's output bytes at interior pixels are
    exact_byte of those sums, carried through relays and the merge.  One forward per site also runs the numpy oracle."""
    sweep = SWEEPS[SWEEP_IDS.index(sid)]
    for i, make in enumerate(sweep.fw):
        r, st, S = want(sweep, i, make)
        for o, v in r.expected_rows(S).items():
            got = interior_rows(r, st["q_out"])[o]
            bad = np.argwhere(got != v)
            assert not len(bad), f"{sid}: channel {o}: {len(bad)} bytes differ from the exact restatement, first {got[tuple(bad[0])]} want {v[tuple(bad[0])]}"
        assert np.array_equal(st["y"], (st["q_out"].astype(F32) - F32(r.net.zero[5])) * F32(1.0))
        assert st["q_out"].min() >= r.net.qlo and st["q_out"].max() <= r.net.qhi
        if sweep.witness and i == 0:
            st2 = O.forward(r.net, r.x)
            assert np.array_equal(st2["q_out"], st["q_out"]) and np.array_equal(st2["y"], st["y"]), sid


def test_every_site_sweeps_every_pair_without_a_gap():
    """The rows of a sweep's forwards, taken together, contain the pair's whole range: nothing shrinks silently when a chunk is dropped."""
    by = {}
    for sw in SWEEPS:
        for make in sw.fw:
            kw = make.keywords
            key = (make.args[0], make.args[1], kw.get("z", -128), kw.get("zmerge", -128), kw.get("cout"), kw.get("klast"), kw.get("cin"), kw.get("b", 8))
            by.setdefault(key, []).extend(ramp_interval(r, kw.get("b", 8)) for r in make.args[2])
    checked = 0
    for (t, Mn, z, zm, cout, klast, cin, b), iv in by.items():
        if t == "m" or Mn == WIDE_PAIR:
            continue
        lo, hi = narrow_range(Mn, b) if b < 8 else sweep_range(Mn, z) if (z != -128 and t != 3) else proof_range(Mn)
        iv.sort()
        reach = iv[0][0] - 1
        for a, b in iv:
            assert a <= reach + 1, f"site {t}, {Mn}, z = {z}: sums {reach + 1} .. {a - 1} are not swept"
            reach = max(reach, b)
        assert iv[0][0] <= lo and reach >= hi, (t, Mn, z, iv[0][0], reach, lo, hi)
        checked += 1
    assert checked >= len(PAIRS) * 7 + 8
    # the top of the biased range is reached by narrow rows, on the biased kernels
    wide, narrow = ramp_cover(LIM - 1000, LIM)
    assert narrow and ramp_interval(narrow[-1])[1] == LIM
    for rows in (wide[-1:], narrow):
        for t in (0, 3, 4):
            v = verdicts(Ramp(t, TINY, rows[:8]).net)[t]
            assert v["saturation_free"] and v["biased_ok"] and v["reach"] == LIM, (t, v)
    with pytest.raises(ValueError, match="outside the biased"):
        ramp_cover(0, BIASED_LIMIT)


def test_coverage_proof_refuses_a_case_that_misses_its_range():
    """assert_covered has teeth: a frame that lacks one (a, b) pair, and a row whose weights do not span 256, are both refused."""
    from oracle import c_oracle as CO
    r = Ramp(2, LONG[0], [ramp(1000), ramp(1000 + 65536)])
    x = r.x.copy()
    x[0, 0, MARGIN + 5, MARGIN + 7] += 1                       # one a value twice, its neighbour never: one sum missing
    with pytest.raises(AssertionError, match="covers"):
        r.assert_covered(CO.forward(r.net, x, keep=True))
    r.net.layers[2].wq[0, 11, 1, 1] = 1                        # a + 255 b: overlapping, not the interval
    with pytest.raises(AssertionError, match="covers"):
        r.assert_covered(CO.forward(r.net, r.x, keep=True))
    with pytest.raises(ValueError, match="rows"):
        Ramp(1, LONG[0], [ramp(0)] * 9)


# ------------------------------------------------------------------------------------------------ GPU part
LAUNCHED = set()       # every instantiation a sweep launched AND named


class Launched(Track):
    """instances.Track that also keeps what was launched inside the block."""

    def __exit__(self, et, ev, tb):
        if et is None:
            import torch
            torch.cuda.synchronize()
            after = {**_lib.instances(), **_lib.narrow_instances()}
            self.hit = {k for k, v in after.items() if v > self.before.get(k, self.narrow_before.get(k, 0))}
        return super().__exit__(et, ev, tb)

    def __enter__(self):
        self.narrow_before = _lib.narrow_instances()      # the width-aware kernels count in a registry of their own
        return super().__enter__()


def expected_forms(net, kw):
    """one_fma_layers() as sesrq_create decides it (requant_form, csrc/sesrq_create.hip) from the host proof and sesrq_options."""
    L, rf = net.L, kw.get("reduced_forms", RF_ALL)
    v = verdicts(net)
    trio = all(x["saturation_free"] and x["biased_ok"] for x in v[1:4])
    out = []
    for k, l in enumerate(net.layers):
        zt = net.zero[L] if k == L - 1 else net.zero[1 if k == 0 else k + 1]
        f1, f2 = proofs((l.M, l.n))
        if l.M_oc is not None or net.quan_bits < 8 or not v[k]["biased_ok"] or (k != L - 2 and zt != -128):
            out.append(0)
        elif k == L - 1:
            out.append(1 if (rf & 16 and f1) else 2 if (rf & 32 and f2) else 0)
        elif k == 0:
            out.append(1 if (rf & 2 and f1) else 0)
        else:
            out.append(1 if (f1 and rf & (4 if (trio and k == L - 2) else 2)) else 0)
    return out


def expected_instance(r, kw, f32, wq, wf):
    """The registry name (or its prefix) of the kernel that runs the probed layer: select_mfma / select_trio restated for these nets."""
    net, t = r.net, (3 if r.t == "m" else r.t)
    L, rf = net.L, kw.get("reduced_forms", RF_ALL)
    v = verdicts(net)
    k = net.layers[t].wq.shape[2]
    narrow = net.quan_bits < 8
    if kw.get("engine") == _lib.ENGINE_DOT4 or net.layers[t].M_oc is not None or (t == L - 1 and k == 3) or (narrow and kw.get("engine") != _lib.ENGINE_MFMA_Q):
        return f"conv_dot4_kernel<{k}, "
    pe = bool(kw.get("force_general"))
    if narrow:      # the width-aware flavours: merged or run-time bounds, generic epilogues, byte-run stores on the merged last layer only
        mode = 2 if pe else 0
        if t < L - 1:
            return f"mfma_h3_kernel_q<{mode}, {1 if t == L - 2 else 0}>" if (pe or not kw.get("fuse_hidden", 1)) else "mfma_trio_kernel_q<1, 0>"
        oc, ps = net.layers[t].wq.shape[0], net.pixel_shuffle
        nv, pair = (3 if oc <= 12 else 4), (oc == 12 and ps == 2)
        run = 0 if (mode or (not pair and ps != 4)) else 2 if pair else ps if nv == 4 else 0
        fast, outf = (run, 0) if (wq and not wf) else (run, 1 if run else 0) if (wf and not wq) else (0, 0)
        return f"mfma_h5_kernel_q<{mode}, 2, {fast}, {nv}, {outf}>"
    mode = 2 if not v[t]["biased_ok"] else 1 if pe else 0
    direct = [0 if not v[j]["biased_ok"] else int(proofs((l.M, l.n))[0]) for j, l in enumerate(net.layers)]
    trio = all(x["saturation_free"] and x["biased_ok"] for x in v[1:4]) and kw.get("fuse_hidden", 1) and not pe
    if 1 <= t <= 3 and trio:
        u8 = net.zero[2] == net.zero[3] == net.zero[4] == -128 and bool(rf & 1)
        ab = u8 and bool(rf & 2) and direct[1] and direct[2] and net.zero[2] == -128 and net.zero[3] == -128
        abc = ab and bool(rf & 4) and direct[3]
        return f"mfma_trio_kernel<1, {15 if (abc and net.zero[1] == -128 and rf & 8) else 7 if abc else 3 if ab else 1 if u8 else 0}>"
    if t == 0:
        src, rc = (1 if f32 else 2), ("true" if net.zero[1] != -128 else "false")
        return f"mfma_f5_kernel_w4<0, {src}, {rc}, 4, 4>" if mode == 0 else f"mfma_f5_kernel<{mode}, {src}, {rc}, 4>"
    if t < L - 1:
        return f"mfma_h3_kernel<{mode}, {1 if t == L - 2 else 0}>"
    oc, ps = net.layers[t].wq.shape[0], net.pixel_shuffle
    if oc <= 4:
        return f"mfma_h5p_kernel<{mode}>"
    nv, pair, anchor = (3 if oc <= 12 else 4), (oc == 12 and ps == 2), bool(kw.get("anchor_add"))
    run = 2 if pair else ps if (nv == 4 and ps in (2, 4)) else 0
    fast = outf = 0
    if wq and not wf:
        fast = run
    elif wf and not wq and not anchor:
        fast, outf = run, (1 if run else 0)
    elif wf and not wq and pair:
        fast, outf = run, (2 if run else 0)
    if fast and mode != 2 and net.zero[L] == -128 and (not anchor or outf == 2):
        fast += 10 * expected_forms(net, kw)[t]
    return f"mfma_h5_kernel<{mode}, 2, {fast}, {nv}, {outf}>"


def assert_bytes(tag, r, S, got, want_q):
    """Bit for bit; a difference is reported by the sums behind it, not by its coordinates alone."""
    got = got.cpu().numpy()
    assert got.shape == want_q.shape and got.dtype == want_q.dtype, f"{tag}: {got.dtype} {got.shape} != {want_q.dtype} {want_q.shape}"
    if np.array_equal(got, want_q):
        return
    g, w = interior_rows(r, got), interior_rows(r, want_q)
    lines = []
    for o in range(g.shape[0]):
        bad = np.argwhere(g[o] != w[o])
        row = o - 8 if (r.t == 0 and r.split and o >= 8) else o
        for y, x in bad[:8]:
            s = int(S[row][y, x]) if row < len(S) else None
            lines.append(f"s = {s}: got {g[o, y, x]} want {w[o, y, x]} (channel {o})")
    inner = int((g != w).sum())
    raise AssertionError(f"{tag}: {int((got != want_q).sum())} bytes differ, {inner} of them at interior pixels; differs at " + "; ".join(sorted(set(lines))[:12]))


def run_sweep(sweep):
    import torch
    for i, make in enumerate(sweep.fw):
        r, st, S = want(sweep, i, make)
        b = bundle_from_oracle(r.net)
        t = 3 if r.t == "m" else r.t
        want_y = st["y"] + np.repeat(np.repeat(r.x, 2, axis=2), 2, axis=3) if sweep.anchor else st["y"]
        frames = {"i8": torch.from_numpy(r.q0).to(device()), "f32": torch.from_numpy(r.x).to(device())}
        for kw in sweep.plans:
            tag = f"{sweep.id}[{i}] {kw}"
            e = sesrq.Engine(b, device(), **kw)
            plan_kw = {k: v for k, v in kw.items() if k != "anchor_add"}
            plan, names = expected_plan_and_engines(r.net, **plan_kw)
            assert e.layer_engines() == names and e.launch_plan() == plan, f"{tag}: {e.layer_engines()} {e.launch_plan()}, expected {names} {plan}"
            assert e.one_fma_layers() == expected_forms(r.net, kw), f"{tag}: forms {e.one_fma_layers()}, expected {expected_forms(r.net, kw)}"
            for src in sweep.ins:
                for wq, wf in sweep.outs:
                    with Launched(pinned=False) as tr:
                        q, y = e.forward(frames[src], want_q=wq, want_f=wf)
                    name = expected_instance(r, kw, src == "f32", wq, wf)
                    hit = [h for h in tr.hit if h.startswith(name)]
                    assert hit, f"{tag} [{src}, q={wq}, f={wf}]: {name} was not launched: {sorted(tr.hit)}"
                    LAUNCHED.update(hit)
                    if wq:
                        assert_bytes(f"{tag} [{src}, q={wq}, f={wf}] q_out", r, S, q, st["q_out"])
                    if wf:      # values, not words: zero[5] == 0 lets rint(-0.3) = -0.0 through on the dot4 kernels, as in test_accumulator_limits
                        same(f"{tag} [{src}, q={wq}, f={wf}] y", y, want_y, values=True)
            e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sid", SWEEP_IDS)
def test_device_sweep(sid):
    """Every forward of the sweep under every plan of its site: names, forms and launch plan as predicted, the probed layer's kernel
    instantiation launched, every output byte the C oracle's, every fp32 value too."""
    run_sweep(SWEEPS[SWEEP_IDS.index(sid)])


def per_channel_case(t):
    """Sixteen rows with sixteen different (M, n); each row sweeps the 65 536 sums that hold what can tell its forms apart (the first
    differing sum where a form is rejected, else the start of the proof's range)."""
    pairs = PAIRS + [(44669, 25), (40011, 24), (50001, 25), (1, 8)]
    assert len(pairs) == 16 and len(set(pairs)) == 16
    rows = []
    for Mn in pairs:
        d = first_difference(Mn, 1)
        lo = (d - 30000) if d is not None else max(proof_range(Mn)[0], -30000)
        rows.append(ramp(lo + 32896))
    return Ramp(t, pairs[0], rows, Mn_oc=pairs, cout=16, ps=4), pairs


@pytest.mark.parametrize("t", [0, 4], ids=["first", "last"])
def test_per_channel_rows_are_the_restatement(t):
    """CPU: the numpy oracle's per-channel requant (parity unpinned: no reference counterpart) against exact_byte per row."""
    r, pairs = per_channel_case(t)
    st = O.forward(r.net, r.q0, keep=True)
    S = r.assert_covered(st)
    for o, v in r.expected_rows(S).items():
        assert np.array_equal(interior_rows(r, st["q_out"])[o], v), (t, o, pairs[o])
    for o, Mn in enumerate(pairs):
        d = first_difference(Mn, 1)
        assert d is None or (S[o] == d).sum() == 1, (Mn, d)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [0, 4], ids=["first", "last"])
def test_per_channel_layer_on_the_device(t):
    """One per-channel layer (M_oc / n_oc) whose sixteen rows carry sixteen different pairs: the dot4 per-channel epilogue against the
    exact-integer restatement per row, and the whole output against the numpy oracle."""
    import torch
    r, pairs = per_channel_case(t)
    st = O.forward(r.net, r.q0, keep=True)
    S = r.assert_covered(st)
    for kw in (dict(), PE, DOT4):
        e = sesrq.Engine(bundle_from_oracle(r.net), device(), **kw)
        assert e.layer_engines()[t].endswith("-perchannel") and e.one_fma_layers()[t] == 0, e.layer_engines()
        with Launched(pinned=False) as tr:
            q, y = e.forward(torch.from_numpy(r.q0).to(device()))
        hit = [h for h in tr.hit if h.startswith(f"conv_dot4_kernel<5, ")]
        assert hit, sorted(tr.hit)
        LAUNCHED.update(hit)
        g = interior_rows(r, q.cpu().numpy())
        for o, v in r.expected_rows(S).items():
            bad = np.argwhere(g[o] != v)
            assert not len(bad), f"{kw} row {o} {pairs[o]}: s = {int(S[o][tuple(bad[0])])}: got {g[o][tuple(bad[0])]} want {v[tuple(bad[0])]}"
        assert_bytes(f"per-channel {kw} q_out", r, S, q, st["q_out"])
        same(f"per-channel {kw} y", y, st["y"], values=True)
        e.close()


REQUIRED = (["mfma_trio_kernel<1, %d>" % u for u in (0, 1, 3, 7, 15)] + ["mfma_h3_kernel<%d, %d>" % (m, e) for m in (0, 1, 2) for e in (0, 1)] +
            ["mfma_f5_kernel_w4<0, %d, %s, 4, 4>" % (s, rc) for s in (1, 2) for rc in ("false", "true")] +
            ["mfma_f5_kernel<%d, %d, %s, 4>" % (m, s, rc) for m in (1, 2) for s in (1, 2) for rc in ("false", "true") if (m, rc) != (2, "true")] +
            ["mfma_h5_kernel<0, 2, %d, 3, %d>" % (f, o) for f in (2, 12, 22) for o in (0, 1, 2)] + ["mfma_h5_kernel<0, 2, 0, 3, 0>"] +
            ["mfma_h5_kernel<0, 2, %d, 4, %d>" % (f, o) for f in (4, 14, 24) for o in (0, 1)] + ["mfma_h5_kernel<0, 2, 0, 4, 0>"] +
            ["mfma_h5_kernel<1, 2, %d, 3, %d>" % (f, o) for f in (2, 12, 22) for o in (0, 1)] + ["mfma_h5_kernel<2, 2, 4, 4, %d>" % o for o in (0, 1)] +
            ["mfma_h5p_kernel<%d>" % m for m in (0, 1)] +
            ["mfma_trio_kernel_q<1, 0>"] + ["mfma_h3_kernel_q<%d, %d>" % (m, e) for m in (0, 2) for e in (0, 1)] +
            ["mfma_h5_kernel_q<0, 2, %d, %d, %d>" % (f, v, o) for f, v in ((2, 3), (4, 4)) for o in (0, 1)] +
            ["mfma_h5_kernel_q<%d, 2, 0, %d, 0>" % (m, v) for m in (0, 2) for v in (3, 4)])


@pytest.mark.gpu
def test_every_named_instantiation_was_launched():
    """The registry counters, through the suite's own bookkeeping (tests/instances.py): every epilogue site the sweep names was run by a
    case that asserted its launch.  The table is printed (pytest -s shows it; profiles/requant_sweep.txt keeps one)."""
    print("\n".join(sorted(LAUNCHED)))
    missing = [n for n in REQUIRED if n not in LAUNCHED]
    assert not missing, f"never launched by a sweep that named it: {missing}"
    assert any(n.startswith("conv_dot4_kernel<3, ") for n in LAUNCHED) and any(n.startswith("conv_dot4_kernel<5, ") for n in LAUNCHED)
