"""The kernels at the accumulator limits sesrq_create accepts.

Random and natural frames keep every PE sum far from the values the kernels' shortcuts depend on.  Here the sums are DRIVEN to them:
constant activation planes (127 or -128, made by a saturating upstream layer or handed in as an int8 / fp32 frame) under weights of one
sign reach the static bounds of the load-time proof (saturation_free, csrc/sesrq_verify.hip) exactly --

  A  the PE clamp at the reference's 18 / 20 bits: acc_lo reached without clamping (merged kernels, the fused trio), acc_lo - 128 and
     acc_hi + 1 clamped by 128 and by exactly one (hybrid: one risky PE; general: two), the hybrid's "the adder clamp cannot fire" at
     equality (3 * acc_lo + acc_lo == add_lo);
  B  run-time bounds (17, 17) and (16, 18): sums at acc_hi, acc_hi + 1, acc_lo, acc_lo - 1 and at add_hi, add_hi + 1, add_lo, add_lo - 1;
  C  the 2^22 limit of the biased accumulator (bits = MAGIC_I + s read as a float, csrc/sesrq_mfma_common.h): sums + add constant at
     +-2^22 and beyond, at (24, 26) bits and through add constants up to the accepted 2^24 at 18 / 20 bits.

Every probed sum is cancelled (other PEs, add constant) into a small total and requantised with M * 2^-n == 1 where the case allows, so
ONE LSB of ONE sum changes the output byte; downstream layers are identities (one centre tap, + 128) that carry the byte to the output.
Expected values: oracle/sesrq_oracle.py; the C oracle is the second witness (CPU test).  The construction asserts through the oracle's
un-saturated taps (pe_raw) that each intended sum IS reached: a case that misses its bound fails, it never passes vacuously.  The CPU
part also pins saturation_free's verdict (sesrq_saturation_verdict, a host entry) to a numpy restatement for every constructed layer.

Case C on the hardware before sesrq_create had its guard (LayerPlan::wide): the MFMA bytes differed from the oracle wherever sum + constant
left [-2^22, 2^22] by enough to move the byte -- (24, 26) last layer: 4 259 840 -> 65 (64), 5 000 000 -> 88 (76), 6 451 600 -> 127 (98),
-4 325 376 -> -64 (-65); add constant 2^23 at 18 / 20 bits: 7 864 320 -> 88 (60); 2^24: 127 (2) -- on the merged, hybrid, literal-clamp
and fused-trio kernels alike; the dot4 kernels were right.  +-2^22 +- 1 itself cannot move a byte at any accepted (M, n); the engine names
(-unbiased from reach == 2^22 on) pin the threshold there.
"""
import numpy as np
import pytest

from constructions import HALF, MARGIN, ONE, _pe_weights, _spread, build_layer, probe, relay, sat
from helpers import bundle_from_oracle, device, same
from oracle import sesrq_oracle as O
from topologies import SEAM_FRAMES as SIZES
from planner import LIMIT, expected_plan_and_engines, np_verdict, verdicts
import sesrq
from sesrq import _lib

TINY = (65024, 32)             # 63.5 * 2^-22: s = 2^22 lands on the tie 63.5, +-6.45 M on +-97.7


class Case:
    """A five-layer net (5x5 cin->16, three 3x3 16->16, 5x5 16->cout) with ONE probed layer t, its frames, the oracle's result and the proof
    that every probed sum is attained."""

    def __init__(self, name, t, rows, cin=3, cout=12, ps=2, bits=(18, 20), frame=None, hi_ch=(), Mn=ONE, z_out=-128, extra=None):
        """rows: the probed layer's output channels (padded with sat(-128)).  frame: the constant of every input channel (t == 0: the probed
        layer's planes).  hi_ch: input channels of the probed layer (t >= 1) that carry the 127 plane, the others carry -128.
        extra: {layer: rows} further probed layers (the trio case); their input planes are what the rows before them leave constant."""
        self.name, self.t, self.bits = name, t, bits
        L = 5
        frame = list(frame if frame is not None else [-128] * cin)
        width = [cin, 16, 16, 16, 16]
        nrow = [16, 16, 16, 16, cout]
        given = dict(extra or {})
        given[t] = rows
        plane_rows = [sat(127 if j in hi_ch else -128) for j in range(16)]
        layer_rows = []
        for k in range(L):
            if k in given:
                r = list(given[k]) + [sat(-128)] * (nrow[k] - len(given[k]))
            elif k < t:
                r = plane_rows if k == t - 1 else [sat(-128)] * 16
            elif k == L - 1:
                r = [relay(j) for j in range(cout)]
            else:
                r = [relay(j) for j in range(16)]
            layer_rows.append(r)
        if t >= 1 and any(j < cout for j in hi_ch) and t == 1:
            raise ValueError("layer 0's output is the residual operand: observed channels must leave it at -128")
        known = list(frame)
        self.probes, layers = {}, []
        for k in range(L):
            mn = Mn if k == t else ONE
            lay, pr = build_layer(5 if k in (0, L - 1) else 3, width[k], layer_rows[k], known, mn, relu=(k != L - 1), bits=bits)
            layers.append(lay)
            if pr:
                self.probes[k] = pr
            out = [row[1] if row[0] == "sat" else None for row in layer_rows[k]]
            if k == L - 2:      # the residual merge: rc (layer 0's row) + ic + 256, times 1, - 128
                rc = [row[1] if row[0] == "sat" else None for row in layer_rows[0]]
                out = [(-128 if (a, b) == (-128, -128) else 127 if 127 in (a, b) and None not in (a, b) else None) for a, b in zip(rc, out)]
            known = out
        # t == 0: layers 1..3 are identities of layer 0's output, which is also the residual operand: (2 q + 256) / 2 - 128 == q
        Mres = HALF if t == 0 else ONE
        zero = [-128] * L + [z_out]
        self.net = O.Net(layers=layers, scale=[1.0] * (L + 1), zero=zero, M_res=Mres[0], n_res=Mres[1], pixel_shuffle=ps,
                         acc_bits=bits[0], add_bits=bits[1], name=name)
        self.frame = frame
        self.cin, self.cout = cin, cout
        self._want = {}

    def frames(self, N, H, W):
        """(int8 q0, the fp32 frame that quantises to it: scale 1, zero point -128)."""
        q0 = np.empty((N, self.cin, H, W), np.int8)
        for c, v in enumerate(self.frame):
            q0[:, c] = v
        return q0, (q0.astype(np.float32) + np.float32(128))

    def want(self, size):
        """The oracle's forward with every tap, after the proof that the construction attains its sums."""
        if size not in self._want:
            q0, x = self.frames(*size)
            st = O.forward(self.net, x, keep=True)
            assert np.array_equal(st["input0"], q0)
            self.assert_attained(st)
            self._want[size] = st
        return self._want[size]

    def assert_attained(self, st):
        m = MARGIN
        for k, pr in self.probes.items():
            raw = st[f"pe_raw{k}"][:, :, :, m:-m, m:-m]
            acc = st[f"pe_add{k}"][:, :, m:-m, m:-m].astype(np.int64) + self.net.layers[k].add_const.astype(np.int64)[None, :, None, None]
            assert raw.size
            for o, (T, s) in pr.items():
                for p in range(4):
                    got = np.unique(raw[:, p, o])
                    assert got.tolist() == [T[p]], f"{self.name}: layer {k} channel {o} PE {p} reaches {got.tolist()}, not {T[p]}"
                got = np.unique(acc[:, o])
                assert got.tolist() == [s], f"{self.name}: layer {k} channel {o}: sum + constant {got.tolist()}, not {s}"

    def verdicts(self):
        return verdicts(self.net)

    def expected_engines(self, **kw):
        """layer_engines() as the shared restatement predicts it (tests/planner.py), with a proven fast division."""
        return expected_plan_and_engines(self.net, **kw)[1]


# ---- the rows of cases A and B: (acc_bits, add_bits) -> probed channels.  c = -128 planes everywhere unless `hi` (channels 12..15 at 127)
def bounds(bits):
    return -(1 << (bits[0] - 1)), (1 << (bits[0] - 1)) - 1, -(1 << (bits[1] - 1)), (1 << (bits[1] - 1)) - 1


def rows_merged(bits, pes, hi):
    """Every PE of `pes` just allowed: acc_lo exactly (S+ = 2^(b-1) / 128 under -128), hi = acc_hi + 1 - 128 (S- one less), and, where a
    127 plane exists, acc_hi exactly; all PEs at acc_lo at once: 4 acc_lo == add_lo at add = acc + 2 bits."""
    aL, aH, dL, dH = bounds(bits)
    rows = []
    for i, p in enumerate(pes):
        q = pes[(i + 1) % len(pes)]
        T = [0] * 4
        T[p] = aL
        if q != p:
            T[q] = aH + 1 - 128
        rows.append(probe(T, 100 + i))
        if hi:
            T = [0] * 4
            T[p] = aH
            if q != p:
                T[q] = aL
            rows.append(probe(T, 60 + i))
    if len(pes) * aL >= dL:
        rows.append(probe([aL if p in pes else 0 for p in range(4)], 200))
    if hi and len(pes) * aH <= dH:
        rows.append(probe([aH if p in pes else 0 for p in range(4)], 201))
    return rows


def rows_risky(bits, risky, pes, hi):
    """The PEs of `risky` one step beyond: acc_lo - 128 (clamped by 128) and acc_hi + 1 (clamped by exactly one), each cancelled by a
    safe PE at its own extreme; then every PE at the extreme of the SAME sign -- the hybrid's three safe sums + one clamped sum
    == add_lo exactly (and 4 acc_hi < add_hi)."""
    aL, aH, dL, dH = bounds(bits)
    safe = [p for p in pes if p not in risky] or list(risky)
    rows = []
    for i, p in enumerate(risky):
        q = safe[i % len(safe)]
        for j, (tp, tq) in enumerate(((aL - 128, aH + 1 - 128), (aH + 1, aL))):
            T = [0] * 4
            T[p] = tp
            if q != p:
                T[q] = tq
            rows.append(probe(T, 90 + 10 * i + j))
    rows.append(probe([(aL - 128 if p in risky else aL) if p in pes else 0 for p in range(4)], 150))
    if hi:
        rows.append(probe([(aH + 1 if p in risky else aH) if p in pes else 0 for p in range(4)], 151))
        rows.append(probe([(aL - 1 if p == risky[0] else 0) for p in range(4)], 152))        # one below acc_lo: clamped by one
    return rows


def rows_adder(bits):
    """add = acc bits (17, 17): one PE alone fills the adder.  Totals at add_hi, add_hi + 1, add_lo, add_lo - 1 and one PE beyond."""
    aL, aH, dL, dH = bounds(bits)
    assert (aL, aH) == (dL, dH)
    return [probe([aH, 0, 0, 0], 70), probe([aH, 1, 0, 0], 71), probe([0, aL, 0, 0], 72), probe([0, aL, -1, 0], 73),
            probe([aH, 0, aH, 0], 74), probe([0, aL, 0, aL], 75), probe([aH + 1, 0, 0, aL - 1], 76)]


HI = (12, 13, 14, 15)      # one channel per PE; never observed (the last layer relays channels 0..11)


def case_a(where, variant):
    """where: first1 / first3 / first4 / hidden1 / hidden3 / last12 / last3; variant: merged, hybrid<p>, general."""
    std = (18, 20)
    cin = int(where[5]) if where.startswith("first") else 3
    pes = list(range(min(cin, 4))) if where.startswith("first") else [0, 1, 2, 3]
    hi = not where.startswith("first")
    if variant == "merged":
        rows = rows_merged(std, pes, hi)
    elif variant.startswith("hybrid"):
        rows = rows_risky(std, [int(variant[6])], pes, hi) + rows_merged(std, [p for p in pes if p != int(variant[6])], hi)[:2]
    else:
        rows = rows_risky(std, pes[:2], pes, hi)
    kw = dict(hi_ch=HI if hi else ())
    if where.startswith("first"):
        return Case(f"A {where} {variant}", 0, rows[:12], cin=cin, **kw)
    if where.startswith("hidden"):
        return Case(f"A {where} {variant}", int(where[6]), rows[:12], **kw)
    cout = int(where[4:])
    return Case(f"A {where} {variant}", 4, rows[:cout], cout=cout, ps=2 if cout == 12 else 1, **kw)


def case_a_trio():
    """All three hidden layers just allowed at once, each with probed channels of its own: layer 1 probes channels 0..3 (carried on by
    relays), layer 2 channels 4..7 from the planes layer 1 leaves on 8..15, layer 3 channels 8..11 from 12..15 (-128 planes only)."""
    std = (18, 20)
    m = rows_merged(std, [0, 1, 2, 3], False)
    l1 = m[:4] + [sat(-128)] * 12
    l2 = [relay(j) for j in range(4)] + [probe(r[1], r[2] + 20) for r in m[1:5]] + [sat(-128)] * 8
    l3 = [relay(j) for j in range(8)] + [probe(r[1], r[2] + 40) for r in (m[4], m[0], m[2], m[3])] + [sat(-128)] * 4
    return Case("A trio: three layers at the threshold", 1, l1, extra={2: l2, 3: l3})


A_CASES = [("first1", "merged"), ("first1", "hybrid0"), ("first3", "merged"), ("first3", "hybrid0"), ("first3", "hybrid1"), ("first3", "hybrid2"),
           ("first3", "general"), ("first4", "merged"), ("first4", "hybrid3"), ("first4", "hybrid0"), ("first4", "general"),
           ("hidden1", "merged"), ("hidden3", "merged"), ("hidden2", "hybrid1"), ("hidden3", "hybrid2"), ("hidden1", "general"), ("hidden3", "general"),
           ("last12", "merged"), ("last12", "hybrid0"), ("last12", "hybrid3"), ("last12", "general"), ("last3", "merged"), ("last3", "hybrid1"),
           ("last3", "general")]


def case_b(bits, where):
    hi = where != "first4"
    pes = [0, 1, 2, 3]
    rows = rows_risky(bits, [1, 2], pes, hi)
    if hi:
        aL, aH, dL, dH = bounds(bits)
        rows = [probe([aH, aL, 0, 0], 50), probe([0, 0, aL, aH], 51)] + rows
        if bits[0] == bits[1]:
            rows = rows_adder(bits) + rows
    if where == "first4":
        return Case(f"B {bits} first", 0, rows[:12], cin=4, bits=bits)
    if where == "hidden3":
        return Case(f"B {bits} hidden", 3, rows[:12], bits=bits, hi_ch=HI)
    return Case(f"B {bits} last", 4, rows[:12], bits=bits, hi_ch=HI)


B_CASES = [(b, w) for b in ((17, 17), (16, 18)) for w in ("first4", "hidden3", "last12")]

# sums + add constant around the biased accumulator's limit, neighbours included, and well beyond it
C_SUMS = [LIMIT - 1, LIMIT, LIMIT + 1, -LIMIT + 1, -LIMIT, -LIMIT - 1, LIMIT + (1 << 16), LIMIT + (1 << 17), -LIMIT - (1 << 17),
          LIMIT + (1 << 18), 5000000, 16 * 25 * 127 * 127]


def case_c_wide(where):
    """Widths (24, 26): saturation-free whatever the weights.  last: 5x5 16->12 under 127 planes, the sums themselves reach the limit
    (the all-127 row: 6 451 600); hidden3 / first3: the add constant carries a moderate sum there."""
    bits = (24, 26)
    if where == "last12":
        rows = []
        for s in C_SUMS:
            m = int(round(s / 127.0))
            m = max(min(m, 4 * 12700), -4 * 12700)
            X = [m // 4 + (1 if i < m % 4 else 0) for i in range(4)]
            rows.append(probe([127 * x for x in X], s))
        return Case("C (24, 26) last layer", 4, rows, bits=bits, hi_ch=tuple(range(16)), Mn=TINY, z_out=0)
    T = [-128 * 3000, 128 * 2000, -128 * 1000, 128 * 2500]
    rows = [probe(T if s > 0 else [-t for t in T], s) for s in C_SUMS]
    if where == "hidden3":
        return Case("C (24, 26) hidden layer", 3, rows, bits=bits, Mn=TINY)
    return Case("C (24, 26) first layer", 0, [probe(r[1][:3] + (0,), r[2]) for r in rows], cin=3, bits=bits, Mn=TINY)


C_CONSTS = [LIMIT - (1 << 19), 1 << 23, 1 << 24]
SMALL = (1 << 15, 32)          # 2^-17: 2^24 lands on 128


def case_c_const(where, variant):
    """18 / 20 bits, add constants of +-(2^22 - 2^19), +-2^23, +-2^24 (sesrq_create accepts |add_const| <= 2^24) over sums at the PE
    extremes.  (2^22 - 2^19) + the adder's 2^19 is the limit itself: the `full` rows reach the adder bound and with it 2^22 exactly."""
    std = (18, 20)
    aL, aH, dL, dH = bounds(std)
    shapes = dict(merged=[[aL, aH + 1 - 128, 0, 0], [aL, aL, aL, aL], [0, 0, aH + 1 - 128, aH + 1 - 128]],
                  hybrid=[[aL - 128, aH + 1 - 128, 0, 0], [aL - 128, aL, aL, aL], [aH + 1, 0, aL, 0]],
                  general=[[aL - 128, aH + 1, 0, 0], [aL - 128, aL - 128, aL, aL], [aH + 1, aH + 1, 0, aL]])[variant]
    rows = []
    for i, c in enumerate(C_CONSTS):
        for sgn in (1, -1):
            T = shapes[(i + (sgn < 0)) % 3]
            tot = min(max(sum(min(max(t, aL), aH) for t in T), dL), dH)
            rows.append(probe(T, tot + sgn * c))
    if where == "last12":
        return Case(f"C const last {variant}", 4, rows, Mn=SMALL, z_out=0)
    if where == "last3":
        return Case(f"C const last3 {variant}", 4, rows[3:6], cout=3, ps=1, Mn=SMALL, z_out=0)
    if where == "first4":
        return Case(f"C const first {variant}", 0, rows, cin=4, Mn=SMALL)
    return Case(f"C const {where} {variant}", int(where[6]), rows, Mn=SMALL)


def case_c_edge(full):
    """The guard's own threshold on a merged last layer: add constant 2^22 - 2^19 and a static worst sum of 2^19 (`full`: reach == 2^22,
    the layer leaves the biased kernels) or 2^19 - 128 (reach 2^22 - 128: it stays on them, and they are exact)."""
    aL, aH, dL, dH = bounds((18, 20))
    c = LIMIT - (1 << 19)
    T = [aL, aL, aL, aL if full else aL + 128]
    return Case(f"C edge reach 2^22{'' if full else ' - 128'}", 4, [probe(T, sum(T) - c), probe([-t - 128 for t in T[:3]] + [0], c + 3 * (-aL - 128)),
                                                                  probe([aL, 0, 0, 0], aL + c)], Mn=SMALL, z_out=0)


C_CONST_CASES = [(w, v) for w in ("last12", "hidden3", "hidden1", "first4") for v in ("merged", "hybrid", "general")] + [("last3", "merged")]


def all_cases():
    for w, v in A_CASES:
        yield case_a(w, v)
    yield case_a_trio()
    for b, w in B_CASES:
        yield case_b(b, w)
    for w in ("last12", "hidden3", "first3"):
        yield case_c_wide(w)
    for w, v in C_CONST_CASES:
        yield case_c_const(w, v)
    yield case_c_edge(True)
    yield case_c_edge(False)


# ------------------------------------------------------------------------------------------------ CPU part
def test_constructions_attain_their_bounds_on_both_oracles():
    """Every case: the oracle's un-saturated PE sums equal the closed-form targets at interior pixels (Case.want asserts it), the probed
    bytes are not saturated where the case promises an LSB, and the C oracle computes the same bytes and taps."""
    from oracle import c_oracle as CO
    n = 0
    for case in all_cases():
        size = (1, 21, 70)
        st = case.want(size)
        _, x = case.frames(*size)
        c = CO.forward(case.net, x, keep=True)
        assert np.array_equal(c["q_out"], st["q_out"]) and np.array_equal(c["y"], st["y"]), case.name
        for k in range(5):
            assert np.array_equal(c[f"pe_out{k}"], st[f"pe_out{k}"]), (case.name, k)
            assert np.array_equal(c[f"pe_add{k}"], st[f"pe_add{k}"]), (case.name, k)
            assert np.array_equal(c[f"input{k}"], st[f"input{k}"]), (case.name, k)
        # one LSB is visible: where M 2^-n == 1 every probed channel's byte lies strictly inside the int8 range at interior pixels
        for k, pr in case.probes.items():
            lay = case.net.layers[k]
            if (lay.M, lay.n) != ONE:
                continue
            for o in pr:
                if o < case.cout:
                    v = st["input5"][:, o, MARGIN:-MARGIN, MARGIN:-MARGIN]
                    assert v.min() > -128 and v.max() < 127, f"{case.name}: layer {k} channel {o} is saturated at the output"
        n += 1
    assert n == len(A_CASES) + 1 + len(B_CASES) + 3 + len(C_CONST_CASES) + 2


def test_static_bounds_are_the_attained_extremes():
    """Closed forms of the issue's four thresholds at 18 / 20 bits, on a hidden layer under -128 planes: S+ = 1024 -> lo = 131072 = -acc_lo
    (allowed), S+ = 1025 -> 131200, S- = 1023 -> hi = 130944 (allowed), S- = 1024 -> hi = 131072 = acc_hi + 1 (clamps by one)."""
    for T, free, mask in (([-131072, 0, 0, 0], True, 0), ([-131200, 0, 0, 0], False, 1), ([0, 130944, 0, 0], True, 0), ([0, 131072, 0, 0], False, 2),
                          ([0, 0, 131071, 0], True, 0), ([0, 0, 0, -131073], False, 8)):
        case = Case(f"bound {T}", 3, [probe(T, 100)], hi_ch=HI)
        st = case.want((1, 21, 70))
        v = case.verdicts()[3]
        assert (v["saturation_free"], v["risky_mask"]) == (free, mask), (T, v)
        assert v["worst_pe"] == max(abs(t) for t in T), (T, v)            # the static bound IS the attained sum
        raw = st["pe_raw3"][0, :, 0, 10, 35]
        assert raw.tolist() == T
        clamped = st["pe_out3"][:, 0, 10, 35].tolist()
        assert clamped == [min(max(t, -131072), 131071) for t in T]


def test_helper_refuses_a_case_that_misses_its_bound():
    """The attainment proof has teeth: a frame that does not carry the planes the weights were built for, and a target no constant plane
    can reach, are both refused."""
    case = case_a("first3", "merged")
    case.frame = [-128, 127, -128]                       # PE 1 now sees +127 under weights built for -128
    with pytest.raises(AssertionError, match="reaches"):
        case.want((1, 21, 70))
    with pytest.raises(ValueError, match="no multiple of 128"):
        Case("unreachable", 0, [probe([-131071, 0, 0, 0], 100)], cin=3)
    with pytest.raises(ValueError, match="does not fit"):
        Case("too large", 0, [probe([-128 * 4000, 0, 0, 0], 100)], cin=3)
    good = case_a("hidden3", "merged")
    good.net.layers[2].add_const[12] = -32768           # the 127 plane of channel 12 is gone: the probed sums move
    with pytest.raises(AssertionError, match="reaches"):
        good.want((1, 21, 70))


def test_saturation_verdict_entry_matches_the_restatement():
    """sesrq_saturation_verdict (the host entry over sesrq_create's own saturation_free) against np_verdict for every layer of every
    case, and the verdicts the cases were built for: merged / which single PE is risky / general, and the biased-range guard."""
    for case in all_cases():
        for k, l in enumerate(case.net.layers):
            got = sesrq.saturation_verdict(l.wq, l.add_const, case.net.zero[k], *case.bits)
            assert got == np_verdict(l.wq, l.add_const, case.net.zero[k], *case.bits), (case.name, k, got)
    for (w, v) in A_CASES:
        case = case_a(w, v)
        vd = case.verdicts()[case.t]
        want_mask = {"merged": 0, "general": 3}.get(v, 1 << int(v[-1]) if v.startswith("hybrid") else None)
        assert vd["risky_mask"] == want_mask and vd["saturation_free"] == (v == "merged") and vd["biased_ok"], (w, v, vd)
        assert all(x["saturation_free"] and x["biased_ok"] for k, x in enumerate(case.verdicts()) if k != case.t)
    assert all(v["saturation_free"] for v in case_a_trio().verdicts())
    # the thresholds themselves: one weight more flips the verdict
    w = np.zeros((1, 16, 3, 3), np.int8)
    w[0, 0].flat[:] = 113
    w[0, 0, 0, 0] = 120                                    # S+ = 1024 on PE 0: lo = 131072 == acc_hi + 1
    assert sesrq.saturation_verdict(w)["saturation_free"] and sesrq.saturation_verdict(w)["worst_pe"] == 131072
    w[0, 0, 0, 0] = 121
    assert sesrq.saturation_verdict(w)["risky_mask"] == 1
    w = -w
    w[0, 0, 0, 0] = -119                                   # S- = 1023: hi = 130944
    assert sesrq.saturation_verdict(w)["saturation_free"]
    w[0, 0, 0, 0] = -120                                   # S- = 1024: hi = 131072 == acc_hi + 1
    assert sesrq.saturation_verdict(w)["risky_mask"] == 1
    # the adder: four PEs at lo = 131072 each are allowed (524288 == add_hi + 1), at (18, 19) they are not -- and no PE is risky
    w4 = np.zeros((1, 16, 3, 3), np.int8)
    for p in range(4):
        w4[0, p].flat[:] = 113
        w4[0, p, 0, 0] = 120
    assert sesrq.saturation_verdict(w4)["saturation_free"] and sesrq.saturation_verdict(w4)["worst_sum"] == 524288
    v = sesrq.saturation_verdict(w4, acc_bits=18, add_bits=19)
    assert not v["saturation_free"] and v["risky_mask"] == 0
    # the biased range: reach = min(worst_sum, 2^(add_bits - 1)) + max |add_const|, allowed below 2^22
    assert sesrq.saturation_verdict(w4, np.array([LIMIT - (1 << 19) - 1], np.int32))["biased_ok"]
    v = sesrq.saturation_verdict(w4, np.array([-(LIMIT - (1 << 19))], np.int32))
    assert v["reach"] == LIMIT and not v["biased_ok"] and v["saturation_free"]
    assert sesrq.saturation_verdict(w4, np.array([32767], np.int32))["reach"] == (1 << 19) + 32767      # the reference configuration's worst
    assert case_c_edge(True).verdicts()[4]["reach"] == LIMIT and case_c_edge(False).verdicts()[4]["reach"] == LIMIT - 128
    with pytest.raises(ValueError, match="sesrq_saturation_verdict"):
        sesrq.saturation_verdict(np.zeros((1, 16, 4, 4), np.int8))
    with pytest.raises(ValueError, match="out of range"):
        sesrq.saturation_verdict(w4, acc_bits=18, add_bits=17)


def _golden_nets():
    from conftest import golden_files
    from helpers import fixture_case
    for path in golden_files():
        if path.endswith((".crop.npz", ".zeros.npz", ".satw.npz", ".satw_zeros.npz", ".stim.npz", ".full.npz")):
            yield path, fixture_case(path)[2]


def test_reference_bundles_stay_inside_the_biased_range():
    """18 / 20 bits and a 16-bit constant bound every sum + constant by 2^19 + 2^15: no golden bundle ever meets the guard, so each keeps
    the kernels it ran before the guard existed (the GPU test below compares the names and the launch plan)."""
    n = 0
    for path, net in _golden_nets():
        for k, l in enumerate(net.layers):
            v = sesrq.saturation_verdict(l.wq, l.add_const, net.zero[k], net.acc_bits, net.add_bits)
            assert v["biased_ok"] and v["reach"] <= (1 << 19) + (1 << 15), (path, k, v)
            assert v == np_verdict(l.wq, l.add_const, net.zero[k], net.acc_bits, net.add_bits), (path, k)
            n += 1
    assert n >= 5 * 20


# ------------------------------------------------------------------------------------------------ GPU part
PLANS = [("trio", dict()), ("mfma", dict(fuse_hidden=0)), ("dot4", dict(engine=_lib.ENGINE_DOT4)), ("general", dict(force_general=True)),
         ("dot4-general", dict(engine=_lib.ENGINE_DOT4, force_general=True))]
FORMS = [("forms-off", dict(reduced_forms=1 | 8)), ("forms-off-mfma", dict(reduced_forms=1 | 8, fuse_hidden=0))]      # PLANS run reduced_forms = 63


def run_case(case, plans, taps=True):
    """Every plan: the engine names the verdict predicts, then fp32 and int8 frames of every size against the oracle; the per-layer plans
    also hand out the PE taps (forward_debug), compared with the oracle's."""
    import torch
    b = bundle_from_oracle(case.net)
    for tag, kw in plans:
        e = sesrq.Engine(b, device(), **kw)
        assert e.layer_engines() == case.expected_engines(**kw), f"{case.name} [{tag}]: {e.layer_engines()}"
        for size in SIZES:
            st = case.want(size)
            q0, x = case.frames(*size)
            for lbl, t in (("f32", torch.from_numpy(x)), ("i8", torch.from_numpy(q0))):
                q, y = e.forward(t.to(device()))
                same(f"{case.name} [{tag}] {size} {lbl} q_out", q, st["q_out"])
                same(f"{case.name} [{tag}] {size} {lbl} y", y, st["y"], values=True)      # z_out == 0: dot4 carries the sign of rint(-0.3) into y
        if taps and tag in ("mfma", "dot4"):
            size = SIZES[1]
            st = case.want(size)
            res = e.forward_debug(torch.from_numpy(case.frames(*size)[0]).to(device()), pe=True, acts=(tag == "dot4"))
            for k in range(5):
                same(f"{case.name} [{tag}] pe_out{k}", res[f"pe_out{k}"][0], st[f"pe_out{k}"])
                same(f"{case.name} [{tag}] pe_add{k}", res[f"pe_add{k}"], st[f"pe_add{k}"])
                if tag == "dot4":
                    same(f"{case.name} [{tag}] input{k}", res[f"input{k}"], st[f"input{k}"])
            same(f"{case.name} [{tag}] q_out (debug)", res["q_out"], st["q_out"])
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("where,variant", A_CASES, ids=[f"{w}-{v}" for w, v in A_CASES])
def test_pe_clamp_thresholds_18_20(where, variant):
    """Case A.  Below the threshold the layer is reported -merged (no clamp in the kernel at all), one PE beyond it -hybrid, two
    -general; the bytes and the PE taps are the oracle's on every plan."""
    case = case_a(where, variant)
    names = case.expected_engines(fuse_hidden=0)
    want = {"merged": "-merged", "general": "-general"}.get(variant, "-general" if where == "last3" else "-hybrid")
    assert names[case.t].endswith(want), names
    run_case(case, PLANS)


@pytest.mark.gpu
def test_trio_with_three_layers_at_the_threshold():
    """Case A inside the fused trio: every hidden layer has PEs at acc_lo exactly and all four at once (== add_lo)."""
    case = case_a_trio()
    assert case.expected_engines()[1:4] == ["mfma-trio-merged"] * 3
    run_case(case, PLANS + FORMS)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,where", B_CASES, ids=[f"{b[0]}-{b[1]}-{w}" for b, w in B_CASES])
def test_run_time_bounds_at_their_limits(bits, where):
    """Case B: the run-time-bounds kernels (GEN_ANY) with sums at acc_hi, acc_hi + 1, acc_lo, acc_lo - 1 and, at (17, 17), totals at
    add_hi, add_hi + 1, add_lo, add_lo - 1."""
    run_case(case_b(bits, where), PLANS[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["last12", "hidden3", "first3"])
def test_biased_limit_at_wide_accumulators(where):
    """Case C at (24, 26) bits: saturation-free by proof, sums + add constant at 2^22 - 1, 2^22, 2^22 + 1, their negatives, neighbours
    up to 2^22 + 2^18 and 6 451 600.  The layer must leave the biased kernels (-unbiased) and give the oracle's bytes."""
    case = case_c_wide(where)
    v = case.verdicts()[case.t]
    assert v["saturation_free"] and not v["biased_ok"]
    assert case.expected_engines(fuse_hidden=0)[case.t].endswith("-unbiased")
    run_case(case, PLANS + FORMS)


@pytest.mark.gpu
@pytest.mark.parametrize("where,variant", C_CONST_CASES, ids=[f"{w}-{v}" for w, v in C_CONST_CASES])
def test_biased_limit_through_add_constants(where, variant):
    """Case C at 18 / 20 bits: add constants +-(2^22 - 2^19), +-2^23, +-2^24 on a layer that would otherwise run merged (the trio
    included), hybrid or with the literal clamps."""
    case = case_c_const(where, variant)
    assert not case.verdicts()[case.t]["biased_ok"]
    assert "mfma-trio-merged" not in case.expected_engines() or case.t == 0 or case.t == 4
    run_case(case, PLANS + FORMS)


@pytest.mark.gpu
@pytest.mark.parametrize("full", [True, False], ids=["reach-2^22", "reach-2^22-128"])
def test_biased_guard_threshold(full):
    """The guard's threshold: reach == 2^22 leaves the biased kernels, reach == 2^22 - 128 stays (and the biased sums are exact there)."""
    case = case_c_edge(full)
    assert case.expected_engines()[4] == ("mfma-h5-unbiased" if full else "mfma-h5-merged")
    run_case(case, PLANS + FORMS)


@pytest.mark.gpu
def test_reference_bundles_keep_their_kernels():
    """Every golden bundle: layer_engines() and launch_plan() are what the saturation verdict alone selects -- the selection rule before
    the biased-range guard existed; no layer is -unbiased."""
    n = 0
    for path, net in _golden_nets():
        if net.quan_bits != 8:
            continue
        assert [l.wq.shape[2] for l in net.layers] == [5, 3, 3, 3, 5]
        for tag, kw in PLANS:
            e = sesrq.Engine(bundle_from_oracle(net), device(), **kw)
            names = e.layer_engines()
            plan, want = expected_plan_and_engines(net, **kw)
            if not e.fast_division_proven() and kw.get("engine") != _lib.ENGINE_DOT4:
                want[0] = want[0].replace("mfma-f5", "dot4")        # no proven division form: layer 0 divides on the dot4 kernel
            assert names == want and not any("unbiased" in s_ for s_ in names), (path, tag, names, want)
            assert e.launch_plan() == plan, (path, tag, e.launch_plan(), plan)
            e.close()
            n += 1
    assert n >= 5 * 20
