"""Constructed nets that DRIVE chosen accumulator values through a kernel -- TEST INFRASTRUCTURE (not collected).

Two constructions over the same five-layer shape (5x5 cin->16, three 3x3 16->16 that form the fused trio, 5x5 16->cout), both with ONE
probed layer and identity relays (one centre tap, + 128, M * 2^-n == 1, zero point -128) everywhere else:

  bound-attaining rows (sat / relay / probe, build_layer): constant planes under weights of one sign reach the static bounds of the
  load-time proof exactly -- tests/test_accumulator_limits.py;

  ramp rows (ramp / off, ramp_layer, Ramp): the frame holds a = (x - m) mod 256 - 128 in channel 0 and b = (y - m) mod 256 - 128 in
  the others, so the interior of a (256 + 2 m)^2 frame contains every (a, b) pair; a ramp row sums a + 256 b + add_const and so takes
  every integer of a 65 536-long interval exactly once -- tests/test_requant_sweep.py.

A third construction, of centre taps only, carries the input quantiser's code of every pixel to the output (Carrier) --
tests/test_input_sweep.py.

exact_byte is the requant restated in exact integer arithmetic: the independent reference of the sweep.
"""
import numpy as np

from oracle import sesrq_oracle as O

ONE = (1 << 15, 15)            # M * 2^-n == 1: the output byte moves with every LSB of the sum
HALF = (1 << 15, 16)           # residual merge of two equal operands: (2 q + 256) / 2 - 128 == q
MARGIN = 8                     # receptive radius of the five layers is 7: pixels further inside see no padding


# ------------------------------------------------------------------------------------------------ bound-attaining construction
def _spread(total, slots):
    """`total` as `slots` weights of one sign, each within int8's symmetric part."""
    sign, rest, out = (1 if total >= 0 else -1), abs(int(total)), []
    for _ in range(slots):
        out.append(sign * min(127, rest))
        rest -= min(127, rest)
    if rest:
        raise ValueError(f"weight sum {total} does not fit {slots} taps")
    return out


def _pe_weights(T, chans, planes, taps):
    """Weights [len(chans)][taps] of one PE whose sum over constant planes is exactly T = 127 A - 128 B, A / B = the weight sums on the
    127 / -128 planes.  The representation with A and B of opposite sign (T >= 0: A >= 0 >= B) makes T the PE's static extreme."""
    chans = [c for c in chans if planes[c] is not None]      # a varying channel (a relayed byte) carries no probe weight
    hi = [c for c in chans if planes[c] == 127]
    lo = [c for c in chans if planes[c] == -128]
    if not chans:
        raise ValueError("a probed PE needs input channels with known constant planes")
    if T == 0:
        A = B = 0
    elif not hi or (lo and T % 128 == 0):
        if T % 128:
            raise ValueError(f"PE sum {T} is no multiple of 128 and the PE has no 127 plane")
        A, B = 0, -T // 128
    elif not lo:
        if T % 127:
            raise ValueError(f"PE sum {T} is no multiple of 127 and the PE has no -128 plane")
        A, B = T // 127, 0
    else:
        A = (-T) % 128 if T >= 0 else -(T % 128)
        B = (127 * A - T) // 128
    assert 127 * A - 128 * B == T
    w = {c: [0] * taps for c in chans}
    for total, group in ((A, hi), (B, lo)):
        if total:
            flat = _spread(total, len(group) * taps)
            for i, c in enumerate(group):
                w[c] = flat[i * taps:(i + 1) * taps]
    return w


def sat(c):
    return ("sat", c)


def relay(j):
    return ("relay", j)


def probe(T, s):
    """An output channel whose four raw PE sums are T[0..3] at interior pixels and whose sum + add constant is s there."""
    return ("probe", tuple(int(t) for t in T), int(s))


def build_layer(k, ic, rows, planes, Mn, relu, bits):
    """rows -> (O.Layer, {row: (T, s)}).  planes[c]: the constant value of input channel c, or None (varying: relays only)."""
    taps, ctr = k * k, (k * k) // 2
    acc_lo, acc_hi = -(1 << (bits[0] - 1)), (1 << (bits[0] - 1)) - 1
    add_lo, add_hi = -(1 << (bits[1] - 1)), (1 << (bits[1] - 1)) - 1
    w = np.zeros((len(rows), ic, taps), np.int64)
    ac = np.zeros(len(rows), np.int64)
    probes = {}
    for o, row in enumerate(rows):
        if row[0] == "sat":           # small weights of one sign, a constant that dominates them, a requant that saturates
            w[o, :, ctr] = 1
            ac[o] = 32767 if row[1] == 127 else -32768
            if row[1] == 127 and (32767 - 128 * ic) * Mn[0] * 2.0 ** -Mn[1] < 255:
                raise ValueError("this requant multiplier cannot saturate a 127 plane")
        elif row[0] == "relay":       # q -> q: one centre tap, + 128, M 2^-n == 1, ReLU a no-op, zero point -128
            if Mn != ONE or row[1] >= ic:
                raise ValueError("a relay needs M * 2^-n == 1 and an existing input channel")
            w[o, row[1], ctr] = 1
            ac[o] = 128
        else:
            _, T, s = row
            for p in range(4):
                chans = list(range(p, ic, 4))
                if T[p] == 0 and not chans:
                    continue
                for c, wc in _pe_weights(T[p], chans, planes, taps).items():
                    w[o, c] = wc
            tot = min(max(sum(min(max(t, acc_lo), acc_hi) for t in T), add_lo), add_hi)
            ac[o] = s - tot
            if abs(ac[o]) > 1 << 24:
                raise ValueError("add constant beyond what sesrq_create accepts")
            probes[o] = (T, s)
    lay = O.Layer(wq=w.reshape(len(rows), ic, k, k).astype(np.int8), add_const=ac.astype(np.int32), M=Mn[0], n=Mn[1], relu=relu)
    return lay, probes


# ------------------------------------------------------------------------------------------------ ramp construction
BIASED_LIMIT = 1 << 22                        # |s| the biased accumulator cannot hold (planner.LIMIT)
RAMP_SIDE = 256 + 2 * MARGIN                  # interior pixels see no padding and carry every (a, b) pair once
WIDE_LO, WIDE_HI = -32896, 32639              # a + 127 b + 127 b + 2 b over a, b in [-128, 127]: 65 536 consecutive integers
WIDE_CONST_MAX = BIASED_LIMIT - 1 - 257 * 128           # reach = worst_sum + max |add_const| < 2^22 with weights 1, 127, 127, 2
NARROW_CONST_MAX = BIASED_LIMIT - 1 - 128               # ... with one weight of -1
B_WEIGHTS = {8: (127, 127, 2), 4: (7, 7, 2), 2: (1, 1, 1, 1)}      # weights within the width's range that sum to 2^b, one per b copy


def ramp(c, narrow=False):
    """A ramp row.  Wide (weights 1 on the a copy, 127, 127, 2 on the b copies): s = a + 256 b + c takes every integer of
    [c - 32896, c + 32639] once.  Narrow (weight -1 on a alone): s = c - a takes every integer of [c - 127, c + 128]; its static worst
    sum is 128, so a layer of narrow rows stays on the biased kernels up to c = 2^22 - 129, where it reaches s = 2^22 - 1 itself
    (weight +1 would stop at 2^22 - 2: the static bound counts |a| = 128 on either side).  At a width b < 8 (Ramp(b=)) the ramps run
    over [-2^(b-1), 2^(b-1) - 1] and a wide row takes the 4^b sums of [c - (2^b + 1) 2^(b-1), c + (2^b + 1) (2^(b-1) - 1)]."""
    c = int(c)
    if abs(c) > (NARROW_CONST_MAX if narrow else 1 << 24):
        raise ValueError("add constant beyond what the row's layer can carry")
    return ("ramp", c, bool(narrow))


def off():
    """A row without weights whose constant -32768 gives 0 behind ReLU: the zero point of the next domain, clamped."""
    return ("off",)


def ramp_interval(row, b=8):
    _, c, narrow = row
    half, span = 1 << (b - 1), 1 << b
    return (c - half + 1, c + half) if narrow else (c - (span + 1) * half, c + (span + 1) * (half - 1))


def ramp_cover(lo, hi, biased=True, b=8):
    """(wide rows, narrow rows) whose intervals together contain [lo, hi] and nothing is left out in between.  biased: keep every row
    on the biased kernels (|lo|, |hi| <= 2^22 - 1): wide rows up to add constant 2^22 - 1 - 32896, i.e. sums up to 4 194 046, narrow
    rows for the 257 sums above.  Downwards the wide rows reach -(2^22 - 1) themselves.  No sum of the biased range stays unreached."""
    lo, hi = int(lo), int(hi)
    if biased and not -(BIASED_LIMIT - 1) <= lo <= hi <= BIASED_LIMIT - 1:
        raise ValueError("range outside the biased accumulator's")
    wlo, whi = ramp_interval(ramp(0), b)
    if b != 8 and hi + 1 - wlo > WIDE_CONST_MAX:
        raise ValueError("the top band needs 8-bit rows")
    wide, narrow, s = [], [], lo
    while s <= hi:
        c = s - wlo
        if biased and c > WIDE_CONST_MAX:
            if s <= WIDE_CONST_MAX + WIDE_HI:               # a last wide row, overlapping the one before
                wide.append(ramp(WIDE_CONST_MAX))
                s = WIDE_CONST_MAX + WIDE_HI + 1
                continue
            c = min(s + 127, NARROW_CONST_MAX)
            narrow.append(ramp(c, True))
            s = c + 129
            continue
        wide.append(ramp(c))
        s = c + whi + 1
    return wide, narrow


def ramp_frame(cin=4, b=8):
    """(int8 q0, the fp32 frame that quantises to it at scale 1, zero point -2^(b-1)): channel 0 = a along x, the others = b along y,
    on a (2^b + 2 m)^2 frame."""
    half, span = 1 << (b - 1), 1 << b
    side = span + 2 * MARGIN
    ax = ((np.arange(side) - MARGIN) % span - half).astype(np.int8)
    q0 = np.empty((1, cin, side, side), np.int8)
    q0[0, 0] = ax[None, :]
    q0[0, 1:] = ax[:, None]
    return q0, q0.astype(np.float32) + np.float32(half)


def ramp_layer(k, ic, rows, src, Mn, relu, Mn_oc=None, b=8):
    """rows of relay / off / ramp -> O.Layer.  src: the input channels that hold a, b, b, b (b = 2: four b copies).  Mn_oc: one (M, n)
    per row (per-channel layer).  b: the width: a relay adds 2^(b-1), the b copies carry B_WEIGHTS[b]."""
    ctr = (k * k) // 2
    w = np.zeros((len(rows), ic, k * k), np.int64)
    ac = np.zeros(len(rows), np.int64)
    for o, row in enumerate(rows):
        if row[0] == "relay":
            if Mn != ONE or Mn_oc is not None or row[1] >= ic:
                raise ValueError("a relay needs M * 2^-n == 1 and an existing input channel")
            w[o, row[1], ctr] = 1
            ac[o] = 1 << (b - 1)
        elif row[0] == "off":
            ac[o] = -32768
        elif row[0] == "ramp":
            if row[2]:
                if b != 8:
                    raise ValueError("narrow rows are 8-bit rows")
                w[o, src[0], ctr] = -1
            else:
                for c, v in zip(src, (1,) + B_WEIGHTS[b]):
                    w[o, c, ctr] += v
            ac[o] = row[1]
        else:
            raise ValueError(f"no ramp-layer row: {row!r}")
    lay = O.Layer(wq=w.reshape(len(rows), ic, k, k).astype(np.int8), add_const=ac.astype(np.int32), M=Mn[0], n=Mn[1], relu=relu)
    if Mn_oc is not None:
        lay.M_oc = np.array([m for m, _ in Mn_oc], np.int64)
        lay.n_oc = np.array([n for _, n in Mn_oc], np.int64)
    return lay


class Ramp:
    """One forward of the sweep: a five-layer net whose layer t carries ramp rows, the frame, and what the construction promises.

    t = 0       rows <= 16, all probed; layers 1..3 are identities of layer 0's output, which is also the residual operand:
                (2 q + 256) / 2 - 128 == q (HALF).  split=True (needed when zero[1] != -128, where layer 0 writes a separate residual
                tensor): rows <= 8; layers 1..3 carry channel o on channel o + 8 and leave 0..7 at -128, layer 0's rows 8..15 are off,
                so with M_res * 2^-n_res == 1 the output shows rc on channel o and q on channel o + 8.
    t = 1..3    rows <= 8 on channels 0..7 (layer 0's rows there are off: rc == -128, the merge passes ic through); channels 8..11
                relay a, b, b, b up to the probed layer.  t = 3 is the merging layer: (M, n) is its FIRST requant, into the fixed -128
                domain of ic; `res` and `zmerge` set the second one.
    t = 4       rows <= cout; a, b, b, b reach it through the merge by the HALF trick.
    t = "m"     the merge's second requant alone: rc = a or b (layer 0 relays it), ic = the other one: u = a + b + 256 takes all 511
                values.  Four rows (a + b, b + a alternately); (M, n) is unused.
    cin: 3 for the x2 anchor add (t >= 1 only).  z: the zero point of the domain layer t requantises into (zero[1], zero[t + 1],
    zero[5]; t = 3: unused, see zmerge).  b: the net's width (define.py QUAN_BIT) 8, 4 or 2, t >= 1: every -128 above reads -2^(b-1),
    every 256 reads 2^b, the frame is (2^b + 2 m)^2 and at b = 2 the relays carry four b copies (channels 9..12).
    """

    def __init__(self, t, Mn, rows, z=None, cout=16, ps=4, klast=5, res=None, zmerge=None, split=False, Mn_oc=None, bits=(18, 20), cin=4,
                 b=8, name=""):
        L = 5
        half = 1 << (b - 1)
        z = -half if z is None else z
        zmerge = -half if zmerge is None else zmerge
        if (cin != 4 or b != 8) and t == 0:
            raise ValueError("the probed first layer reads the four 8-bit frame channels a, b, b, b")
        self.t, self.Mn, self.rows, self.z, self.cout, self.split, self.zmerge, self.b = t, Mn, list(rows), z, cout, split, zmerge, b
        cap = 4 if t == "m" else cout if t == 4 else 16 if (t == 0 and not split) else 8
        if not 0 < len(self.rows) <= cap:
            raise ValueError(f"{len(self.rows)} rows, the position carries 1..{cap}")
        R = len(self.rows)
        nsrc = 1 + len(B_WEIGHTS[b])
        src_hidden = tuple(range(8, 8 + nsrc))
        offs = [off()] * 16
        rows_of = [list(offs) for _ in range(L)]
        rows_of[L - 1] = [off()] * cout
        if t == "m":
            for r in range(4):
                rows_of[0][r] = relay(r % 2)
                rows_of[1][r] = relay(r ^ 1)
                rows_of[2][r] = rows_of[3][r] = relay(r)
            seen = list(range(4))
        elif t == 0:
            rows_of[0][:R] = self.rows
            for k in (1, 2, 3):
                for o in range(R):
                    rows_of[k][o + 8 if split else o] = relay(o if (k == 1 or not split) else o + 8)
            seen = list(range(16 if split else R))
        else:
            for i in range(nsrc):
                rows_of[0][8 + i] = relay(min(i, cin - 1))          # a three-channel frame a, b, b: the last b twice
            for k in range(1, min(t, 4)):
                for c in src_hidden:
                    rows_of[k][c] = relay(c)
            if t == 4:
                rows_of[4][:R] = self.rows
                seen = []
            else:
                rows_of[t][:R] = self.rows
                for k in range(t + 1, 4):
                    for o in range(R):
                        rows_of[k][o] = relay(o)
                seen = list(range(R))
        for o in seen:
            if o < cout:
                rows_of[L - 1][o] = relay(o)
        res = res if res is not None else (HALF if (t == 4 or (t == 0 and not split)) else ONE)
        self.res = res
        zero = [-half] * (L + 1)
        zero[L - 1] = zmerge
        if t != "m" and t != 3:
            zero[1 if t == 0 else t + 1] = z
        layers = []
        for k in range(L):
            kk = klast if k == L - 1 else 5 if k == 0 else 3
            probed = k == t
            layers.append(ramp_layer(kk, cin if k == 0 else 16, rows_of[k], (0, 1, 2, 3) if k == 0 else src_hidden, Mn if probed else ONE,
                                     relu=(k != L - 1), Mn_oc=Mn_oc if probed else None, b=b))
        self.net = O.Net(layers=layers, scale=[1.0] * (L + 1), zero=zero, M_res=res[0], n_res=res[1], pixel_shuffle=ps,
                         acc_bits=bits[0], add_bits=bits[1], quan_bits=b, name=name or f"ramp t={t} {Mn} z={z} b={b}")
        self.q0, self.x = ramp_frame(cin, b)

    def intervals(self):
        return [ramp_interval(r, self.b) for r in self.rows]

    def sums(self, st):
        """[row] -> the sums + add constant of layer t at interior pixels (H, W) from an oracle's pe_add tap; t = "m": u = rc + ic + 2^b."""
        m = MARGIN
        if self.t == "m":
            return [st["input1"][0, r, m:-m, m:-m].astype(np.int64) + st["input3"][0, r, m:-m, m:-m].astype(np.int64) + (1 << self.b)
                    for r in range(4)]
        ac = self.net.layers[self.t].add_const.astype(np.int64)
        return [st[f"pe_add{self.t}"][0, o, m:-m, m:-m].astype(np.int64) + ac[o] for o in range(len(self.rows))]

    def assert_covered(self, st):
        """Every row takes every sum of its interval, each exactly once (a narrow row: once per frame row), and nothing else: a case
        that misses its range fails."""
        S = self.sums(st)
        if self.t == "m":
            for r, u in enumerate(S):
                assert np.array_equal(np.unique(u), np.arange((2 << self.b) - 1)), f"{self.net.name}: row {r} misses values of u"
            return S
        for o, (lo, hi) in enumerate(self.intervals()):
            got, count = np.unique(S[o], return_counts=True)
            each = 256 if self.rows[o][2] else 1                # a narrow row does not depend on b: every sum once per frame row
            assert np.array_equal(got, np.arange(lo, hi + 1)) and (count == each).all(), \
                f"{self.net.name}: row {o} covers [{got[0]}, {got[-1]}] in {got.size} values, not [{lo}, {hi}] {each} time(s) each"
        return S

    def expected_rows(self, S):
        """{output channel: bytes (H, W) at interior pixels} from the exact-integer restatement alone."""
        t, (M, n), b = self.t, self.Mn, self.b
        half = 1 << (b - 1)
        out = {}
        if t == "m":
            for r, u in enumerate(S):
                out[r] = exact_byte(u, self.res[0], self.res[1], self.zmerge, relu=False, b=b)
            return out
        oc = self.net.layers[t].M_oc
        for o, s in enumerate(S):
            if oc is not None:
                M, n = int(self.net.layers[t].M_oc[o]), int(self.net.layers[t].n_oc[o])
            if t == 3:
                ic = exact_byte(s, M, n, -half, relu=True, b=b)
                out[o] = exact_byte(ic.astype(np.int64) + half, self.res[0], self.res[1], self.zmerge, relu=False, b=b)
            elif t == 0 and self.split:
                out[o] = exact_byte(s, M, n, -128, relu=True)            # rc
                out[o + 8] = exact_byte(s, M, n, self.z, relu=True)      # q in the domain zero[1]
            else:
                out[o] = exact_byte(s, M, n, self.z, relu=(t != 4), b=b)
        return {o: v for o, v in out.items() if o < self.cout}


# ------------------------------------------------------------------------------------------------ carrier construction
class Carrier:
    """A five-layer net of centre taps only that CARRIES the input quantiser's code of every pixel to the output: the first layer has
    weight 1 at (2, 2) from input channel c to output channel c, relays stand behind it, and output channel o shows input channel
    o mod cin.  Every output pixel depends on its own input pixel only: every pixel of a frame is a probe of q0, and padding plays no
    part.  tests/test_input_sweep.py.

    rc=False    zero[1] = -2^(b-1): layer 0's output is the residual operand too; layers 1..3 relay, the merge halves the two equal
                operands (HALF).
    rc=True     zero[1] = z1 != -2^(b-1): layer 0 writes a separate residual tensor, and THAT copy carries the probe: layers 1..3 are
                off (ic == -2^(b-1), constant), the merge adds it with M_res * 2^-n_res == 1.
    risky       output rows of layer 0 that carry no probe and whose weights (127 on every tap of input channel 0) let PE 0 leave its
                accumulator: they choose the hybrid kernel (one row, or rows of one accumulator register: 4 i .. 4 i + 3; rows of two
                registers: "clamp all four") without touching a probed channel.  Nothing behind layer 0 reads them.
    bits        the PE accumulator / adder widths: anything but (18, 20) takes the run-time bounds (GEN_ANY) under force_general.
    The expected output byte of a pixel is lut()[o][q0 - qlo]: the LUT comes from an oracle's forward of a frame of all 2^b codes."""

    def __init__(self, cin, s0, z0, b=8, rc=False, risky=(), cout=16, ps=1, bits=(18, 20), z1=None, name=""):
        L, half = 5, 1 << (b - 1)
        if not 1 <= cin <= 4 or cout % (ps * ps) or any(r < cin or r >= 16 for r in risky):
            raise ValueError("carrier: 1..4 input channels, whole output channels, risky rows beside the probed ones")
        self.cin, self.b, self.rc, self.cout, self.ps = cin, b, rc, cout, ps
        rows_of = [[off()] * 16 for _ in range(L)]
        for c in range(cin):
            rows_of[0][c] = relay(c)
            if not rc:
                for k in (1, 2, 3):
                    rows_of[k][c] = relay(c)
        rows_of[L - 1] = [relay(o % cin) for o in range(cout)]
        zero = [-half] * (L + 1)
        zero[0] = int(z0)
        if rc:
            zero[1] = (-half + 28 if b == 8 else -half + 1) if z1 is None else z1
            if zero[1] == -half:
                raise ValueError("carrier: rc=True needs zero[1] != -2^(b-1)")
        layers = [ramp_layer(5 if k in (0, L - 1) else 3, cin if k == 0 else 16, rows_of[k], (), ONE, relu=(k != L - 1), b=b) for k in range(L)]
        for r in risky:
            layers[0].wq[r, 0] = 127
        res = ONE if rc else HALF
        self.net = O.Net(layers=layers, scale=[float(s0)] + [1.0] * L, zero=zero, M_res=res[0], n_res=res[1], pixel_shuffle=ps,
                         acc_bits=bits[0], add_bits=bits[1], quan_bits=b, name=name or f"carrier cin={cin} s0={s0} z0={z0} b={b} rc={rc}")

    def all_codes(self):
        """int8 (1, cin, 1, 2^b): every code of the width in every channel, channel c rotated by c."""
        q = np.arange(-(1 << (self.b - 1)), 1 << (self.b - 1), dtype=np.int64)
        return np.stack([np.roll(q, c) for c in range(self.cin)]).astype(np.int8)[None, :, None, :]

    def unshuffle(self, a):
        """(1, cout / ps^2, H ps, W ps) -> (cout, H, W): the inverse of O.pixel_shuffle (numpy arrays and torch tensors alike)."""
        r = self.ps
        _, c, Hr, Wr = a.shape
        return a.reshape(c, Hr // r, r, Wr // r, r).permute(0, 2, 4, 1, 3).reshape(c * r * r, Hr // r, Wr // r) if hasattr(a, "permute") else \
            a.reshape(c, Hr // r, r, Wr // r, r).transpose(0, 2, 4, 1, 3).reshape(c * r * r, Hr // r, Wr // r)

    def lut(self, forward):
        """int8 (cout, 2^b): the output byte of channel o for every code of its input channel, by `forward` (an oracle's) on the frame
        of all codes."""
        q0 = self.all_codes()
        out = self.unshuffle(forward(self.net, q0)["q_out"])[:, 0, :]
        lut = np.empty((self.cout, 1 << self.b), np.int8)
        for o in range(self.cout):
            lut[o] = np.roll(out[o], -(o % self.cin))            # undo the channel's rotation: index = q0 - qlo
        return lut


# ------------------------------------------------------------------------------------------------ the requant in exact integers
def _round24(x):
    """int64 -> the nearest integer with 24 significant bits, ties to even: what one fp32 rounding does to an exact value."""
    x = np.asarray(x, np.int64)
    a = np.abs(x)
    e = np.zeros(a.shape, np.int64)
    for k in range(24, 50):
        e += a >= (np.int64(1) << k)                      # bit length - 24, where positive
    q = a >> e
    rem = a - (q << e)
    half = np.where(e > 0, np.int64(1) << np.maximum(e - 1, 0), np.int64(0))
    q = q + (((rem > half) | ((rem == half) & (q & 1 == 1))) & (e > 0))
    return np.sign(x) * (q << e)


def exact_byte(s, M, n, z, relu, b=8):
    """clamp_b(rint(f32(f32(s * M) * 2^-n + z))) with ReLU on the product, in exact integer arithmetic (units of 2^-n): both fp32
    roundings by hand as round-half-even to 24 significant bits.  Every intermediate fits int64: |s * M| < 2^38 (asserted below 2^49),
    |z| * 2^n < 2^48 for n <= 32, |z| <= 2^15.  For the merge: s = u = rc + ic + 2^b, (M, n) = (M_res, n_res), z = zero[L - 1], no ReLU
    (u >= 0).  b: the width whose range clamps the result."""
    s = np.asarray(s, np.int64)
    M, n, z = int(M), int(n), int(z)
    assert 0 <= n <= 32 and abs(z) <= 1 << 15 and 0 <= M < 1 << 16 and np.abs(s).max(initial=0) < 1 << 26
    p = _round24(s * M)                                    # f32(s * M), times 2^-n exactly
    if relu:
        p = np.maximum(p, 0)
    v = _round24(p + (np.int64(z) << n))                   # f32(t' + z)
    q = v >> n                                             # floor
    rem, half = v - (q << n), (np.int64(1) << (n - 1)) if n else np.int64(0)
    if n:
        q = q + ((rem > half) | ((rem == half) & (q & 1 == 1)))
    return np.clip(q, -(1 << (b - 1)), (1 << (b - 1)) - 1).astype(np.int8)
