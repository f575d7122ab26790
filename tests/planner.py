"""The planner, restated: the ONE prediction of layer_engines() and launch_plan() the suite compares an engine with -- TEST
INFRASTRUCTURE.  A change to the kernel selection (choose_layer, select_mfma) or to the load-time proof is mirrored here and nowhere else.

np_verdict restates saturation_free and the biased-range guard from their definition; expected_plan_and_engines derives kernel kinds,
modes, trios and the launch plan from an oracle Net alone.  Tests that only hold a Bundle file keep their name checks: there is no
second path from bundles to verdicts.
"""
import numpy as np

from sesrq import _lib

LIMIT = 1 << 22                # |s| the biased accumulator cannot hold (one binade of 1.5 * 2^23 + s)


# Launch geometry, restated (csrc: MTW / TV / TW, cut_runs and xcd_block): columns per block in x of the per-layer MFMA kernels, the fused
# trio (60 valid columns of a 64-column window) and the dot4 kernels; the block -> (strip, run) split of the MFMA kernels and the trio is
# a multiply-high while strips and strips * runs stay below 2^16, and a division from there on.
STRIP_COLS = {"mfma": 64, "trio": 60, "dot4": 32}
SPLIT_LIMIT = 1 << 16


def strip_count(W, family):
    return -(-W // STRIP_COLS[family])


def widths_around(strips, family):
    """(the largest width with `strips` strips, the smallest with one more)."""
    return strips * STRIP_COLS[family], strips * STRIP_COLS[family] + 1


def run_count(strips, units, N, slots):
    """cut_runs' k: vertical runs per strip for a chip of `slots` workgroup slots."""
    return max(1, min(slots // (strips * N), units))


def split_divides(strips, runs):
    """True where the kernels' prologue divides (inv_nx == 0), False where it multiplies."""
    return not (strips * runs < SPLIT_LIMIT and strips < SPLIT_LIMIT)


def xcd_split(nx, ny, multiply):
    """xcd_block, restated for a whole grid of nx strips x ny runs: the (strip, run) every block (x, y) works on, as two int64 arrays
    in block order id = y nx + x.  The first total - total % 8 blocks are dealt round-robin to eight groups (v = (id & 7) per + (id >> 3)),
    then v is split into (v mod nx, v div nx): with `multiply` the quotient is mulhi(v, ceil(2^32 / nx)) as the kernels form it while
    inv_nx != 0, else the division."""
    total = nx * ny
    per = total >> 3
    ident = np.arange(total, dtype=np.int64)
    v = np.where(ident < per * 8, (ident & 7) * per + (ident >> 3), ident)
    inv = ((1 << 32) + nx - 1) // nx
    assert int(v.max()) * inv < 1 << 63                   # the 64-bit product the kernels' __umulhi takes the high word of
    q = (v * inv) >> 32 if multiply else v // nx
    by = np.where(ident < per * 8, q, ident // nx)
    bx = np.where(ident < per * 8, v - q * nx, ident % nx)
    return bx, by


def np_verdict(wq, add_const, zero, acc_bits, add_bits):
    """saturation_free + the biased-range guard, restated from their definition: per output channel and PE (input channels p mod 4) the
    extreme sums over q in [-128, 127] are hi = 127 S+ + 128 S-, -lo = -(128 S+ + 127 S-)."""
    oc, ic = wq.shape[:2]
    w = wq.astype(np.int64).reshape(oc, ic, -1)
    acc_hi, add_hi = (1 << (acc_bits - 1)) - 1, (1 << (add_bits - 1)) - 1
    hi = np.zeros((oc, 4), np.int64)
    lo = np.zeros((oc, 4), np.int64)
    for p in range(4):
        sp = np.clip(w[:, p::4], 0, None).sum((1, 2))
        sn = np.clip(-w[:, p::4], 0, None).sum((1, 2))
        hi[:, p], lo[:, p] = 127 * sp + 128 * sn, 128 * sp + 127 * sn
    risky = (hi > acc_hi) | (lo > acc_hi + 1)
    mask = sum(1 << p for p in range(4) if risky[:, p].any())
    worst_pe, worst_sum = int(max(hi.max(), lo.max())), int(max(hi.sum(1).max(), lo.sum(1).max()))
    free = -128 <= max(zero, -128) <= 127 and mask == 0 and not ((hi.sum(1) > add_hi) | (lo.sum(1) > add_hi + 1)).any()
    reach = min(worst_sum, 1 << (add_bits - 1)) + int(np.abs(np.asarray(add_const, np.int64)).max())
    return dict(saturation_free=bool(free), biased_ok=reach < LIMIT, risky_mask=mask, worst_pe=worst_pe, worst_sum=worst_sum, reach=reach)


def verdicts(net):
    return [np_verdict(l.wq, l.add_const, net.zero[k], net.acc_bits, net.add_bits) for k, l in enumerate(net.layers)]


def expected_plan_and_engines(net, engine=_lib.ENGINE_AUTO, force_general=False, fuse_hidden=1, fast_division=True, **_):
    """launch_plan() and layer_engines() from the net alone.  Kernel kind by position and kernel size (first: 5x5 MFMA, 3x3 dot4; hidden:
    h3 / h5; last: 5x5 h5, h5p for <= 4 channels, 3x3 dot4); mode from the saturation verdict (merged / one risky PE at 18 / 20 bits:
    hybrid / general / beyond the biased range: unbiased); trios greedy from L-2 backwards over 3x3 16->16 saturation-free layers.
    A net narrower than 8 bits has MFMA kinds under ENGINE_MFMA_Q only, and no hybrid there."""
    L, b = net.L, net.quan_bits
    v = verdicts(net)
    sfx = f"-q{b}" if b < 8 else ""
    narrow = b < 8
    dot4_only = engine == _lib.ENGINE_DOT4 or (narrow and engine != _lib.ENGINE_MFMA_Q)
    kinds, names = [], []
    for k, l in enumerate(net.layers):
        oc, ic, kk = l.wq.shape[:3]
        if dot4_only or (narrow and not v[k]["biased_ok"]):
            kind = None
        elif k == 0:
            kind = "f5" if kk == 5 else None
        elif kk == 3:
            kind = None if k == L - 1 else "h3"
        else:
            kind = "h5p" if (k == L - 1 and oc <= 4) else "h5"
        kinds.append(kind)
        d4 = ("dot4-merged" if v[k]["saturation_free"] else "dot4-general") + sfx
        if kind is None or (k == 0 and not fast_division):
            names.append(d4)
            continue
        one = bin(v[k]["risky_mask"]).count("1") == 1 and (net.acc_bits, net.add_bits) == (18, 20) and kind != "h5p" and not narrow
        mode = "unbiased" if not v[k]["biased_ok"] else "merged" if v[k]["saturation_free"] else "hybrid" if one else "general"
        names.append(f"mfma-{kind}-{mode}{sfx}")

    def trio_ok(k):
        oc, ic = net.layers[k].wq.shape[:2]
        return 1 <= k <= L - 2 and kinds[k] == "h3" and v[k]["saturation_free"] and v[k]["biased_ok"] and ic == 16 and oc == 16

    trio = set()
    k = L - 4
    while k >= 1 and trio_ok(k) and trio_ok(k + 1) and trio_ok(k + 2):
        trio.add(k)
        k -= 3
    if not fuse_hidden or force_general or engine == _lib.ENGINE_DOT4:
        trio = set()
    plan, k = [], 0
    while k < L:
        n = 3 if k in trio else 1
        if n == 3:
            names[k:k + 3] = ["mfma-trio-merged" + sfx] * 3
        plan.append((k, n))
        k += n
    return plan, names
