"""Seeded integer nets of every topology sesrq_create accepts (depth 3..16, 1..16 channels per layer, 3x3 / 5x5 anywhere) -- TEST
INFRASTRUCTURE: oracle.synth_net and test_instances.craft_net draw 16-wide nets of depth 5 / 8 only.  tests/test_topologies.py runs these.

topo_net draws as synth_net draws (same distributions, same order per layer), with the channel counts and kernel sizes of the caller;
with `risky` it draws as craft_net draws: every (output channel, PE) weight group provably safe except the named ones.
"""
import functools

import numpy as np

from oracle import sesrq_oracle as O


def topo_net(widths, ks, cin, cout, ps, seed, hard=False, quan_bits=8, risky=None, zeros=None, gain=1.3) -> O.Net:
    """widths: the L - 1 hidden channel counts (layer k maps chans[k] -> chans[k + 1], chans = [cin] + widths + [cout]); ks: the L kernel
    sizes.  hard=False: weights normal x 14 with one 127 centre tap, add constants in +-6000, (M, n) = qconst(60 / (sqrt(fan) w_rms 74)
    U(0.6, 1.6)), zero points -128.  hard=True: weights from {-128, -100, 90, 127} with 15 % uniform, constants out to +-32767, zero points
    in [-150, -100).  risky={layer: (PEs, output channels)}: those (oc, PE) groups wide enough for the 18-bit PE clamp, every other group
    of every layer provably safe (128 sum|w| <= 131071), as craft_net.  zeros: the L + 1 zero points.  quan_bits < 8: _synth_narrow's
    multipliers, sized on a probe frame so that both clamp ends are reached."""
    L = len(ks)
    widths = list(widths)
    if len(widths) != L - 1 or L < 3:
        raise ValueError(f"{L} kernel sizes need {L - 1} hidden widths")
    if widths[0] != widths[-1]:
        raise ValueError("layer 0 and layer L-2 share the residual domain: equal widths")
    chans = [cin] + widths + [cout]
    shapes = [(chans[k + 1], chans[k], ks[k]) for k in range(L)]
    rng = np.random.default_rng(seed)
    name = f"topo_{'-'.join(map(str, widths))}_{seed}{'_hard' if hard else ''}"
    if quan_bits != 8:
        if risky is not None:
            raise ValueError("risky= places 8-bit weights")
        net = O._synth_narrow(name, seed, rng, cin, ps, shapes, hard, quan_bits, gain)
        net.name = f"{name}_q{quan_bits}"
        if zeros is not None:
            net.zero = list(zeros)
        return net
    layers = []
    for k, (oc, ic, kk) in enumerate(shapes):
        fan = ic * kk * kk
        if risky is not None:
            per_group = kk * kk * max(1, (ic + 3) // 4) if k > 0 else kk * kk      # weights per (oc, PE); first layer: one channel per PE
            wsafe = max(1, min(127, 1023 // per_group))
            w = rng.integers(-wsafe, wsafe + 1, size=(oc, ic, kk, kk))
            pes, ocs = risky.get(k, ((), ()))
            for p in pes:
                for o in ocs:
                    if o < oc:
                        w[o, p::4] = rng.choice(np.array([-128, -110, 100, 127]), size=w[o, p::4].shape)
            wr = float(np.sqrt(np.mean(w.astype(np.float64) ** 2))) + 1e-9
        elif hard:
            w = rng.choice(np.array([-128, -100, 90, 127], dtype=np.int64), size=(oc, ic, kk, kk))
            w = np.where(rng.random(w.shape) < 0.15, rng.integers(-128, 128, w.shape), w)
            wr = 110.0
        else:
            w = np.clip(np.rint(rng.standard_normal((oc, ic, kk, kk)) * 14.0), -128, 127)
            w[rng.integers(oc), rng.integers(ic), kk // 2, kk // 2] = 127
            wr = 14.0
        M, n = O.qconst(float(60.0 / (np.sqrt(fan) * wr * 74.0) * rng.uniform(0.6, 1.6)))
        ac = np.clip(rng.integers(-40000, 40000, oc), -32768, 32767).astype(np.int32) if hard else rng.integers(-6000, 6000, oc).astype(np.int32)
        layers.append(O.Layer(wq=w.astype(np.int8), add_const=ac, M=M, n=n, relu=(k != L - 1)))
    zero = [int(z) for z in rng.integers(-150, -100, L + 1)] if hard else [-128] * (L + 1)
    if zeros is not None:
        if len(zeros) != L + 1:
            raise ValueError(f"{L} layers have {L + 1} zero points")
        zero = [int(z) for z in zeros]
    scale = [float(s) for s in rng.uniform(0.003, 0.04, L + 1)]
    scale[0] = 1.0 / 255.0
    M_res, n_res = O.qconst(float(rng.uniform(0.2, 0.9)))
    return O.Net(layers=layers, scale=scale, zero=zero, M_res=M_res, n_res=n_res, pixel_shuffle=ps, name=name)


# (N, H, W) frames.  SEAM_FRAMES cross a 64-column strip, a row tile and (N = 2) a frame seam; RAGGED_FRAMES walk the tile edges of
# the dot4 and MFMA kernels from one pixel up, with batches
SEAM_FRAMES = ((2, 21, 70), (1, 41, 130))
RAGGED_FRAMES = [(1, 1, 1), (1, 3, 5), (1, 8, 32), (1, 9, 33), (2, 17, 70), (1, 40, 129), (3, 31, 64), (1, 26, 121)]

# id -> (kernel sizes, hidden widths, cin, cout, PixelShuffle): what each row reaches is told in tests/test_topologies.py
TOPOLOGIES = {
    "t3": ((5, 3, 5), (16, 16), 3, 12, 2),
    "t3n": ((3, 3, 3), (8, 8), 1, 4, 2),
    "t4": ((5, 3, 3, 5), (12, 9, 12), 2, 8, 2),
    "t4s": ((5, 3, 5, 5), (5, 7, 5), 1, 16, 4),
    "t6": ((5, 3, 3, 3, 3, 5), (16,) * 5, 3, 3, 1),
    "t7": ((5,) + (3,) * 5 + (5,), (16,) * 6, 3, 12, 2),
    "t16": ((5,) + (3,) * 14 + (5,), (16,) * 15, 3, 12, 2),
    "t16n": ((5,) + (3,) * 14 + (5,), (13,) * 15, 4, 9, 3),
    "t1": ((5, 3, 3, 3, 5), (1, 1, 1, 1), 1, 1, 1),
    "t15": ((5, 3, 3, 3, 5), (15, 15, 15, 15), 3, 12, 2),
    "tmix": ((5, 3, 3, 3, 5), (16, 4, 16, 16), 3, 12, 2),
}
# The seed of each (id, hard) case, default 1.  Chosen on the CPU, on the oracle alone, where the default draw is dead on the test frames
# (test_topologies.py::test_cases_are_live): a one-channel net multiplies one centre tap per layer, most draws saturate it.
SEEDS = {("t1", False, 8): 10, ("t3n", True, 8): 2,
         ("t4", False, 4): 2, ("t4", True, 4): 4, ("t4", False, 2): 2, ("t6", True, 4): 4, ("t6", False, 2): 11,
         ("t6", False, 4): 16, ("t6", True, 2): 7, ("t3", True, 2): 8, ("t4", True, 2): 79}
# ... and its gain where no seed at synth_net's 1.3 is live
GAINS = {("t6", False, 4): 3.0, ("t6", True, 2): 2.0, ("t3", True, 2): 10.0, ("t4", True, 2): 20.0}
# The narrow cases: (id, quan_bits, hard), every id x width x draw.  A width has 2^b codes; where the multipliers _synth_narrow sizes on its
# probe frame leave one code on nearly every pixel at every seed, the case is drawn with another gain (GAINS) -- at 2 bits with weights
# in {-2, 1} and zero points down to -170 only a large one lets the activations leave the lower clamp.
NARROW = [("t3", 4, False), ("t3", 4, True), ("t3", 2, False), ("t4", 4, False), ("t4", 4, True), ("t4", 2, False), ("t6", 4, True), ("t6", 2, False), ("t6", 4, False), ("t6", 2, True), ("t3", 2, True), ("t4", 2, True)]
# One risky PE in a narrow hidden layer: (id, layer, PE, seed, what the PE owns).  t4's layer 2 reads 9 channels: PE 0 owns 0, 4, 8, the
# others two each (the fewest); t15's layers read 15: PE 3 owns three, the others four.
RISKY = [("t4", 2, 1, 1, "two channels"), ("t4", 2, 3, 1, "the fewest (two)"), ("t4", 1, 0, 1, "three of 12"),
         ("t15", 2, 3, 2, "the fewest (three)"), ("t15", 1, 0, 2, "four of 15")]


@functools.lru_cache(maxsize=None)
def case_net(tid, hard=False, quan_bits=8, seed=None, gain=None) -> O.Net:
    ks, widths, cin, cout, ps = TOPOLOGIES[tid]
    if seed is None:
        seed = SEEDS.get((tid, hard, quan_bits), 1)
    if gain is None:
        gain = GAINS.get((tid, hard, quan_bits), 1.3)
    net = topo_net(widths, ks, cin, cout, ps, seed, hard=hard, quan_bits=quan_bits, gain=gain)
    net.name = f"{tid}{'_hard' if hard else ''}" + (f"_q{quan_bits}" if quan_bits != 8 else "")
    return net


@functools.lru_cache(maxsize=None)
def risky_net(tid, layer, pe, seed=1) -> O.Net:
    """The topology with craft_net's provably safe weights and ONE risky PE in `layer` (every output channel)."""
    ks, widths, cin, cout, ps = TOPOLOGIES[tid]
    net = topo_net(widths, ks, cin, cout, ps, seed, risky={layer: ((pe,), range(16))})
    net.name = f"{tid}_risky_l{layer}_pe{pe}"
    return net
