"""Frame geometry at the limits the library accepts: 4M-wide, 16M-tall, bases past 4 GiB, 65537 frames.

Every arithmetic edge is pinned elsewhere; here the frames stop looking like images.  frame_fits_32bit_offsets admits any H W < 2^24 and
validate_forward any N H W <= 2^31: between the largest frame of the other modules (3840 wide, 4097 tall, 72 frames, no tensor of 2^31
bytes) and those bounds lie the dividing branch of xcd_block (65536 and more strips), per-frame bases above 2^31 and 2^32 bytes, grids
with more than 65535 blocks in y and z, and runs cut from two million row steps.  tests/geometry.py builds each frame periodic
(P = 61) on the device and predicts EVERY output byte from a small C-oracle run; only mismatch counts and the first mismatching
(n, c, y, x) come back.  Every case asserts its plan by name (launch_plan, layer_engines against tests/planner.py, plus what the plan
must contain), so that a case cannot silently move to another kernel.

  1. wide    W = 4 194 240 / 4 194 241 (65535 / 65536 strips of 64: the last multiply-high grid, the first dividing one) and
             W = 3 932 100 / 3 932 101 (the same step of the trio's 60-column strips), H = 1 and 3; and W = 12 800 000 / 12 000 000,
             H = 1: 200 000 strips of 64 / of 60, grids on which only the division is right (at 65536 strips the multiply-high is
             exact, its factor is 2^16; test_the_division_branch_is_needed_where_case_1_says restates xcd_block and shows both)
  2. tall    W x H = 1 x (2^24 - 1), 4 x 4 194 303, 31 x 524 288 and 31 x 524 289 (65536 / 65537 eight-row blocks in gridDim.y of dot4
             and of the calibration conv, which is compared with oracle/calib_oracle.py through the same gather); on dot4 alone one
             row and one column of 2^24 + 5 pixels (it has no per-frame bound; the MFMA plans refuse the frame)
  3. bases   batches of 256 x 260 frames whose tensors cross 2^32 bytes (table below)
  4. many    N = 65535, 65536, 65537 frames of 3 x 5 and 1 x 1: gridDim.z
  5. refusals through the C ABI with pointers that are never dereferenced: sesrq_forward past 2^31 pixels; the raw and the sensor
     unpack at the first item count segment_items refuses.  One item below it nothing but the launch follows the check, so the
     accepting half runs on real buffers: a one-pixel-wide raw frame of 2 146 959 359 rows (at 256 CUs), every q0 byte compared
  6. the side libraries at the same extremes, each against its numpy restatement (tests/sensor_oracle.py, image_oracle.py,
     quality_oracle.py, mosaic_oracle.py): raw / sensor unpack (uint16, RAW10, RAW12), image decode (RGB, Y) and export (fp32, int8)
     on one row of 2^24 - 2 pixels, on 2^24 - 2 rows of two, and on batches whose outputs cross 2^32 bytes; PSNR / SSIM and the mosaic
     form on 7 x 600 000 and 600 000 x 7 (the full length: the restatements take 0.4 .. 2.1 s there).  RAW10 packs four pixels: its
     row is 2^24 - 4 wide and its column frame four

Plans: default (merged first-layer kernel, fused trio, last-layer kernel), per-layer (fuse_hidden = 0: the merged hidden kernel), dot4,
and ENGINE_MFMA_Q on a 4-bit net (its trio and its per-layer kernels).  Nets: synth_net sesr_x2, nrdm, sesr_x4, plain draws, and the
hard sesr_x4 draw (per-PE / general kernels, odd zero points: layer 0 writes a separate residual operand RC; it has no trio, so its
default plan IS its per-layer plan and runs once).  The last layer of the 8-bit plain draws is one the saturation verdict sends to its
per-PE form (mfma-h5-general, nrdm: mfma-h5p-general); "mlast" is the plain draw with the last layer's weights at three quarters, which
the verdict leaves merged (mfma-h5-merged).  The names are asserted as tests/planner.py derives them.

Case 3: which tensor class crosses 2^32 bytes in which test, and which kernels address it there, by the role the asserted kernel names
give (first layer: reads the input, writes S and RC; hidden layers: read / write S, A, B, the merging one reads RC; last layer: reads
A / B and the anchor, writes out_q / out_f).  S / A / B / RC: the workspace tensors, N H W > 2^28; out_q and out_f of sesr_x4 at 16 and
64 B/px; in32: the fp32 3-channel planes of nrdm, N H W > 2^30 / 3; N = frames of 256 x 260.  test_case_tables_are_well_formed derives
the roles from the names and requires, per class, every role that addresses it (ROLES_OF): no empty cell.

  test id             net            N     first    hidden   last     crossed
  ws-default          sesr_x4        4034  merged   trio     per-PE   S A B out_q
  ws-per-layer        sesr_x4        4034  merged   merged   per-PE   S A B out_q
  ws-hard             sesr_x4 hard   4034  per-PE   per-PE   per-PE   S A B RC out_q
  ws-dot4             sesr_x4        4034  dot4     dot4     dot4     S A B out_q
  rc-default          sesr_x4 z1     4034  merged   trio     per-PE   S A B RC out_q
  rc-per-layer        sesr_x4 z1     4034  merged   merged   per-PE   S A B RC out_q
  rc-dot4             sesr_x4 z1     4034  dot4     dot4     dot4     S A B RC out_q
  ws-mlast-default    sesr_x4 mlast  4034  merged   trio     merged   S A B out_q
  ws-mlast-per-layer  sesr_x4 mlast  4034  merged   merged   merged   S A B out_q
  outf-<plan>         sesr_x4        1009  as the ws- row of the plan         out_f
  outf-mlast          sesr_x4 mlast  1009  merged   trio     merged   out_f
  in32-default        nrdm           5378  merged   trio     per-PE   in32 S A B
  in32-per-layer      nrdm           5378  merged   merged   per-PE   in32 S A B
  in32-hard           nrdm hard      5378  per-PE   per-PE   per-PE   in32 S A B RC
  in32-dot4           nrdm           5378  dot4     dot4     dot4     in32 S A B
  anchor-<plan>       sesr_x2        2689  as above (hard: per-PE)            anchor past 2^31 only
  anchor-mlast        sesr_x2 mlast  2689  merged   trio     merged   anchor past 2^31 only

The anchor of the x2 anchored engine is the fp32 input frame (12 B/px) and needs the fp32 output (48 B/px) and the workspace
(48 B/px): crossing 2^32 bytes with it takes 108 B/px x 2^30 / 3 px = 38.7 GB, more than the 32 GiB a test may hold.  It crosses 2^31
bytes here (N H W > 2^29 / 3).  What that guards is small: the anchor's base is an expression of its own, an ELEMENT index into a
float pointer ((size_t)n_img * cout * H * W in the MFMA last layer, ((size_t)n * cout + c) * HW in dot4), 5.4e8 at these sizes and
below 2^31, so a dropped (size_t) there would still pass the anchor- rows; they pin the byte offset past 2^31 and the bytes, not that
cast.

Found: on the MFMA kernels and the trio a frame of more than 2^20 rows (then at most 15 pixels wide) came out wrong from row 2^20 on --
131 759 553 of 201 326 580 bytes on the one-pixel-wide frame of 16 777 215 rows, first at output (0, 0, 2097149, 1), -64 for -65; dot4
was right.  The three input stages marked a staged pixel whose column lies outside the frame with tile row -(2^20) so that their row
test lo <= ty < hi would pad it; with the tile at row 2^20 + halo or below, lo reaches -(2^20), the marker passes, and the pixel is
staged as the 0 of its out-of-range load instead of the pad byte.  The marker is now below every lo (NO_ROW, csrc/sesrq_common.h);
test_tall_frames on 16777215x1 and 4194303x4 are the regression cases.  Nothing else mismatched: 65535 / 65536 / 200 000 strips,
65536 / 65537 / 2 097 152 blocks in gridDim.y, 65536 / 65537 frames in gridDim.z (the runtime launches them; no refusal was needed) and
every base past 2^32 bytes.  Edited scratch copy of the library, frame base of make_rowio formed in 32 bits (unsigned, so offsets only
shrink), the whole module of 191 tests: the ten MFMA rows of case 3 that cross 2^32 with a workspace tensor failed (ws-default,
ws-per-layer, ws-hard, rc-default, rc-per-layer, in32-default, in32-per-layer, in32-hard, ws-mlast-default, ws-mlast-per-layer), the
other 181 passed.

What ties the restated split to the library: tests/planner.py's split_divides and xcd_split agree with cut_runs' inv_nx expression by
reading, and the bytes of the 200 000-strip cases show that the library divides THERE.  A threshold moved anywhere between 65537 and
200 000 strips would still pass: the grids in between on which the multiply-high is wrong are not run.

The sensor unpack's accepting half (one item below its limit) is not run: the raw library's shares its host check (segment_items) and
its device body (sesrq_bayer_unpack.h), and that one is.
"""
import copy
import ctypes as C
import functools
import time

import numpy as np
import pytest

from helpers import bundle_from_oracle, device, stream_ptr
from oracle import c_oracle as CO
from oracle import sesrq_oracle as O
from planner import SPLIT_LIMIT, expected_plan_and_engines, run_count, split_divides, strip_count, widths_around, xcd_split
from topologies import topo_net
import geometry as G
import sesrq
from sesrq import _lib

GIB = 1 << 30
KINDS = {"sesr_x4": (1, 16, 4), "sesr_x2": (3, 12, 2), "nrdm": (3, 3, 1)}


# The seed of each draw: chosen on the CPU, on the oracle alone, so that one-row and one-column frames are live too (most draws leave
# -128 on two thirds of a 1 x W frame; test_case_tables_are_well_formed holds every case to the rule)
SEEDS = {("sesr_x4", False, 8): 1, ("sesr_x4", True, 8): 0, ("sesr_x4", False, 4): 2, ("sesr_x2", False, 8): 2, ("sesr_x2", True, 8): 0,
         ("nrdm", False, 8): 3, ("nrdm", True, 8): 0}


@functools.lru_cache(maxsize=None)
def geo_net(kind, hard=False, qbits=8, z1=None):
    """The nets of this module: synth_net's draws at SEEDS.  z1 == "mlast": the plain draw with a last layer that stays merged (below).
    Any other z1: a plain, saturation-free draw whose layer 0 requantises into zero point z1 != -128, so that the merged kernels and
    the trio run with a separate residual operand."""
    if z1 is None:
        return O.synth_net(kind, SEEDS[kind, hard, qbits], hard=hard, quan_bits=qbits)
    if z1 == "mlast":
        # the plain draw with the last layer's weights at three quarters: its PE and adder sums then provably fit 18 / 20 bits, the
        # saturation verdict leaves the layer merged (mfma-h5-merged / mfma-h5p-merged); every other layer is the plain draw's
        net = copy.deepcopy(O.synth_net(kind, SEEDS[kind, hard, qbits], hard=hard, quan_bits=qbits))
        net.layers[-1].wq = np.rint(net.layers[-1].wq.astype(np.float64) * 0.75).astype(np.int8)
        net.name += "_mlast"
        return net
    cin, cout, ps = KINDS[kind]
    net = topo_net((16,) * 4, (5, 3, 3, 3, 5), cin, cout, ps, 1, zeros=[-128, z1, -128, -128, -128, -128])
    net.name = f"{kind}_z1_{z1}"
    return net


NETS8 = [("sesr_x2", False, 8, None), ("nrdm", False, 8, None), ("sesr_x4", False, 8, None), ("sesr_x4", True, 8, None)]
NET_Q4 = ("sesr_x4", False, 4, None)
PLANS = {"default": dict(), "per-layer": dict(fuse_hidden=0), "dot4": dict(engine=_lib.ENGINE_DOT4),
         "mfma-q": dict(engine=_lib.ENGINE_MFMA_Q), "mfma-q-per-layer": dict(engine=_lib.ENGINE_MFMA_Q, fuse_hidden=0)}
# the hard draw has no trio: its default and per-layer plans are the same kernels, one of them runs
NET_PLANS = [(k, p) for k in NETS8 for p in ("default", "per-layer", "dot4") if not (k[1] and p == "per-layer")] + \
            [(NET_Q4, "mfma-q"), (NET_Q4, "mfma-q-per-layer")]

W_MFMA = widths_around(SPLIT_LIMIT - 1, "mfma")          # 65535 | 65536 strips of 64 columns
W_TRIO = widths_around(SPLIT_LIMIT - 1, "trio")          # 65535 | 65536 strips of 60 columns
WIDE = [(1, h, w) for w in W_MFMA + W_TRIO for h in (1, 3)]
# 200 000 strips of 64 / of 60 columns, one row: grids on which a multiply-high split WOULD be wrong (ceil(2^32 / 200000) = 21475 sends
# v = 199 999 to run 1, strip -1), so that a threshold in cut_runs that multiplies too far shows; at 65536 strips it is exact (2^16)
W_DIVIDE = {"mfma": 200000 * 64, "trio": 200000 * 60}
WIDE_DIVIDE = [(1, 1, W_DIVIDE["mfma"]), (1, 1, W_DIVIDE["trio"])]
DOT4_BIG = [(1, 1, (1 << 24) + 5), (1, (1 << 24) + 5, 1)]          # H W >= 2^24: the dot4 engine alone
TALL = [(1, (1 << 24) - 1, 1), (1, 4194303, 4), (1, 524288, 31), (1, 524289, 31)]
BH, BW = 256, 260
MANY = [(n, h, w) for n in (65535, 65536, 65537) for h, w in ((3, 5), (1, 1))]
F_MANY, F_BASES = 61, 3


def _tag(key):
    kind, hard, qbits, z1 = key
    return kind + ("-hard" if hard else "") + (f"-q{qbits}" if qbits != 8 else "") + ("-mlast" if z1 == "mlast" else f"-z{-z1}" if z1 is not None else "")


def _ids(keys_plans):
    return [f"{_tag(k)}-{p}" for k, p in keys_plans]


def _cin(key):
    return KINDS[key[0]][0]


def _small(key, F, shape):
    N, H, W = shape
    return G.small_run(geo_net, key, _cin(key), F, 1000 + F, H, W)


def _plan_must_hold(key, plan, names):
    """What the plan tag promises, by kernel name."""
    kind, hard, qbits, z1 = key
    sfx = f"-q{qbits}" if qbits != 8 else ""
    if plan == "dot4":
        assert all(n.startswith("dot4-") for n in names) and (hard or all(n == "dot4-merged" + sfx for n in names[:4])), names
    elif hard:
        assert not any("trio" in n for n in names) and not any(n.endswith("-merged") for n in names), names
        assert all(n.startswith("mfma-") and n.rsplit("-", 1)[1] in ("general", "hybrid", "unbiased") for n in names), names
    else:
        hidden = "mfma-trio-merged" if plan in ("default", "mfma-q") else "mfma-h3-merged"
        assert names[0] == "mfma-f5-merged" + sfx and names[1:4] == [hidden + sfx] * 3, names
        assert names[4].startswith("mfma-h5p-" if kind == "nrdm" else "mfma-h5-"), names
        if z1 == "mlast" or qbits != 8:
            assert names[4].endswith("-merged" + sfx), names


# ================================================================================================================== CPU part
CPU_SHAPES = [("wide", (1, 3, 6 * G.P + 13)), ("tall", (1, 5 * G.P + 20, 3)), ("batch", (7, 4 * G.P + 12, 4 * G.P + 16))]


@pytest.mark.parametrize("kind", ["sesr_x2", "nrdm", "sesr_x4"])
@pytest.mark.parametrize("what,shape", CPU_SHAPES, ids=[w for w, _ in CPU_SHAPES])
def test_gather_map_equals_a_direct_oracle_run(kind, what, shape):
    """The periodic frame's output, computed directly by the C oracle, IS the small run's output gathered through the map -- int8 and
    fp32 words, wide, tall and a batch of 7 frames from 3 base frames, each with more than 100 distinct output bytes."""
    key = (kind, False, 8, None)
    net = geo_net(*key)
    N, H, W = shape
    F = 3 if N > 1 else 1
    s = _small(key, F, shape)
    assert s["x"].shape == (F, _cin(key), G.small_len(H), G.small_len(W)) and (G.small_len(H) < H or G.small_len(W) < W)
    direct = CO.forward(net, G.tile_frame(s["pattern"], N, H, W))
    r = net.pixel_shuffle
    np.testing.assert_array_equal(G.gathered(s["q_out"], N, H, W, r), direct["q_out"])
    np.testing.assert_array_equal(G.gathered(s["y"], N, H, W, r).view(np.uint32), direct["y"].view(np.uint32))
    assert len(np.unique(direct["q_out"])) > 100
    vals, counts = np.unique(direct["q_out"], return_counts=True)
    n, top = G.liveness(s["q_out"], N, H, W, r)
    assert n == len(vals) and abs(top - counts.max() / direct["q_out"].size) < 1e-12


def test_gather_map_properties():
    """m is the identity on short axes; on long ones it keeps the phase, the 7 border pixels of each side, and sends the interior at
    least 7 pixels away from both borders of the small axis."""
    for D in (1, 7, 4 * G.P, 4 * G.P + 1, 1000, (1 << 24) - 1, W_MFMA[1]):
        m, Ds = G.gather_map(D), G.small_len(D)
        assert m.shape == (D,) and m.min() >= 0 and m.max() < Ds
        if D <= 4 * G.P:
            assert Ds == D and np.array_equal(m, np.arange(D))
            continue
        assert Ds == 3 * G.P + D % G.P and np.array_equal(m % G.P, np.arange(D) % G.P)
        assert np.array_equal(m[:G.R], np.arange(G.R)) and np.array_equal(Ds - m[D - G.R:], D - np.arange(D - G.R, D))
        mid = m[G.R:D - G.R]
        assert mid.min() >= G.P >= 2 * G.R and mid.max() < 2 * G.P <= Ds - 2 * G.R
    assert np.array_equal(G.out_map(200, 1), G.gather_map(200))
    assert np.array_equal(G.out_map(300, 2)[:6], [0, 1, 2, 3, 4, 5]) and G.out_map(300, 4)[-1] == 4 * G.small_len(300) - 1


def test_planner_strip_counts_at_the_split_limit():
    """The widths of case 1 from the planner restatement: 65535 strips multiply, 65536 divide, for the 64-column kernels and for the
    trio's 60-column strips; the tall frames' run counts keep strips x runs on the multiplying side."""
    assert W_MFMA == (4194240, 4194241) and W_TRIO == (3932100, 3932101)
    for fam, (a, b) in (("mfma", W_MFMA), ("trio", W_TRIO)):
        assert strip_count(a, fam) == SPLIT_LIMIT - 1 and strip_count(b, fam) == SPLIT_LIMIT
        for slots in (256, 512, 1024, 2048):       # any chip: one run per strip at these widths
            assert run_count(SPLIT_LIMIT - 1, 1, 1, slots) == 1
            assert not split_divides(strip_count(a, fam), 1) and split_divides(strip_count(b, fam), 1)
    assert strip_count(W_MFMA[0], "trio") > SPLIT_LIMIT and strip_count(W_TRIO[1], "mfma") < SPLIT_LIMIT - 1
    for _, H, W in WIDE + TALL:
        assert H * W < 1 << 24                     # what the MFMA plans accept
    for _, H, W in TALL:
        for slots in (256, 512, 1024, 2048):
            assert not split_divides(strip_count(W, "mfma"), run_count(strip_count(W, "mfma"), -(-H // 8), 1, slots))
    assert [-(-H // 8) for _, H, W in TALL[2:]] == [65536, 65537] and -(-TALL[0][1] // 8) == 2097152


def test_the_division_branch_is_needed_where_case_1_says():
    """xcd_block restated on whole grids (planner.xcd_split): the dividing split hands every (strip, run) to exactly one block on every
    grid of case 1; the multiply-high split does so up to 65536 strips (exact there: the factor is 2^16) and on the 69905 / 213334
    strips the other family has at those widths (the wrong v lie among the total % 8 blocks that keep their place), and does NOT on
    200 000 strips: one block lands on strip -1 of run 1.  W_DIVIDE are the widths with that count, in both families."""
    for fam in ("mfma", "trio"):
        assert strip_count(W_DIVIDE[fam], fam) == 200000 and split_divides(200000, 1) and W_DIVIDE[fam] < 1 << 24
    grids = sorted({strip_count(w, fam) for _, _, w in WIDE + WIDE_DIVIDE for fam in ("mfma", "trio")})
    assert {SPLIT_LIMIT - 1, SPLIT_LIMIT, 69905, 200000}.issubset(grids)
    for nx in grids:
        for multiply in (False, True):
            bx, by = xcd_split(nx, 1, multiply)
            whole = bool((by == 0).all()) and np.array_equal(np.sort(bx), np.arange(nx))
            assert whole == (not multiply or nx != 200000), (nx, multiply)
    bx, by = xcd_split(200000, 1, True)
    assert int(bx.min()) == -1 and int(by.max()) == 1 and int((by != 0).sum()) == 1
    for nx, ny in ((1, 2048), (1, 1024), (8, 64)):          # tall frames: strips x runs stays far below 2^16, both forms agree
        for multiply in (False, True):
            bx, by = xcd_split(nx, ny, multiply)
            assert np.array_equal(np.sort(by * nx + bx), np.arange(nx * ny))


def _bases_cases():
    """(id, net key, plan, N, input dtype, want_q, want_f, anchor, tensors that cross 2^32 bytes)."""
    x4, x4h, x4z = ("sesr_x4", False, 8, None), ("sesr_x4", True, 8, None), ("sesr_x4", False, 8, -120)
    nr, nrh = ("nrdm", False, 8, None), ("nrdm", True, 8, None)
    x2, x2h = ("sesr_x2", False, 8, None), ("sesr_x2", True, 8, None)
    x4m, x2m = ("sesr_x4", False, 8, "mlast"), ("sesr_x2", False, 8, "mlast")
    cases = [("ws-default", x4, "default", 4034, "f32", True, False, False, "S A B out_q"),
             ("ws-per-layer", x4, "per-layer", 4034, "i8", True, False, False, "S A B out_q"),
             ("ws-hard", x4h, "default", 4034, "f32", True, False, False, "S A B RC out_q"),
             ("ws-dot4", x4, "dot4", 4034, "f32", True, False, False, "S A B out_q"),
             ("rc-default", x4z, "default", 4034, "f32", True, False, False, "S A B RC out_q"),
             ("rc-per-layer", x4z, "per-layer", 4034, "f32", True, False, False, "S A B RC out_q"),
             ("rc-dot4", x4z, "dot4", 4034, "i8", True, False, False, "S A B RC out_q")]
    cases += [(f"outf-{p}", k, pl, 1009, "f32", True, True, False, "out_f")
              for p, k, pl in (("default", x4, "default"), ("per-layer", x4, "per-layer"), ("hard", x4h, "default"), ("dot4", x4, "dot4"))]
    cases += [("in32-default", nr, "default", 5378, "f32", True, False, False, "in32 S A B"),
              ("in32-per-layer", nr, "per-layer", 5378, "f32", True, False, False, "in32 S A B"),
              ("in32-hard", nrh, "default", 5378, "f32", True, False, False, "in32 S A B RC"),
              ("in32-dot4", nr, "dot4", 5378, "f32", True, False, False, "in32 S A B")]
    cases += [(f"anchor-{p}", k, pl, 2689, "f32", False, True, True, "anchor past 2^31")
              for p, k, pl in (("default", x2, "default"), ("per-layer", x2, "per-layer"), ("hard", x2h, "default"), ("dot4", x2, "dot4"))]
    # the merged last-layer kernel: its stage reads A / B, its store writes out_q / out_f, its epilogue reads the anchor
    cases += [("ws-mlast-default", x4m, "default", 4034, "f32", True, False, False, "S A B out_q"),
              ("ws-mlast-per-layer", x4m, "per-layer", 4034, "i8", True, False, False, "S A B out_q"),
              ("outf-mlast", x4m, "default", 1009, "f32", True, True, False, "out_f"),
              ("anchor-mlast", x2m, "default", 2689, "f32", False, True, True, "anchor past 2^31")]
    return cases


BASES = _bases_cases()

# Which kernel addresses which tensor class, by role: the first layer reads the input and writes S (and RC); the hidden layers read and
# write S / A / B and the residual-merging one reads RC; the last layer reads A / B and the anchor and writes out_q / out_f.
ROLES_OF = {"S": ("first-merged", "first-per-PE", "hidden-merged", "trio", "hidden-per-PE", "dot4"),
            "A": ("hidden-merged", "trio", "hidden-per-PE", "last-merged", "last-per-PE", "dot4"),
            "B": ("hidden-merged", "trio", "hidden-per-PE", "last-merged", "last-per-PE", "dot4"),
            "RC": ("first-merged", "first-per-PE", "hidden-merged", "trio", "hidden-per-PE", "dot4"),
            "out_q": ("last-merged", "last-per-PE", "dot4"), "out_f": ("last-merged", "last-per-PE", "dot4"),
            "in32": ("first-merged", "first-per-PE", "dot4"), "anchor": ("last-merged", "last-per-PE", "dot4")}


def _roles(names):
    """The roles a plan's kernels play, from the names layer_engines() gives (and the GPU part asserts)."""
    def mode(n):
        return "merged" if n.endswith("-merged") else "per-PE"
    out = set()
    for pos, ns in (("first", names[:1]), ("hidden", names[1:-1]), ("last", names[-1:])):
        for n in ns:
            out.add("dot4" if n.startswith("dot4-") else "trio" if "trio" in n else f"{pos}-{mode(n)}")
    return out


def _bases_bytes(key, N, dt, want_q, want_f):
    """(bytes per tensor class, device bytes the test holds): input, workspace slots, outputs, and the compare's slice (expected
    slice, mismatch mask, the base frames) of at most 3 GiB."""
    kind, hard, qbits, z1 = key
    cin, cout, r = KINDS[kind]
    net = geo_net(*key)
    px = N * BH * BW
    slot = -(-px * 16 // 256) * 256
    sizes = dict(input=px * cin * (4 if dt == "f32" else 1), slot=slot, slots=4 if net.zero[1] != -128 else 3,
                 out_q=px * cout if want_q else 0, out_f=px * cout * 4 if want_f else 0)
    return sizes, sizes["input"] + sizes["slot"] * sizes["slots"] + sizes["out_q"] + sizes["out_f"] + 3 * GIB


def test_case_tables_are_well_formed():
    """Every case of the GPU part: the oracle is live on it (at least 32 distinct output bytes, none on more than 60 % of the pixels),
    its plan holds what its tag promises, case 3 crosses what its row says and stays below 32 GiB, and the coverage table of the
    docstring has no empty column."""
    for key, plan in NET_PLANS:
        net = geo_net(*key)
        _, names = expected_plan_and_engines(net, **PLANS[plan])
        _plan_must_hold(key, plan, names)
    for key in NETS8 + [NET_Q4]:
        net = geo_net(*key)
        for shape in WIDE + WIDE_DIVIDE + TALL + (DOT4_BIG if key == NETS8[2] else []):
            s = _small(key, 1, shape)
            n, top = G.liveness(s["q_out"], *shape, net.pixel_shuffle)
            # a width b < 8 has 2^b codes: more than half of them, as test_topologies.py asks of its narrow cases
            assert n >= (32 if net.quan_bits == 8 else (1 << net.quan_bits) // 2 + 1) and top <= 0.6, (key, shape, n, top)
    for key in (NETS8[0], NETS8[2]):
        for shape in MANY:
            n, top = G.liveness(_small(key, F_MANY, shape)["q_out"], *shape, geo_net(*key).pixel_shuffle)
            assert n >= 32 and top <= 0.6, (key, shape, n, top)
    seen = {}
    for cid, key, plan, N, dt, want_q, want_f, anchor, crossed in BASES:
        net = geo_net(*key)
        _, names = expected_plan_and_engines(net, **PLANS[plan])
        _plan_must_hold(key, plan, names)
        n, top = G.liveness(_small(key, F_BASES, (N, BH, BW))["q_out"], N, BH, BW, net.pixel_shuffle)
        assert n >= 32 and top <= 0.6, (cid, n, top)
        sizes, total = _bases_bytes(key, N, dt, want_q, want_f)
        assert total <= 32 * GIB, (cid, total / GIB)
        roles = _roles(names)
        for t in ([] if anchor else crossed.split()):
            if t in ("S", "A", "B"):
                assert sizes["slot"] > 1 << 32, cid
            elif t == "RC":
                assert sizes["slot"] > 1 << 32 and sizes["slots"] == 4, cid
            elif t in ("out_q", "out_f"):
                assert sizes[t] > 1 << 32, cid
            elif t == "in32":
                assert dt == "f32" and sizes["input"] > 1 << 32, cid
            seen.setdefault(t, set()).update(roles & set(ROLES_OF[t]))
        if anchor:
            assert 1 << 31 < sizes["input"] < 1 << 32 and dt == "f32" and want_f, cid
            seen.setdefault("anchor", set()).update(roles & set(ROLES_OF["anchor"]))
    for t, want in ROLES_OF.items():          # no empty cell: every kernel role that addresses a class has a row that crosses it
        assert seen[t] == set(want), (t, set(want) - seen[t])


# ================================================================================================================== GPU part
def _engine(key, plan, **more):
    """An engine and the proof that it runs the kernels the case names."""
    net = geo_net(*key)
    kw = dict(PLANS[plan], **more)
    e = sesrq.Engine(bundle_from_oracle(net), device(), **kw)
    want_plan, names = expected_plan_and_engines(net, fast_division=e.fast_division_proven(), **kw)
    assert e.launch_plan() == want_plan, (net.name, plan, e.launch_plan(), want_plan)
    assert e.layer_engines() == names, (net.name, plan, e.layer_engines(), names)
    _plan_must_hold(key, plan, names)
    return e, net


def _release(e):
    import torch
    e._ws.clear()
    e.close()
    torch.cuda.empty_cache()


def _report(what, **kw):
    print("GEOM| " + what + " | " + " | ".join(f"{k}={v}" for k, v in kw.items()), flush=True)


def _assert_same(what, got, expect):
    bad, first = G.compare_all(got, expect)
    assert bad == 0, f"{what}: {bad} of {got.numel()} differ, first at (n, c, y, x) = {first[0]}: got {first[1]} want {first[2]}"


def _run_shape(e, net, key, F, shape, what):
    """One shape on one engine: fp32 frame -> int8 and fp32 outputs, int8 q0 frame -> int8 output alone; every element compared."""
    import torch
    N, H, W = shape
    s = _small(key, F, shape)
    r = net.pixel_shuffle
    n, top = G.liveness(s["q_out"], N, H, W, r)
    assert top <= 0.6 and n >= (32 if net.quan_bits == 8 else (1 << net.quan_bits) // 2 + 1), (what, n, top)
    eq, ef = G.Expect(s["q_out"], H, W, r, device()), G.Expect(s["y"], H, W, r, device())
    x = G.device_frame(s["pattern"], N, H, W, device())
    q, y = e.forward(x)
    torch.cuda.synchronize()
    assert tuple(q.shape) == tuple(y.shape) == e.out_shape(N, H, W)
    _assert_same(f"{what} {shape} q_out", q, eq)
    _assert_same(f"{what} {shape} y", y, ef)
    del x, q, y, ef
    if net.quan_bits == 8:          # a narrow net's int8 frame is in its own width's domain: the fp32 route covers it
        x8 = G.device_frame(s["q0_pattern"], N, H, W, device())
        q, y = e.forward(x8, want_f=False)
        torch.cuda.synchronize()
        assert y is None
        _assert_same(f"{what} {shape} q_out (int8 q0 in, int8 out alone)", q, eq)
        del x8, q
    e._ws.clear()
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("w", W_MFMA + W_TRIO)
@pytest.mark.parametrize("key,plan", NET_PLANS, ids=_ids(NET_PLANS))
def test_wide_frames_at_the_strip_count_limit(key, plan, w):
    """1.  65535 and 65536 strips: the last grid xcd_block splits with a multiply-high and the first it divides, for the 64-column
    kernels and for the trio's 60-column strips; H = 1 and 3."""
    t0 = time.time()
    e, net = _engine(key, plan)
    for h in (1, 3):
        _run_shape(e, net, key, 1, (1, h, w), f"{net.name} [{plan}]")
    _release(e)
    _report("wide", net=_tag(key), plan=plan, shape=f"1x{{1,3}}x{w}", strips64=strip_count(w, "mfma"), strips60=strip_count(w, "trio"),
            seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("key,plan", NET_PLANS, ids=_ids(NET_PLANS))
def test_wide_frames_where_only_the_division_is_right(key, plan):
    """1b.  One row of 12 800 000 and of 12 000 000 pixels: 200 000 strips of 64 and of 60 columns, the grids on which a multiply-high
    split sends a block to strip -1 (test_the_division_branch_is_needed_where_case_1_says): the library divides there and gives the
    oracle's bytes."""
    t0 = time.time()
    e, net = _engine(key, plan)
    for shape in WIDE_DIVIDE:
        _run_shape(e, net, key, 1, shape, f"{net.name} [{plan}]")
    _release(e)
    _report("wide-divide", net=_tag(key), plan=plan, shape="1x1x{12800000,12000000}", strips64="200000|187500", strips60="213334|200000",
            seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DOT4_BIG, ids=[f"{h}x{w}" for _, h, w in DOT4_BIG])
def test_dot4_frames_past_2_24_pixels(shape):
    """The dot4 engine has no per-frame bound (include/sesrq.h): one row and one column of 2^24 + 5 pixels give the oracle's bytes; the
    MFMA plans refuse the frame with their message."""
    import torch
    t0 = time.time()
    key = NETS8[2]
    e, net = _engine(key, "dot4")
    _run_shape(e, net, key, 1, shape, f"{net.name} [dot4]")
    _release(e)
    e, net = _engine(key, "default")
    x = G.device_frame(_small(key, 1, shape)["pattern"], *shape, device())
    with pytest.raises(RuntimeError, match="too large for 32-bit buffer offsets"):
        e.forward(x, want_f=False)
    torch.cuda.synchronize()
    del x
    _release(e)
    _report("dot4-big", net=_tag(key), plan="dot4", shape="x".join(map(str, shape)), seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TALL, ids=[f"{h}x{w}" for _, h, w in TALL])
@pytest.mark.parametrize("key,plan", NET_PLANS, ids=_ids(NET_PLANS))
def test_tall_frames(key, plan, shape):
    """2.  Runs cut from up to 2 097 152 eight-row steps, and 65536 / 65537 blocks in gridDim.y of the dot4 kernels."""
    t0 = time.time()
    e, net = _engine(key, plan)
    _run_shape(e, net, key, 1, shape, f"{net.name} [{plan}]")
    _release(e)
    _report("tall", net=_tag(key), plan=plan, shape="x".join(map(str, shape)), steps=-(-shape[1] // 8), seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid,key,plan,N,dt,want_q,want_f,anchor,crossed", BASES, ids=[c[0] for c in BASES])
def test_frame_bases_past_4_gib(cid, key, plan, N, dt, want_q, want_f, anchor, crossed):
    """3.  Batches of periodic 256 x 260 frames whose workspace tensors, outputs or input cross 2^32 bytes (table in the module's
    docstring): a frame base formed in 32 bits anywhere shows as wrong bytes from the frame behind the crossing on."""
    import torch
    t0 = time.time()
    sizes, total = _bases_bytes(key, N, dt, want_q, want_f)
    assert total <= 32 * GIB
    torch.cuda.reset_peak_memory_stats(device())
    held = torch.cuda.memory_allocated(device())          # what earlier tests of the process still hold (a failed one keeps its tensors)
    free = torch.cuda.mem_get_info(device())[0]
    if free < total:
        pytest.skip(f"{total / GIB:.1f} GiB needed, {free / GIB:.1f} GiB free")
    e, net = _engine(key, plan, anchor_add=anchor)
    shape = (N, BH, BW)
    s = _small(key, F_BASES, shape)
    r = net.pixel_shuffle
    assert e.workspace(N, BH, BW).numel() == sizes["slot"] * sizes["slots"]
    x = G.device_frame(s["pattern"] if dt == "f32" else s["q0_pattern"], N, BH, BW, device())
    assert x.numel() * x.element_size() == sizes["input"]
    q, y = e.forward(x, want_q=want_q, want_f=want_f)
    torch.cuda.synchronize()
    if want_q:
        assert q.numel() == sizes["out_q"]
        _assert_same(f"{cid} q_out", q, G.Expect(s["q_out"], BH, BW, r, device()))
    if want_f:
        assert y.numel() * 4 == sizes["out_f"]
        want = s["y"]
        if anchor:       # test.py:148-155: the nearest-upsampled fp32 input added once, in fp32
            want = (want + np.repeat(np.repeat(s["x"], r, axis=2), r, axis=3)).astype(np.float32)
        _assert_same(f"{cid} y", y, G.Expect(want, BH, BW, r, device()))
    peak = torch.cuda.max_memory_allocated(device()) - held
    del x, q, y
    _release(e)
    assert peak <= total, f"{cid}: {peak} bytes allocated at the peak, {total} computed"
    _report("bases", id=cid, net=_tag(key), plan=plan, shape=f"{N}x{BH}x{BW}", crossed=crossed, computed_bytes=total,
            seconds=f"{time.time() - t0:.2f}", peak_allocated=peak)


def _forward_abi(e, x, dt, q, N, H, W, ws):
    rc = _lib.lib().sesrq_forward(e._h, x.data_ptr(), dt, q.data_ptr(), None, N, H, W, ws.data_ptr(), ws.numel(), stream_ptr())
    return rc, _lib.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["default", "per-layer", "dot4"])
@pytest.mark.parametrize("key", [NETS8[0], NETS8[2]], ids=[_tag(NETS8[0]), _tag(NETS8[2])])
def test_many_frames(key, plan):
    """4.  65535, 65536 and 65537 frames of 3 x 5 and 1 x 1 ride in gridDim.z: the runtime launches them and every shape gives the oracle's
    bytes (include/sesrq.h states it: N is bounded by N H W <= 2^31 alone).  The output is pre-filled, so a launch that did not happen
    would show."""
    import torch
    t0 = time.time()
    e, net = _engine(key, plan)
    for shape in MANY:
        N, H, W = shape
        s = _small(key, F_MANY, shape)
        x = G.device_frame(s["pattern"], N, H, W, device())
        q = torch.full(e.out_shape(N, H, W), 0x33, dtype=torch.int8, device=device())
        ws = torch.full((_lib.lib().sesrq_workspace_bytes(e._h, N, H, W),), 0x5A, dtype=torch.uint8, device=device())
        rc, msg = _forward_abi(e, x, _lib.F32, q, N, H, W, ws)
        torch.cuda.synchronize()
        assert rc == 0, (shape, msg)
        _assert_same(f"{net.name} [{plan}] {shape} q_out", q, G.Expect(s["q_out"], H, W, net.pixel_shuffle, device()))
        del x, q, ws
    _release(e)
    _report("many", net=_tag(key), plan=plan, shapes="{65535,65536,65537}x{3x5,1x1}", seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
def test_forward_refuses_a_batch_past_2_31_pixels_without_touching_memory():
    """5.  sesrq_forward at N H W = 2^31 + 65536 through the C ABI with non-null, aligned pointers that are never dereferenced: refused
    with its message before anything is enqueued.  (The net is real: the checks read it.)"""
    import torch
    e, net = _engine(NETS8[1], "default")
    fake = C.c_void_p(1 << 20)
    N, H, W = 32769, 256, 256
    assert N * H * W == (1 << 31) + 65536
    lib = _lib.lib()
    need = lib.sesrq_workspace_bytes(e._h, N, H, W)
    rc = lib.sesrq_forward(e._h, fake, _lib.F32, fake, fake, N, H, W, fake, need, stream_ptr())
    assert rc != 0 and _lib.last_error() == "sesrq_forward: frame batch too large (N*H*W > 2^31)", _lib.last_error()
    rc = lib.sesrq_forward(e._h, fake, _lib.F32, fake, fake, 1 << 15, 256, 256, fake, 0, stream_ptr())        # 2^31 itself: not for size
    assert rc != 0 and "workspace too small" in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    _release(e)


@pytest.mark.gpu
def test_raw_and_sensor_unpack_refuse_the_first_item_count_past_the_int_range():
    """5.  segment_items refuses N H ceil(W / seg) > 2^31 - 1 - one grid round (256 threads x 8 blocks x the device's CUs): the raw unpack
    (8 pixels a segment) and the sensor unpack (uint16: 8, RAW10: 16) at the first refused count, with pointers that are never
    dereferenced -- the refusal comes before any launch.  (The contexts are real: the round is read from them.  One item less is
    accepted for size and nothing stands between that check and the launch on one device, so that call needs real buffers of 2^31
    segments: it is not made here.)"""
    import torch
    from sesrq import raw as R
    from sesrq import sensor as S
    cus = torch.cuda.get_device_properties(device()).multi_processor_count
    first = 0x7FFFFFFF - 256 * 8 * cus + 1
    fake = 1 << 20
    h = R._so.context(device(), 1.0 / 255.0, -128, 0)
    for N, H, W in ((1, first, 8), (1, first, 1), (2, (first + 1) // 2, 5)):
        assert N * H * -(-W // 8) >= first
        assert R.lib().sesrq_raw_unpack(h, fake, fake, None, N, H, W, None) != 0
        assert R.last_error() == f"sesrq_raw_unpack: frame of {N} x {H} x {W} is too large", R.last_error()
    for fmt, seg in ((S.Format(cfa="bggr"), 8), (S.Format(packing="raw10", white=1023), 16), (S.Format(packing="raw12"), 16)):
        h = S.context(device(), fmt, 1.0 / 255.0, -128, 0)
        N, H, W = 1, first, seg
        assert S.lib().sesrq_sensor_unpack(h, fake, 4096, fake, None, N, H, W, None) != 0
        assert S.last_error() == f"sesrq_sensor_unpack: frame of {N} x {H} x {W} is too large", (fmt, S.last_error())
    torch.cuda.synchronize()


CALIB_TALL = [(3, 5, 3, 524288), (3, 5, 3, 524289), (5, 16, 16, 524288), (5, 16, 16, 524289)]


@pytest.mark.gpu
@pytest.mark.parametrize("K,ic,oc,H", CALIB_TALL, ids=[f"k{k}-ic{i}-oc{o}-{h}x31" for k, i, o, h in CALIB_TALL])
def test_calib_conv_on_tall_frames(K, ic, oc, H):
    """2.  sesrq_calib_conv launches dim3(ceil(W / 32), ceil(H / 8), N) too: 31 x 524 288 and 31 x 524 289 (65536 / 65537 blocks in
    gridDim.y), ReLU and skip, every fp32 value against oracle/calib_oracle.py through the same gather (a single conv reaches 2
    pixels, inside the 7 the map keeps; the skip is periodic as well).  Compared as values, as tests/test_calib_kernels.py does."""
    import torch
    from calib_cases import F32, bias, frame, weights, zero_domain
    from oracle import calib_oracle as CAL
    t0 = time.time()
    W, b = 31, 8
    rng = np.random.default_rng(4000 + K)
    mn, mx = zero_domain("low", b)
    d0 = CAL.domain(mn, mx, b, 0.0113, np.zeros(oc, F32))
    d = CAL.domain(mn, mx, b, 0.0113, bias(rng, oc, d0.ss))
    pat = frame(rng, (1, ic, G.P, G.P), d, b)
    skp = (rng.standard_normal((1, oc, G.P, G.P)) * 3.0).astype(F32)
    wq = weights(rng, oc, ic, K, b)
    Hs = G.small_len(H)
    want = np.asarray(CAL.conv(G.tile_frame(pat, 1, Hs, W), wq, d, b, True, G.tile_frame(skp, 1, Hs, W))).astype(F32)
    assert want.shape == (1, oc, Hs, W) and len(np.unique(want)) > 100
    x, sk = G.device_frame(pat, 1, H, W, device()), G.device_frame(skp, 1, H, W, device())
    wt = torch.from_numpy(np.ascontiguousarray(wq)).to(device())
    qb = torch.from_numpy(np.ascontiguousarray(d.qbias.astype(F32))).to(device())
    out = torch.full((1, oc, H, W), float("nan"), dtype=torch.float32, device=device())
    desc = _lib.CalibConvDesc(k=K, ic=ic, oc=oc, w=wt.data_ptr(), qbias=qb.data_ptr(), in_scale=float(d.scale32), in_zero=d.zero,
                              ss=float(d.ss), acc_lo=float(d.acc_lo), acc_hi=float(d.acc_hi), add_lo=float(d.add_lo),
                              add_hi=float(d.add_hi), relu=1)
    _lib.check(_lib.lib().sesrq_calib_conv_q(C.byref(desc), x.data_ptr(), sk.data_ptr(), out.data_ptr(), 1, H, W, b, stream_ptr()))
    torch.cuda.synchronize()
    _assert_same(f"calib conv k{K} {H}x{W}", out, G.Expect(want, H, W, 1, device(), words=False))
    del x, sk, out
    torch.cuda.empty_cache()
    _report("calib-tall", conv=f"k{K} {ic}->{oc}", shape=f"1x{H}x{W}", blocks_y=-(-H // 8), seconds=f"{time.time() - t0:.2f}")


# ================================================================================================== 6. the side libraries
# Pointwise operations: the frame is tiled from a (SIDE_PY, SIDE_PX) block (both even: Bayer sites keep their parity; 244 pixels are
# whole RAW10 and RAW12 pack groups), the numpy restatement runs on the block, and every output element is compared with the block's
# output at (y mod SIDE_PY, x mod SIDE_PX).  Frames: one row of 2^24 - 2 pixels (RAW10 packs four pixels: 2^24 - 4), one frame of
# 2^24 - 2 rows two pixels wide (RAW10: four), and a batch of 256 x 260 frames whose fp32 output (12 B/px) crosses 2^32 bytes.
SIDE_PY, SIDE_PX, SIDE_F = 122, 244, 3
SIDE_FRAMES = {"row": (1, 1, (1 << 24) - 2), "column": (1, (1 << 24) - 2, 2), "batch": (5378, BH, BW)}
SIDE_FORMATS = {"raw": None, "u16": dict(cfa="bggr", black=64, white=1023), "raw10": dict(cfa="grbg", black=16, white=1000, packing="raw10"),
                "raw12": dict(cfa="gbrg", black=0, white=4095, packing="raw12")}


def _side_shape(frame, packing):
    N, H, W = SIDE_FRAMES[frame]
    if packing == "raw10" and W % 4:
        W = W - 2 if W > 4 else 4
    return N, H, W


def _side_bundle(kind):
    return bundle_from_oracle(geo_net(kind))


@pytest.mark.gpu
@pytest.mark.parametrize("frame", list(SIDE_FRAMES))
@pytest.mark.parametrize("name", list(SIDE_FORMATS))
def test_raw_and_sensor_unpack_at_the_extremes(name, frame):
    """6.  The Bayer unpack of both raw libraries (the reference's 12-bit RGGB; uint16, RAW10 and RAW12 rows in other CFA orders and
    levels): q0 and the fp32 frame, every element, against tests/sensor_oracle.py."""
    import torch
    import sensor_oracle as SO
    from sesrq import sensor as S
    t0 = time.time()
    kw = SIDE_FORMATS[name]
    fmt = S.Format(**kw) if kw else None
    cfa, black, white, packing = (fmt.cfa, fmt.black, fmt.white, fmt.packing) if fmt else ("rggb", 0, 4095, "u16")
    N, H, W = _side_shape(frame, packing)
    F = SIDE_F if N > 1 else 1
    b = _side_bundle("nrdm")
    top = {"u16": 65535, "raw10": 1023, "raw12": 4095}[packing]
    codes = np.random.default_rng(60 + len(name)).integers(0, min(top, white + 200) + 1, (F, SIDE_PY, SIDE_PX))      # below black, above white too
    table = np.asarray(SO.q_table(black, white, b.scale[0], b.zero[0])).astype(np.int8)
    want_q = SO.spread(codes, table, table[0], cfa, black, white)
    want_f = SO.spread(codes, SO.levels(black, white), np.float32(0), cfa, black, white)
    if packing == "u16":
        raw = G.device_frame(codes.astype(np.uint16).view(np.int16)[:, None], N, H, W, device())[:, 0].view(torch.uint16)
    else:
        S_bytes = fmt.row_bytes(W)
        raw = G.device_frame(SO.pack_rows(codes, packing)[:, None], N, H, S_bytes, device())[:, 0]
    q0, sp = S.unpack(b, raw, fmt, want_q=True, want_spread=True)
    torch.cuda.synchronize()
    assert tuple(q0.shape) == tuple(sp.shape) == (N, 3, H, W)
    _assert_same(f"{name} {frame} q0", q0, G.Expect(want_q, H, W, 1, device(), tiled=True))
    _assert_same(f"{name} {frame} spread", sp, G.Expect(want_f, H, W, 1, device(), tiled=True))
    nbytes = sp.numel() * 4
    assert frame != "batch" or nbytes > 1 << 32
    del raw, q0, sp
    torch.cuda.empty_cache()
    _report("side-unpack", op=name, shape=f"{N}x{H}x{W}", out_bytes=nbytes, seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
def test_raw_unpack_accepts_one_item_below_the_limit():
    """5 / 6.  The accepting half of the size refusal, and the upper half of the item range: one frame of (first refused count - 1)
    rows, one pixel wide -- one segment a row, 2.1e9 items of the int grid-stride loop, q0 planes at byte offsets up to 6.4e9 --
    is not refused and every byte of q0 is the oracle's."""
    import torch
    import sensor_oracle as SO
    from sesrq import raw as R
    t0 = time.time()
    cus = torch.cuda.get_device_properties(device()).multi_processor_count
    H = 0x7FFFFFFF - 256 * 8 * cus
    need = H * 2 + H * 3 + 3 * GIB
    assert need <= 32 * GIB
    if torch.cuda.mem_get_info(device())[0] < need:
        pytest.skip(f"{need / GIB:.1f} GiB needed")
    b = _side_bundle("nrdm")
    codes = np.random.default_rng(77).integers(0, 4300, (1, SIDE_PY, 1))
    table = np.asarray(SO.q_table(0, 4095, b.scale[0], b.zero[0])).astype(np.int8)
    want = SO.spread(codes, table, table[0], "rggb", 0, 4095)
    raw = G.device_frame(codes.astype(np.uint16).view(np.int16)[:, None], 1, H, 1, device())[:, 0].view(torch.uint16)
    q0, _ = R.unpack(b, raw, want_q=True, want_spread=False)
    torch.cuda.synchronize()
    assert tuple(q0.shape) == (1, 3, H, 1) and q0.numel() > 1 << 32
    _assert_same("raw unpack, one item below the limit", q0, G.Expect(want, H, 1, 1, device(), tiled=True))
    del raw, q0
    torch.cuda.empty_cache()
    _report("side-unpack", op="raw, limit - 1", shape=f"1x{H}x1", out_bytes=3 * H, seconds=f"{time.time() - t0:.2f}")


def _image_tile(F, seed):
    return np.random.default_rng(seed).integers(0, 256, (F, SIDE_PY, SIDE_PX, 3)).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", list(SIDE_FRAMES))
@pytest.mark.parametrize("form,order", [("rgb", "rgb"), ("rgb", "bgr"), ("y", "rgb")])
def test_image_decode_at_the_extremes(form, order, frame):
    """6.  8-bit images to q0 and to the fp32 frame, RGB and Y, every element against tests/image_oracle.py."""
    import torch
    import image_oracle as IO
    from sesrq import image as I
    t0 = time.time()
    N, H, W = SIDE_FRAMES[frame]
    F = SIDE_F if N > 1 else 1
    b = _side_bundle("nrdm" if form == "rgb" else "sesr_x4")
    tile = _image_tile(F, 81)
    want_f = IO.decode(tile, form, order)
    want_q = np.asarray(IO.q0(want_f, b.scale[0], b.zero[0])).astype(np.int8)
    img = G.device_frame(np.ascontiguousarray(tile.transpose(0, 3, 1, 2)), N, H, W, device()).permute(0, 2, 3, 1).contiguous()
    q0, x = I.decode(b, img, form, order=order, want_q=True, want_f=True)
    torch.cuda.synchronize()
    C_ = 3 if form == "rgb" else 1
    assert tuple(q0.shape) == tuple(x.shape) == (N, C_, H, W)
    _assert_same(f"decode {form} {order} {frame} q0", q0, G.Expect(want_q, H, W, 1, device(), tiled=True))
    _assert_same(f"decode {form} {order} {frame} x", x, G.Expect(want_f, H, W, 1, device(), tiled=True))
    nbytes = x.numel() * 4
    assert not (frame == "batch" and form == "rgb") or nbytes > 1 << 32
    del img, q0, x
    torch.cuda.empty_cache()
    _report("side-decode", op=f"{form}/{order}", shape=f"{N}x{H}x{W}", out_bytes=nbytes, seconds=f"{time.time() - t0:.2f}")


EXPORTS = [("f32", 3, "rgb", "row"), ("f32", 3, "bgr", "column"), ("f32", 1, "rgb", "row"), ("i8", 3, "rgb", "column"), ("i8", 1, "rgb", "row"),
           ("f32", 3, "rgb", "batch"), ("i8", 3, "bgr", "big-batch")]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,C_,order,frame", EXPORTS, ids=[f"{d}-c{c}-{o}-{f}" for d, c, o, f in EXPORTS])
def test_image_export_at_the_extremes(dtype, C_, order, frame):
    """6.  fp32 and int8 predictions to interleaved 8-bit images, every byte against tests/image_oracle.py.  "batch": the fp32
    prediction crosses 2^32 bytes; "big-batch": 21511 frames of 256 x 260, the int8 prediction and the 8-bit output both do."""
    import torch
    import image_oracle as IO
    from sesrq import image as I
    t0 = time.time()
    N, H, W = (21511, BH, BW) if frame == "big-batch" else SIDE_FRAMES[frame]
    F = SIDE_F if N > 1 else 1
    rng = np.random.default_rng(90 + C_)
    scale, zero = np.float32(0.0047), -118
    if dtype == "f32":
        tile = rng.uniform(-0.1, 1.1, (F, C_, SIDE_PY, SIDE_PX)).astype(np.float32)
        seen, kw = tile, {}
    else:
        tile = rng.integers(-128, 128, (F, C_, SIDE_PY, SIDE_PX)).astype(np.int8)
        seen, kw = IO.dequant(tile, scale, zero), dict(scale=scale, zero=zero)
    want = np.ascontiguousarray(IO.export(seen, order).transpose(0, 3, 1, 2))          # (F, C, PY, PX)
    pred = G.device_frame(tile, N, H, W, device())
    out = I.export(pred, order=order, **kw)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (N, H, W, C_)
    if frame == "big-batch":
        assert out.numel() > 1 << 32 and pred.numel() > 1 << 32
    if frame == "batch":
        assert pred.numel() * 4 > 1 << 32
    _assert_same(f"export {dtype} c{C_} {order} {frame}", out.permute(0, 3, 1, 2), G.Expect(want, H, W, 1, device(), tiled=True))
    nbytes = out.numel()
    del pred, out
    torch.cuda.empty_cache()
    _report("side-export", op=f"{dtype}/c{C_}/{order}", shape=f"{N}x{H}x{W}", out_bytes=nbytes, seconds=f"{time.time() - t0:.2f}")


QUALITY = [(mflag, shape) for shape in ((7, 600000), (600000, 7)) for mflag in (3, 6, 5, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("mflag,shape", QUALITY, ids=[f"mflag{m}-{h}x{w}" for m, (h, w) in QUALITY])
def test_quality_scores_on_strip_frames(mflag, shape):
    """6.  PSNR / SSIM (MFLAG 3 RGB, 6 luma, 5 Y x 255) and the mosaic form (MFLAG 1) on 7 x 600 000 and 600 000 x 7 frames: a one-row
    and a one-column SSIM map of 4.2 M pixels.  The numpy restatements take 0.4 .. 2.1 s on these, so the full length is used.  Bounds
    as tests/test_quality.py holds these kernels to the restatement: PSNR within 1e-5 dB, SSIM within 1e-6."""
    import mosaic_oracle as MO
    import quality_oracle as QO
    from helpers import score
    t0 = time.time()
    H, W = shape
    C_ = 1 if mflag == 5 else 3
    rng = np.random.default_rng(100 + mflag)
    gt = rng.random((1, C_, H, W), dtype=np.float32)
    pred = (gt + rng.normal(0, 0.02, gt.shape)).astype(np.float32)
    pred[0, :, :3, :50] = 1.2                                        # clipped
    want = MO.metrics(pred, gt) if mflag == 1 else QO.metrics(pred, gt, mflag)
    got = score(pred, gt, mflag)
    assert got.shape == (1, 3) and np.isfinite(want).all()
    assert abs(got[0, 1] - want[0, 1]) <= 1e-5 and abs(got[0, 2] - want[0, 2]) <= 1e-6, (mflag, shape, got, want)
    _report("side-quality", op=f"mflag {mflag}", shape=f"1x{C_}x{H}x{W}", psnr=f"{got[0, 1]:.6f}", ssim=f"{got[0, 2]:.8f}",
            seconds=f"{time.time() - t0:.2f}")


def test_tiled_frames_predict_pointwise_operations():
    """CPU: what case 6 rests on.  For the pointwise side operations the restatement of a frame tiled from a (122, 244) block is the
    block's restatement tiled -- Bayer sites, levels and every packing, image decode and export -- at a size that is no multiple of
    the block; and packed rows of the tiled frame are the block's packed rows repeated and cut."""
    import image_oracle as IO
    import sensor_oracle as SO
    H, W = 2 * SIDE_PY + 6, 2 * SIDE_PX + 8
    yy, xx = np.arange(H) % SIDE_PY, np.arange(W) % SIDE_PX
    codes = np.random.default_rng(1).integers(0, 1100, (1, SIDE_PY, SIDE_PX))
    big = codes[:, yy][:, :, xx]
    for cfa in SO.SITE:
        lv = SO.levels(16, 1000)
        assert np.array_equal(SO.spread(big, lv, np.float32(0), cfa, 16, 1000), SO.spread(codes, lv, np.float32(0), cfa, 16, 1000)[:, :, yy][:, :, :, xx])
    for packing, nb in (("u16", 488), ("raw10", 305), ("raw12", 366)):
        small = SO.pack_rows(codes % 1024, packing)
        assert small.shape[2] == nb
        rows = SO.pack_rows(big % 1024, packing)
        assert np.array_equal(rows, small[:, yy][:, :, np.arange(rows.shape[2]) % nb])
    tile = _image_tile(1, 2)
    img = tile[:, yy][:, :, xx]
    for form in ("rgb", "y"):
        assert np.array_equal(IO.decode(img, form, "bgr"), IO.decode(tile, form, "bgr")[:, :, yy][:, :, :, xx])
    pred = np.random.default_rng(3).uniform(-0.1, 1.1, (1, 3, SIDE_PY, SIDE_PX)).astype(np.float32)
    assert np.array_equal(IO.export(pred[:, :, yy][:, :, :, xx], "bgr"), IO.export(pred, "bgr")[:, yy][:, :, xx])
    for frame in SIDE_FRAMES:
        for packing in ("u16", "raw10", "raw12"):
            N, Hh, Ww = _side_shape(frame, packing)
            assert Ww % {"u16": 1, "raw10": 4, "raw12": 2}[packing] == 0 and Ww % 2 == 0
