"""libsesrq_noise.so (include/sesrq_noise.h) past its first tests: both grid-stride loops beyond their first trip, frame geometry at
the limits the library accepts, the corners of the Box-Muller stage, every code at every Bayer phase with noise on, and the noise
levels at the edges of what the header accepts.

Large frames are compared on the device by tests/noise_device.py (pinned to tests/noise_oracle.py by tests/test_noise_device.py): the
device's fp32 deviates against float64 ones at T_Z = 2^-19, the one tolerance (tests/test_noise.py); given the device's deviates, the
fp32 frame and q0 bit for bit.  Frames are tiled from a small block of codes and packed on the device; only counts come back.

  B. loops     for each packing a frame just above one trip of noise_unpack's loop (compute units x 8 x 256 segments, read from the
               device), one just above two trips with a ragged last one (odd H, a partial last segment), and one with W % SEG == 0
               and aligned buffers (wide loads and stores in the later trips); each is many trips of noise_deviates (2048 x 256
               pixels).  All three output sets run on each; the launch counters name them.  A batch of three that wraps as a batch
               equals its three single-frame calls, none of which wraps.
  C. geometry  one row of 16 777 208 / 16 777 213 (u16) and 16 777 212 (raw10) pixels; 16 777 214 rows of two (u16, raw12);
               1 048 577 frames of 2 x 8 with per-frame levels from frame 2^32 - 2^19 (the carry into the high counter word falls
               inside the batch); fp32 outputs across 2^32 bytes (18 920 x 18 920; 3 x 10 924 x 10 928); q0 across 2^32 bytes
               (37 840 x 37 840); raw rows across 2^32 bytes through the stride; one item below the size refusal (shot = read = 0
               against the sensor library's q0); the refusals themselves on pointers that are never dereferenced; the deviates at
               the largest N H W they accept.
  D. corners   the 16 (word, target) corners of tests/golden/noise/corners.json inside 16 frames of 2048 x 2048: all 2.0e8 deviates
               against the float64 ones, exact zeros on the quadrant boundaries, |z| <= Z_MAX.
  E. codes and levels  every code 0 .. 65535 at every Bayer phase under each CFA order (u16 at two level pairs, raw10 and raw12 on
               their ranges), exact_div 0 and 2; the level pairs (0, 1e-40), (1e-45, 0), (FLT_MAX, 0), (0, FLT_MAX), (FLT_MAX, FLT_MAX);
               sigma = inf on a deviate that is exactly zero (the header: the clamp is fminf(fmaxf(y, 0), 1), the frame never holds a
               NaN); a device levels array with one bad pair spoils that frame only.

Every case prints one "NOISE|" line (shape, bytes held, seconds, the deviates' largest error): profiles/noise_limits.txt is made
of them."""
import json
import os
import time

import numpy as np
import pytest

import geometry as G
import noise_device as ND
import noise_oracle as NO
from conftest import GOLDEN
from helpers import Arena, device, same, stream_ptr
from test_noise import CFAS, DOMAINS, SEED, T_Z, _unpack
from test_sensor import every_code_frame

F32 = np.float32
GIB = 1 << 30
ROOM = 3 * GIB                       # what tests/noise_device.py may hold at its peak
FLT_MAX = float(np.finfo(F32).max)
SEG = {"u16": 8, "raw10": 16, "raw12": 16}
TOP = {"u16": 65535, "raw10": 1023, "raw12": 4095}
# (cfa, black, white) of each packing in the geometry cases
FORMATS = {"u16": ("bggr", 64, 1023), "raw10": ("grbg", 16, 1000), "raw12": ("gbrg", 0, 4095)}
OUTS = ("q0", "spread", "q0+spread")
TILE = (3, 62, 244)                  # frames, rows, columns of the block of codes a big frame repeats: even, whole pack groups
CORNERS = os.path.join(GOLDEN, "noise", "corners.json")


def _report(what, **kw):
    print("NOISE| " + what + " | " + " | ".join(f"{k}={v}" for k, v in kw.items()), flush=True)


def _fmt(packing):
    from sesrq import sensor as S
    cfa, black, white = FORMATS[packing]
    return S.Format(cfa=cfa, black=black, white=white, packing=packing)


def _tile(packing, seed=0):
    """The block of codes: below black and above white too, black and white themselves among them."""
    import torch
    _, black, white = FORMATS[packing]
    t = np.random.default_rng(700 + seed + white).integers(0, min(TOP[packing], white + 200) + 1, TILE).astype(np.int32)
    t[:, 0, :2], t[:, 1, :2] = (white, black), (black, white)
    return ND.Tiled(torch.from_numpy(t).to(device()))


def _room(need):
    import torch
    assert need <= 32 * GIB, need / GIB
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(device())[0]
    if free < need:
        pytest.skip(f"{need / GIB:.1f} GiB needed, {free / GIB:.1f} GiB free")


def _free():
    import torch
    torch.cuda.empty_cache()


def _z(nhw, frame0, seed=SEED):
    import torch
    from sesrq import noise
    z = noise.deviates(nhw, seed, frame0, device())
    torch.cuda.synchronize()
    return z


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _differ(a, b, step=1 << 28):
    """How many elements of two equal-shaped device tensors differ as words, in pieces of at most 2^28 elements."""
    import torch
    a, b = _bits(a).reshape(-1), _bits(b).reshape(-1)
    assert a.shape == b.shape
    return sum(int(torch.count_nonzero(a[i:i + step] != b[i:i + step])) for i in range(0, a.numel(), step))


def _names(before):
    from sesrq import noise
    return sorted(n for n, c in noise.instances().items() if c != before[n])


def _case(what, packing, N, H, W, levels, frame0, *, stride=None, outs=("q0+spread",), check_z=True, dom=0, ed=0, tile_seed=0):
    """One frame tiled from the block through sesrq_noise_deviates and sesrq_noise_unpack: every output set of `outs`, each compared
    whole.  -> (report of the first set, bytes held)."""
    import torch
    t0 = time.time()
    fmt, codes = _fmt(packing), _tile(packing, tile_seed)
    s0, z0 = DOMAINS[dom]
    px = N * H * W
    raw = ND.build_raw(codes, N, H, W, packing, stride, 0xEE, device())
    held = raw.numel() + 12 * px + max((3 * px if "q0" in o else 0) + (12 * px if "spread" in o else 0) for o in outs) + ROOM
    z = _z((N, H, W), frame0)
    first = None
    for o in outs:
        q, sp = _unpack(fmt, s0, z0, ed, raw, W, levels, SEED, frame0, "q0" in o, "spread" in o)
        rep = ND.compare(codes, N, H, W, z, seed=SEED, frame0=frame0, tol=T_Z, cfa=fmt.cfa, black=fmt.black, white=fmt.white,
                         levels=levels, s0=s0, z0=z0, exact_div=ed, spread=sp, q0=q, check_z=check_z and first is None)
        rep.clean(f"{what} [{o}]")
        assert rep.compared["q0"] == (3 * px if q is not None else 0) and rep.compared["spread"] == (3 * px if sp is not None else 0)
        first = first or rep
        del q, sp
    del raw, z
    _free()
    _report(what, packing=packing, shape=f"{N}x{H}x{W}", outs="/".join(outs), held_bytes=held, z_err=f"{first.z_err:.3e}",
            z_err_at=first.z_at, z_there=f"{first.z_there:.6f}", seconds=f"{time.time() - t0:.2f}")
    return first, held


# ===================================================================================================================== B. loops
def _trips():
    import torch
    cus = torch.cuda.get_device_properties(device()).multi_processor_count
    return cus * 8 * 256, 2048 * 256


def _wrap_shape(packing, kind, trip):
    """The smallest frame of `kind` for this trip size: 129 segments a row with half a segment at the end ("one": just above one
    trip, "two": just above two), or 128 whole segments ("aligned", just above one trip); H odd."""
    seg = SEG[packing]
    segs, W = (128, 128 * seg) if kind == "aligned" else (129, 128 * seg + seg // 2)
    H = ((2 if kind == "two" else 1) * trip // segs + 1) | 1
    return H, W, segs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["one", "two", "aligned"])
@pytest.mark.parametrize("packing", list(SEG))
def test_both_loops_run_past_their_first_trip(packing, kind):
    from sesrq import noise
    trip, ztrip = _trips()
    H, W, segs = _wrap_shape(packing, kind, trip)
    items, k = H * segs, 2 if kind == "two" else 1
    assert H % 2 == 1 and k * trip < items < (k + 1) * trip and items % trip != 0 and H * W > 2 * ztrip and (H * W) % ztrip != 0
    assert (W % SEG[packing] == 0) == (kind == "aligned") and W % 4 == 0
    before = noise.instances()
    _case(f"loops {kind}", packing, 1, H, W, (0.01, 0.0005), 2 ** 32 - 1, outs=OUTS)
    assert _names(before) == sorted([f"noise_unpack<{packing},{o}>" for o in OUTS] + ["noise_deviates"]), _names(before)


@pytest.mark.gpu
@pytest.mark.parametrize("packing", list(SEG))
def test_a_batch_that_wraps_is_its_frames_that_do_not(packing):
    """Needs no comparator: three frames whose batch is more than one trip of each loop, each frame less than one."""
    import torch
    trip, ztrip = _trips()
    seg = SEG[packing]
    W, segs = 128 * seg + seg // 2, 129
    H = (trip // (2 * segs)) | 1
    assert H * segs <= trip < 3 * H * segs
    fmt, codes = _fmt(packing), _tile(packing, 1)
    s0, z0 = DOMAINS[1]
    raw = ND.build_raw(codes, 3, H, W, packing, None, 0xEE, device())
    plv = np.array([[0.001, 1e-5], [0.004, 1e-4], [0.012, 1e-3]], F32)
    f0 = 2 ** 32 - 2
    qb, spb = _unpack(fmt, s0, z0, 0, raw, W, plv, SEED, f0)
    for n in range(3):
        q1, sp1 = _unpack(fmt, s0, z0, 0, raw[n:n + 1], W, tuple(plv[n]), SEED, f0 + n)
        assert _differ(q1[0], qb[n]) == 0 and _differ(sp1[0], spb[n]) == 0, n
    assert _differ(qb[0], qb[1]) > 0
    h, w = ztrip // (2 * 1028), 1028
    assert h * w <= ztrip < 3 * h * w
    zb = _z((3, h, w), f0)
    for n in range(3):
        assert _differ(_z((1, h, w), f0 + n)[0], zb[n]) == 0, n
    del raw, qb, spb, zb
    _free()


# ================================================================================================================== C. geometry
ROWS = [("u16", (1 << 24) - 8), ("u16", (1 << 24) - 3), ("raw10", (1 << 24) - 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("packing,W", ROWS, ids=[f"{p}-{w}" for p, w in ROWS])
def test_one_row(packing, W):
    """16 777 208 pixels take the wide loads and stores, 16 777 213 the per-pixel ones with a partial segment; RAW10: 16 777 212."""
    assert (W % SEG[packing] == 0) == (W == (1 << 24) - 8)
    _room(W * 2 + 27 * W + ROOM)
    _case("one row", packing, 1, 1, W, (0.006, 2e-4), 7)


@pytest.mark.gpu
@pytest.mark.parametrize("packing", ["u16", "raw12"])
def test_one_column(packing):
    """16 777 214 rows of two pixels: the counter word y, and the row index the segment walk divides, up to 2^24 - 3."""
    H = (1 << 24) - 2
    _room(H * 4 + 27 * 2 * H + ROOM)
    _case("one column", packing, 1, H, 2, (0.006, 2e-4), 7)


@pytest.mark.gpu
def test_many_frames_across_the_carry_of_the_frame_number():
    """1 048 577 frames of 2 x 8, a (shot, read) pair per frame, from frame 2^32 - 2^19: frame 2^19 of the batch is the first whose
    high counter word is 1."""
    N, f0 = (1 << 20) + 1, 2 ** 32 - 2 ** 19
    assert f0 < 2 ** 32 < f0 + N
    rng = np.random.default_rng(20)
    lv = np.stack([rng.uniform(0, 0.012, N), rng.uniform(0, 1e-3, N)], 1).astype(F32)
    lv[:3] = ((0, 0), (0.012, 0), (0, 1e-3))
    _room(N * 16 * 29 + ROOM)
    _case("many frames", "u16", N, 2, 8, lv, f0)


F32_CROSS = [(1, 18920, 18920), (3, 10924, 10928)]


@pytest.mark.gpu
@pytest.mark.parametrize("packing", list(SEG))
@pytest.mark.parametrize("nhw", F32_CROSS, ids=["x".join(map(str, s)) for s in F32_CROSS])
def test_fp32_outputs_across_4_gib(nhw, packing):
    """N H W >= 357 913 942: the deviates and the fp32 frame end beyond byte 2^32, so `base + c * plane` and `(n * 3 + c) * plane + p`
    must be formed in 64 bits; with three frames `(n * 3 + c) * plane` crosses as well.  noise_deviates and the spread and q0+spread
    instantiations; the deviates are compared with the float64 ones once per shape (under u16), they do not depend on the packing.
    Held: raw + z (12 B/px) + q0 and spread (15 B/px) + the comparator."""
    N, H, W = nhw
    px = N * H * W
    assert px >= 357913942 and 12 * px > 1 << 32
    need = ND.row_bytes(packing, W) * N * H + 12 * px + 15 * px + ROOM
    _room(need)
    _, held = _case("fp32 across 2^32 bytes", packing, N, H, W, (0.01, 0.0005) if N == 1 else np.array([[0.003 * (n + 1), 1e-4] for n in range(N)], F32),
                    2 ** 32 - 2, outs=("spread", "q0+spread"), check_z=packing == "u16")
    assert held == need


@pytest.mark.gpu
@pytest.mark.parametrize("packing", ["raw10", "u16", "raw12"])
def test_q0_across_4_gib(packing):
    """One frame of 37 840 x 37 840 = 1 431 865 600 pixels on the q0-only instantiations: q0 ends beyond byte 2^32, compared box by
    box from the device's deviates of the same geometry.  Held (raw10): 1.79 GB of rows + 17.18 GB of deviates + 4.30 GB of q0 =
    23.27 GB = 21.7 GiB, and the comparator's 3 GiB: 24.7 GiB.  The deviates' element index passes 2^32 here and nowhere else; they are
    compared with the float64 ones in every eighth box and the last (under raw10), all of them in the fp32 case above."""
    import torch
    from sesrq import noise
    t0 = time.time()
    H = W = 37840
    px = H * W
    assert px >= 1431655766 and 3 * px > 1 << 32
    raw_bytes = ND.row_bytes(packing, W) * H
    need = raw_bytes + 12 * px + 3 * px + ROOM
    assert packing != "raw10" or (raw_bytes, 12 * px, 3 * px) == (1789832000, 17182387200, 4295596800)
    _room(need)
    fmt, codes = _fmt(packing), _tile(packing, 2)
    s0, z0 = DOMAINS[0]
    lv, f0 = (0.008, 3e-4), 5
    raw = ND.build_raw(codes, 1, H, W, packing, None, 0xEE, device())
    z = _z((1, H, W), f0)
    before = noise.instances()
    q, _ = _unpack(fmt, s0, z0, 0, raw, W, lv, SEED, f0, True, False)
    assert _names(before) == [f"noise_unpack<{packing},q0>"]
    kw = dict(seed=SEED, frame0=f0, tol=T_Z, cfa=fmt.cfa, black=fmt.black, white=fmt.white, levels=lv, s0=s0, z0=z0, exact_div=0)
    rep = ND.compare(codes, 1, H, W, z, q0=q, check_z=False, **kw)
    rep.clean(f"q0 across 2^32 bytes {packing}")
    assert rep.compared["q0"] == 3 * px
    zerr = "-"
    if packing == "raw10":
        boxes = ND.chunks(1, H, W)
        zr = ND.compare(codes, 1, H, W, z, boxes=boxes[::8] + boxes[-1:], **kw)
        zr.clean("deviates past element 2^32")
        zerr = f"{zr.z_err:.3e}"
    del raw, z, q
    _free()
    _report("q0 across 2^32 bytes", packing=packing, shape=f"1x{H}x{W}", outs="q0", held_bytes=need, z_err=zerr, seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [61440, 61441])
def test_raw_rows_across_4_gib_through_the_stride(stride):
    """70 000 rows of 64 pixels, 61 440 bytes apart (aligned: wide loads) and 61 441 (byte loads): `row * stride` passes 2^32; the
    padding holds 0xEE."""
    H, W = 70000, 64
    assert H * stride > 1 << 32
    _room(H * stride + 27 * H * W + ROOM)
    _case(f"raw stride {stride}", "u16", 1, H, W, (0.01, 0.0005), 3, stride=stride)


@pytest.mark.gpu
def test_one_item_below_the_size_refusal():
    """The largest frame sesrq_noise_unpack accepts, one pixel wide: its loop variable comes closest to 2^31.  No comparator fits (the
    deviates alone would take 25.8 GB), so the header's identity is used: with shot = read = 0 every byte is sesrq_sensor_unpack's.
    q0 only, compared on the device.  Held: 2 H of rows and twice 3 H of q0."""
    import torch
    from sesrq import noise, sensor as S
    t0 = time.time()
    trip, _ = _trips()
    H = 0x7FFFFFFF - trip
    need = 2 * H + 6 * H + GIB
    _room(need)
    fmt = _fmt("u16")
    s0, z0 = DOMAINS[0]
    t = np.random.default_rng(77).integers(0, 1300, (1, 1, 122, 1)).astype(np.uint16)
    raw = G.device_frame(t.view(np.int16), 1, H, 1, device())[:, 0].view(torch.uint8).view(1, H, 2)
    before = noise.instances()
    q, _ = _unpack(fmt, s0, z0, 0, raw, 1, (0.0, 0.0), SEED, 2 ** 64 - 1, True, False)
    assert _names(before) == ["noise_unpack<u16,q0>"]
    q2 = torch.full((1, 3, H, 1), 99, dtype=torch.int8, device=device())
    S.launch(device(), fmt, s0, z0, 0, raw, 1, 2, q2, None, torch.cuda.current_stream(device()))
    torch.cuda.synchronize()
    bad = _differ(q, q2)
    assert bad == 0, f"{bad} of {q.numel()} bytes differ from the sensor library's"
    assert int(torch.count_nonzero(q2[0, :, :4096] != q2[0, :, :1])) > 0          # the frame is not flat
    del raw, q, q2
    _free()
    _report("one item below the refusal", packing="u16", shape=f"1x{H}x1", outs="q0", held_bytes=need, seconds=f"{time.time() - t0:.2f}")


@pytest.mark.gpu
def test_size_refusals_launch_nothing():
    """The first refused item count of sesrq_noise_unpack for each packing, sesrq_noise_deviates at N H W = 2^31 and at N H = 2^31,
    with pointers that are never dereferenced; no launch counter moves."""
    import torch
    from sesrq import noise
    trip, _ = _trips()
    first = 0x7FFFFFFF - trip + 1
    fake = 1 << 20
    before = noise.instances()
    lib = noise.lib()
    for packing in SEG:
        h = noise.context(device(), _fmt(packing), *DOMAINS[0], 0)
        for N, H, W in ((1, first, SEG[packing]), (1, first, 4), (2, (first + 1) // 2, SEG[packing] + 4)):
            assert N * H * -(-W // SEG[packing]) >= first
            assert lib.sesrq_noise_unpack(h, fake, 4096, fake, None, N, H, W, 0.01, 1e-4, None, SEED, 0, None) != 0
            assert noise.last_error() == f"sesrq_noise_unpack: frame of {N} x {H} x {W} is too large", noise.last_error()
    for N, H, W in ((1 << 15, 1 << 8, 1 << 8), (2, 1 << 30, 1), (1, 0x7FFFFFFF, 2)):
        assert lib.sesrq_noise_deviates(fake, N, H, W, SEED, 0, None) != 0
        assert noise.last_error() == f"sesrq_noise_deviates: frame of {N} x {H} x {W} is too large", noise.last_error()
    assert noise.instances() == before
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_deviates_at_the_largest_size_they_accept():
    """N H W = 2^31 - 1, one pixel wide: not refused.  24 GiB of deviates: the first box, every 64th and the last are compared with the
    float64 ones (the whole would take as long as the rest of this module); every deviate is within Z_MAX."""
    import torch
    t0 = time.time()
    H = 0x7FFFFFFF
    need = 12 * H + ROOM
    _room(need)
    z = _z((1, H, 1), 9)
    boxes = ND.chunks(1, H, 1)
    rep = ND.compare(None, 1, H, 1, z, seed=SEED, frame0=9, tol=T_Z, boxes=boxes[::64] + boxes[-1:])
    rep.clean("deviates at 2^31 - 1 pixels")
    flat = z.view(-1)
    step = 1 << 28
    assert all(bool((flat[i:i + step].abs() <= NO.Z_MAX).all()) for i in range(0, flat.numel(), step))
    del z, flat
    _free()
    _report("deviates at the largest size", shape=f"1x{H}x1", held_bytes=need, z_err=f"{rep.z_err:.3e}", seconds=f"{time.time() - t0:.2f}")


# =================================================================================================================== D. corners
def _corners():
    with open(CORNERS) as fh:
        return json.load(fh)


R_TARGETS = (0, 2 ** 23 - 1)
T_TARGETS = (0, 1, 2 ** 22, 2 ** 23, 3 * 2 ** 22, 2 ** 24 - 1)


def test_corner_fixture_lists_every_corner():
    """tests/golden/noise/corners.json (make_noise_corners.py): the oracle's words at the listed pixels are the targets, and all 16
    (word, target) pairs are there."""
    c = _corners()
    assert c["seed"] == SEED and (c["frames"], c["H"], c["W"]) == (16, 2048, 2048)
    seen = set()
    for f, y, x, k, t in c["hits"]:
        assert 0 <= f < 16 and 0 <= y < 2048 and 0 <= x < 2048
        w = NO.words_at(SEED, f, y, x)
        assert w[k] >> (9 if k % 2 == 0 else 8) == t, (f, y, x, k, t, w)
        seen.add((k, t))
    want = {(k, t) for k in (0, 2) for t in R_TARGETS} | {(k, t) for k in (1, 3) for t in T_TARGETS}
    assert seen == want, want - seen
    assert NO.words_at(SEED, 2 ** 32 + 5, 3, 2) == tuple(int(w[3, 2]) for w in NO.words(SEED, 2 ** 32 + 5, 4, 6))


@pytest.mark.gpu
def test_deviates_at_the_corners_and_over_a_real_sample():
    """sesrq_noise_deviates on (16, 2048, 2048) from frame 0: 2.0e8 deviates, all compared with the float64 ones at T_Z and with Z_MAX.
    At the listed pixels, what the header implies exactly: angle 2 u_t = 0.5 or 1.5 -> cospi is 0 and the cosine deviates are +-0,
    sinpi is +-1; 2 u_t = 0 or 1 -> sinpi is 0 and z[1] is +-0, cospi is +-1; rho at u_r = 2^-24 is Z_MAX and the pair's length
    stays below it.  The measured maximum goes to profiles/noise_limits.txt; the bound stays T_Z."""
    import torch
    t0 = time.time()
    N, H, W = 16, 2048, 2048
    _room(12 * N * H * W + ROOM)
    z = _z((N, H, W), 0)
    rep = ND.compare(None, N, H, W, z, seed=SEED, frame0=0, tol=T_Z)
    hits = _corners()["hits"]
    idx = torch.tensor([h[:3] for h in hits], device=device())
    got = z[idx[:, 0], :, idx[:, 1], idx[:, 2]].cpu().numpy()              # (hits, 3)
    _report("corners", shape=f"{N}x{H}x{W}", deviates=3 * N * H * W, held_bytes=12 * N * H * W + ROOM, z_err=f"{rep.z_err:.3e}",
            z_err_at=rep.z_at, z_there=f"{rep.z_there:.6f}", bound=f"{T_Z:.3e}", seconds=f"{time.time() - t0:.2f}")
    rep.clean("16 frames of 2048 x 2048")
    assert rep.compared["z"] == 3 * N * H * W
    for (f, y, x, k, t), zz in zip(hits, got):
        w = NO.words_at(SEED, f, y, x)
        rho = [float(np.sqrt(-2.0 * np.log(NO.u_r(np.uint64(w[j]))))) for j in (0, 2)]
        at = f"(frame {f}, y {y}, x {x}) w{k} -> {t}: z = {zz.tolist()}"
        if k == 1 and t in (2 ** 22, 3 * 2 ** 22):
            assert zz[0] == 0 and abs(zz[1] - (rho[0] if t == 2 ** 22 else -rho[0])) <= T_Z, at
        if k == 1 and t in (0, 2 ** 23):
            assert zz[1] == 0 and abs(zz[0] - (rho[0] if t == 0 else -rho[0])) <= T_Z, at
        if k == 3 and t in (2 ** 22, 3 * 2 ** 22):
            assert zz[2] == 0, at
        if k == 3 and t in (0, 2 ** 23):
            assert abs(zz[2] - (rho[1] if t == 0 else -rho[1])) <= T_Z, at
        if k == 0:
            assert abs(float(np.hypot(*zz[:2].astype(np.float64))) - rho[0]) <= 2 * T_Z and np.abs(zz[:2]).max() <= NO.Z_MAX, at
            assert (t == 0) == (abs(rho[0] - NO.Z_MAX) < 1e-12) and (t != 0) == (rho[0] < 3.5e-4), at
        if k == 2:
            assert abs(zz[2]) <= rho[1] + T_Z and (t == 0) == (abs(rho[1] - NO.Z_MAX) < 1e-12) and (t != 0) == (rho[1] < 3.5e-4), at
    del z
    _free()


# ========================================================================================================== E. codes and levels
EVERY = [("u16", 64, 1023), ("u16", 4096, 65535), ("raw10", 16, 1023), ("raw12", 64, 4095)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("packing,black,white", EVERY, ids=[f"{p}-{b}-{w}" for p, b, w in EVERY])
def test_every_code_at_every_phase_with_noise_on(packing, black, white, cfa):
    """512 x 516 pixels, every code 0 .. 65535 (RAW10 / RAW12: every code of the packing, the frame's low bits) at all four Bayer
    phases, exact_div 0 and 2: noise_oracle.frame on the device's deviates, bit for bit."""
    from sesrq import sensor as S
    codes = (every_code_frame() & TOP[packing])[None]
    for py in (0, 1):
        for px in (0, 1):
            assert len(np.unique(codes[0, py::2, px::2])) == TOP[packing] + 1
    fmt = S.Format(cfa=cfa, black=black, white=white, packing=packing)
    rows = S.pack(codes, fmt)
    f0 = 40 + CFAS.index(cfa)
    z = _z(codes.shape, f0).cpu().numpy()
    for (s0, z0), ed in zip(DOMAINS, (0, 2)):
        want_sp, want_q = NO.frame(codes, cfa, black, white, (0.01, 0.0005), z, s0, z0, ed)
        q, sp = _unpack(fmt, s0, z0, ed, rows, 516, (0.01, 0.0005), SEED, f0)
        same(f"{packing} {cfa} exact_div {ed} spread", sp, want_sp)
        same(f"{packing} {cfa} exact_div {ed} q0", q, want_q)
    assert len(np.unique(want_q)) > 200


def _edge_frame():
    """(2, 6, 40) uint16 at black 64, white 1023: black, white, codes beyond both and mid codes at every Bayer phase."""
    c = np.random.default_rng(5).integers(0, 1200, (2, 6, 40)).astype(np.uint16)
    c[:, :2, :8] = np.array([[64, 1023, 0, 65535, 500, 501, 1023, 64], [1023, 64, 600, 2, 64, 1023, 63, 1024]], np.uint16)
    return c


EDGES = [(0.0, 1e-40), (1e-45, 0.0), (FLT_MAX, 0.0), (0.0, FLT_MAX), (FLT_MAX, FLT_MAX)]


@pytest.mark.gpu
@pytest.mark.parametrize("levels", EDGES, ids=[f"{s:g}-{r:g}" for s, r in EDGES])
def test_levels_at_the_edges_of_what_is_accepted(levels):
    """Subnormal variances (a flushed v or sigma would show: the non-sites hold fl(sigma z) of about 1e-20), the largest finite levels
    and v = inf, as scalars and as a device levels array: noise_oracle.frame on the device's deviates, bit for bit, and no NaN."""
    from sesrq import sensor as S
    codes = _edge_frame()
    fmt = S.Format(cfa="gbrg", black=64, white=1023)
    rows = S.pack(codes, fmt)
    z = _z(codes.shape, 17).cpu().numpy()
    for (s0, z0), ed in zip(DOMAINS, (0, 2)):
        want_sp, want_q = NO.frame(codes, "gbrg", 64, 1023, levels, z, s0, z0, ed)
        assert not np.isnan(want_sp).any()
        if levels == (0.0, 1e-40):
            assert ((want_sp > 0) & (want_sp < 1e-19)).sum() > 100 and F32(1e-40) > 0
        if levels == (1e-45, 0.0):
            assert 0 < NO.variance(F32(1), *levels) < 1e-44          # sigma = 3.7e-23 is absorbed at the sites; the non-sites have v = 0
        for lv in (levels, np.array([levels, levels], F32)):
            q, sp = _unpack(fmt, s0, z0, ed, rows, 40, lv, SEED, 17)
            same(f"levels {levels} exact_div {ed} spread", sp, want_sp)
            same(f"levels {levels} exact_div {ed} q0", q, want_q)


ZERO_AT = [(1, 2 ** 22, 0), (1, 0, 1), (1, 2 ** 23, 1), (3, 2 ** 22, 2), (3, 3 * 2 ** 22, 2)]      # (word, target, channel whose deviate is 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k,t,c", ZERO_AT, ids=[f"w{k}-{t}-c{c}" for k, t, c in ZERO_AT])
def test_infinite_sigma_on_a_zero_deviate_gives_zero(k, t, c):
    """A corner pixel whose deviate on channel c is exactly zero, a white code there under a CFA order that makes c its site channel,
    levels (FLT_MAX, FLT_MAX): v = inf, sigma = inf, sigma z = NaN, y = NaN, and the header's clamp fminf(fmaxf(y, 0), 1) gives 0.
    The whole frame is the restatement's (tests/noise_device.py clamps the same way) and holds no NaN."""
    import torch
    from sesrq import sensor as S
    f, y, x = next(h[:3] for h in _corners()["hits"] if (h[3], h[4]) == (k, t))
    cfa = next(o for o in CFAS if ND.SITE[o][y & 1][x & 1] == c)
    H, W = (y + 2) & ~1, (x + 8) & ~7
    rng = np.random.default_rng(k + t)
    codes = rng.integers(0, 1100, (1, H, W)).astype(np.uint16)
    codes[0, y, x] = 1023
    fmt = S.Format(cfa=cfa, black=64, white=1023)
    ct = torch.from_numpy(codes.astype(np.int32)).to(device())
    z = _z((1, H, W), f)
    assert float(z[0, c, y, x]) == 0.0
    s0, z0 = DOMAINS[0]
    lv = (FLT_MAX, FLT_MAX)
    q, sp = _unpack(fmt, s0, z0, 0, ND.build_raw(ND.Dense(ct), 1, H, W, "u16", None, 0, device()), W, lv, SEED, f)
    assert float(sp[0, c, y, x]) == 0.0 and int(q[0, c, y, x]) == int(NO.O.quantize_input(F32(0), s0, z0))
    assert int(torch.count_nonzero(torch.isnan(sp))) == 0
    rep = ND.compare(ND.Dense(ct), 1, H, W, z, seed=SEED, frame0=f, tol=T_Z, cfa=cfa, black=64, white=1023, levels=lv, s0=s0, z0=z0,
                     spread=sp, q0=q, check_z=False)
    rep.clean(f"inf * 0 at ({f}, {y}, {x})")
    # the numpy oracle says the same on the rows around the pixel
    y0 = y & ~1
    crop = np.s_[:, :, y0:y0 + 2, :]
    want_sp, want_q = NO.frame(codes[:, y0:y0 + 2], cfa, 64, 1023, lv, z[crop].cpu().numpy(), s0, z0)
    same("oracle spread", sp[crop], want_sp)
    same("oracle q0", q[crop], want_q)
    with np.errstate(over="ignore"):
        assert want_sp[0, c, y - y0, x] == 0 and np.isinf(NO.variance(F32(1), *lv))


BAD_PAIRS = [(float("nan"), 1e-4), (-1.0, 0.0), (float("inf"), float("inf"))]


@pytest.mark.gpu
@pytest.mark.parametrize("bad", BAD_PAIRS, ids=["nan", "negative", "inf"])
def test_a_bad_pair_in_a_device_levels_array_spoils_that_frame_only(bad):
    """include/sesrq_noise.h: a negative or non-finite pair in a device levels array "gives unspecified values in that frame only".
    One bad pair in the middle of a batch of five: the four other frames are their single-frame runs bit for bit and no byte outside
    the outputs changes (the arena of tests/test_noise_buffers.py); the bad frame's values are not asserted."""
    import torch
    from sesrq import noise, sensor as S
    from test_caller_buffers import NAN, _clean, _put
    N, H, W = 5, 6, 40
    codes = np.concatenate([_edge_frame(), _edge_frame()[::-1], _edge_frame()[:1]])
    fmt = S.Format(cfa="rggb", black=64, white=1023)
    rows = S.pack(codes, fmt)
    lv = np.array([[0.002 * (n + 1), 1e-4 * (n + 1)] for n in range(N)], F32)
    lv[2] = bad
    s0, z0 = DOMAINS[1]
    f0 = 2 ** 32 - 3
    ctx = noise.context(device(), fmt, s0, z0, 0)
    for qo, so in ((1, 4), (0, 0)):          # per-pixel stores, wide stores
        ain = Arena(device(), Arena.room(rows.nbytes, lv.nbytes), 0x7F)
        rin, lin = _put(ain, rows, 0, "raw"), _put(ain, lv, 4, "levels")
        aq, asp = Arena(device(), Arena.room(3 * codes.size), 0x5A), Arena(device(), Arena.room(12 * codes.size), NAN)
        q, sp = aq.place((N, 3, H, W), torch.int8, qo, name="q0"), asp.place((N, 3, H, W), torch.float32, so, name="spread")
        rc = noise.lib().sesrq_noise_unpack(ctx, rin.data_ptr(), rows.shape[2], q.data_ptr(), sp.data_ptr(), N, H, W, 0.0, 0.0, lin.data_ptr(),
                                            SEED, f0, stream_ptr())
        assert rc == 0, noise.last_error()
        _clean(f"bad pair {bad}", ain, aq, asp)
        same("raw is not written", rin, rows)
        same("levels are not written", lin, lv)
        for n in (0, 1, 3, 4):
            q1, sp1 = _unpack(fmt, s0, z0, 0, rows[n:n + 1], W, tuple(lv[n]), SEED, (f0 + n) % 2 ** 64)
            same(f"frame {n} q0", q[n], q1[0])
            same(f"frame {n} spread", sp[n], sp1[0])
