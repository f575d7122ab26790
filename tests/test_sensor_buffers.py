"""Caller buffers of sesrq_sensor_unpack (include/sesrq_sensor.h, "Caller buffers"), in the arena tests/test_caller_buffers.py uses for
libsesrq_raw.so: every buffer an arena placement surrounded by canaries (0x5A / 0xA5; NaN around the fp32 frame), at the address
classes that flip the wide loads and the wide stores by the address alone.  Packed bytes sit at 0, 1, 2, 3, 7 modulo 16, uint16 frames
at 0, 2, 6; q0 at 0, 1, 3, 7; the fp32 frame at 0, 4, 8, 12.  Results are bit-equal to tests/sensor_oracle.py, no byte outside the
outputs changes, stride padding (hostile bytes) never shows, and a refused call launches nothing."""
import numpy as np
import pytest
import torch

import sensor_oracle as SO
from helpers import Arena, device, same, stream_ptr
from test_caller_buffers import NAN, _clean, _put

pytestmark = pytest.mark.gpu

F32 = np.float32
S0, Z0 = 0.0031, -140
# (raw, q0, spread) address classes modulo 16
PACKED_PLACES = ((0, 0, 0), (1, 0, 0), (2, 1, 4), (3, 3, 8), (7, 7, 12), (4, 0, 0), (0, 8, 0), (0, 0, 4))
U16_PLACES = ((0, 0, 0), (2, 0, 0), (6, 1, 4), (0, 3, 8), (2, 7, 12), (0, 8, 0), (0, 0, 4))
# (canary of the outputs, what surrounds the raw bytes and fills their stride padding)
ROUNDS = ((0x5A, 0x7F), (0xA5, 0x80))


def _ctx(fmt, ed=0):
    from sesrq import sensor as S
    return S.context(device(), fmt, S0, Z0, ed)


def _run(what, fmt, codes, rows, W, places, outs_of):
    """`rows` (N, H, stride) uint8 at each address class of `places`, against the oracle on `codes`."""
    from sesrq import sensor as S
    N, H = codes.shape[:2]
    t = SO.q_table(fmt.black, fmt.white, S0, Z0)
    want_q = SO.spread(codes, t, t[0], fmt.cfa, fmt.black, fmt.white)
    want_sp = SO.spread(codes, SO.levels(fmt.black, fmt.white), F32(0), fmt.cfa, fmt.black, fmt.white)
    ctx = _ctx(fmt)
    seen = [set(), set(), set()]
    for i, (ro, qo, so) in enumerate(places):
        for outs in outs_of(i):
            for r, (canary, around) in enumerate(ROUNDS):
                w = f"{what} at ({ro}, {qo}, {so}) q0={outs[0]} spread={outs[1]} run {r + 1}"
                ain = Arena(device(), Arena.room(rows.nbytes), around)
                rin = _put(ain, rows, ro, "raw")
                aq = Arena(device(), Arena.room(want_q.nbytes), canary)
                asp = Arena(device(), Arena.room(want_sp.nbytes), NAN)
                q = aq.place(want_q.shape, torch.int8, qo, name="q0") if outs[0] else None
                sp = asp.place(want_sp.shape, torch.float32, so, name="spread") if outs[1] else None
                before = sum(S.instances().values())
                rc = S.lib().sesrq_sensor_unpack(ctx, rin.data_ptr(), rows.shape[2], q.data_ptr() if q is not None else None,
                                                 sp.data_ptr() if sp is not None else None, N, H, W, stream_ptr())
                assert rc == 0, (w, S.last_error())
                assert sum(S.instances().values()) == before + 1
                _clean(w, ain, aq, asp)
                same(w + " raw is not written", rin, rows)
                if outs[0]:
                    same(w + " q0", q, want_q)
                if outs[1]:
                    same(w + " spread", sp, want_sp)
                for s, o in zip(seen, (ro, qo, so)):
                    s.add(o)
    return seen


def _outs(i):
    return ((True, True), (True, False), (False, True)) if i in (0, 4) else ((True, True),)


@pytest.mark.parametrize("packing,white", [("raw10", 1023), ("raw12", 4095)])
@pytest.mark.parametrize("nhw,extra", [((2, 6, 32), 0), ((2, 6, 32), 4), ((2, 5, 40), 3), ((1, 3, 8), 0)])
def test_packed_frames_in_hostile_surroundings(packing, white, nhw, extra):
    """W = 32: whole segments and wide stores where the addresses allow; stride + 4 keeps rows 4-byte aligned, + 3 does not; W = 40 adds a
    tail of half a segment and per-pixel stores; W = 8 is less than one segment."""
    from sesrq import sensor as S
    N, H, W = nhw
    fmt = S.Format(cfa="grbg", black=16, white=white, packing=packing)
    rng = np.random.default_rng(W + extra + white)
    codes = rng.integers(0, white + 1, (N, H, W)).astype(np.uint16)
    codes[0, 0, 0], codes[-1, -1, -1] = white, 0
    for pad in (0xFF, 0x00):
        rows = S.pack(codes, fmt, fmt.row_bytes(W) + extra, pad)
        seen = _run(f"{packing} {nhw} +{extra} pad {pad:#x}", fmt, codes, rows, W, PACKED_PLACES, _outs)
    assert seen[0] >= {0, 1, 2, 3, 7} and seen[1] >= {0, 1, 3, 7} and seen[2] >= {0, 4, 8, 12}


@pytest.mark.parametrize("levels", [(64, 1023), (4096, 65535)], ids=["table", "steps"])
@pytest.mark.parametrize("nhw,extra", [((2, 6, 32), 0), ((2, 6, 32), 16), ((2, 5, 21), 0), ((2, 5, 21), 6)])
def test_u16_frames_in_hostile_surroundings(levels, nhw, extra):
    """W = 32 with 64-byte rows: 16-byte loads and 8-byte q0 stores where the addresses allow (q0 at 8 modulo 16 still stores wide);
    W = 21: rows never 16-byte aligned, a tail of 5 pixels, per-pixel stores; extra: stride padding behind every row."""
    from sesrq import sensor as S
    N, H, W = nhw
    fmt = S.Format(cfa="bggr", black=levels[0], white=levels[1])
    rng = np.random.default_rng(W + extra + levels[1])
    codes = rng.integers(0, 65536, (N, H, W)).astype(np.uint16)
    codes[0, 0, 0], codes[-1, -1, -1], codes[0, 1, 1] = levels[1], levels[0], 65535
    for pad in (0xFF, 0x00):
        rows = S.pack(codes, fmt, 2 * W + extra, pad)
        seen = _run(f"u16 {levels} {nhw} +{extra} pad {pad:#x}", fmt, codes, rows, W, U16_PLACES, _outs)
    assert seen[0] >= {0, 2, 6} and seen[1] >= {0, 1, 3, 7} and seen[2] >= {0, 4, 8, 12}


def test_a_refused_call_launches_nothing():
    from sesrq import sensor as S
    fmt = S.Format(white=1023, packing="raw10")
    ctx, u16 = _ctx(fmt), _ctx(S.Format(white=1023))
    N, H, W = 1, 4, 16
    ain = Arena(device(), Arena.room(N * H * 32), 0x7F)
    rin = ain.place((N, H, 32), torch.uint8, 0, fill=0, name="raw")
    aout = Arena(device(), Arena.room(3 * N * H * W, 12 * N * H * W), 0x5A)
    q = aout.place((N, 3, H, W), torch.int8, 0, name="q0")
    sp = aout.place((N, 3, H, W), torch.float32, 0, name="spread")
    before = S.instances()
    lib = S.lib()
    for args, word in (((ctx, rin.data_ptr(), 19, q.data_ptr(), sp.data_ptr(), N, H, W), "row_stride_bytes 19 is less than the 20"),
                       ((u16, rin.data_ptr(), 31, q.data_ptr(), sp.data_ptr(), N, H, W), "row_stride_bytes 31 is less than the 32"),
                       ((ctx, rin.data_ptr(), 32, q.data_ptr(), sp.data_ptr(), N, H, 14), "pack group"),
                       ((ctx, None, 32, q.data_ptr(), sp.data_ptr(), N, H, W), "raw is NULL"),
                       ((ctx, rin.data_ptr(), 32, None, None, N, H, W), "neither q0 nor spread"),
                       ((ctx, rin.data_ptr(), 32, q.data_ptr(), sp.data_ptr() + 2, N, H, W), "4-byte aligned"),
                       ((ctx, rin.data_ptr(), 32, q.data_ptr(), sp.data_ptr(), 0, H, W), "empty frame"),
                       ((ctx, rin.data_ptr(), 32, q.data_ptr(), sp.data_ptr(), N, H, 0), "empty frame"),
                       ((None, rin.data_ptr(), 32, q.data_ptr(), sp.data_ptr(), N, H, W), "ctx is NULL")):
        assert lib.sesrq_sensor_unpack(*args, stream_ptr()) != 0 and word in S.last_error(), (word, S.last_error())
    assert S.instances() == before
    _clean("refused calls", ain, aout)
