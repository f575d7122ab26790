"""Caller buffers of sesrq_noise_unpack and sesrq_noise_deviates (include/sesrq_noise.h, "Caller buffers"), as
tests/test_sensor_buffers.py pins sesrq_sensor_unpack: every buffer an arena placement surrounded by canaries (0x5A / 0xA5; NaN around
the fp32 frames), at the element-aligned address classes that test uses.  Results are bit-equal to tests/noise_oracle.py on the
device's deviates, no byte outside the outputs changes, raw and the levels array are not written, stride padding (hostile bytes) never
shows, and a refused call launches nothing."""
import numpy as np
import pytest
import torch

import noise_oracle as NO
from helpers import Arena, device, same, stream_ptr
from test_caller_buffers import NAN, _clean, _put
from test_sensor_buffers import PACKED_PLACES, ROUNDS, U16_PLACES, _outs

pytestmark = pytest.mark.gpu

F32 = np.float32
S0, Z0 = 0.0031, -140
SEED, FRAME0 = 0xFEEDFACECAFEBEEF, 2 ** 32 - 2


def _ctx(fmt, ed=0):
    from sesrq import noise
    return noise.context(device(), fmt, S0, Z0, ed)


def _deviates(N, H, W, off=0, canary=0x5A):
    """sesrq_noise_deviates into an arena placement at `off` modulo 256."""
    from sesrq import noise
    az = Arena(device(), Arena.room(12 * N * H * W), NAN)
    z = az.place((N, 3, H, W), torch.float32, off, name="z")
    before = noise.instances()["noise_deviates"]
    assert noise.lib().sesrq_noise_deviates(z.data_ptr(), N, H, W, SEED, FRAME0, stream_ptr()) == 0, noise.last_error()
    assert noise.instances()["noise_deviates"] == before + 1
    _clean(f"deviates at {off}", az)
    return z.cpu().numpy()


def _run(what, fmt, codes, rows, W, places, levels):
    from sesrq import noise
    N, H = codes.shape[:2]
    z = _deviates(N, H, W)
    for off in (4, 8, 12):
        same(f"{what} z at {off}", _deviates(N, H, W, off), z)
    want_sp, want_q = NO.frame(codes, fmt.cfa, fmt.black, fmt.white, levels, z, S0, Z0)
    ctx = _ctx(fmt)
    lv = np.asarray(levels, F32)
    seen = [set(), set(), set()]
    for i, (ro, qo, so) in enumerate(places):
        for outs in _outs(i):
            for r, (canary, around) in enumerate(ROUNDS):
                w = f"{what} at ({ro}, {qo}, {so}) q0={outs[0]} spread={outs[1]} run {r + 1}"
                ain = Arena(device(), Arena.room(rows.nbytes, lv.nbytes), around)
                rin = _put(ain, rows, ro, "raw")
                lin = _put(ain, lv, 4 * (i % 4), "levels") if lv.ndim == 2 else None
                aq = Arena(device(), Arena.room(want_q.nbytes), canary)
                asp = Arena(device(), Arena.room(want_sp.nbytes), NAN)
                q = aq.place(want_q.shape, torch.int8, qo, name="q0") if outs[0] else None
                sp = asp.place(want_sp.shape, torch.float32, so, name="spread") if outs[1] else None
                before = sum(noise.instances().values())
                rc = noise.lib().sesrq_noise_unpack(ctx, rin.data_ptr(), rows.shape[2], q.data_ptr() if q is not None else None,
                                                    sp.data_ptr() if sp is not None else None, N, H, W,
                                                    0.0 if lin is not None else float(lv[0]), 0.0 if lin is not None else float(lv[1]),
                                                    lin.data_ptr() if lin is not None else None, SEED, FRAME0, stream_ptr())
                assert rc == 0, (w, noise.last_error())
                assert sum(noise.instances().values()) == before + 1
                _clean(w, ain, aq, asp)
                same(w + " raw is not written", rin, rows)
                if lin is not None:
                    same(w + " levels are not written", lin, lv)
                if outs[0]:
                    same(w + " q0", q, want_q)
                if outs[1]:
                    same(w + " spread", sp, want_sp)
                for s, o in zip(seen, (ro, qo, so)):
                    s.add(o)
    return seen


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
    levels = (0.01, 5e-4) if extra else np.array([[0.002 * (n + 1), 1e-4] for n in range(N)], F32)
    for pad in (0xFF, 0x00):
        rows = S.pack(codes, fmt, fmt.row_bytes(W) + extra, pad)
        seen = _run(f"{packing} {nhw} +{extra} pad {pad:#x}", fmt, codes, rows, W, PACKED_PLACES, levels)
    assert seen[0] >= {0, 1, 2, 3, 7} and seen[1] >= {0, 1, 3, 7} and seen[2] >= {0, 4, 8, 12}


@pytest.mark.parametrize("levels16", [(64, 1023), (4096, 65535)], ids=["10-bit", "16-bit"])
@pytest.mark.parametrize("nhw,extra", [((2, 6, 32), 0), ((2, 6, 32), 16), ((2, 5, 21), 0), ((2, 5, 21), 6)])
def test_u16_frames_in_hostile_surroundings(levels16, nhw, extra):
    """W = 32 with 64-byte rows: 16-byte loads and 8-byte q0 stores where the addresses allow (q0 at 8 modulo 16 still stores wide);
    W = 21: rows never 16-byte aligned, a tail of 5 pixels, per-pixel stores; extra: stride padding behind every row."""
    from sesrq import sensor as S
    N, H, W = nhw
    fmt = S.Format(cfa="bggr", black=levels16[0], white=levels16[1])
    rng = np.random.default_rng(W + extra + levels16[1])
    codes = rng.integers(0, 65536, (N, H, W)).astype(np.uint16)
    codes[0, 0, 0], codes[-1, -1, -1], codes[0, 1, 1] = levels16[1], levels16[0], 65535
    levels = (0.012, 1e-3) if extra else np.array([[0.002 * (n + 1), 1e-4] for n in range(N)], F32)
    for pad in (0xFF, 0x00):
        rows = S.pack(codes, fmt, 2 * W + extra, pad)
        seen = _run(f"u16 {levels16} {nhw} +{extra} pad {pad:#x}", fmt, codes, rows, W, U16_PLACES, levels)
    assert seen[0] >= {0, 2, 6} and seen[1] >= {0, 1, 3, 7} and seen[2] >= {0, 4, 8, 12}


def test_a_refused_call_launches_nothing():
    from sesrq import noise, sensor as S
    fmt = S.Format(white=1023, packing="raw10")
    ctx, u16 = _ctx(fmt), _ctx(S.Format(white=1023))
    N, H, W = 1, 4, 16
    ain = Arena(device(), Arena.room(N * H * 32, 8 * N), 0x7F)
    rin = ain.place((N, H, 32), torch.uint8, 0, fill=0, name="raw")
    lin = ain.place((N, 2), torch.float32, 0, fill=0.001, name="levels")
    aout = Arena(device(), Arena.room(3 * N * H * W, 12 * N * H * W, 12 * N * H * W), 0x5A)
    q = aout.place((N, 3, H, W), torch.int8, 0, name="q0")
    sp = aout.place((N, 3, H, W), torch.float32, 0, name="spread")
    z = aout.place((N, 3, H, W), torch.float32, 0, name="z")
    before = noise.instances()
    lib = noise.lib()
    R, Q, SP, L = rin.data_ptr(), q.data_ptr(), sp.data_ptr(), lin.data_ptr()
    ok = (0.01, 1e-4, None, 1, 0)
    for args, word in (((ctx, R, 19, Q, SP, N, H, W) + ok, "row_stride_bytes 19 is less than the 20"),
                       ((u16, R, 31, Q, SP, N, H, W) + ok, "row_stride_bytes 31 is less than the 32"),
                       ((ctx, R, 32, Q, SP, N, H, 14) + ok, "pack group"),
                       ((ctx, None, 32, Q, SP, N, H, W) + ok, "raw is NULL"),
                       ((ctx, R, 32, None, None, N, H, W) + ok, "neither q0 nor spread"),
                       ((ctx, R, 32, Q, SP + 2, N, H, W) + ok, "4-byte aligned"),
                       ((ctx, R, 32, Q, SP, 0, H, W) + ok, "empty frame"),
                       ((ctx, R, 32, Q, SP, N, H, 0) + ok, "empty frame"),
                       ((None, R, 32, Q, SP, N, H, W) + ok, "ctx is NULL"),
                       ((ctx, R, 32, Q, SP, N, H, W, -1e-9, 1e-4, None, 1, 0), "shot noise level"),
                       ((ctx, R, 32, Q, SP, N, H, W, float("nan"), 1e-4, None, 1, 0), "shot noise level"),
                       ((ctx, R, 32, Q, SP, N, H, W, 0.01, float("inf"), None, 1, 0), "read noise level"),
                       ((ctx, R, 32, Q, SP, N, H, W, 0.01, -0.5, None, 1, 0), "read noise level"),
                       ((ctx, R, 32, Q, SP, N, H, W, 0.01, 1e-4, L + 2, 1, 0), "levels is not 4-byte aligned"),
                       ((u16, R, 0x7fffffff * 2, Q, SP, 0x7fffffff, 2, 8) + ok, "too large")):
        assert lib.sesrq_noise_unpack(*args, stream_ptr()) != 0 and word in noise.last_error(), (word, noise.last_error())
    for args, word in (((None, N, H, W), "z is NULL"), ((z.data_ptr() + 1, N, H, W), "4-byte aligned"), ((z.data_ptr(), N, 0, W), "empty frame"),
                       ((z.data_ptr(), 0x7fffffff, 0x7fffffff, 2), "too large"), ((z.data_ptr(), 2, 0x7fffffff, 1), "too large")):
        assert lib.sesrq_noise_deviates(*args, SEED, 0, stream_ptr()) != 0 and word in noise.last_error(), (word, noise.last_error())
    assert noise.instances() == before
    _clean("refused calls", ain, aout)
    # negative zero is no negative level, and scalars are not looked at when a levels array replaces them
    assert lib.sesrq_noise_unpack(ctx, R, 32, Q, SP, N, H, W, -0.0, 0.0, None, 1, 0, stream_ptr()) == 0, noise.last_error()
    assert lib.sesrq_noise_unpack(ctx, R, 32, Q, SP, N, H, W, -1.0, float("nan"), L, 1, 0, stream_ptr()) == 0, noise.last_error()
    _clean("accepted calls", ain, aout)
