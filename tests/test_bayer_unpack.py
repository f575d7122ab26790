"""The Bayer unpack body libsesrq_raw.so and libsesrq_sensor.so share (csrc/sesrq_bayer_unpack.h) and the one raw route of the package
(sesrq.sensor.route).  Since both libraries instantiate one body, a comparison of one with the other no longer compares two
implementations: here each library alone is held against tests/sensor_oracle.py's numpy restatement of the header and against the
reference's per-code levels (tests/golden/raw), at the smallest shapes that reach every arm of the body, and the launch counters of
both libraries say which library every entry point of the route launches.  Every comparison is exact.

CPU: the two host tables against each other, the oracle and the reference's fixture.  GPU: the oracle comparison, the route."""
import json
import os

import numpy as np
import pytest

import sensor_oracle as SO
from conftest import GOLDEN
from helpers import device, raw_frame, reference_levels, same, sha256, spread_like, stream_ptr
from oracle import sesrq_oracle as O
from test_caller_buffers import RAW_PLACES

RAW = os.path.join(GOLDEN, "raw")
NETS = ("nrdm_3", "nrdm_3_qat")
F32 = np.float32
N, H = 2, 3                                   # both row parities and a frame boundary
WIDTHS = (1, 7, 8, 9, 16, 24)                  # a tail alone, whole 8-pixel segments, segments and a tail
OUTS = ((True, False), (False, True), (True, True))


def _meta(net):
    return json.loads(str(np.load(os.path.join(RAW, net + ".npz"), allow_pickle=False)["meta"]))


# ------------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("net", NETS)
def test_both_host_tables_equal_the_oracle_and_the_reference(net):
    from sesrq import raw as R, sensor as S
    meta = _meta(net)
    s0, z0 = meta["scale"][0], meta["zero"][0]
    lv = reference_levels()
    same("oracle levels", SO.levels(0, 4095), lv)
    for ed in (0, 1, 2):
        t_raw, t_sensor = R.table(s0, z0, ed), S.table(S.Format(), s0, z0, ed)
        same(f"{net} exact_div {ed}: sesrq_raw_table against sesrq_sensor_table", t_raw, t_sensor)
        same(f"{net} exact_div {ed}: against the oracle's quantiser of the reference's levels", t_raw,
             O.quantize_input(lv, s0, z0, reciprocal=ed == 2))
        same(f"{net} exact_div {ed}: against the restatement", t_sensor, SO.q_table(0, 4095, s0, z0, ed))
        if ed != 2:                            # the reference divides: its input.0 of the fixture frames
            for t in (t_raw, t_sensor):
                for f in ("a", "b", "c"):
                    assert sha256(spread_like(raw_frame(f)[0], t, t[0])[None]) == meta["sha"][f"input0_{f}"], (net, ed, f)


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _codes(W):
    """(N, H, W) uint16 with 0, 4095, 4096 and 65535 among seeded 13-bit codes (so some lie above the white level)."""
    c = np.random.default_rng(W).integers(0, 8192, (N, H, W)).astype(np.uint16)
    flat = c.reshape(-1)
    flat[np.linspace(0, flat.size - 1, 4).astype(int)] = (0, 4095, 4096, 65535)
    assert {0, 4095, 4096, 65535} <= set(flat.tolist())
    return c


def _want(codes, s0, z0):
    """(q0, spread) of the restatement, which at this format are the reference's per-code levels at the RGGB sites."""
    lv = SO.levels(0, 4095)
    t = SO.q_table(0, 4095, s0, z0)
    q, sp = SO.spread(codes, t, t[0], "rggb", 0, 4095), SO.spread(codes, lv, F32(0), "rggb", 0, 4095)
    ref = reference_levels()
    tq = O.quantize_input(ref, s0, z0)
    same("q0 of the reference's levels", q, np.stack([spread_like(f, tq, tq[0]) for f in codes]))
    same("the reference's levels", sp, np.stack([spread_like(f, ref, F32(0)) for f in codes]))
    return q, sp


def _at(shape, dtype, offset, fill):
    """A contiguous device tensor whose address is `offset` modulo 256, filled with `fill` (a value, or an array copied in)."""
    import torch
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    pool = torch.empty(n + 512, dtype=torch.uint8, device=device())
    start = -pool.data_ptr() % 256 + offset
    view = pool[start:start + n].view(dtype).reshape(shape)
    assert view.data_ptr() % 256 == offset
    if isinstance(fill, np.ndarray):
        view.copy_(torch.from_numpy(fill))
    else:
        view.fill_(fill)
    return view


def _outputs(shape, outs, q_off=0, sp_off=0):
    import torch
    return (_at(shape, torch.int8, q_off, 0x55) if outs[0] else None, _at(shape, torch.float32, sp_off, float("nan")) if outs[1] else None)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _compare(what, outs, q, sp, want):
    import torch
    torch.cuda.synchronize()
    if outs[0]:
        same(what + " q0", q, want[0])
    if outs[1]:
        same(what + " spread", sp, want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("W", WIDTHS)
def test_libsesrq_sensor_at_the_default_format_equals_the_oracle(W):
    import torch
    from sesrq import sensor as S
    s0, z0 = _meta("nrdm_3")["scale"][0], _meta("nrdm_3")["zero"][0]
    codes = _codes(W)
    want = _want(codes, s0, z0)
    ctx = S.context(device(), S.Format(), s0, z0, 0)
    for offset in (0, 2):                      # the input at a 16-byte address, then at a 2-byte one
        x = _at(codes.shape, torch.uint16, offset, codes)
        for outs in OUTS:
            before = S.instances()
            q, sp = _outputs(want[0].shape, outs)
            rc = S.lib().sesrq_sensor_unpack(ctx, x.data_ptr(), 2 * W, _ptr(q), _ptr(sp), N, H, W, stream_ptr())
            assert rc == 0, S.last_error()
            _compare(f"sensor W={W} input at {offset} outs {outs}", outs, q, sp, want)
            ran = [n for n, c in S.instances().items() if c != before[n]]
            assert len(ran) == 1 and ran[0].startswith("sensor_unpack<u16,table,"), ran


@pytest.mark.gpu
@pytest.mark.parametrize("W", WIDTHS)
def test_libsesrq_raw_equals_the_oracle(W):
    import torch
    from sesrq import raw as R
    s0, z0 = _meta("nrdm_3")["scale"][0], _meta("nrdm_3")["zero"][0]
    codes = _codes(W)
    want = _want(codes, s0, z0)
    ctx = R._so.context(device(), s0, z0, 0)
    for ro, qo, so in RAW_PLACES:              # the (raw, q0, spread) address classes of tests/test_caller_buffers.py
        x = _at(codes.shape, torch.uint16, ro, codes)
        for outs in OUTS:
            before = R.instances()
            q, sp = _outputs(want[0].shape, outs, qo, so)
            rc = R.lib().sesrq_raw_unpack(ctx, x.data_ptr(), _ptr(q), _ptr(sp), N, H, W, stream_ptr())
            assert rc == 0, R.last_error()
            _compare(f"raw W={W} at ({ro}, {qo}, {so}) outs {outs}", outs, q, sp, want)
            assert sum(R.instances().values()) == sum(before.values()) + 1


@pytest.mark.gpu
def test_every_entry_point_launches_the_library_its_fmt_names():
    """fmt=None adds launches to raw_unpack<...> instances only, a Format -- the default one too -- to sensor_unpack<u16,table,...>
    only, and the unpack leaves libsesrq.so's own instance table alone: the guard of sesrq.sensor.route, the one decision point."""
    import sesrq
    import torch
    from calib_cases import calibrators
    from sesrq import _lib, quality, raw as R, sensor as S
    from sesrq.bundle import Bundle
    b = Bundle.load(os.path.join(RAW, "nrdm_3.npz"))
    e = sesrq.Engine(b, device())
    cal = calibrators("nrdm_3")[0]
    rng = np.random.default_rng(48)
    frame = rng.integers(0, 4096, (4, 8)).astype(np.uint16)
    gt16 = rng.integers(0, 4096, (3, 4, 8)).astype(np.uint16)
    x = torch.from_numpy(frame).to(device())

    def evaluate_raw(fmt):                     # the forward, and with it the unpack, is enqueued before the score refuses the size
        with pytest.raises(ValueError, match="smaller than the 7x7 SSIM window"):
            quality.evaluate_raw(e, [frame], [gt16], 3, fmt=fmt)

    entries = {"raw.unpack": lambda fmt: R.unpack(b, x),
               "sensor.unpack": lambda fmt: S.unpack(b, x, fmt),
               "Engine.forward_raw": lambda fmt: e.forward_raw(x, fmt=fmt),
               "Calibrator.enqueue_raw": lambda fmt: cal.enqueue_raw(x, fmt=fmt),
               "quality.evaluate_raw": evaluate_raw}
    for name, call in entries.items():
        for fmt in (None,) if name == "raw.unpack" else (None, S.Format()):
            core, raw_before, sensor_before = _lib.instances(), R.instances(), S.instances()
            call(fmt)
            torch.cuda.synchronize()
            ran_raw = [n for n, c in R.instances().items() if c != raw_before[n]]
            ran_sensor = [n for n, c in S.instances().items() if c != sensor_before[n]]
            what = f"{name} fmt={fmt}"
            if fmt is None:
                assert len(ran_raw) == 1 and ran_raw[0].startswith("raw_unpack<") and not ran_sensor, (what, ran_raw, ran_sensor)
            else:
                assert len(ran_sensor) == 1 and ran_sensor[0].startswith("sensor_unpack<u16,table,") and not ran_raw, (what, ran_raw, ran_sensor)
            after = _lib.instances()
            assert sorted(after) == sorted(core) and not any(n.startswith(("raw_unpack<", "sensor_unpack<")) for n in after), what
            if name.endswith(".unpack"):       # the unpack alone: nothing of libsesrq.so runs
                assert after == core, what
