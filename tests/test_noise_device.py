"""tests/noise_device.py, the chunked torch restatement of include/sesrq_noise.h, pinned to tests/noise_oracle.py before
tests/test_noise_limits.py relies on it: on the CPU, and again with its tensors on the device (another build of every torch kernel
it calls).  On the frames of test_noise.SHAPES and on test_sensor.every_code_frame(): words equal, float64 deviates within 1e-12,
fp32 frame and q0 bit-equal for exact_div 0 and 2 and both DOMAINS, through boxes small enough that every frame is cut by frames, by
rows and by columns.  A comparator that cannot fail proves nothing, so each case also plants one wrong word in each output and
expects exactly that coordinate back.

On an MI355X (torch 2.10 for ROCm 7.0) every step is bit-equal as written, subnormal results included: none had to be replaced."""
import numpy as np
import pytest

import noise_device as ND
import noise_oracle as NO
import sensor_oracle as SO
from test_noise import DOMAINS, SEED, SHAPES, WHITE, _codes
from test_sensor import every_code_frame

F32 = np.float32
T_ROUND = 2.0 ** -22          # |z| < 8: rounding a float64 deviate to fp32 moves it by at most half an ulp of [4, 8)
CASES = [(p, nhw, 3 if i else 2 ** 32 - 2, 16 if nhw[1] * nhw[2] < 4096 else 1 << 14) for i, (p, nhw, _) in enumerate(SHAPES)]
DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="device", marks=pytest.mark.gpu)]


def _device(kind):
    import torch
    if kind == "cpu":
        return torch.device("cpu")
    from helpers import device
    return device()


def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(dev)


def _pin(dev, codes, cfa, black, white, frame0, px, domains=DOMAINS):
    import torch
    N, H, W = codes.shape
    boxes = ND.chunks(N, H, W, px)
    assert sum((b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4]) for b in boxes) == N * H * W
    frames = [(frame0 + n) % 2 ** 64 for n in range(N)]
    # words, whole and through the boxes
    w = ND.words(SEED, frames, 0, H, 0, W, dev)
    for n in range(N):
        want = NO.words(SEED, frames[n], H, W)
        for k in range(4):
            assert np.array_equal(w[k][n].cpu().numpy().astype(np.uint64), np.broadcast_to(want[k], (H, W))), (n, k)
    n0, n1, r0, r1, x0, x1 = boxes[-1]
    wb = ND.words(SEED, frames[n0:n1], r0, r1, x0, x1, dev)
    assert all(torch.equal(wb[k], w[k][n0:n1, r0:r1, x0:x1]) for k in range(4))
    # deviates
    z64 = NO.deviates(SEED, frame0, N, H, W)
    err = float(np.abs(ND.deviates(w).cpu().numpy() - z64).max())
    assert err <= 1e-12, err
    # the exact part, on fp32 deviates standing in for the device's
    z32 = z64.astype(F32)
    zt, ct = _t(z32, dev), ND.Dense(_t(codes.astype(np.int32), dev))
    levels = (0.01, 0.0005) if N == 1 else np.array([[0.003 * (n + 1), 1e-5 * (n + 1)] for n in range(N)], F32)
    for ed in (0, 2):
        for s0, z0 in domains:
            want_sp, want_q = NO.frame(codes, cfa, black, white, levels, z32, s0, z0, ed)
            kw = dict(seed=SEED, frame0=frame0, tol=T_ROUND, cfa=cfa, black=black, white=white, levels=levels, s0=s0, z0=z0,
                      exact_div=ed, boxes=boxes)
            sp, q = _t(want_sp, dev), _t(want_q, dev)
            rep = ND.compare(ct, N, H, W, zt, spread=sp, q0=q, **kw)
            rep.clean(f"{codes.shape} exact_div {ed} z0 {z0}")
            assert rep.compared == {"z": 3 * N * H * W, "z_range": 3 * N * H * W, "spread": 3 * N * H * W, "q0": 3 * N * H * W}
    # one wrong word in each output comes back, with its coordinate
    at = (N - 1, 2, H - 1, W // 2)
    sp.view(torch.int32)[at] ^= 1
    q[at] = q[at] + 1 if int(q[at]) < 127 else -128
    zbad = zt.clone()
    zbad[at] = zbad[at] + 4 * T_ROUND
    rep = ND.compare(ct, N, H, W, zbad, spread=sp, q0=q, **kw)
    assert rep.bad["z"] == 1 and rep.first["z"][0][0] == at, rep
    # the planted deviate moves the expected frame at that pixel too: the planted output words are compared with another value
    assert rep.bad["spread"] <= 1 and rep.bad["q0"] <= 1
    rep = ND.compare(ct, N, H, W, zt, spread=sp, q0=q, **kw)
    assert rep.bad == {"z": 0, "z_range": 0, "spread": 1, "q0": 1}, rep
    assert rep.first["spread"][0][0] == at and rep.first["q0"][0][0] == at, rep
    assert rep.z_err <= T_ROUND and rep.z_at is not None


@pytest.mark.parametrize("kind", DEVICES)
@pytest.mark.parametrize("packing,nhw,frame0,px", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in CASES])
def test_the_restatement_is_the_oracle_on_the_small_frames(kind, packing, nhw, frame0, px):
    cfa = ("rggb", "grbg", "gbrg", "bggr")[(nhw[1] + nhw[2]) % 4]
    _pin(_device(kind), _codes(packing, nhw), cfa, 16, WHITE[packing], frame0, px)


@pytest.mark.parametrize("kind", DEVICES)
@pytest.mark.parametrize("cfa,levels", [("grbg", (64, 1023)), ("bggr", (4096, 65535))])
def test_the_restatement_is_the_oracle_on_every_code(kind, cfa, levels):
    _pin(_device(kind), every_code_frame()[None], cfa, *levels, 5, 1 << 16)


@pytest.mark.parametrize("kind", DEVICES)
def test_pack_and_tiled_frames(kind):
    """pack is tests/sensor_oracle.py's byte layout; a Tiled frame is its tile repeated; build_raw lays the boxes side by side and
    leaves the pad byte behind every row."""
    dev = _device(kind)
    rng = np.random.default_rng(3)
    tile = rng.integers(0, 1024, (3, 6, 8))
    N, H, W = 5, 15, 44
    big = tile[np.arange(N) % 3][:, np.arange(H) % 6][:, :, np.arange(W) % 8]
    t = ND.Tiled(_t(tile.astype(np.int32), dev))
    assert np.array_equal(t(0, N, 0, H, 0, W).cpu().numpy(), big)
    assert np.array_equal(t(3, 5, 7, 9, 4, 40).cpu().numpy(), big[3:5, 7:9, 4:40])
    for packing in ("u16", "raw10", "raw12"):
        assert np.array_equal(ND.pack(_t(big, dev), packing).cpu().numpy(), SO.pack_rows(big, packing))
        nb = ND.row_bytes(packing, W)
        old = ND.CHUNK_PX
        for px in (old, 64, 16):          # whole frames, whole rows, parts of a row
            ND.CHUNK_PX = px
            try:
                raw = ND.build_raw(t, N, H, W, packing, nb + 5, 0xEE, dev).cpu().numpy()
            finally:
                ND.CHUNK_PX = old
            assert np.array_equal(raw, SO.pack_rows(big, packing, nb + 5, 0xEE)), (packing, px)


def test_chunks_tile_the_frame_within_their_size():
    for N, H, W, px in ((1, 1, 1, 16), (5, 3, 2, 16), (2, 7, 5, 16), (2, 3, 37, 16), (1048577, 2, 8, 1 << 21), (1, 1, (1 << 24) - 8, 1 << 21),
                        (1, (1 << 24) - 2, 2, 1 << 21), (3, 10924, 10928, 1 << 21)):
        boxes = ND.chunks(N, H, W, px)
        assert all((b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4]) <= max(px, 1) for b in boxes)
        assert all(b[4] % 2 == 0 for b in boxes)
        assert sum((b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4]) for b in boxes) == N * H * W
        assert boxes[0][0] == 0 and boxes[-1][1] == N and boxes[-1][3] == H and boxes[-1][5] == W
