"""Predictions out at any size (sesrq.resize, libsesrq_resize.so, Engine.forward_resized) against Pillow itself: every comparison is
exact against PIL.Image.resize((Wo, Ho), Image.BICUBIC) of the bytes image.export writes.  Sizes are (rows, columns)."""
import ctypes as C
import os

import numpy as np
import pytest

pytest.importorskip("PIL")
from PIL import Image

from conftest import GOLDEN
from helpers import Arena, device, same, stream_ptr
from sesrq import resize

gpu = pytest.mark.gpu
TILE_W = {1: 192, 3: 64}                     # output pixels of a tile row (csrc/sesrq_resize.hip: 192 bytes)
TILE_H = {"x1.5": 64, "/1.33": 32}           # output rows of a tile: the tallest whose source window fits 80 LDS rows
RATIO = {"x1.5": 2 / 3, "/1.33": 4 / 3}      # n_in / n_out
DOMAINS = ((1 / 255, -128), (0.0052, -7))    # int8 output domains: the whole byte range; both clips reached
PAIRS = [((40, 70), (60, 105)), ((90, 120), (67, 91)), ((33, 31), (77, 13)), ((16, 16), (16, 24)), ((64, 64), (16, 16)),
         ((63, 63), (16, 16)), ((5, 6), (37, 44)), ((1, 1), (5, 7)), ((4, 3), (1, 1))]


def pillow(img, Ho, Wo):
    """(N, H, W, C) uint8 -> (N, Ho, Wo, C): Pillow's bicubic resize of every frame."""
    return np.stack([np.asarray(Image.fromarray(f[..., 0] if f.shape[2] == 1 else f).resize((Wo, Ho), Image.BICUBIC)).reshape(Ho, Wo, -1)
                     for f in img])


def frames(rng, N, H, W, Ch):
    """Random bytes above, {0, 255} bytes below: both clamps of both passes fire."""
    f = rng.integers(0, 256, (N, H, W, Ch), dtype=np.uint8)
    f[:, H // 2:] = rng.integers(0, 2, f[:, H // 2:].shape, dtype=np.uint8) * 255
    return f


def pred_bytes(p):
    """image.export's byte of an fp32 prediction (N, C, H, W), interleaved: trunc(fl32(clip(p, 0, 1) * 255)), a NaN gives 0."""
    return (np.fmin(np.fmax(p, np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------------------- no device
@pytest.mark.parametrize("n_in,n_out", [(37, 29), (64, 96), (33, 77), (8, 3), (4, 1), (1, 5)])
def test_tables_reproduce_pillows_row(n_in, n_out):
    xmin, cnt, w = resize.coeffs(n_in, n_out)
    row = frames(np.random.default_rng(n_in), 1, 2, n_in, 1)[0, 1:]                      # (1, n_in, 1): {0, 255} bytes
    row = np.concatenate([row, np.random.default_rng(n_out).integers(0, 256, row.shape, dtype=np.uint8)])
    got = np.empty((2, n_out), np.uint8)
    for i in range(n_out):
        taps = row[:, xmin[i]:xmin[i] + cnt[i], 0].astype(np.int64)
        got[:, i] = np.clip(((1 << 21) + taps @ w[i, :cnt[i]].astype(np.int64)) >> 22, 0, 255)
        assert 255 * np.abs(w[i]).astype(np.int64).sum() + (1 << 21) < 1 << 31 and not w[i, cnt[i]:].any()
    same(f"{n_in} -> {n_out}", got, pillow(row[None], 2, n_out)[0, :, :, 0])


def test_equal_sizes_give_the_identity_table():
    xmin, cnt, w = resize.coeffs(7, 7)
    for i in range(7):
        assert w[i, i - xmin[i]] == 1 << 22 and np.count_nonzero(w[i]) == 1 and xmin[i] <= i < xmin[i] + cnt[i]


def test_refusals_through_the_c_abi_without_a_device():
    """Pointers that are never dereferenced: every refusal comes before any HIP call.  (A context of another size needs a device to
    exist: test_caller_buffers_and_a_context_of_another_size.)"""
    lib, h, fake = resize.lib(), C.c_void_p(), 4096
    assert len(resize.coeffs(8, 2)[0]) == 2
    for args, msg in (((9, 2), "ratio above 4"), ((0, 2), "at least 1"), ((2, 0), "at least 1")):
        with pytest.raises(ValueError, match=msg):
            resize.coeffs(*args)
    for args, msg in (((9, 8, 2, 8), "height 9 -> 2 is a downscale ratio above 4"), ((8, 9, 8, 2), "width 9 -> 2"), ((0, 8, 2, 2), "at least 1"),
                      ((8, 8, 2, 0), "at least 1")):
        assert lib.sesrq_resize_create(*args, C.byref(h)) != 0 and msg in resize.last_error(), (args, resize.last_error())
    run = lambda ctx=fake, src=fake, dt=0, s=1.0, z=0, Ch=3, o=0, out=fake, N=1: lib.sesrq_resize_run(ctx, src, dt, s, z, Ch, o, out, N, 8, 8, 4, 4, None)
    for kw, msg in ((dict(ctx=None), "ctx is NULL"), (dict(src=None), "src is NULL"), (dict(out=None), "out is NULL"), (dict(dt=3), "src_dtype 3"),
                    (dict(dt=2, s=0.0), "positive, finite"), (dict(dt=2, z=128), "zero 128"), (dict(dt=1, src=4098), "4-byte aligned"),
                    (dict(Ch=2), "2 channels"), (dict(o=2), "order 2"), (dict(N=0), "empty batch")):
        assert run(**kw) != 0 and msg in resize.last_error(), (kw, resize.last_error())


# ------------------------------------------------------------------------------------------------------------------- device
def _check(src, want, order="rgb", **kw):
    """One launch of its instantiation -> every byte equals `want` (N, Ho, Wo, C), reversed along C for "bgr"."""
    import torch
    N, Ho, Wo, Ch = want.shape
    t = torch.from_numpy(np.ascontiguousarray(src)).to(device())
    H, W = (t.shape[1], t.shape[2]) if t.dtype == torch.uint8 else (t.shape[2], t.shape[3])
    before = resize.instances()
    got = resize.run(resize.plan(H, W, Ho, Wo, device()), t, order=order, **kw)
    torch.cuda.synchronize()
    after = resize.instances()
    name = f"resize<{ {torch.uint8: 'u8', torch.float32: 'f32', torch.int8: 'i8'}[t.dtype]},C{Ch}>"
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}
    same(f"{name} {N} x {H} x {W} -> {Ho} x {Wo} {order}", got, want[..., ::-1] if order == "bgr" else want)


@gpu
@pytest.mark.parametrize("Ch", [1, 3])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_uint8_images_equal_pillow(pair, Ch):
    (H, W), (Ho, Wo) = pair
    src = frames(np.random.default_rng(H * W + Ch), 3, H, W, Ch)
    want = pillow(src, Ho, Wo)
    for order in ("rgb", "bgr"):
        _check(src, want, order)
        _check(src[:1], want[:1], order)


@gpu
@pytest.mark.parametrize("Ch", [1, 3])
@pytest.mark.parametrize("ratio", list(RATIO))
def test_sizes_on_the_tile_seams(ratio, Ch):
    tw, th, s = TILE_W[Ch], TILE_H[ratio], RATIO[ratio]
    rng = np.random.default_rng(Ch)
    assert resize.plan(round(4 * th * s), 8, 4 * th, 8, device()).tile == (192, th)
    # a frame shorter than two tiles of 32 rows fits one of 64 at / 1.33: the seams at 2 th are the ones that exist there
    for Ho, Wo in [(9, w) for w in (tw - 1, tw, tw + 1, 2 * tw + 1)] + [(h, 9) for h in (th - 1, th, th + 1, 2 * th - 1, 2 * th, 2 * th + 1)]:
        src = frames(rng, 2, round(Ho * s), round(Wo * s), Ch)
        _check(src, pillow(src, Ho, Wo))


@gpu
@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[1]], ids=["up", "down"])
@pytest.mark.parametrize("kind", ["i8-a", "i8-b", "f32"])
def test_predictions_equal_pillow_on_the_exported_bytes(kind, pair):
    (H, W), (Ho, Wo) = pair
    rng = np.random.default_rng(H)
    for Ch in (1, 3):
        if kind == "f32":
            p = rng.uniform(-0.3, 1.3, (2, Ch, H, W)).astype(np.float32)
            p.reshape(-1)[:7] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 255.5]
            _check(p, pillow(pred_bytes(p), Ho, Wo))
        else:
            s, z = DOMAINS[kind == "i8-b"]
            q = rng.permutation(np.resize(np.arange(-128, 128, dtype=np.int8), 2 * Ch * H * W)).reshape(2, Ch, H, W)      # all 256 codes
            p = (q.astype(np.int32) - z).astype(np.float32) * np.float32(s)
            _check(q, pillow(pred_bytes(p), Ho, Wo), scale=s, zero=z)


@gpu
@pytest.mark.parametrize("kind", ["u8", "i8", "f32"])
def test_caller_buffers_and_a_context_of_another_size(kind):
    """src and out at odd addresses (fp32: 4 mod 16) inside canary arenas, through the C ABI; Wo * C = 207 has whole 16-byte runs that
    are aligned in some rows only."""
    import torch
    (H, W), (Ho, Wo), Ch, N = (40, 70), (27, 69), 3, 2
    rng = np.random.default_rng(3)
    if kind == "u8":
        src = frames(rng, N, H, W, Ch)
        want = pillow(src, Ho, Wo)
    else:
        src = rng.uniform(-0.2, 1.2, (N, Ch, H, W)).astype(np.float32) if kind == "f32" else rng.integers(-128, 128, (N, Ch, H, W), dtype=np.int8)
        want = pillow(pred_bytes(src if kind == "f32" else (src.astype(np.int32) + 128).astype(np.float32) * np.float32(1 / 255)), Ho, Wo)
    t = torch.from_numpy(src)
    arena = Arena(device(), Arena.room(t.numel() * t.element_size(), want.size), 0xA5)
    d_src = arena.place(t.shape, t.dtype, 4 if kind == "f32" else 3, fill=t)
    d_out = arena.place(want.shape, torch.uint8, 5)
    p, dt = resize.plan(H, W, Ho, Wo, device()), {"u8": resize.U8, "f32": resize.F32, "i8": resize.I8}[kind]
    run = lambda *size: resize.lib().sesrq_resize_run(p.handle, d_src.data_ptr(), dt, 1 / 255, -128, Ch, 0, d_out.data_ptr(), N, *size, stream_ptr())
    for size in ((H, W, Ho, Wo + 1), (W, H, Ho, Wo)):
        assert run(*size) != 0 and "the context resizes 40 x 70 -> 27 x 69" in resize.last_error()
    assert run(H, W, Ho, Wo) == 0, resize.last_error()
    torch.cuda.synchronize()
    same(kind, d_out, want)
    same(kind + " src untouched", d_src, src)
    assert not arena.check(), arena.check()[:4]


@gpu
@pytest.mark.parametrize("net,anchor", [("sesr_x4", False), ("sesr_x2_rand", True), ("sesr_x2_rand", False)])
def test_forward_resized_equals_pillow_on_the_exported_image(net, anchor):
    import sesrq
    import torch
    from sesrq import image
    from sesrq.bundle import Bundle
    b = Bundle.load(os.path.join(GOLDEN, "image", net + ".npz"))
    e = sesrq.Engine(b, device(), anchor_add=anchor)
    lr = torch.from_numpy(np.load(os.path.join(GOLDEN, "image", "frames.npz"), allow_pickle=False)["lr_a"]).to(device())[None]
    q, y = e.forward_image(lr)
    full = image.export(y) if anchor else image.export(q, scale=b.scale[b.L], zero=b.zero[b.L])
    for order, (Ho, Wo) in (("rgb", (130, 200)), ("bgr", (54, 300))):
        got = e.forward_resized(lr.flip(-1) if order == "bgr" else lr, (Ho, Wo), order=order)
        torch.cuda.synchronize()
        want = pillow(full.cpu().numpy(), Ho, Wo)
        same(f"{net} {order}", got, want[..., ::-1] if order == "bgr" else want)
    out = torch.empty((1, 54, 300, b.out_channels), dtype=torch.uint8, device=device())
    assert e.forward_resized(lr, (54, 300), out=out) is out
    with pytest.raises(ValueError, match="output shape"):
        e.forward_resized(lr, (54, 301), out=out)
    with pytest.raises(ValueError, match="ratio above 4"):
        e.forward_resized(lr, (5, 300))


@gpu
def test_zz_every_instantiation_ran():
    """Last in the module: every instantiation the library lists has been launched by the tests above."""
    inst = resize.instances()
    assert sorted(inst) == sorted(f"resize<{s},C{c}>" for s in ("u8", "f32", "i8") for c in (1, 3))
    assert all(n > 0 for n in inst.values()), inst
