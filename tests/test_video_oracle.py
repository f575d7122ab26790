"""The video route's restatement (tests/video_oracle.py) anchored outside itself, and the host side of libsesrq_video.so and
sesrq.video (include/sesrq_video.h): no test here needs a device.

  table       sesrq_video_table equals sesrq_image_table (q and x, every code) and the restatement, under three input domains
  decode      a decoded frame equals oracle/'s input quantiser on fl32(v / 255.0), formed here without the table
  luma        the restated Y plane equals the image restatement's export at C = 1, fp32 and int8
  chroma      the Q6 upscale is colour_oracle.upscale of 64 c, and a scalar loop straight from the header gives the same plane and crop
  bicubic     the final chroma bytes against PIL's BICUBIC resize on the interior
  int16       every intermediate of planes of {0, 255} and of random planes lies inside the header's bounds, which are reached
  files       frame_bytes / load_yuv / save_yuv / Surface round trips: odd and even sizes, both formats, multi-frame files, pitches
  ABI         the library exports exactly the header's symbols and links no sibling; every refusal is reached without a device"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import colour_oracle as CO
import image_oracle as IO
import video_oracle as VO

HEADER = os.path.join(ROOT, "include", "sesrq_video.h")
NAMES = sorted(f"video_decode<{o}>" for o in ("q0", "x", "q0,x")) + \
    sorted(f"video_export<{d},r{r},{f}>" for d in ("i8", "f32") for r in (2, 4) for f in ("nv12", "i420"))


def domains():
    """The golden SESR-x4 input domain (tests/golden/sesr_x4.crop.npz), the natural-frame domain of the image fixtures' SESR-x4 net
    and one reciprocal-division domain: (scale_in, zero_in, exact_div)."""
    out = []
    for name in ("sesr_x4.crop.npz", os.path.join("image", "sesr_x4.npz")):
        meta = json.loads(str(np.load(os.path.join(GOLDEN, name), allow_pickle=False)["meta"]))
        out.append((meta["scale"][0], meta["zero"][0], len(out)))
    return out + [(0.0052, -120, 2)]


def test_table_equals_the_image_librarys_and_the_restatement():
    from sesrq import image, video
    for s0, z0, ed in domains():
        q, x = video.table(s0, z0, ed)
        qi, xi = image.table(s0, z0, ed)
        qo, xo = VO.table(s0, z0, ed)
        assert q.dtype == np.int8 and x.dtype == np.float32 and q.shape == x.shape == (256,)
        assert np.array_equal(q, qi) and x.tobytes() == xi.tobytes(), (s0, z0, ed)
        assert np.array_equal(q, qo) and x.tobytes() == xo.tobytes(), (s0, z0, ed)
    assert len({video.table(*d)[0].tobytes() for d in domains()}) == 3
    for s0, z0, ed in ((0.0, -128, 0), (float("nan"), 0, 0), (0.01, -128, 3), (0.01, 1 << 25, 0)):
        with pytest.raises(ValueError, match="sesrq_video_table"):
            video.table(s0, z0, ed)


def test_decoded_frame_equals_the_oracles_quantiser_on_the_float_frame():
    from oracle import sesrq_oracle as O
    from sesrq import video
    rng = np.random.default_rng(2)
    y = np.concatenate([np.arange(256, dtype=np.uint8), rng.integers(0, 256, 3 * 33 * 31 - 256).astype(np.uint8)]).reshape(3, 33, 31)
    x = (y.astype(np.float64) / 255.0).astype(np.float32)[:, None]              # formed without the table
    assert x.min() == 0 and x.max() == 1
    for s0, z0, ed in domains():
        want = O.quantize_input(x, s0, z0, reciprocal=ed == 2)
        q0, xf = VO.decode(y, s0, z0, ed)
        assert q0.dtype == np.int8 and np.array_equal(q0, want) and xf.tobytes() == x.tobytes()
        q, xt = video.table(s0, z0, ed)
        assert np.array_equal(q[y][:, None], want) and xt[y][:, None].tobytes() == x.tobytes()
    assert VO.decode(y)[0] is None


def test_luma_equals_the_image_export_at_one_channel():
    rng = np.random.default_rng(3)
    special = np.array([0x7fc00000, 0xffc00000, 0x7f800000, 0xff800000, 0x80000000, 0, 1, 0x3f800000, 0x3f800001, 0x3f7fffff], np.uint32)
    p = np.concatenate([special.view(np.float32), (np.arange(256) / 255).astype(np.float32), (rng.random(246) * 1.4 - 0.2).astype(np.float32)])
    p = p.reshape(2, 1, 16, 16)
    with np.errstate(invalid="ignore"):
        want = IO.export(np.nan_to_num(p, nan=0.0, posinf=np.inf, neginf=-np.inf))
    assert np.array_equal(VO.luma(p), want[..., 0])
    assert VO.luma(p).reshape(-1)[:4].tolist() == [0, 0, 255, 0]                 # NaN as 0, then +inf, -inf
    q = rng.integers(-128, 128, (2, 1, 16, 16)).astype(np.int8)
    q.reshape(-1)[:256] = np.arange(-128, 128)
    for scale, zero in ((0.0047, -119), (0.0039, -128), (1.0, 0), (1e30, 127)):
        assert np.array_equal(VO.luma(q, scale, zero), IO.export(IO.dequant(q, scale, zero))[..., 0]), (scale, zero)


def _scalar_chroma(c, r, H, W):
    """Step 3 straight from the header, sample by sample, in Python integers."""
    hc, wc = c.shape
    w, first = CO.WEIGHTS[r], CO.FIRST[r]
    h = [[(sum(w[X % r][k] * 64 * int(c[y][min(max(X // r + first[X % r] + k, 0), wc - 1)]) for k in range(4)) + 512) >> 10
          for X in range(r * wc)] for y in range(hc)]
    v = [[(sum(w[Y % r][k] * h[min(max(Y // r + first[Y % r] + k, 0), hc - 1)][X] for k in range(4)) + 512) >> 10
          for X in range(r * W // 2)] for Y in range(r * H // 2)]
    return np.array([[min(max((s + 32) >> 6, 0), 255) for s in row] for row in v], np.uint8).reshape(r * H // 2, r * W // 2)


@pytest.mark.parametrize("r", [2, 4])
def test_chroma_is_the_colour_upscale_of_64c_and_the_headers_crop(r):
    rng = np.random.default_rng(4 + r)
    for H, W in ((1, 1), (3, 5), (5, 3), (6, 8), (9, 14)):
        hc, wc = VO.chroma_size(H, W)
        assert (hc, wc) == (-(-H // 2), -(-W // 2))
        for kind in ("random", "extreme"):
            c = VO.random_frames(rng, 2, H, W, kind)["cb"]
            q6 = VO.chroma_q6(c, r)
            assert np.array_equal(q6, CO.upscale(c.astype(np.int64) * 64, r)) and q6.shape == (2, r * hc, r * wc)
            got = VO.chroma(c, r, H, W)
            assert got.shape == (2, r * H // 2, r * W // 2) and got.dtype == np.uint8
            for n in range(2):
                assert np.array_equal(got[n], _scalar_chroma(c[n], r, H, W)), (H, W, kind, n)
    const = np.full((1, 3, 4), 201, np.uint8)
    assert (VO.chroma(const, r, 6, 8) == 201).all()


@pytest.mark.parametrize("r", [2, 4])
def test_chroma_bytes_against_pil_bicubic(r):
    """PIL's BICUBIC (Keys a = -1/2, half-pixel centres) on the same plane in mode "F", the anchor of the colour library's upscale:
    away from the border (PIL renormalises there, the header replicates) the integer bytes are within 1 of the clipped float plane;
    measured 0.514 at both r.  PIL's 8-bit mode "L" is no anchor: it clamps the HORIZONTAL pass to 0 .. 255, so on random bytes,
    whose first pass overshoots, it lies up to 17 away (measured) from any resize that carries the overshoot into the second pass."""
    Image = pytest.importorskip("PIL.Image")
    H, W = 37, 29
    c = np.random.default_rng(3729).integers(0, 256, (H, W)).astype(np.uint8)
    got = VO.chroma_bytes(VO.chroma_q6(c, r)).astype(np.float64)
    ref = np.clip(np.asarray(Image.fromarray(c.astype(np.float32), mode="F").resize((r * W, r * H), Image.BICUBIC), np.float64), 0, 255)
    inner = (slice(2 * r, r * H - 2 * r), slice(2 * r, r * W - 2 * r))
    err = np.abs(got[inner] - ref[inner]).max()
    print(f"r = {r}: max |integer byte - PIL| = {err:.3f} on the interior")
    assert err <= 1, err


BOUNDS = {4: ((-1912, 18233), (-4273, 20594)), 2: ((-1530, 17850), (-3347, 19667))}      # the header's: (horizontal, vertical)


@pytest.mark.parametrize("r", [2, 4])
def test_intermediates_stay_inside_int16_and_the_headers_bounds(r):
    src = open(HEADER).read()
    for lo, hi in BOUNDS[r]:
        assert f"{lo} .. {hi}" in src, "the header states these bounds"
    rng = np.random.default_rng(16 + r)
    lo, hi = [0, 0], [0, 0]
    planes = [VO.random_frames(rng, 64, 40, 40, kind)["cb"] for kind in ("extreme", "random")]
    # the planes that reach the ends: 255 where row and column are both among the positive taps or both among the negative ones
    # (the maximum), and the complement (the minimum)
    mid = np.zeros(24, bool)
    mid[10:12] = True
    both = mid[:, None] == mid[None, :]
    planes.append(np.stack([both, ~both, np.broadcast_to(mid[None, :], (24, 24)), np.broadcast_to(~mid[None, :], (24, 24))]).astype(np.uint8) * 255)
    for c in planes:
        v, h = VO.chroma_q6(c, r, keep=True)
        for k, a in enumerate((h, v)):
            lo[k], hi[k] = min(lo[k], int(a.min())), max(hi[k], int(a.max()))
    for k in range(2):
        assert BOUNDS[r][k][0] == lo[k] and hi[k] == BOUNDS[r][k][1], (r, k, lo, hi)
        assert -(1 << 15) <= lo[k] and hi[k] < (1 << 15)
    assert max(abs(x) * 1024 * 4 for x in (lo[0], hi[0])) < 1 << 31            # four products of a vertical sum fit int32


# ------------------------------------------------------------------------------------------------------------------------ files
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_files_round_trip(tmp_path, fmt):
    from sesrq import video
    rng = np.random.default_rng(8)
    for N, H, W in ((1, 1, 1), (2, 3, 5), (3, 6, 8), (2, 5, 4), (4, 7, 7)):
        fr = VO.random_frames(rng, N, H, W)
        data = VO.pack(fr, fmt)
        assert video.frame_bytes(fmt, H, W) == VO.frame_bytes(H, W) == len(data) // N
        assert video.chroma_size(H, W) == VO.chroma_size(H, W)
        path = str(tmp_path / f"{N}_{H}_{W}.yuv")
        with open(path, "wb") as f:
            f.write(data)
        s = video.load_yuv(path, W, H, fmt)
        assert (s.N, s.H, s.W, s.fmt_name) == (N, H, W, fmt) and not s.is_torch and s.pitch_y == W
        assert np.array_equal(s.y, fr["y"])
        if fmt == "nv12":
            assert np.array_equal(s.c0[..., 0::2], fr["cb"]) and np.array_equal(s.c0[..., 1::2], fr["cr"]) and s.c1 is None
        else:
            assert np.array_equal(s.c0, fr["cb"]) and np.array_equal(s.c1, fr["cr"])
        assert s.tobytes() == data
        back = VO.unpack(data, fmt, H, W)
        assert all(np.array_equal(back[k], fr[k]) for k in fr)
        out = str(tmp_path / "out.yuv")
        video.save_yuv(out, s)
        assert open(out, "rb").read() == data
        if N > 1:                                     # a part of the sequence, and a file written in two parts
            part = video.load_yuv(path, W, H, fmt, frames=(1, N))
            assert part.N == N - 1 and part.tobytes() == data[len(data) // N:]
            assert video.load_yuv(path, W, H, fmt, frames=(0, 1)).tobytes() == data[:len(data) // N]
            video.save_yuv(out, s[:1])
            video.save_yuv(out, s[1:], append=True)
            assert open(out, "rb").read() == data
            with pytest.raises(ValueError, match="frames"):
                video.load_yuv(path, W, H, fmt, frames=(1, N + 1))
        # the same frames behind pitches: a decoder's surface
        p = video.Surface.alloc(fmt, N, H, W, pitch_y=W + 3, pitch_c=2 * W + 5)
        p.buf[:] = 0xEE
        for dst, srcp in zip(p.planes(), s.planes()):
            dst[...] = srcp
        assert p.pitch_y == W + 3 and p.pitch_c == 2 * W + 5 and p.tobytes() == data
        with open(path, "ab") as f:
            f.write(b"\0")
        with pytest.raises(ValueError, match="whole number"):
            video.load_yuv(path, W, H, fmt)


def test_surface_refusals_without_a_device():
    import torch
    from sesrq import video
    y, c = np.zeros((1, 4, 6), np.uint8), np.zeros((1, 2, 6), np.uint8)
    video.Surface("nv12", 4, 6, y, c)
    with pytest.raises(ValueError, match="pixel format"):
        video.Surface("yv12", 4, 6, y, c)
    with pytest.raises(ValueError, match="i420 has the planes"):
        video.Surface("i420", 4, 6, y, c[..., :3])
    with pytest.raises(ValueError, match="plane c0"):
        video.Surface("nv12", 4, 6, y, c[..., :3])
    with pytest.raises(ValueError, match="uint8"):
        video.Surface("nv12", 4, 6, y.astype(np.int8), c)
    with pytest.raises(ValueError, match="strides"):
        video.Surface("nv12", 4, 6, np.zeros((1, 4, 12), np.uint8)[..., ::2], c)
    with pytest.raises(ValueError, match="one kind"):
        video.Surface("nv12", 4, 6, torch.from_numpy(y), c)
    with pytest.raises(ValueError, match="share one pitch"):
        video.Surface("i420", 4, 6, y, np.zeros((1, 2, 3), np.uint8), np.zeros((1, 2, 4), np.uint8)[..., :3])
    with pytest.raises(ValueError, match="at least 1 x 1"):
        video.frame_bytes("nv12", 0, 4)
    with pytest.raises(ValueError, match="2 or 4"):
        video._factor(3)
    host = video.Surface("nv12", 4, 6, torch.from_numpy(y), torch.from_numpy(c))
    for s in (video.Surface("nv12", 4, 6, y, c), host):
        with pytest.raises(ValueError, match="HIP device"):
            video.decode(None, s, want_q=False, want_f=True)
        with pytest.raises(ValueError, match="HIP device"):
            video.export(torch.zeros((1, 1, 16, 24)), s, 4)
    with pytest.raises(ValueError, match="Surface"):
        video.decode(None, y, want_q=False, want_f=True)
    w, first = video.weights(4)
    assert tuple(map(tuple, w.tolist())) == CO.WEIGHTS[4] and tuple(first.tolist()) == CO.FIRST[4]


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_video_library_exports_exactly_the_header():
    from sesrq import video
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_video[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 9, names
    assert sorted(video.SYMBOLS) == names, "python binding and header disagree"
    nm = subprocess.run(["nm", "-D", "--defined-only", video.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r" T (sesrq\w*)", nm))) == names
    assert (video.TILE_OUT_W, video.TILE_OUT_H) == VO.header_tile() and VO.tile(4) == (32, 8) and VO.tile(2) == (64, 16)
    assert C.sizeof(video.SurfaceDesc) == 64
    ldd = subprocess.run(["readelf", "-d", video.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libsesrq" not in ldd.replace("libsesrq_video.so", ""), "the video library links another library of the project"


def test_other_libraries_instances_unchanged_by_the_video_library():
    from sesrq import _lib, colour, image, video
    assert sorted(video.instances()) == sorted(NAMES)
    assert not any("video" in n for n in list(_lib.instances()) + list(image.instances()) + list(colour.instances()))


def _surf(fmt=0, y=4096, c0=4096, c1=4096, pitch_y=64, pitch_c=64, frame_y=1 << 20, frame_c=1 << 20):
    from sesrq import video
    return video.SurfaceDesc(fmt, y, c0, c1, pitch_y, pitch_c, frame_y, frame_c)


def test_argument_checks_without_a_device():
    """Every refusal comes before any HIP call: the pointers are never dereferenced, no context exists."""
    from sesrq import video
    lib = video.lib()
    launches = sum(video.instances().values())
    fake, odd = C.c_void_p(4096), C.c_void_p(4098)
    ctx = C.c_void_p(4096)              # never dereferenced: the refusals below come before the context is looked at
    S = _surf
    for args, msg in (((None, S(), fake, fake, 1, 8, 8, None), "ctx is NULL"),
                      ((ctx, None, fake, fake, 1, 8, 8, None), "src is NULL"),
                      ((ctx, S(y=None), fake, fake, 1, 8, 8, None), "Y plane of src is NULL"),
                      ((ctx, S(), None, None, 1, 8, 8, None), "neither q0 nor x"),
                      ((ctx, S(), fake, odd, 1, 8, 8, None), "4-byte aligned"),
                      ((ctx, S(), fake, fake, 0, 8, 8, None), "empty frame"),
                      ((ctx, S(), fake, fake, 1, 8, 0, None), "empty frame"),
                      ((ctx, S(pitch_y=7), fake, fake, 1, 8, 8, None), "pitch_y 7 is below the row's 8 bytes"),
                      ((ctx, S(frame_y=-1), fake, fake, 2, 8, 8, None), "frame_y -1 is negative"),
                      ((ctx, S(pitch_y=1 << 20), fake, fake, 1 << 12, 1 << 20, 16, None), "too large"),
                      ((ctx, S(pitch_y=1 << 20), fake, fake, 1 << 10, 1 << 12, 1 << 20, None), "too large")):
        a = list(args)
        a[1] = C.byref(a[1]) if a[1] is not None else None
        assert lib.sesrq_video_decode(*a) != 0 and msg in video.last_error(), (msg, video.last_error())
    assert lib.sesrq_video_create(1.0, 0, 0, None) != 0 and "NULL" in video.last_error()
    h = C.c_void_p()
    assert lib.sesrq_video_create(0.0, 0, 0, C.byref(h)) != 0 and "scale_in" in video.last_error() and not h.value
    lib.sesrq_video_destroy(None)
    nan, inf = float("nan"), float("inf")
    big = dict(pitch_y=1 << 40, pitch_c=1 << 40, frame_y=1 << 62, frame_c=1 << 62)
    for args, msg in (((None, 0, 1.0, 0, S(), 4, S(), 1, 8, 8, None), "y is NULL"),
                      ((fake, 0, 1.0, 0, None, 4, S(), 1, 8, 8, None), "lr is NULL"),
                      ((fake, 0, 1.0, 0, S(), 4, None, 1, 8, 8, None), "out is NULL"),
                      ((fake, 2, 1.0, 0, S(), 4, S(), 1, 8, 8, None), "y_dtype"),
                      ((fake, 1, 0.0, 0, S(), 4, S(), 1, 8, 8, None), "scale"),
                      ((fake, 1, -0.01, 0, S(), 4, S(), 1, 8, 8, None), "scale"),
                      ((fake, 1, nan, 0, S(), 4, S(), 1, 8, 8, None), "scale"),
                      ((fake, 1, inf, 0, S(), 4, S(), 1, 8, 8, None), "scale"),
                      ((fake, 1, 0.01, 128, S(), 4, S(), 1, 8, 8, None), "int8 range"),
                      ((fake, 1, 0.01, -129, S(), 4, S(), 1, 8, 8, None), "int8 range"),
                      ((odd, 0, 1.0, 0, S(), 4, S(), 1, 8, 8, None), "4-byte aligned"),
                      ((fake, 0, 1.0, 0, S(fmt=2), 4, S(), 1, 8, 8, None), "lr format 2"),
                      ((fake, 0, 1.0, 0, S(), 4, S(fmt=-1), 1, 8, 8, None), "out format -1"),
                      ((fake, 0, 1.0, 0, S(), 3, S(), 1, 8, 8, None), "r = 3"),
                      ((fake, 0, 1.0, 0, S(), 1, S(), 1, 8, 8, None), "r = 1"),
                      ((fake, 0, 1.0, 0, S(), 8, S(), 1, 8, 8, None), "r = 8"),
                      ((fake, 0, 1.0, 0, S(), 4, S(), 0, 8, 8, None), "empty frame"),
                      ((fake, 0, 1.0, 0, S(), 4, S(), 1, 8, -1, None), "empty frame"),
                      ((fake, 0, 1.0, 0, S(c0=None), 4, S(), 1, 8, 8, None), "chroma plane of lr is NULL"),
                      ((fake, 0, 1.0, 0, S(fmt=1, c1=None), 4, S(), 1, 8, 8, None), "chroma plane of lr is NULL"),
                      ((fake, 0, 1.0, 0, S(y=None), 4, S(y=None), 1, 8, 8, None), "Y plane of out is NULL"),
                      ((fake, 0, 1.0, 0, S(), 4, S(c0=None), 1, 8, 8, None), "chroma plane of out is NULL"),
                      ((fake, 0, 1.0, 0, S(), 4, S(fmt=1, c1=None), 1, 8, 8, None), "chroma plane of out is NULL"),
                      ((fake, 0, 1.0, 0, S(**big), 4, S(**big), 1 << 20, 1 << 12, 1 << 12, None), "too large"),      # the grid
                      ((fake, 0, 1.0, 0, S(**big), 4, S(**big), 1, 1, 1 << 29, None), "too large"),                  # r W
                      ((fake, 0, 1.0, 0, S(**big), 2, S(**big), 1, 1 << 30, 1, None), "too large"),                  # r H
                      ((fake, 0, 1.0, 0, S(pitch_c=7), 4, S(), 1, 8, 8, None), "pitch_c 7 of lr is below the row's 8 bytes"),
                      ((fake, 0, 1.0, 0, S(fmt=1, pitch_c=4), 4, S(), 1, 8, 9, None), "pitch_c 4 of lr is below the row's 5 bytes"),
                      ((fake, 0, 1.0, 0, S(), 4, S(pitch_y=31), 1, 8, 8, None), "pitch_y 31 of out is below the row's 32 bytes"),
                      ((fake, 0, 1.0, 0, S(), 4, S(pitch_c=31), 1, 8, 8, None), "pitch_c 31 of out is below the row's 32 bytes"),
                      ((fake, 0, 1.0, 0, S(), 4, S(fmt=1, pitch_c=15), 1, 8, 8, None), "pitch_c 15 of out is below the row's 16 bytes"),
                      ((fake, 0, 1.0, 0, S(frame_c=-1), 4, S(), 2, 8, 8, None), "frame_c -1 of lr is negative"),
                      ((fake, 0, 1.0, 0, S(), 4, S(frame_y=31 * 64 + 31), 2, 8, 8, None), "below its plane's extent"),
                      ((fake, 0, 1.0, 0, S(), 4, S(frame_c=15 * 64 + 31), 2, 8, 8, None), "below its plane's extent")):
        a = list(args)
        for k in (4, 6):
            a[k] = C.byref(a[k]) if a[k] is not None else None
        assert lib.sesrq_video_export(*a) != 0 and msg in video.last_error(), (msg, video.last_error())
    assert lib.sesrq_video_instance_count() == len(NAMES)
    assert lib.sesrq_video_instance_name(len(NAMES)) is None and lib.sesrq_video_instance_launches(-1) == -1
    assert sum(video.instances().values()) == launches, "a refused call launched a kernel"
