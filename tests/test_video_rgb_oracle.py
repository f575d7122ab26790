"""The RGB video route's restatement (tests/video_rgb_oracle.py) anchored outside itself, and the host side of libsesrq_video_rgb.so
and sesrq.video_rgb (include/sesrq_video_rgb.h): no test here needs a device.

  facts       over all 2^24 byte triples: the integer luma against rint of sesrq_image.h's float64 line (120 differences, all among
              the 194 exact ties), the one-pixel Cb and Cr forms against rint of sesrq_colour.h's float64 lines (0 of 0 ties, 6 of 12),
              and forward-then-decode (within 2 per channel, 99.65 % within 1, 15.9 % exact) -- as the header states them
  constant    the decode of a constant-colour surface is the inverse matrix of its bytes (the bicubic weights sum to 1024)
  chroma      the upscaled chroma is video_oracle.export's r = 2 chroma before its >> 6
  decode      the decoded q0 / x are the image restatement's decode of the restated RGB bytes
  export      the export's bytes are the image restatement's export followed by a scalar loop straight from the header
  bounds      the intermediates of D1 stay inside the header's bounds
  ABI         the table equals sesrq_image_table; the library exports exactly the header's symbols and links no sibling; every
              refusal is reached through the C ABI on pointers that are never dereferenced"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import colour_oracle as CO
import image_oracle as IO
import video_oracle as VO
import video_rgb_oracle as RO

F32 = np.float32
HEADER = os.path.join(ROOT, "include", "sesrq_video_rgb.h")
NAMES = sorted([f"vrgb_decode<{f},{o}>" for f in ("nv12", "i420") for o in ("q0", "x", "q0,x")] +
               [f"vrgb_export<{d},{f}>" for d in ("f32", "i8") for f in ("nv12", "i420")])
DOMAINS = ((0.0039, -128, 0), (0.0047, -119, 1), (0.0052, -120, 2))


@pytest.fixture(scope="module")
def triples():
    """Every byte triple (2^24, 3) int64, R slowest."""
    v = np.arange(256, dtype=np.int64)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)


def _one_pixel(rgb):
    """E2 and the one-pixel forms of E3 on (n, 3) triples -> (Y, Cb, Cr) int64."""
    cb = (2 * RO.chroma_term(rgb, RO.KCB) + 65535000) // 510000
    cr = (2 * RO.chroma_term(rgb, RO.KCR) + 65535000) // 510000
    return RO.luma_of(rgb), cb, cr


def test_integer_forms_against_the_float64_lines_over_all_triples(triples):
    src = re.sub(r"\s*\*\s*", " ", open(HEADER).read())
    for fact in ("differs from rint of sesrq_image.h's float64 line at 120 triples, all among the 194 exact ties",
                 "never differs from rint of the float64 cb (there are 0 ties)", "form differs at 6 of 12 ties"):
        assert fact in src, f"the header states: {fact}"
    d = triples.astype(np.float64) / 255.0
    Y, cb, cr = _one_pixel(triples)
    yf = np.rint(65.481 * d[:, 0] + 128.553 * d[:, 1] + 24.966 * d[:, 2] + 16.0).astype(np.int64)       # sesrq_image.h's line, x 255
    ties = (RO.chroma_term(triples, RO.KY) + 4207500) % 255000 == 0                                      # exact: the fraction is 1/2
    diff = yf != Y
    assert (int(diff.sum()), int(ties.sum()), int((diff & ~ties).sum())) == (120, 194, 0)
    assert (Y[diff] == yf[diff] + 1).all(), "the integer form rounds half up, rint to even"
    assert (Y.min(), Y.max()) == (16, 235)
    for got, k, c, want in ((cb, RO.KCB, (-37.797, -74.203, 112.0), (0, 0)), (cr, RO.KCR, (112.0, -93.786, -18.214), (6, 12))):
        f = np.rint(((c[0] * d[:, 0] + c[1] * d[:, 1]) + c[2] * d[:, 2]) + 128.0).astype(np.int64)          # sesrq_colour.h step 1, / 64
        t = (2 * RO.chroma_term(triples, k) + 65535000) % 510000 == 0
        assert (int((got != f).sum()), int(t.sum()), int(((got != f) & ~t).sum())) == (want[0], want[1], 0)
        assert (got.min(), got.max()) == (16, 240)
    # the 2 x 2 form on a constant block is the one-pixel form, and its numerator stays positive and below 2^31
    for k in (RO.KCB, RO.KCR):
        S = 4 * RO.chroma_term(triples, k)
        assert np.array_equal((2 * S + 262140000) // 2040000, (2 * RO.chroma_term(triples, k) + 65535000) // 510000)
        assert (2 * S + 262140000).min() > 0 and (2 * S + 262140000).max() < 1 << 31
    assert 65481 * 255 + 128553 * 255 + 24966 * 255 + 4207500 < 1 << 31


def test_forward_then_decode_returns_every_triple_within_two(triples):
    src = re.sub(r"\s*\*\s*", " ", open(HEADER).read())
    assert "within 2 per channel: 99.65 % within 1, 15.9 % exact" in src
    Y, cb, cr = _one_pixel(triples)
    back = np.stack(CO.to_rgb(Y.astype(F32), 64 * cb, 64 * cr), -1).astype(np.int64)
    err = np.abs(back - triples).max(-1)
    assert err.max() == 2
    assert round(100 * float((err <= 1).mean()), 2) == 99.65 and round(100 * float((err == 0).mean()), 1) == 15.9


def _inverse(y, cb, cr):
    """Step 4 of sesrq_colour.h on bytes, scalar, in np.float32 operations."""
    a = F32(1.16438356) * (F32(y) - F32(16.0))
    cbf, crf = F32(64 * cb - 8192) * F32(0.015625), F32(64 * cr - 8192) * F32(0.015625)
    v = (a + F32(1.59602679) * crf, (a - F32(0.39176229) * cbf) - F32(0.81296765) * crf, a + F32(2.01723214) * cbf)
    return [int(min(max(np.rint(t), 0), 255)) for t in v]


def test_constant_colour_surface_decodes_to_the_inverse_matrix_of_its_bytes():
    for r in (2, 4):
        assert all(sum(w) == 1024 for w in CO.WEIGHTS[r])
    rng = np.random.default_rng(1)
    for y, cb, cr in [(16, 128, 128), (235, 128, 128), (0, 0, 0), (255, 255, 255), (16, 240, 16), (235, 16, 240), (81, 90, 240)] + \
            [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(20)]:
        H, W = 5, 7
        hc, wc = VO.chroma_size(H, W)
        fr = {"y": np.full((1, H, W), y, np.uint8), "cb": np.full((1, hc, wc), cb, np.uint8), "cr": np.full((1, hc, wc), cr, np.uint8)}
        assert (RO.chroma444(fr["cb"], H, W) == 64 * cb).all()
        img = RO.rgb_bytes(fr)
        assert img.shape == (1, H, W, 3) and (img == np.array(_inverse(y, cb, cr), np.uint8)).all(), (y, cb, cr)
    assert _inverse(16, 128, 128) == [0, 0, 0] and _inverse(235, 128, 128) == [255, 255, 255]


def test_upscaled_chroma_is_the_video_exports_r2_chroma_before_its_shift():
    rng = np.random.default_rng(2)
    for H, W in ((1, 1), (2, 2), (3, 5), (6, 8), (9, 14), (33, 31)):
        for kind in ("random", "extreme"):
            fr = VO.random_frames(rng, 2, H, W, kind)
            hc, wc = VO.chroma_size(H, W)
            q6 = RO.chroma444(fr["cb"], H, W)
            assert q6.shape == (2, H, W)
            full = CO.upscale(fr["cb"].astype(np.int64) * 64, 2)
            assert full.shape == (2, 2 * hc, 2 * wc) and np.array_equal(q6, full[..., :H, :W])
            # the video export at r = 2 of the chroma planes as the LR planes of a 2 hc x 2 wc ... frame: its bytes are (C + 32) >> 6
            want = VO.chroma(fr["cb"], 2, 2 * hc, 2 * wc)
            assert np.array_equal(VO.chroma_bytes(full)[..., :2 * hc, :2 * wc], want)
            assert np.array_equal(np.clip((q6 + 32) >> 6, 0, 255), want[..., :H, :W])


def test_decode_is_the_image_decode_of_the_restated_rgb_bytes():
    rng = np.random.default_rng(3)
    for H, W in ((1, 1), (3, 5), (8, 6), (17, 33)):
        fr = VO.random_frames(rng, 2, H, W)
        img = RO.rgb_bytes(fr)
        assert img.dtype == np.uint8 and img.shape == (2, H, W, 3)
        # D2 pixel by pixel, scalar, from the Q6 planes
        cb, cr = RO.chroma444(fr["cb"], H, W), RO.chroma444(fr["cr"], H, W)
        for n, yy, xx in ((0, 0, 0), (1, H - 1, W - 1), (0, H // 2, W // 2)):
            a = F32(1.16438356) * (F32(fr["y"][n, yy, xx]) - F32(16.0))
            cbf, crf = F32(cb[n, yy, xx] - 8192) * F32(0.015625), F32(cr[n, yy, xx] - 8192) * F32(0.015625)
            v = (a + F32(1.59602679) * crf, (a - F32(0.39176229) * cbf) - F32(0.81296765) * crf, a + F32(2.01723214) * cbf)
            assert img[n, yy, xx].tolist() == [int(min(max(np.rint(t), 0), 255)) for t in v]
        for s0, z0, ed in DOMAINS:
            q0, x = RO.decode(fr, s0, z0, ed)
            assert q0.shape == x.shape == (2, 3, H, W) and q0.dtype == np.int8 and x.dtype == F32
            assert x.tobytes() == IO.decode(img, "rgb").tobytes() and np.array_equal(q0, IO.q0(IO.decode(img, "rgb"), s0, z0, ed))
            tq, tx = VO.table(s0, z0, ed)
            planes = img.transpose(0, 3, 1, 2)
            assert np.array_equal(q0, tq[planes]) and x.tobytes() == tx[planes].tobytes()
        assert RO.decode(fr)[0] is None


def _scalar_export(img):
    """E2 and E3 straight from the header, pixel by pixel, in Python integers."""
    N, H, W, _ = img.shape
    hc, wc = (H + 1) // 2, (W + 1) // 2
    out = {"y": np.zeros((N, H, W), np.uint8), "cb": np.zeros((N, hc, wc), np.uint8), "cr": np.zeros((N, hc, wc), np.uint8)}
    for n in range(N):
        for y in range(H):
            for x in range(W):
                R, G, B = (int(v) for v in img[n, y, x])
                out["y"][n, y, x] = (65481 * R + 128553 * G + 24966 * B + 4207500) // 255000
        for i in range(hc):
            for j in range(wc):
                sb = sr = 0
                for dy in range(2):
                    for dx in range(2):
                        R, G, B = (int(v) for v in img[n, min(2 * i + dy, H - 1), min(2 * j + dx, W - 1)])
                        sb += -37797 * R - 74203 * G + 112000 * B
                        sr += 112000 * R - 93786 * G - 18214 * B
                out["cb"][n, i, j] = (2 * sb + 262140000) // 2040000
                out["cr"][n, i, j] = (2 * sr + 262140000) // 2040000
    return out


def test_export_is_the_image_export_then_the_headers_integers():
    rng = np.random.default_rng(4)
    special = np.array([0x7fc00000, 0xffc00000, 0x7f800000, 0xff800000, 0x80000000, 0, 1, 0x3f800000, 0x3f800001, 0x3f7fffff], np.uint32).view(F32)
    for H, W in ((1, 1), (2, 2), (3, 5), (4, 7), (6, 4)):
        p = (rng.random((2, 3, H, W)) * 1.3 - 0.15).astype(F32)
        p.reshape(-1)[:min(p.size, len(special))] = special[:min(p.size, len(special))]
        with np.errstate(invalid="ignore"):
            img = IO.export(np.nan_to_num(p, nan=0.0, posinf=np.inf, neginf=-np.inf))
        got, want = RO.export(p), _scalar_export(img)
        assert got["cb"].shape == (2, (H + 1) // 2, (W + 1) // 2)
        assert all(np.array_equal(got[k], want[k]) and got[k].dtype == np.uint8 for k in want), (H, W)
        q = rng.integers(-128, 128, (2, 3, H, W)).astype(np.int8)
        for scale, zero in ((0.0047, -119), (1.0, 0), (1e30, 127)):
            got, want = RO.export(q, scale, zero), _scalar_export(IO.export(IO.dequant(q, scale, zero)))
            assert all(np.array_equal(got[k], want[k]) for k in want), (H, W, scale, zero)
    assert RO.export(np.full((1, 3, 2, 2), np.nan, F32))["y"].tolist() == [[[16, 16], [16, 16]]]


def test_intermediates_stay_inside_the_stated_bounds():
    src = open(HEADER).read()
    assert "-1530 .. 17850" in src and "-3347 .. 19667" in src and "-1530 .. 17850" in open(VO.HEADER).read()
    rng = np.random.default_rng(5)
    lo, hi = [0, 0], [0, 0]
    planes = [VO.random_frames(rng, 64, 80, 80, kind)["cb"] for kind in ("extreme", "random")]
    mid = np.zeros(24, bool)
    mid[10:12] = True
    both = mid[:, None] == mid[None, :]
    planes.append(np.stack([both, ~both, np.broadcast_to(mid[None, :], (24, 24)), np.broadcast_to(~mid[None, :], (24, 24))]).astype(np.uint8) * 255)
    for c in planes:
        v, h = RO.chroma444(c, 2 * c.shape[-2], 2 * c.shape[-1], keep=True)
        for k, a in enumerate((h, v)):
            lo[k], hi[k] = min(lo[k], int(a.min())), max(hi[k], int(a.max()))
    assert (lo[0], hi[0]) == (-1530, 17850) and (lo[1], hi[1]) == (-3347, 19667)
    assert -(1 << 15) <= min(lo) and max(hi) < 1 << 15


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_table_equals_the_image_librarys():
    from sesrq import image, video_rgb
    for s0, z0, ed in DOMAINS:
        q, x = video_rgb.table(s0, z0, ed)
        qi, xi = image.table(s0, z0, ed)
        qo, xo = VO.table(s0, z0, ed)
        assert q.dtype == np.int8 and x.dtype == F32 and q.shape == x.shape == (256,)
        assert np.array_equal(q, qi) and x.tobytes() == xi.tobytes() and np.array_equal(q, qo) and x.tobytes() == xo.tobytes()
    for s0, z0, ed in ((0.0, -128, 0), (float("nan"), 0, 0), (0.01, -128, 3), (0.01, 1 << 25, 0)):
        with pytest.raises(ValueError, match="sesrq_video_rgb_table"):
            video_rgb.table(s0, z0, ed)


def test_library_exports_exactly_the_header_and_links_no_sibling():
    from sesrq import _lib, colour, image, video, video_rgb
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_video_rgb[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 9, names
    assert sorted(video_rgb.SYMBOLS) == names, "python binding and header disagree"
    nm = subprocess.run(["nm", "-D", "--defined-only", video_rgb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r" T (sesrq\w*)", nm))) == names
    d = RO.header_defines()
    assert (video_rgb.TILE_W, video_rgb.TILE_H) == RO.tile() == (d["TILE_W"], d["TILE_H"])
    assert (video_rgb.EXPORT_BLOCK_W, video_rgb.EXPORT_LANES, video_rgb.CODES) == (d["EXPORT_BLOCK_W"], d["EXPORT_LANES"], d["CODES"])
    assert video_rgb.Surface is video.Surface and video_rgb.load_yuv is video.load_yuv and video_rgb.check_out is video.check_out
    needed = subprocess.run(["readelf", "-d", video_rgb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libsesrq" not in needed.replace("libsesrq_video_rgb.so", ""), "the library links another library of the project"
    ldd = subprocess.run(["ldd", video_rgb.LIB_PATH], capture_output=True, text=True).stdout
    assert "libsesrq" not in ldd, "ldd shows another library of the project"
    assert sorted(video_rgb.instances()) == NAMES
    assert not any("vrgb" in n for m in (_lib, image, colour, video) for n in m.instances())


def _surf(fmt=0, y=4096, c0=4096, c1=4096, pitch_y=64, pitch_c=64, frame_y=1 << 20, frame_c=1 << 20):
    from sesrq import video
    return video.SurfaceDesc(fmt, y, c0, c1, pitch_y, pitch_c, frame_y, frame_c)


def test_argument_checks_without_a_device():
    """Every refusal comes before any HIP call: the pointers are never dereferenced, no context exists."""
    from sesrq import video_rgb
    lib = video_rgb.lib()
    launches = sum(video_rgb.instances().values())
    fake, odd = C.c_void_p(4096), C.c_void_p(4098)
    ctx = C.c_void_p(4096)              # never dereferenced: the refusals below come before the context is looked at
    S = _surf
    big = dict(pitch_y=1 << 40, pitch_c=1 << 40, frame_y=1 << 62, frame_c=1 << 62)
    for args, msg in (((None, S(), fake, fake, 1, 8, 8, None), "ctx is NULL"),
                      ((ctx, None, fake, fake, 1, 8, 8, None), "src is NULL"),
                      ((ctx, S(fmt=2), fake, fake, 1, 8, 8, None), "src format 2"),
                      ((ctx, S(y=None), fake, fake, 1, 8, 8, None), "Y plane of src is NULL"),
                      ((ctx, S(c0=None), fake, fake, 1, 8, 8, None), "chroma plane of src is NULL"),
                      ((ctx, S(fmt=1, c1=None), fake, fake, 1, 8, 8, None), "chroma plane of src is NULL"),
                      ((ctx, S(), None, None, 1, 8, 8, None), "neither q0 nor x"),
                      ((ctx, S(), fake, odd, 1, 8, 8, None), "4-byte aligned"),
                      ((ctx, S(), fake, fake, 0, 8, 8, None), "empty frame"),
                      ((ctx, S(), fake, fake, 1, 8, 0, None), "empty frame"),
                      ((ctx, S(), fake, fake, 1, -1, 8, None), "empty frame"),
                      ((ctx, S(pitch_y=7), fake, fake, 1, 8, 8, None), "pitch_y 7 is below the row's 8 bytes"),
                      ((ctx, S(pitch_c=9), fake, fake, 1, 8, 9, None), "pitch_c 9 is below the row's 10 bytes"),
                      ((ctx, S(fmt=1, pitch_c=4), fake, fake, 1, 8, 9, None), "pitch_c 4 is below the row's 5 bytes"),
                      ((ctx, S(frame_y=-1), fake, fake, 2, 8, 8, None), "frame_y -1 is negative"),
                      ((ctx, S(frame_c=-1), fake, fake, 2, 8, 8, None), "frame_c -1 is negative"),
                      ((ctx, S(**big), fake, fake, 1 << 20, 1 << 12, 1 << 12, None), "too large")):
        a = list(args)
        a[1] = C.byref(a[1]) if a[1] is not None else None
        assert lib.sesrq_video_rgb_decode(*a) != 0 and msg in video_rgb.last_error(), (msg, video_rgb.last_error())
    assert lib.sesrq_video_rgb_create(1.0, 0, 0, None) != 0 and "NULL" in video_rgb.last_error()
    h = C.c_void_p()
    assert lib.sesrq_video_rgb_create(0.0, 0, 0, C.byref(h)) != 0 and "scale_in" in video_rgb.last_error() and not h.value
    lib.sesrq_video_rgb_destroy(None)
    nan, inf = float("nan"), float("inf")
    for args, msg in (((None, 0, 1.0, 0, S(), 1, 8, 8, None), "pred is NULL"),
                      ((fake, 2, 1.0, 0, S(), 1, 8, 8, None), "dtype 2"),
                      ((fake, 1, 0.0, 0, S(), 1, 8, 8, None), "scale"),
                      ((fake, 1, -0.01, 0, S(), 1, 8, 8, None), "scale"),
                      ((fake, 1, nan, 0, S(), 1, 8, 8, None), "scale"),
                      ((fake, 1, inf, 0, S(), 1, 8, 8, None), "scale"),
                      ((fake, 1, 0.01, 128, S(), 1, 8, 8, None), "int8 range"),
                      ((fake, 1, 0.01, -129, S(), 1, 8, 8, None), "int8 range"),
                      ((odd, 0, 1.0, 0, S(), 1, 8, 8, None), "4-byte aligned"),
                      ((fake, 0, 1.0, 0, None, 1, 8, 8, None), "out is NULL"),
                      ((fake, 0, 1.0, 0, S(fmt=-1), 1, 8, 8, None), "out format -1"),
                      ((fake, 0, 1.0, 0, S(y=None), 1, 8, 8, None), "Y plane of out is NULL"),
                      ((fake, 0, 1.0, 0, S(c0=None), 1, 8, 8, None), "chroma plane of out is NULL"),
                      ((fake, 0, 1.0, 0, S(fmt=1, c1=None), 1, 8, 8, None), "chroma plane of out is NULL"),
                      ((fake, 0, 1.0, 0, S(), 0, 8, 8, None), "empty frame"),
                      ((fake, 0, 1.0, 0, S(), 1, 8, -1, None), "empty frame"),
                      ((fake, 0, 1.0, 0, S(pitch_y=7), 1, 8, 8, None), "pitch_y 7 of out is below the row's 8 bytes"),
                      ((fake, 0, 1.0, 0, S(pitch_c=9), 1, 8, 9, None), "pitch_c 9 of out is below the row's 10 bytes"),
                      ((fake, 0, 1.0, 0, S(fmt=1, pitch_c=4), 1, 8, 9, None), "pitch_c 4 of out is below the row's 5 bytes"),
                      ((fake, 0, 1.0, 0, S(frame_y=-1), 1, 8, 8, None), "is negative"),
                      ((fake, 0, 1.0, 0, S(frame_y=7 * 64 + 7), 2, 8, 8, None), "below its plane's extent"),
                      ((fake, 0, 1.0, 0, S(frame_c=3 * 64 + 7), 2, 8, 8, None), "below its plane's extent"),
                      ((fake, 0, 1.0, 0, S(**big), 1 << 20, 1 << 14, 1 << 14, None), "too large"),
                      ((fake, 0, 1.0, 0, S(**big), 1 << 30, 8, 8, None), "too large")):
        a = list(args)
        a[4] = C.byref(a[4]) if a[4] is not None else None
        assert lib.sesrq_video_rgb_export(*a) != 0 and msg in video_rgb.last_error(), (msg, video_rgb.last_error())
    assert lib.sesrq_video_rgb_instance_count() == len(NAMES)
    assert lib.sesrq_video_rgb_instance_name(len(NAMES)) is None and lib.sesrq_video_rgb_instance_launches(-1) == -1
    assert sum(video_rgb.instances().values()) == launches, "a refused call launched a kernel"


def test_python_refusals_without_a_device():
    import torch
    from sesrq import video_rgb
    from sesrq.bundle import Bundle
    from conftest import GOLDEN
    y, c = np.zeros((1, 4, 6), np.uint8), np.zeros((1, 2, 6), np.uint8)
    host = video_rgb.Surface("nv12", 4, 6, torch.from_numpy(y), torch.from_numpy(c))
    for s in (video_rgb.Surface("nv12", 4, 6, y, c), host):
        with pytest.raises(ValueError, match="HIP device"):
            video_rgb.decode(None, s, want_q=False, want_f=True)
    with pytest.raises(ValueError, match="Surface"):
        video_rgb.decode(None, y, want_q=False, want_f=True)
    with pytest.raises(ValueError, match="q0, x or both"):
        video_rgb.decode(None, host, want_q=False, want_f=False)
    with pytest.raises(ValueError, match="input domain"):
        video_rgb.decode(None, host)
    with pytest.raises(ValueError, match="3 channels in"):
        video_rgb.decode(Bundle.load(os.path.join(GOLDEN, "image", "sesr_x4.npz")), host)
    with pytest.raises(ValueError, match="HIP device"):
        video_rgb.export(torch.zeros((1, 3, 4, 6)))
    with pytest.raises(ValueError, match=r"\(N, 3, H, W\)"):
        video_rgb.export(torch.zeros((1, 1, 4, 6)))
    with pytest.raises(ValueError, match=r"\(N, 3, H, W\)"):
        video_rgb.export(np.zeros((1, 3, 4, 6), np.float32))
