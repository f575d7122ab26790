"""The colour export's restatement (tests/colour_oracle.py) anchored outside itself, and the host side of libsesrq_colour.so
(include/sesrq_colour.h): no test here needs a device.

  weights     the table equals the Keys a = -1/2 polynomial in fractions.Fraction x 1024, is integral, every row sums to 1024, and
              sesrq_colour_weights returns it
  round trip  every one of the 2^24 RGB triples: luma by tests/image_oracle.py (pinned to the reference), chroma by step 1; step 4
              gives back the exact three bytes -- the chroma matrix and the inverse are tied to the reference's luma line
  bicubic     the integer upscale against PIL's BICUBIC resize of the same plane in mode "F", away from the border
  constant    a constant image of any size gives a constant chroma plane
  ABI         the library exports exactly the header's symbols; the other libraries' instance lists are unchanged; every refusal
              is reached without a device"""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

import colour_oracle as CO
import image_oracle as IO

HEADER = os.path.join(ROOT, "include", "sesrq_colour.h")


def keys(t):
    """The Keys cubic convolution kernel with a = -1/2 at a rational t, exactly."""
    t = abs(Fraction(t))
    if t <= 1:
        return Fraction(3, 2) * t ** 3 - Fraction(5, 2) * t ** 2 + 1
    if t < 2:
        return Fraction(-1, 2) * t ** 3 + Fraction(5, 2) * t ** 2 - 4 * t + 2
    return Fraction(0)


@pytest.mark.parametrize("r", [2, 4])
def test_weights_are_the_keys_polynomial(r):
    from sesrq import colour
    w_lib, first_lib = colour.weights(r)
    assert w_lib.shape == (r, 4) and w_lib.dtype == np.int16 and first_lib.dtype == np.int8
    for phi in range(r):
        centre = Fraction(2 * phi + 1, 2 * r) - Fraction(1, 2)          # of output r j + phi, in LR pixels from j (half-pixel centres)
        first = -2 if centre < 0 else -1                                # the four taps within distance 2
        w = [keys(centre - (first + k)) * 1024 for k in range(4)]
        assert all(x.denominator == 1 for x in w), (r, phi, w)
        assert sum(w) == 1024
        assert keys(centre - (first - 1)) == 0 and keys(centre - (first + 4)) == 0      # no fifth tap
        assert tuple(int(x) for x in w) == CO.WEIGHTS[r][phi] and first == CO.FIRST[r][phi], (r, phi, w)
        assert tuple(int(x) for x in w_lib[phi]) == CO.WEIGHTS[r][phi] and int(first_lib[phi]) == first
    for bad in (0, 1, 3, 8):
        with pytest.raises(ValueError, match="sesrq_colour_weights"):
            colour.weights(bad)


def test_round_trip_every_triple_gives_back_its_bytes():
    """All 2^24 triples: the reference's luma (image_oracle.decode_y, as the net's ideal output) and step 1's chroma through
    steps 3 and 4 give the three bytes back, exactly."""
    bad = 0
    lo, hi = [1 << 15] * 2, [0] * 2
    for r in range(0, 256, 32):                                         # 8 slabs of 2^21 triples
        v = np.arange(r << 16, (r + 32) << 16, dtype=np.uint32)
        img = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], 1).astype(np.uint8).reshape(1, 2048, 1024, 3)
        y = IO.decode_y(img)
        c = CO.chroma(img).astype(np.int64)
        R, G, B = CO.to_rgb(CO.luma(y)[:, 0], c[:, 0], c[:, 1])
        bad += int((np.stack((R, G, B), -1) != img).any(-1).sum())
        for k in range(2):
            lo[k], hi[k] = min(lo[k], int(c[:, k].min())), max(hi[k], int(c[:, k].max()))
    assert bad == 0, f"{bad} of 16777216 triples do not come back"
    assert lo == [1024, 1024] and hi == [15360, 15360]                  # the header's range, reached


@pytest.mark.parametrize("r", [2, 4])
def test_bicubic_against_pil(r):
    """PIL's BICUBIC (Keys a = -1/2, half-pixel centres) on the same Q6 plane in float: away from the border (PIL renormalises
    there, the header replicates) the integer upscale differs by the two half-unit roundings, the first carried through the second
    pass's weights: at most 1/2 * max sum |w| / 1024 + 1/2 < 2."""
    Image = pytest.importorskip("PIL.Image")
    H, W = 37, 29
    rng = np.random.default_rng(3729)
    c = rng.integers(1024, 15361, (H, W))
    got, h = CO.upscale(c, r, keep=True)
    assert got.shape == (r * H, r * W) and h.shape == (H, r * W)
    ref = np.asarray(Image.fromarray(c.astype(np.float32), mode="F").resize((r * W, r * H), Image.BICUBIC), np.float64)
    inner = (slice(2 * r, r * H - 2 * r), slice(2 * r, r * W - 2 * r))
    err = np.abs(got[inner] - ref[inner]).max()
    print(f"r = {r}: max |integer - PIL| = {err:.3f} Q6 units on the interior")
    wsum = max(sum(abs(x) for x in row) for row in CO.WEIGHTS[r]) / 1024
    assert 0.5 * wsum + 0.5 < 2
    assert err <= 2, err
    # the order of the passes matters to the bits: the header says horizontal first
    assert not np.array_equal(got, CO.upscale_axis(CO.upscale_axis(c, r, -2), r, -1))
    assert np.abs(h).max() <= 19000 and h.min() >= -(1 << 15) and h.max() < (1 << 15)


def test_constant_image_gives_constant_chroma():
    rng = np.random.default_rng(7)
    for H, W in ((1, 1), (1, 5), (3, 2), (9, 40)):
        for r in (2, 4):
            t = rng.integers(0, 256, 3).astype(np.uint8)
            img = np.broadcast_to(t, (1, H, W, 3))
            c = CO.chroma(img)
            up = CO.upscale(c, r)
            assert up.shape == (1, 2, r * H, r * W)
            for k in range(2):
                assert (up[:, k] == c[0, k, 0, 0]).all(), (H, W, r, k)
            y = np.full((1, 1, r * H, r * W), 0.5, np.float32)
            out = CO.export(y, img, r)
            assert (out == out[0, 0, 0]).all()


def test_export_order_is_the_images_order():
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (2, 5, 7, 3)).astype(np.uint8)
    y = rng.random((2, 1, 20, 28)).astype(np.float32)
    rgb = CO.export(y, img, 4)
    assert np.array_equal(CO.export(y, np.ascontiguousarray(img[..., ::-1]), 4, "bgr"), rgb[..., ::-1])
    q = rng.integers(-128, 128, y.shape).astype(np.int8)
    assert np.array_equal(CO.export(q, img, 4, scale=0.004, zero=-120), CO.export(CO.dequant(q, 0.004, -120), img, 4))


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_colour_library_exports_exactly_the_header():
    from sesrq import colour
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_colour[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 7, names
    assert sorted(colour.SYMBOLS) == names, "python binding and header disagree"
    nm = subprocess.run(["nm", "-D", "--defined-only", colour.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r" T (sesrq\w*)", nm))) == names
    assert (colour.TILE_W, colour.TILE_H) == CO.header_tile() == CO.tile(4) and CO.tile(2) == (2 * colour.TILE_W, 2 * colour.TILE_H)


def test_other_libraries_instances_unchanged_by_the_colour_library():
    from sesrq import _lib, colour, image
    before, before_img = _lib.instances(), image.instances()
    assert len(before) == 258 and len(before_img) == 10
    assert sorted(colour.instances()) == sorted(["colour_export<i8,r2>", "colour_export<i8,r4>", "colour_export<f32,r2>",
                                                 "colour_export<f32,r4>", "colour_chroma"])
    assert sorted(_lib.instances()) == sorted(before) and sorted(image.instances()) == sorted(before_img)
    assert not any("colour" in n for n in list(before) + list(before_img))
    ldd = subprocess.run(["readelf", "-d", colour.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libsesrq" not in ldd.replace("libsesrq_colour.so", ""), "the colour library links another library of the project"


def test_argument_checks_without_a_device():
    from sesrq import colour
    lib = colour.lib()
    fake = C.c_void_p(4096)                       # never dereferenced: every failing check comes before any HIP call
    odd = C.c_void_p(4097)
    for args, msg in (((None, 0, fake, 1, 8, 8, None), "img is NULL"),
                      ((fake, 0, None, 1, 8, 8, None), "cbcr is NULL"),
                      ((fake, 0, odd, 1, 8, 8, None), "2-byte aligned"),
                      ((fake, 2, fake, 1, 8, 8, None), "order"),
                      ((fake, 0, fake, 1, 0, 8, None), "empty frame"),
                      ((fake, 0, fake, 0, 8, 8, None), "empty frame")):
        assert lib.sesrq_colour_chroma(*args) != 0 and msg in colour.last_error(), (msg, colour.last_error())
    nan, inf = float("nan"), float("inf")
    for args, msg in (((None, 0, 1.0, 0, fake, 0, 4, fake, 1, 8, 8, None), "y is NULL"),
                      ((fake, 0, 1.0, 0, None, 0, 4, fake, 1, 8, 8, None), "img is NULL"),
                      ((fake, 0, 1.0, 0, fake, 0, 4, None, 1, 8, 8, None), "out is NULL"),
                      ((fake, 2, 1.0, 0, fake, 0, 4, fake, 1, 8, 8, None), "y_dtype"),
                      ((fake, 1, 0.0, 0, fake, 0, 4, fake, 1, 8, 8, None), "scale"),
                      ((fake, 1, -0.01, 0, fake, 0, 4, fake, 1, 8, 8, None), "scale"),
                      ((fake, 1, nan, 0, fake, 0, 4, fake, 1, 8, 8, None), "scale"),
                      ((fake, 1, inf, 0, fake, 0, 4, fake, 1, 8, 8, None), "scale"),
                      ((fake, 1, 0.01, 128, fake, 0, 4, fake, 1, 8, 8, None), "int8 range"),
                      ((fake, 1, 0.01, -129, fake, 0, 4, fake, 1, 8, 8, None), "int8 range"),
                      ((odd, 0, 1.0, 0, fake, 0, 4, fake, 1, 8, 8, None), "4-byte aligned"),
                      ((fake, 0, 1.0, 0, fake, 5, 4, fake, 1, 8, 8, None), "order"),
                      ((fake, 0, 1.0, 0, fake, 0, 3, fake, 1, 8, 8, None), "r = 3"),
                      ((fake, 0, 1.0, 0, fake, 0, 1, fake, 1, 8, 8, None), "r = 1"),
                      ((fake, 0, 1.0, 0, fake, 0, 8, fake, 1, 8, 8, None), "r = 8"),
                      ((fake, 0, 1.0, 0, fake, 0, 4, fake, 0, 8, 8, None), "empty frame"),
                      ((fake, 0, 1.0, 0, fake, 0, 4, fake, 1, 8, 0, None), "empty frame"),
                      ((fake, 0, 1.0, 0, fake, 0, 4, fake, 1, -1, 8, None), "empty frame"),
                      ((fake, 0, 1.0, 0, fake, 0, 4, fake, 1 << 20, 1 << 12, 1 << 12, None), "too large"),      # the grid
                      ((fake, 0, 1.0, 0, fake, 0, 4, fake, 1, 1, 1 << 29, None), "too large"),                  # r W
                      ((fake, 0, 1.0, 0, fake, 0, 2, fake, 1, 1 << 30, 1, None), "too large")):                 # r H
        assert lib.sesrq_colour_export(*args) != 0 and msg in colour.last_error(), (msg, colour.last_error())
    assert lib.sesrq_colour_instance_name(5) is None and lib.sesrq_colour_instance_launches(-1) == -1


def test_python_refusals_without_a_device():
    import torch
    from sesrq import colour
    with pytest.raises(ValueError, match="order"):
        colour._order("rbg")
    with pytest.raises(ValueError, match="2 or 4"):
        colour._factor(3)
    with pytest.raises(ValueError, match="HIP device"):
        colour.chroma(torch.zeros((4, 4, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        colour.chroma(torch.zeros((4, 4, 3)))
