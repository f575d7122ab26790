"""The bicubic downscale's restatement (tests/downscale_oracle.py) anchored outside itself, and the host side of
libsesrq_downscale.so (include/sesrq_downscale.h): no test here needs a device.

  weights     equal the Keys a = -1/2 polynomial in fractions.Fraction, stretched by r, times D; symmetric; sum to D; and
              sesrq_downscale_weights returns them
  PIL         the restatement equals PIL's BICUBIC resize of the TRANSPOSED image (PIL runs the horizontal pass first) on EVERY LR
              pixel whose taps lie inside the frame -- LR rows and columns 2 .. n / r - 3 -- with zero mismatches: smooth, noise and
              {0, 255} images of 192 x 240, r = 2 and 4.  (At the border PIL truncates its kernel; only the restatement pins it.)
  constants   all 256 constant images come back unchanged
  clamps      both clamps of each pass fire on a named LR pixel
  small       frames of r, 2 r, 3 r pixels a side, where the mirror wraps more than once, against a direct per-pixel evaluation
  modcrop     the GTmod12 crop, as a view
  ABI         the library exports exactly the header's symbols and links no other library of the project; every refusal of the C ABI
              and of the Python layer is reached without a device"""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

import downscale_oracle as DO
import image_oracle as IO

HEADER = os.path.join(ROOT, "include", "sesrq_downscale.h")
H, W = 192, 240


def keys(t):
    """The Keys cubic convolution kernel with a = -1/2 at a rational t, exactly."""
    t = abs(Fraction(t))
    if t <= 1:
        return Fraction(3, 2) * t ** 3 - Fraction(5, 2) * t ** 2 + 1
    if t < 2:
        return Fraction(-1, 2) * t ** 3 + Fraction(5, 2) * t ** 2 - 4 * t + 2
    return Fraction(0)


@pytest.mark.parametrize("r", [2, 4])
def test_weights_are_the_stretched_keys_polynomial(r):
    from sesrq import downscale
    w_lib, D = downscale.weights(r)
    assert w_lib.shape == (4 * r,) and w_lib.dtype == np.int16 and D == DO.D[r]
    d = 5
    c = Fraction(r * d) + Fraction(r - 1, 2)                     # the centre of LR index d in HR pixels (half-pixel centres)
    j0 = r * d - 3 * r // 2
    w = [keys((Fraction(j0 + k) - c) / r) / r * D for k in range(4 * r)]
    assert all(x.denominator == 1 for x in w), (r, w)
    assert tuple(int(x) for x in w) == DO.WEIGHTS[r] == tuple(int(x) for x in w_lib)
    assert sum(w) == D and w == w[::-1]
    assert keys((Fraction(j0 - 1) - c) / r) == 0 and keys((Fraction(j0 + 4 * r) - c) / r) == 0      # no further tap
    assert 255 * sum(x for x in DO.WEIGHTS[4] if x > 0) == 255 * 4448 < 2 ** 31       # the largest sum of either factor
    for bad in (0, 1, 3, 8):
        with pytest.raises(ValueError, match="sesrq_downscale_weights"):
            downscale.weights(bad)


def _images():
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = np.stack([127 + 120 * np.sin(xx / 9. + yy / 13.), 127 + 120 * np.cos(xx / 5. - yy / 17.), (xx + yy) / 432 * 255], -1)
    return {"smooth": smooth.clip(0, 255).astype(np.uint8), "noise": rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
            "extreme": (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)}


@pytest.mark.parametrize("r", [2, 4])
def test_equals_pil_on_every_interior_pixel(r):
    Image = pytest.importorskip("PIL.Image")
    for name, img in _images().items():
        mine = DO.downscale(img, r)[0]
        t = np.ascontiguousarray(img.transpose(1, 0, 2))
        pil = np.asarray(Image.fromarray(t).resize((H // r, W // r), Image.BICUBIC)).transpose(1, 0, 2)
        assert pil.shape == mine.shape == (H // r, W // r, 3)
        inner = (slice(2, H // r - 2), slice(2, W // r - 2))       # LR index 2 .. n / r - 3 on both axes, all of them
        assert mine[inner].shape == (H // r - 4, W // r - 4, 3)
        bad = np.argwhere(mine[inner] != pil[inner])
        assert len(bad) == 0, f"{name} r={r}: {len(bad)} interior pixels differ from PIL, first at {bad[0]}"
        # the region is exactly the pixels whose taps stay inside the frame
        for n in (H, W):
            tp = r * np.arange(n // r)[:, None] - 3 * r // 2 + np.arange(4 * r)[None, :]
            inside = np.flatnonzero(((tp >= 0) & (tp < n)).all(1))
            assert inside[0] == 2 and inside[-1] == n // r - 3 and len(inside) == n // r - 4


@pytest.mark.parametrize("r", [2, 4])
def test_all_256_constant_images_come_back_unchanged(r):
    for H_, W_ in ((r, r), (3 * r, 5 * r), (48, 36)):
        img = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, H_, W_, 3))
        assert np.array_equal(DO.downscale(img, r), img[:, :H_ // r, :W_ // r])


@pytest.mark.parametrize("r", [2, 4])
def test_both_clamps_of_each_pass_fire_on_a_named_pixel(r):
    n, d = 12 * r, 5
    want = {True: 255 * sum(w for w in DO.WEIGHTS[r] if w > 0), False: 255 * sum(w for w in DO.WEIGHTS[r] if w < 0)}
    assert [round(want[k] / DO.D[r], 1) for k in (True, False)] == ([278.9, -23.9] if r == 2 else [276.9, -21.9])
    for high in (True, False):
        line = DO.clamp_pattern(n, r, d, high)
        rows = np.ascontiguousarray(np.broadcast_to(line[:, None, None], (n, n, 3)))         # HR rows set: the vertical pass clamps
        cols = np.ascontiguousarray(np.broadcast_to(line[None, :, None], (n, n, 3)))         # HR columns set: the horizontal one
        s_v = DO.one_pass(rows[None], r, 1, sums=True)[0]
        assert (s_v[d] == want[high]).all() and ((s_v[d] + DO.D[r] // 2) // DO.D[r] > 255 if high else (s_v[d] < -DO.D[r]).all()).all()
        lr, v = DO.downscale(rows, r, keep=True)
        assert (v[0, d] == (255 if high else 0)).all() and (lr[0, d] == (255 if high else 0)).all()
        lr, v = DO.downscale(cols, r, keep=True)
        assert np.array_equal(v[0], cols[:n // r])                                      # constant columns pass the vertical pass
        s_h = DO.one_pass(v, r, 2, sums=True)[0]
        assert (s_h[:, d] == want[high]).all()
        assert (lr[0, :, d] == (255 if high else 0)).all()
        assert lr.min() == 0 and lr.max() == 255


def _direct(img, r):
    """The header evaluated pixel by pixel with Python integers: the small-frame check of the vectorised restatement."""
    def mirror(j, n):
        i = j % (2 * n)
        return i if i < n else 2 * n - 1 - i

    def run(a, axis):
        a = np.moveaxis(a, axis, 0)
        n = a.shape[0]
        out = np.empty((n // r,) + a.shape[1:], np.uint8)
        for d in range(n // r):
            s = sum(int(w) * a[mirror(r * d - 3 * r // 2 + k, n)].astype(object) for k, w in enumerate(DO.WEIGHTS[r]))
            out[d] = np.clip((s + DO.D[r] // 2) // DO.D[r], 0, 255).astype(np.uint8)
        return np.moveaxis(out, 0, axis)
    return run(run(img, 0), 1)


@pytest.mark.parametrize("r", [2, 4])
def test_frames_narrower_than_the_kernel(r):
    rng = np.random.default_rng(r)
    for h in (r, 2 * r, 3 * r):
        for w in (r, 2 * r, 3 * r, 7 * r):
            for kind in range(2):
                img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if kind == 0 else (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
                assert np.array_equal(DO.downscale(img, r)[0], _direct(img, r)), (r, h, w, kind)
    # an axis of r pixels: every tap is one of its r samples, each taken equally often from both ends
    assert sorted(DO.taps(r, r)[0]) == sorted(list(range(r)) * 4)


def test_decode_is_the_image_oracles_on_the_lr_bytes():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 8, 12, 3), dtype=np.uint8)
    for r in (2, 4):
        for form in ("y", "rgb"):
            lr, x, q = DO.decode(img, r, form, "rgb", 0.0039, -128)
            assert x.shape == (2, 1 if form == "y" else 3, 8 // r, 12 // r) and q.dtype == np.int8 and q.shape == x.shape
            lr_b, x_b, _ = DO.decode(np.ascontiguousarray(img[..., ::-1]), r, form, "bgr")
            assert np.array_equal(lr_b, lr[..., ::-1]) and np.array_equal(x_b, x)
            assert np.array_equal(x, IO.decode(lr, form))


def test_modcrop():
    import torch
    from sesrq import downscale
    a = np.arange(50 * 40 * 3, dtype=np.uint8).reshape(50, 40, 3)
    c = downscale.modcrop(a)
    assert c.shape == (48, 36, 3) and np.shares_memory(c, a) and np.array_equal(c, a[:48, :36])
    assert downscale.modcrop(a[None], 4).shape == (1, 48, 40, 3)
    assert downscale.modcrop(a[:48, :36]).shape == (48, 36, 3)
    t = torch.from_numpy(a)
    ct = downscale.modcrop(t, 8)
    assert tuple(ct.shape) == (48, 40, 3) and ct.data_ptr() == t.data_ptr()
    for bad, msg in ((a[:11], "no 12 x 12"), (a[..., 0], "interleaved"), (a[None, None], "interleaved")):
        with pytest.raises(ValueError, match=msg):
            downscale.modcrop(bad)
    with pytest.raises(ValueError, match="positive"):
        downscale.modcrop(a, 0)


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_downscale_library_exports_exactly_the_header():
    from sesrq import downscale
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_downscale[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 8, names
    assert sorted(downscale.SYMBOLS) == names, "python binding and header disagree"
    nm = subprocess.run(["nm", "-D", "--defined-only", downscale.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r" T (sesrq\w*)", nm))) == names
    (tw, th), hr = DO.header_tile()
    assert (downscale.TILE_W, downscale.TILE_H) == (tw, th) == DO.tile(4) and DO.tile(2) == (2 * tw, 2 * th) and hr == DO.HR_TILE
    ldd = subprocess.run(["readelf", "-d", downscale.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libsesrq" not in ldd.replace("libsesrq_downscale.so", ""), "the downscale library links another library of the project"
    assert sorted(downscale.instances()) == sorted(f"downscale<r{r},{f}>" for r in (2, 4) for f in ("lr", "Y", "RGB"))


def c_abi_refusals():
    """Every refusal of sesrq_downscale_run and _create, on pointers that are never dereferenced: each check comes before any HIP call."""
    from sesrq import downscale
    lib = downscale.lib()
    fake, odd = C.c_void_p(4096), C.c_void_p(4098)
    ok = dict(ctx=fake, img=fake, order=0, r=4, form=0, lr=fake, q0=None, x=None, N=1, H=8, W=8)
    cases = ((dict(img=None), "img is NULL"),
             (dict(lr=None), "none of lr, q0 and x"),
             (dict(ctx=None, q0=fake), "ctx is NULL"),
             (dict(ctx=None, lr=None, x=fake), "ctx is NULL"),
             (dict(order=2), "order"),
             (dict(r=3), "r = 3"), (dict(r=1), "r = 1"), (dict(r=8), "r = 8"),
             (dict(q0=fake, form=2), "form 2"),
             (dict(x=odd), "4-byte aligned"),
             (dict(N=0), "empty frame"), (dict(H=0), "empty frame"), (dict(W=-4), "empty frame"),
             (dict(H=10), "modcrop"), (dict(W=6), "modcrop"), (dict(r=2, H=7), "modcrop"), (dict(H=2), "modcrop"),
             (dict(N=1 << 20, H=1 << 12, W=1 << 13), "too large"))
    for change, msg in cases:
        a = dict(ok, **change)
        rc = lib.sesrq_downscale_run(a["ctx"], a["img"], a["order"], a["r"], a["form"], a["lr"], a["q0"], a["x"], a["N"], a["H"], a["W"],
                                     None)
        assert rc != 0 and msg in downscale.last_error(), (change, msg, downscale.last_error())
    h = C.c_void_p()
    for args, msg in (((0.0, 0, 0), "scale_in"), ((float("nan"), 0, 0), "scale_in"), ((0.01, 1 << 25, 0), "zero_in"), ((0.01, 0, 3), "exact_div")):
        assert lib.sesrq_downscale_create(*args, C.byref(h)) != 0 and msg in downscale.last_error() and not h.value
    assert lib.sesrq_downscale_create(0.01, 0, 0, None) != 0 and "ctx is NULL" in downscale.last_error()
    lib.sesrq_downscale_destroy(None)
    assert lib.sesrq_downscale_instance_name(6) is None and lib.sesrq_downscale_instance_launches(-1) == -1


def test_argument_checks_without_a_device():
    c_abi_refusals()


def test_python_refusals_without_a_device():
    import torch
    from sesrq import downscale, quality
    hr = torch.zeros((8, 12, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="modcrop"):
        downscale.downscale(torch.zeros((10, 12, 3), dtype=torch.uint8), 4)            # H % r
    with pytest.raises(ValueError, match="modcrop"):
        downscale.decode(None, torch.zeros((8, 7, 3), dtype=torch.uint8), 2, "rgb", want_q=False, want_f=True)
    with pytest.raises(ValueError, match="uint8"):
        downscale.downscale(hr.float(), 4)
    with pytest.raises(ValueError, match="uint8"):
        downscale.downscale(hr.numpy(), 4)
    with pytest.raises(ValueError, match="2 or 4"):
        downscale.downscale(hr, 3)
    with pytest.raises(ValueError, match="interleaved"):
        downscale.downscale(hr.permute(2, 0, 1), 4)
    with pytest.raises(ValueError, match="order"):
        downscale.downscale(hr, 4, order="rbg")
    with pytest.raises(ValueError, match="MFLAG 3"):
        downscale.factor_of(3)
    with pytest.raises(ValueError, match="MFLAG 3"):
        quality.evaluate_hr(None, [hr], 3)
    assert downscale.factor_of(5) == 4 and downscale.factor_of(6) == 2
    for name, bad in (("short", torch.empty((1, 2, 2, 3), dtype=torch.uint8)), ("no batch", torch.empty((2, 3, 3), dtype=torch.uint8)),
                      ("int8", torch.empty((1, 2, 3, 3), dtype=torch.int8)),
                      ("strided", torch.empty((1, 2, 6, 3), dtype=torch.uint8)[:, :, ::2]), ("array", np.empty((1, 2, 3, 3), np.uint8))):
        with pytest.raises(ValueError, match="out must be a contiguous uint8 tensor of the output shape"):
            downscale.downscale(hr, 4, out=bad)
    with pytest.raises(ValueError, match="HIP device"):                                 # everything else is fine: only the device is missing
        downscale.downscale(hr, 4, out=torch.empty((1, 2, 3, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="q0, x or both"):
        downscale.decode(None, hr, 4, "y", want_q=False, want_f=False)
    with pytest.raises(ValueError, match="input domain"):
        downscale.decode(None, hr, 4, "y")
    with pytest.raises(ValueError, match="form"):
        downscale.decode(None, hr, 4, "yuv", want_q=False, want_f=True)
