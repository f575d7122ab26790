"""The shared comparator of the suite (tests/helpers.py::same), pinned on the CPU: a comparator that passes silently hides every
failure behind it.  And the tile counts the quality tests reason with, against the geometry of csrc/sesrq_eval_tile.h."""
import numpy as np
import pytest

from helpers import nbx, nby, same, sha256


def _f32(*words):
    return np.array(words, np.uint32).view(np.float32)


def test_same_passes_on_identical_arrays():
    rng = np.random.default_rng(0)
    for a in (rng.integers(-128, 128, (2, 3, 5, 7)).astype(np.int8), rng.integers(-1 << 20, 1 << 20, (4, 9)).astype(np.int32),
              rng.standard_normal((3, 11)).astype(np.float32), rng.standard_normal(6), _f32(0x7FC00001, 0x80000000, 0)):
        same("identical", a, a.copy())
    want = rng.standard_normal((5, 8)).astype(np.float32)
    want.setflags(write=False)
    same("read-only want", want.copy(), want)
    wide = np.zeros((5, 16), np.float32)
    wide[:, ::2] = want
    got = wide[:, ::2]
    assert not got.flags.c_contiguous
    same("non-contiguous got", got, want)
    same("non-contiguous want", want, got)


def test_same_refuses_another_shape_of_equal_size():
    a = np.arange(24, dtype=np.int32)
    with pytest.raises(AssertionError, match=r"int32 \(4, 6\) != int32 \(24,\)"):
        same("shape", a.reshape(4, 6), a)
    with pytest.raises(AssertionError, match="shape"):
        same("shape", a.reshape(1, 24), a.reshape(24, 1))
    same("reshape", a.reshape(4, 6), a.reshape(2, 12), reshape=True)
    with pytest.raises(AssertionError, match="24 elements"):
        same("reshape", a, np.arange(25, dtype=np.int32), reshape=True)
    b = a.reshape(2, 12).copy()
    b[1, 3] += 1
    with pytest.raises(AssertionError, match=r"1 of 24 differ, first at \(1, 3\)"):      # the index is reported in want's shape
        same("reshape", a.reshape(4, 6), b, reshape=True)


def test_same_refuses_another_dtype_of_equal_values():
    a = np.arange(-5, 5)
    for values in (False, True):
        with pytest.raises(AssertionError, match=r"int8 \(10,\) != int32 \(10,\)"):
            same("dtype", a.astype(np.int8), a.astype(np.int32), values=values)
        with pytest.raises(AssertionError, match="float32"):
            same("dtype", a.astype(np.float32), a.astype(np.float64), values=values)
    same("cast", a.astype(np.float32), a.astype(np.float64), cast=np.float32)
    same("cast", a.astype(np.int8), a.astype(np.int64), cast=np.int8)
    with pytest.raises(AssertionError, match="1 of 10 differ"):      # the cast does not hide a value
        same("cast", a.astype(np.float32), np.where(a == 2, 2.5, a), cast=np.float32)


@pytest.mark.parametrize("dtype", [np.int8, np.int32, np.float32])
def test_same_finds_one_element_among_ten_thousand(dtype):
    want = np.random.default_rng(1).integers(-100, 100, (4, 25, 100)).astype(dtype)
    got = want.copy()
    got[2, 17, 63] += 1
    for kw in (dict(), dict(values=True)):
        with pytest.raises(AssertionError) as ei:
            same("one element", got, want, **kw)
        msg = str(ei.value)
        assert "one element: 1 of 10000 differ, first at (2, 17, 63)" in msg
        assert f"got {got[2, 17, 63]} want {want[2, 17, 63]}" in msg
    got[0, 0, 1] -= 1
    with pytest.raises(AssertionError, match=r"2 of 10000 differ, first at \(0, 0, 1\)"):
        same("two elements", got, want)


def test_same_compares_floats_as_words_unless_told_values():
    neg, pos = _f32(0x80000000, 0x3F800000), _f32(0x00000000, 0x3F800000)
    assert neg[0] == pos[0]
    with pytest.raises(AssertionError, match=r"1 of 2 differ, first at \(0,\): got -0.0 want 0.0"):
        same("signed zero", neg, pos)
    same("signed zero by value", neg, pos, values=True)
    n1, n2 = _f32(0x7FC00000, 0), _f32(0x7FC00001, 0)
    with pytest.raises(AssertionError, match="1 of 2 differ"):
        same("NaN payloads", n1, n2)
    same("one NaN payload", n1, n1.copy())
    with pytest.raises(AssertionError):            # by value a NaN equals nothing, itself included
        same("NaN by value", n1, n1.copy(), values=True)
    d = np.array([-0.0, 1.0])
    with pytest.raises(AssertionError, match="1 of 2 differ"):
        same("float64 words", d, np.array([0.0, 1.0]))


def test_same_takes_tensors():
    import torch
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    same("tensor", torch.from_numpy(a.copy()), a)
    same("tensor, strided", torch.from_numpy(a.copy()).t(), a.T)
    with pytest.raises(AssertionError, match=r"first at \(2, 1\)"):
        b = a.copy()
        b[2, 1] = -1
        same("tensor", torch.from_numpy(b), a)


def test_sha256_is_of_the_c_ordered_bytes():
    import hashlib
    a = np.arange(30, dtype=np.int16).reshape(5, 6)
    assert sha256(a) == sha256(a.copy()) == hashlib.sha256(a.tobytes()).hexdigest()
    assert sha256(a.T) == hashlib.sha256(np.ascontiguousarray(a.T).tobytes()).hexdigest() != sha256(a)


def test_tile_counts_on_each_side_of_every_seam():
    """geometry() of csrc/sesrq_eval_tile.h: a tile gives 248 SSIM columns x 32 SSIM rows, a frame H - 6 rows of W - 6 columns."""
    for W, want in ((7, 1), (254, 1), (255, 2), (502, 2)):
        assert nbx(W) == (W - 6 + 247) // 248 == want, W
    for H, want in ((7, 1), (38, 1), (39, 2), (70, 2)):
        assert nby(H) == (H - 6 + 31) // 32 == want, H
