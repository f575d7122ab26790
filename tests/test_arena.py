"""The arena of tests/helpers.py on CPU tensors: it must be shown to detect faults before tests/test_caller_buffers.py rests on it."""
import numpy as np
import pytest
import torch

from helpers import Arena

CPU = torch.device("cpu")


def _arena(canary=0x5A):
    a = Arena(CPU, Arena.room(60, 4 * 35, 17), canary)
    q = a.place((3, 20), torch.int8, 7, name="q")
    f = a.place((5, 7), torch.float32, 12, fill=1.5, name="f")
    w = a.place(17, torch.uint8, 16, fill=0xFF, name="w")
    return a, q, f, w


def test_placements_are_aligned_as_asked_and_apart():
    a, q, f, w = _arena()
    assert a.buf.data_ptr() % 256 == 0
    assert (q.data_ptr() % 256, f.data_ptr() % 256, w.data_ptr() % 256) == (7, 12, 16)
    assert q.dtype == torch.int8 and tuple(q.shape) == (3, 20) and q.is_contiguous()
    assert f.dtype == torch.float32 and tuple(f.shape) == (5, 7) and f.is_contiguous()
    assert (q == 0x5A).all() and (f == 1.5).all() and (w == 0xFF).all()          # no fill: the canary; else the fill
    spans = sorted(a.spans)
    assert spans[0][0] >= Arena.GAP and a.nbytes - spans[-1][1] >= Arena.GAP
    for (s0, e0, _), (s1, e1, _) in zip(spans, spans[1:]):
        assert s1 - e0 >= Arena.GAP
    for view, (s, e, _) in zip((q, f, w), a.spans):
        assert view.data_ptr() - a.buf.data_ptr() == s and e - s == view.numel() * view.element_size()


def test_untouched_arena_and_writes_inside_placements_report_nothing():
    a, q, f, w = _arena()
    assert a.check() == []
    q.fill_(-3)
    f.fill_(float("nan"))
    w.zero_()
    assert a.check() == []


@pytest.mark.parametrize("who", ["q", "f", "w"])
def test_stray_bytes_are_reported_at_their_offset(who):
    a, q, f, w = _arena()
    s, e, _ = {n: sp for sp in a.spans for n in [sp[2]]}[who]
    for pos, side, off in ((s - 1, "before", -1), (e, "behind", 1), (e + 254, "behind", 255)):
        a.buf[pos] = 0x11
        got = a.check()
        assert len(got) == 1, got
        assert (got[0].name, got[0].side, got[0].offset, got[0].length) == (who, side, off, 1), got
        assert bytes(got[0].data) == b"\x11"
        a.buf[pos] = 0x5A
        assert a.check() == []
    # a run that spills three bytes past the end, and one byte in front, at once: two reports, in address order
    a.buf[e:e + 3] = 0
    a.buf[s - 1] = 0
    got = a.check()
    assert [(g.name, g.side, g.offset, g.length) for g in got] == [(who, "before", -1, 1), (who, "behind", 1, 3)], got


def test_a_stray_byte_equal_to_the_canary_shows_after_a_repaint():
    """Why every case runs under two canaries: a spilled 0x5A is invisible on 0x5A."""
    a, q, f, w = _arena(0x5A)
    e = a.spans[0][1]
    a.buf[e] = 0x5A
    assert a.check() == []
    q.fill_(9)
    a.repaint(0xA5)
    assert (q == 9).all() and (f == 1.5).all()                 # placements keep their contents
    assert a.check() == []
    a.buf[e] = 0x5A
    got = a.check()
    assert [(g.name, g.side, g.offset, g.length) for g in got] == [("q", "behind", 1, 1)]


def test_pattern_canary_reads_as_one_float_at_every_element_address():
    nan = np.array([np.nan], np.float32).tobytes()
    a = Arena(CPU, Arena.room(4 * 6), nan)
    x = a.place((2, 3), torch.float32, 4, fill=np.arange(6, dtype=np.float32).reshape(2, 3), name="x")
    assert x.flatten().tolist() == [0, 1, 2, 3, 4, 5]
    s, e, _ = a.spans[0]
    around = torch.cat([a.buf[s - 64:s], a.buf[e:e + 64]]).view(torch.float32)
    assert torch.isnan(around).all()
    a.repaint(np.array([-3e38], np.float32).tobytes())
    around = torch.cat([a.buf[s - 64:s], a.buf[e:e + 64]]).view(torch.float32)
    assert (around == np.float32(-3e38)).all() and a.check() == []
    a.buf[e + 4] ^= 1
    assert [(g.side, g.offset) for g in a.check()] == [("behind", 5)]


def test_refusals():
    a = Arena(CPU, Arena.room(64))
    for dtype, off in ((torch.float32, 2), (torch.float32, 7), (torch.int16, 1), (torch.float64, 4), (torch.int8, 256), (torch.int8, -1)):
        with pytest.raises(ValueError, match="offset_mod"):
            a.place(4, dtype, off)
    assert a.spans == []
    with pytest.raises(ValueError, match="cannot hold"):
        a.place(4096, torch.uint8)
    with pytest.raises(ValueError, match="fill is"):
        a.place((2, 2), torch.float32, 0, fill=np.zeros((2, 2), np.float64))
    with pytest.raises(ValueError, match="canary"):
        Arena(CPU, 1024, b"\x01\x02\x03")


def test_room_holds_its_placements_at_the_worst_offsets():
    sizes = (1, 255, 256, 257, 4 * 1001)
    a = Arena(CPU, Arena.room(*sizes))
    for n in sizes:
        a.place(n, torch.uint8, 255)
    assert a.check() == []
