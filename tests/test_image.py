"""8-bit images into and out of the super-resolution nets (sesrq.image, libsesrq_image.so, Engine.forward_image, quality.evaluate_image,
sim.py --input *.png / --save-png) against the reference's own dataset class, integer simulation and PNG export (tests/golden/image/,
made by make_image_golden.py) and against the numpy restatement (tests/image_oracle.py).

CPU: the C ABI, the argument checks, the fixtures' SHA-256 values, the restatement against the reference's inp / gt / input.0 and
export bytes, load_image.  GPU: decode against the reference and, exhaustively, against the restatement; load_gt; forward_image against
the reference's outputs and against forward() on the fp32 frame; evaluate_image; export; sim.py; a side stream; the refusals; and
that every kernel instantiation ran."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import device, sha256

import image_oracle as IO

IMG = os.path.join(GOLDEN, "image")
HEADER = os.path.join(ROOT, "include", "sesrq_image.h")
NETS = {"sesr_x4": 5, "sesr_x4_qat": 5, "sesr_x2_rand": 6}
FRAMES = ("a", "b", "c")
FORM = {5: "y", 6: "rgb"}


def frames():
    return np.load(os.path.join(IMG, "frames.npz"), allow_pickle=False)


def frames_sha():
    return json.loads(str(frames()["meta"]))["sha"]


def net_fixture(net):
    z = np.load(os.path.join(IMG, net + ".npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def frame(f, mflag):
    """(LR (H, W, 3), HR (uH, uW, 3)) uint8 RGB of frame f for MFLAG 5 / 6, the bytes the reference ran on: frame (a) is stored, (b)
    and (c) are regenerated (make_image_golden.natural_image)."""
    if f == "a":
        F = frames()
        lr, hr = F["lr_a"], F[f"hr{mflag}_a"]
    else:
        sys.path.insert(0, GOLDEN)
        from make_image_golden import natural_image
        lr, hr = natural_image(f, mflag)
    s = frames_sha()
    assert sha256(lr) == s[f"lr_{f}"] and sha256(hr) == s[f"hr{mflag}_{f}"], f"frame {f} differs from the one the reference ran on"
    return lr, hr


def ref_inp(f, mflag):
    """The reference's fp32 input frame (1, C, H, W), restated and checked against its SHA-256."""
    x = IO.decode(frame(f, mflag)[0], FORM[mflag])
    assert sha256(x) == frames_sha()[f"inp{mflag}_{f}"], (f, mflag)
    return x


def ref_gt(f, mflag):
    g = IO.decode(frame(f, mflag)[1], FORM[mflag])
    assert sha256(g) == frames_sha()[f"gt{mflag}_{f}"], (f, mflag)
    return g


def bgr(img):
    return np.ascontiguousarray(img[..., ::-1])


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_fixture_frames_hold_their_sha_and_frame_a_every_code():
    s = frames_sha()
    for m in (5, 6):
        for f in FRAMES:
            lr, hr = frame(f, m)
            assert lr.dtype == np.uint8 and lr.shape[2] == 3 and hr.shape == (lr.shape[0] * {5: 4, 6: 2}[m], lr.shape[1] * {5: 4, 6: 2}[m], 3)
    assert frame("c", 5)[0].shape[:2] == (75, 101) and frame("b", 6)[0].shape[:2] == (80, 960)
    lr = frame("a", 5)[0].reshape(-1, 3)
    for c in range(3):
        assert set(lr[:, c].tolist()) == set(range(256)), c
    for t in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)):
        assert (lr == t).all(1).any(), t
    for net in NETS:
        z, meta = net_fixture(net)
        assert meta["mflag"] == NETS[net] and len(meta["sha"]) >= 15
    assert len(s) == 3 + 3 * 6          # lr per frame; hr, inp, gt per frame and MFLAG


@pytest.mark.parametrize("mflag", [5, 6])
def test_restatement_equals_reference_inp_gt_and_input0(mflag):
    for f in FRAMES:
        ref_inp(f, mflag), ref_gt(f, mflag)            # SHA-checked inside
        for bo in ("rgb", "bgr"):                       # the byte order is the caller's: a BGR image gives the same frame
            lr = frame(f, mflag)[0]
            assert np.array_equal(IO.decode(bgr(lr) if bo == "bgr" else lr, FORM[mflag], bo), ref_inp(f, mflag))
    for net, m in NETS.items():
        if m != mflag:
            continue
        _, meta = net_fixture(net)
        for f in FRAMES:
            assert sha256(IO.q0(ref_inp(f, m), meta["scale"][0], meta["zero"][0])) == meta["sha"][f"input0_{f}"], (net, f)


@pytest.mark.parametrize("net", ["sesr_x4", "sesr_x2_rand"])
def test_export_restatement_equals_reference_bytes(net):
    """The oracle's forward of the small frames hashes to the reference's fp32 output; the restated export of that output (anchored
    for MFLAG 6) hashes to the reference's sim.py export bytes, in RGB and BGR order."""
    from oracle import sesrq_oracle as O
    z, meta = net_fixture(net)
    m = NETS[net]
    onet = O.net_from_fixture(z)
    for f in ("a", "c"):
        x = ref_inp(f, m)
        st = O.forward(onet, x)
        y = st["y"].astype(np.float32)
        assert sha256(y) == meta["sha"][f"out_{f}"] and sha256(st["q_out"]) == meta["sha"][f"out_q_{f}"], (net, f)
        if m == 6:
            y = (y + IO.upsample2(x)).astype(np.float32)
            assert sha256(y) == meta["sha"][f"anchored_{f}"]
        else:
            assert np.array_equal(IO.dequant(st["q_out"], np.float32(meta["scale"][5]), meta["zero"][5]), y)
        for bo in ("rgb", "bgr"):
            assert sha256(IO.export(y, bo)) == meta["sha"][f"png_{bo}_{f}"], (net, f, bo)


def test_rgb_table_equals_the_restatement():
    from sesrq import image as I
    codes = np.arange(256, dtype=np.uint8)
    x_ref = IO.decode_rgb(np.stack([codes] * 3, 1)[None])[0, 0, 0]
    for s0, z0 in ((0.0022352789546929153, -214), (0.0039, -128), (0.0052, -120)):
        for ed in (0, 1, 2):
            q, x = I.table(s0, z0, ed)
            assert x.tobytes() == x_ref.tobytes()
            assert np.array_equal(q, IO.q0(x_ref, s0, z0, ed)), (s0, z0, ed)
    for s0, z0, ed in ((0.0, -128, 0), (float("nan"), 0, 0), (0.01, -128, 3), (0.01, 1 << 25, 0)):
        with pytest.raises(ValueError, match="sesrq_image_table"):
            I.table(s0, z0, ed)


def test_form_of_and_names():
    from sesrq import image as I
    assert I.form_of(5) == "y" and I.form_of(6) == "rgb"
    for m in (1, 2, 3, 4, 7):
        with pytest.raises(ValueError, match="super-resolution"):
            I.form_of(m)
    with pytest.raises(ValueError, match="form"):
        I._form("yuv")
    with pytest.raises(ValueError, match="order"):
        I._order("rbg")


def test_load_image_npy_and_png(tmp_path):
    from sesrq import image as I
    a = frame("c", 6)[0]
    np.save(str(tmp_path / "lr.npy"), a)
    got = I.load_image(str(tmp_path / "lr.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, a)
    np.save(str(tmp_path / "bad.npy"), a.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        I.load_image(str(tmp_path / "bad.npy"))
    with pytest.raises(ValueError, match="png"):
        I.load_image(str(tmp_path / "lr.jpg"))
    pytest.importorskip("PIL")
    I.save_png(str(tmp_path / "lr.png"), a)
    assert np.array_equal(I.load_image(str(tmp_path / "lr.png")), a)
    I.save_png(str(tmp_path / "grey.png"), a[:, :, :1])
    g = I.load_image(str(tmp_path / "grey.png"))
    assert g.shape == a.shape and np.array_equal(g, np.repeat(a[:, :, :1], 3, axis=2))


def test_image_library_exports_exactly_the_header():
    from sesrq import image as I
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sesrq_image[a-z_0-9]*)\s*\(", src)))
    assert len(names) == 9, names
    assert sorted(I.SYMBOLS) == names, "python binding and header disagree"
    nm = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r" T (sesrq\w*)", nm))) == names


def test_libsesrq_instances_unchanged_by_the_image_library():
    from sesrq import _lib, image as I
    before = _lib.instances()
    assert len(before) == 258
    assert len(I.instances()) == 10
    after = _lib.instances()
    assert sorted(before) == sorted(after)
    assert not any("image" in n for n in after)


def test_decode_and_export_argument_checks_without_a_device():
    import ctypes as C
    from sesrq import image as I
    lib = I.lib()
    fake = C.c_void_p(4096)                       # never dereferenced: every failing check comes before any HIP call
    assert lib.sesrq_image_decode(None, fake, 0, 0, fake, fake, 1, 8, 8, None) != 0 and "ctx is NULL" in I.last_error()
    assert lib.sesrq_image_create(1.0, 0, 0, None) != 0 and "NULL" in I.last_error()
    for args, msg in (((None, 0, 1.0, 0, 3, 0, fake, 1, 8, 8, None), "pred is NULL"),
                      ((fake, 0, 1.0, 0, 3, 0, None, 1, 8, 8, None), "out is NULL"),
                      ((fake, 2, 1.0, 0, 3, 0, fake, 1, 8, 8, None), "pred_dtype"),
                      ((fake, 1, 0.0, 0, 3, 0, fake, 1, 8, 8, None), "scale"),
                      ((fake, 1, 0.01, 200, 3, 0, fake, 1, 8, 8, None), "int8 range"),
                      ((fake, 0, 1.0, 0, 2, 0, fake, 1, 8, 8, None), "channels"),
                      ((fake, 0, 1.0, 0, 3, 5, fake, 1, 8, 8, None), "order"),
                      ((fake, 0, 1.0, 0, 3, 0, fake, 0, 8, 8, None), "empty frame"),
                      ((fake, 0, 1.0, 0, 3, 0, fake, 1 << 20, 1 << 12, 1 << 12, None), "too large")):
        assert lib.sesrq_image_export(*args) != 0 and msg in I.last_error(), (msg, I.last_error())
    assert lib.sesrq_image_instance_name(10) is None and lib.sesrq_image_instance_launches(-1) == -1


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _bundle(net):
    from sesrq.bundle import Bundle
    return Bundle.load(os.path.join(IMG, net + ".npz"))


def _engine(net, **kw):
    import sesrq
    return sesrq.Engine(_bundle(net), device(), **kw)


def _u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(device())


def _batch(lr, n):
    """n images of lr's size: lr itself first, then its pixels shuffled (seeded)."""
    rng = np.random.default_rng(11)
    px = lr.reshape(-1, 3)
    return np.stack([lr] + [px[rng.permutation(len(px))].reshape(lr.shape) for _ in range(n - 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("net", ["sesr_x4", "sesr_x2_rand"])
def test_decode_equals_reference_inp_and_input0(net, N, order):
    import torch
    from sesrq import image as I
    m = NETS[net]
    b = _bundle(net)
    _, meta = net_fixture(net)
    for f in FRAMES:
        imgs = _batch(frame(f, m)[0], N)
        dimg = _u8(bgr(imgs) if order == "bgr" else imgs)
        q_both, x_both = I.decode(b, dimg, FORM[m], order=order, want_q=True, want_f=True)
        q_only, _ = I.decode(b, dimg if N > 1 else dimg[0], FORM[m], order=order)
        _, x_only = I.decode(None, dimg, FORM[m], order=order, want_q=False, want_f=True)
        torch.cuda.synchronize()
        for q in (q_both, q_only):
            q = q.cpu().numpy()
            assert sha256(q[:1]) == meta["sha"][f"input0_{f}"], (net, f)
            for n in range(1, N):
                assert np.array_equal(q[n], IO.q0(IO.decode(imgs[n], FORM[m]), b.scale[0], b.zero[0])[0]), (f, n)
        for x in (x_both, x_only):
            x = x.cpu().numpy()
            assert sha256(x[:1]) == frames_sha()[f"inp{m}_{f}"], (net, f)
            for n in range(1, N):
                assert x[n].tobytes() == IO.decode(imgs[n], FORM[m])[0].tobytes(), (f, n)


def _all_triples():
    """Every (R, G, B) triple once: a 4096 x 4096 x 3 uint8 image."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], 1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.gpu
def test_decode_y_exhaustive_every_triple():
    """All 2^24 triples: x and q0 of the Y form equal the restatement under exact_div 0, 1 and 2 (two input domains), both orders."""
    import torch
    from sesrq import image as I
    img = _all_triples()
    x_ref = IO.decode_y(img[None])
    d = _u8(img[None])
    db = _u8(bgr(img)[None])
    q = torch.empty((1, 1, 4096, 4096), dtype=torch.int8, device=device())
    x = torch.empty((1, 1, 4096, 4096), dtype=torch.float32, device=device())
    st = torch.cuda.current_stream(device())
    for s0, z0 in ((0.0022352789546929153, -214), (0.0037, -145)):
        for ed in (0, 1, 2):
            for src, order in ((d, "rgb"), (db, "bgr")):
                I.launch(device(), s0, z0, ed, src, "y", order, q, x, st)
                torch.cuda.synchronize()
                assert x.cpu().numpy().tobytes() == x_ref.tobytes(), (s0, ed, order)
                assert np.array_equal(q.cpu().numpy(), IO.q0(x_ref, s0, z0, ed)), (s0, z0, ed, order)


@pytest.mark.gpu
def test_decode_rgb_exhaustive_every_code():
    import torch
    from sesrq import image as I
    codes = np.arange(256, dtype=np.uint8)
    img = np.stack([codes, codes[::-1], np.roll(codes, 77)], 1).reshape(16, 16, 3)
    x_ref = IO.decode_rgb(img[None])
    for s0, z0 in ((0.0039215, -128), (0.0052, -120)):
        for ed in (0, 1, 2):
            for order in ("rgb", "bgr"):
                d = _u8((bgr(img) if order == "bgr" else img)[None])
                q = torch.empty((1, 3, 16, 16), dtype=torch.int8, device=device())
                x = torch.empty((1, 3, 16, 16), dtype=torch.float32, device=device())
                I.launch(device(), s0, z0, ed, d, "rgb", order, q, x, torch.cuda.current_stream(device()))
                torch.cuda.synchronize()
                assert x.cpu().numpy().tobytes() == x_ref.tobytes(), (s0, ed, order)
                assert np.array_equal(q.cpu().numpy(), IO.q0(x_ref, s0, z0, ed)), (s0, z0, ed, order)


@pytest.mark.gpu
def test_load_gt_equals_reference_gt():
    from sesrq import image as I
    for m in (5, 6):
        for f in FRAMES:
            hr = frame(f, m)[1]
            g = I.load_gt(hr, m, device()).cpu().numpy()
            assert g.dtype == np.float32 and sha256(g) == frames_sha()[f"gt{m}_{f}"], (m, f)
            assert sha256(I.load_gt(bgr(hr), m, device(), order="bgr").cpu().numpy()) == frames_sha()[f"gt{m}_{f}"]


@pytest.mark.gpu
@pytest.mark.parametrize("net", list(NETS))
def test_forward_image_equals_reference_outputs(net):
    import torch
    m = NETS[net]
    _, meta = net_fixture(net)
    e = _engine(net, anchor_add=m == 6)
    for f in FRAMES:
        for order in ("rgb", "bgr"):
            lr = frame(f, m)[0]
            q, y = e.forward_image(_u8(bgr(lr) if order == "bgr" else lr), order=order)
            torch.cuda.synchronize()
            assert sha256(q.cpu().numpy()) == meta["sha"][f"out_q_{f}"], (net, f)
            assert sha256(y.cpu().numpy()) == meta["sha"][f"anchored_{f}" if m == 6 else f"out_{f}"], (net, f)


@pytest.mark.gpu
@pytest.mark.parametrize("anchor", [False, True])
def test_forward_image_equals_forward_on_the_fp32_frame_1080p(anchor):
    import torch
    from sesrq import image as I
    rng = np.random.default_rng(1080)
    img = rng.integers(0, 256, (1, 1080, 1920, 3)).astype(np.uint8)
    e = _engine("sesr_x2_rand", anchor_add=anchor)
    d = _u8(img)
    q, y = e.forward_image(d)
    _, x = I.decode(None, d, "rgb", want_q=False, want_f=True)
    q2, y2 = e.forward(x)
    torch.cuda.synchronize()
    assert x.cpu().numpy().tobytes() == IO.decode_rgb(img).tobytes()
    assert q.cpu().numpy().tobytes() == q2.cpu().numpy().tobytes() and y.cpu().numpy().tobytes() == y2.cpu().numpy().tobytes()
    q3, none = e.forward_image(d, want_f=False, slot=1)
    torch.cuda.synchronize()
    assert none is None and torch.equal(q3, q)


@pytest.mark.gpu
def test_evaluate_image_equals_evaluate_on_the_fp32_frames():
    import torch
    from sesrq import quality
    for net, m in NETS.items():
        e = _engine(net, anchor_add=m == 6)
        lrs = [frame(f, m)[0] for f in FRAMES]
        hrs = [frame(f, m)[1] for f in FRAMES]
        got = quality.evaluate_image(e, lrs, hrs, m)
        want = quality.evaluate(e, [torch.from_numpy(ref_inp(f, m)) for f in FRAMES], [torch.from_numpy(ref_gt(f, m)) for f in FRAMES], m)
        assert got.shape == (3, 3) and got.tobytes() == want.tobytes(), net
        got_bgr = quality.evaluate_image(e, [bgr(a) for a in lrs], [bgr(a) for a in hrs], m, order="bgr")
        assert got_bgr.tobytes() == want.tobytes(), net
    with pytest.raises(ValueError, match="anchor_add"):
        quality.evaluate_image(_engine("sesr_x2_rand"), lrs, hrs, 6)
    with pytest.raises(ValueError, match="super-resolution"):
        quality.evaluate_image(e, lrs, hrs, 3)


@pytest.mark.gpu
def test_export_equals_restatement_and_reference_bytes():
    import torch
    from sesrq import image as I
    rng = np.random.default_rng(255)
    # fp32 and int8 predictions of odd and aligned sizes, values around and outside [0, 1], both orders, 1 and 3 channels
    for shape in ((1, 3, 7, 9), (2, 3, 16, 32), (3, 1, 5, 33), (1, 1, 64, 64), (2, 3, 75, 101)):
        p = (rng.standard_normal(shape) * 0.6 + 0.5).astype(np.float32)
        p.reshape(-1)[:6] = [0.0, 1.0, -0.0, 1.0000001, np.float32(254.5 / 255), np.float32(1 / 255)]
        qi = rng.integers(-128, 128, shape).astype(np.int8)
        for order in ("rgb", "bgr"):
            got = I.export(torch.from_numpy(p).to(device()), order=order).cpu().numpy()
            assert np.array_equal(got, IO.export(p, order)), (shape, order)
            for s, z in ((0.0049, -128), (0.0031, -77)):
                got = I.export(torch.from_numpy(qi).to(device()), order=order, scale=s, zero=z).cpu().numpy()
                assert np.array_equal(got, IO.export(IO.dequant(qi, np.float32(s), z), order)), (shape, order, s)
    # the nets' outputs: int8 (MFLAG 5) and the anchored fp32 x2 output against the reference's export bytes
    for net, m in NETS.items():
        _, meta = net_fixture(net)
        e = _engine(net, anchor_add=m == 6)
        L = e.bundle.L
        for f in FRAMES:
            q, y = e.forward_image(_u8(frame(f, m)[0]))
            for order in ("rgb", "bgr"):
                assert sha256(I.export(y, order=order).cpu().numpy()) == meta["sha"][f"png_{order}_{f}"], (net, f, order)
                if m == 5:
                    u = I.export(q, order=order, scale=e.bundle.scale[L], zero=e.bundle.zero[L]).cpu().numpy()
                    assert sha256(u) == meta["sha"][f"png_{order}_{f}"], (net, f, order)
    with pytest.raises(ValueError, match="scale and zero"):
        I.export(q)
    with pytest.raises(ValueError, match="channels"):
        I.export(torch.zeros((1, 2, 4, 4), device=device()))


@pytest.mark.gpu
def test_sim_png_input_gt_and_save_png(capsys, tmp_path):
    pytest.importorskip("PIL")
    import sim
    from sesrq import image as I
    from sesrq.store import STORE
    params = os.path.join(GOLDEN, "sesr_x2_rand_nat.params.npz")
    lr, hr = frame("c", 6)
    I.save_png(str(tmp_path / "lr.png"), lr)
    I.save_png(str(tmp_path / "hr.png"), hr)
    np.save(str(tmp_path / "lr_bgr.npy"), bgr(lr))
    np.save(str(tmp_path / "inp.npy"), ref_inp("c", 6))
    np.save(str(tmp_path / "gt.npy"), ref_gt("c", 6))
    STORE.clear()
    y_img = sim.main(["--mflag", "6", "--params", params, "--input", str(tmp_path / "lr.png"), "--gt", str(tmp_path / "hr.png"),
                      "--save-png", str(tmp_path / "sr.png")])
    out_img = capsys.readouterr().out.strip().split("\n")
    STORE.clear()
    y_f32 = sim.main(["--mflag", "6", "--params", params, "--input", str(tmp_path / "inp.npy"), "--gt", str(tmp_path / "gt.npy")])
    out_f32 = capsys.readouterr().out.strip().split("\n")
    STORE.clear()
    y_npy = sim.main(["--mflag", "6", "--params", params, "--input", str(tmp_path / "lr_bgr.npy"), "--image", "--order", "bgr"])
    capsys.readouterr()
    assert out_f32[-1].startswith("srx2 mean psnr is: ")
    assert out_img[-2] == out_f32[-1] and out_img[-3] == out_f32[-2] and out_img[-1].startswith("png:")
    assert y_img.cpu().numpy().tobytes() == y_f32.cpu().numpy().tobytes() == y_npy.cpu().numpy().tobytes()
    x = ref_inp("c", 6)
    want = IO.export((y_f32.cpu().numpy() + IO.upsample2(x)).astype(np.float32))[0]
    assert np.array_equal(I.load_image(str(tmp_path / "sr.png")), want)


@pytest.mark.gpu
def test_forward_image_refusals():
    import torch
    import sesrq
    from sesrq.bundle import Bundle
    lr = _u8(frame("c", 5)[0])
    e5 = _engine("sesr_x4")
    with pytest.raises(ValueError, match="3 channel"):
        e5.forward_image(lr, form="rgb")
    e6 = _engine("sesr_x2_rand", anchor_add=True)
    with pytest.raises(ValueError, match="1 channel"):
        e6.forward_image(lr, form="y")
    nrdm = Bundle.load(os.path.join(GOLDEN, "raw", "nrdm_3.npz"))
    chained = sesrq.Engine(_bundle("sesr_x2_rand"), device(), upstream=nrdm)
    with pytest.raises(ValueError, match="upstream"):
        chained.forward_image(lr)
    with pytest.raises(ValueError, match="uint8"):
        e5.forward_image(lr.to(torch.int16))
    with pytest.raises(ValueError, match="interleaved"):
        e5.forward_image(lr.permute(2, 0, 1).contiguous())
    with pytest.raises(ValueError, match="order"):
        e5.forward_image(lr, order="rbg")
    with pytest.raises(ValueError, match="ask for"):
        e5.forward_image(lr, want_q=False, want_f=False)


@pytest.mark.gpu
@pytest.mark.parametrize("net", ["sesr_x4", "sesr_x2_rand"])
def test_forward_image_on_a_side_stream(net):
    import torch
    m = NETS[net]
    e = _engine(net, anchor_add=m == 6)
    want = net_fixture(net)[1]["sha"]["out_q_b"]
    dev = device()
    side = torch.cuda.Stream(device=dev)
    src = torch.from_numpy(frame("b", m)[0].astype(np.int32)).to(dev)
    for _ in range(3):
        x = (src * 1).to(torch.uint8)                 # produced on the current stream just before the call
        q, y = e.forward_image(x, stream=side)
        side.synchronize()
        assert sha256(q.cpu().numpy()) == want
        del x


@pytest.mark.gpu
def test_zz_every_image_instance_ran():
    """LAST in this file: every kernel instantiation libsesrq_image.so can launch was launched by a checked case above."""
    from sesrq import image as I
    k = I.instances()
    assert len(k) == 10, k
    missing = sorted(n for n, c in k.items() if c == 0)
    assert not missing, f"never launched by a checked case: {missing}"
