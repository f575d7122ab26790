#!/usr/bin/env python3
"""8-bit image fixtures made by the reference.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference's sources).

The reference feeds its super-resolution nets (MFLAG 5: SESR-x4, Y in / Y out; MFLAG 6: SESR-x2, RGB) from 8-bit PNGs through its own
dataset class (self_dataset_sr.py TestDataset.__getitem__): the LR image (``LRbicx4`` / ``LRbicx2``) and the HR ground truth
(``GTmod12``) are read as uint8 BGR, flipped to RGB and divided by 255 in float64; MFLAG 5 then forms the luma
(65.481 R + 128.553 G + 24.966 B + 16) / 255 in float64, clipped.  This script puts stub ``cv2`` / ``h5py`` / ``scipy.io`` modules in
``sys.modules`` (the ``imread`` stub hands back synthetic uint8 BGR images for the GTmod12 / LRbicx4 / LRbicx2 paths) and calls the
reference's own ``TestDataset.__getitem__`` on an instance made with ``object.__new__``.  It harvests ``inp`` and ``gt``, calibrates
each net on frame (b) with the reference's mode-0 pass (as the *_nat cases of make_golden.py do: ``x4sesr.pth`` and ``sr_qat_G.pth``
for MFLAG 5, the seeded random x2 init for MFLAG 6), runs the reference's integer simulation on every frame and harvests ``input.0``
and the fp32 output.  MFLAG 6 adds the eval loop's anchor (test.py:148-155, gfake + inps_x2).  The export bytes are the reference's
PNG export (sim.py:163-168) applied to the fp32 output (the anchored one for MFLAG 6): np.clip(., 0, 1) * 255.0 in fp32, RGB -> BGR
(cvtColor is a channel flip), astype(np.uint8).

Frames (LR size; the HR image is 4x (MFLAG 5) or 2x (MFLAG 6) of it):
  (a) 24 x 64: every byte code in every channel position (three permutations of 0 .. 255), the extremes and primaries, then seeded
      random triples; random HR bytes
  (b) a natural-ish 80 x 960 LR frame (natural.py x 255) with a natural-ish HR frame
  (c) an odd-size 75 x 101 one

Output (tests/golden/image/, never the top level: every tests/golden/*.npz is taken as a net fixture).  Only what cannot be
regenerated is stored; every frame and every result is pinned by SHA-256:
  frames.npz   lr_a (24, 64, 3) uint8 RGB, hr5_a / hr6_a the HR images of frame (a) for MFLAG 5 / 6 (frames b and c: natural_image(),
               regenerated); meta.sha: SHA-256 of lr_<f>, hr<m>_<f> and of the reference's inp<m>_<f> and gt<m>_<f> (1, C, H, W) fp32
  <net>.npz    the calibrated net (Bundle.load reads it); meta.sha: SHA-256 of input0_<f> (1, C, H, W) int8, of the int8 output
               out_q_<f> (recovered from the fp32 output exactly), of the fp32 output out_<f>, for MFLAG 6 of the anchored output
               anchored_<f>, and of the export bytes png_rgb_<f> / png_bgr_<f> (1, H', W', C) uint8

Usage:  python tests/golden/make_image_golden.py
"""
import hashlib
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "image")
NETS = {"sesr_x4": dict(mflag=5, ckpt="model_params/x4sesr.pth", qat=False),
        "sesr_x4_qat": dict(mflag=5, ckpt="model_params/sr_qat_G.pth", qat=True),
        # x2sesr.pth.tar is refused by torch.load(weights_only=True): the reference's own random init, seeded (make_golden.py)
        "sesr_x2_rand": dict(mflag=6, ckpt=None, qat=False, seed=1234)}
FRAMES = ("a", "b", "c")
CAL_FRAME = "b"
UP = {5: 4, 6: 2}
LR_DIR = {5: "LRbicx4", 6: "LRbicx2"}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


NATURAL = {"b": (80, 960, 5101), "c": (75, 101, 5102)}     # frame -> (LR H, LR W, natural_frame seed; the HR one uses seed + 50)


def natural_image(f, mflag):
    """Frames (b) and (c): (LR (H, W, 3) uint8 RGB, HR (uH, uW, 3) uint8 RGB), regenerated the same anywhere (natural.py)."""
    sys.path.insert(0, HERE)
    from natural import natural_frame
    h, w, seed = NATURAL[f]
    u = UP[mflag]

    def u8(x):
        return np.rint(x[0].astype(np.float64) * 255).astype(np.uint8).transpose(1, 2, 0).copy()
    return u8(natural_frame(3, h, w, seed)), u8(natural_frame(3, u * h, u * w, seed + 50))


def frame_a():
    """(LR (24, 64, 3), {mflag: HR}) uint8 RGB: every code at every channel position, extremes and primaries, random rest."""
    rng = np.random.default_rng(255)
    H, W = 24, 64
    v = np.arange(256)
    lr = rng.integers(0, 256, (H * W, 3))
    lr[:256] = np.stack([v, rng.permutation(v), rng.permutation(v)], 1)
    lr[256:512] = np.stack([rng.permutation(v), v, rng.permutation(v)], 1)
    lr[512:768] = np.stack([rng.permutation(v), rng.permutation(v), v], 1)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)]
                       + [[1, 0, 0], [0, 1, 0], [0, 0, 1], [254, 255, 255], [128, 128, 128], [127, 127, 127]])
    lr[768:768 + len(corners)] = corners
    lr = lr.astype(np.uint8).reshape(H, W, 3)
    hr = {m: rng.integers(0, 256, (UP[m] * H, UP[m] * W, 3)).astype(np.uint8) for m in (5, 6)}
    return lr, hr


def make_frames():
    """{(frame, mflag): (LR, HR)} uint8 RGB (H, W, 3)"""
    lr_a, hr_a = frame_a()
    out = {}
    for m in (5, 6):
        out[("a", m)] = (lr_a, hr_a[m])
        for f in NATURAL:
            out[(f, m)] = natural_image(f, m)
    return out


def export_bytes(y, bgr):
    """sim.py:163-168 on a (1, C, H, W) fp32 output: clip, * 255.0 (fp32), RGB -> BGR (a channel flip), astype(uint8) -> (1, H, W, C)."""
    g = np.clip(y[0].transpose(1, 2, 0), 0, 1)
    s = g * 255.0
    assert s.dtype == np.float32
    if bgr and s.shape[2] == 3:
        s = np.ascontiguousarray(s[:, :, ::-1])
    return s.astype(np.uint8)[None]


def main():
    sys.dont_write_bytecode = True
    frames = make_frames()
    scratch = tempfile.mkdtemp(prefix="imagegolden")
    cwd = os.getcwd()
    os.chdir(scratch)
    try:
        run(frames, scratch)
    finally:
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)


def run(frames, scratch):
    # ---- the reference's dataset class on stub cv2 / h5py / scipy.io
    images_bgr = {}
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2RGB, cv2.COLOR_RGB2BGR = 4, 4
    cv2.imread = lambda path, flag=None: images_bgr[path].copy()
    cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[:, :, ::-1])
    sys.modules["cv2"] = cv2
    sys.modules["h5py"] = types.ModuleType("h5py")
    sio = types.ModuleType("scipy.io")
    sio.loadmat = lambda *a, **k: None
    sys.modules["scipy.io"] = sio
    sys.path.insert(0, REF)
    import torch
    import define
    define.MFLAG = 5
    import self_dataset_sr

    fx, fsha = {}, {}
    for m in (5, 6):
        paths = []
        for f in FRAMES:
            lr, hr = frames[(f, m)]
            gtp = os.path.join(scratch, f"x{UP[m]}", "GTmod12", f"frame{f}.png")
            images_bgr[gtp] = np.ascontiguousarray(hr[:, :, ::-1])
            images_bgr[gtp.replace("GTmod12", LR_DIR[m])] = np.ascontiguousarray(lr[:, :, ::-1])
            paths.append(gtp)
        ds = object.__new__(self_dataset_sr.TestDataset)
        ds.rggb, ds.ps, ds.mflag = paths, 128, m
        for i, f in enumerate(FRAMES):
            inp, gt = ds[i]
            assert inp.dtype == torch.float32 and gt.dtype == torch.float32
            fx[f"inp{m}_{f}"] = inp.numpy()[None]
            fx[f"gt{m}_{f}"] = gt.numpy()[None]
            fsha[f"lr_{f}"] = sha(frames[(f, m)][0])
            fsha[f"hr{m}_{f}"] = sha(frames[(f, m)][1])
            fsha[f"inp{m}_{f}"] = sha(fx[f"inp{m}_{f}"])
            fsha[f"gt{m}_{f}"] = sha(fx[f"gt{m}_{f}"])
    keep = dict(lr_a=frames[("a", 5)][0], hr5_a=frames[("a", 5)][1], hr6_a=frames[("a", 6)][1])
    keep["meta"] = np.array(json.dumps(dict(natural=NATURAL, up=UP, sha=fsha)))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "frames.npz"), **keep)
    print("[frames]", {k: v.shape for k, v in fx.items()}, flush=True)

    # ---- the nets: calibrated on frame (b) by the reference's mode-0 pass, then its integer simulation on every frame
    from torch import nn
    from myQL import quan_func as qf
    from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
    from myQL.graph_modify import insert_before, insert_bias_bypass, insert_after
    from models import sesr, sesr_sim, sesr_arch, sesr_arch_sim

    def pack(fn, kw):
        mp = NodeInsertMapping()
        mp.add_config(NodeInsertMappingElement(nn.Conv2d, FunctionPackage(fn, kw)))
        return mp

    def splice(model, qmode):
        model = qf.quantize_model_weight(model, define.QUAN_BIT, qmode)
        mp = NodeInsertMapping()
        fp = FunctionPackage(qf.quantize_asymmetrical_by_tensor, {"width": define.QUAN_BIT, "exe_mode": qmode})
        mp.add_config(NodeInsertMappingElement(nn.Conv2d, fp))
        if qmode == 0:
            mp.add_config(NodeInsertMappingElement(nn.PixelShuffle, fp))
        model = insert_before(model_input=model, insert_mapping=mp, has_func_id=True)
        model = insert_before(model_input=model, insert_mapping=pack(qf.reshape_input_for_hardware_pe, {"pe_num": define.PE}))
        if qmode == 1:
            model = insert_after(model_input=model, insert_mapping=pack(qf.requan_conv2d_output, {"exe_mode": 1}))
        return insert_bias_bypass(model_input=model, insert_mapping=pack(
            qf.PEs_and_bias_adder, {"pe_add_width": define.PE_ADD_BIT, "pe_acc_width": define.PE_ACC_BIT,
                                    "bias_width": define.BIAS_BIT, "pe_num": define.PE, "exe_mode": qmode}))

    for net, cfg in NETS.items():
        m = cfg["mflag"]
        qf.MFLAG = define.MFLAG = m
        shutil.rmtree("output_pt", ignore_errors=True)
        float_cls, sim_cls = {5: (sesr.sesr, sesr_sim.sesr), 6: (sesr_arch.sesr, sesr_arch_sim.sesr)}[m]
        if cfg["ckpt"] is None:        # random init: the float and the sim model share weights -> build once, copy
            torch.manual_seed(cfg["seed"])
            proto_sd = {k: v.clone() for k, v in float_cls().state_dict().items()}

        def make(cls):
            mdl = cls()
            if cfg["ckpt"] is None:
                mdl.load_state_dict(proto_sd, strict=False)
            mdl.train()
            if cfg["qat"]:
                from models import quantize_utils_pt as quantize
                quantize.prepare(mdl, inplace=True, a_bits=8, w_bits=8, q_type=0, q_level="C")
            if cfg["ckpt"] is not None:
                mdl.load_state_dict(torch.load(os.path.join(REF, cfg["ckpt"]), weights_only=True, map_location="cpu"), strict=False)
            mdl = mdl.float()
            mdl.collapse()
            return mdl

        x_cal = torch.from_numpy(fx[f"inp{m}_{CAL_FRAME}"])
        with torch.no_grad():
            splice(make(float_cls), 0)(x_cal)
        for i in range(6):                 # test.py:185-217: (scale, zero) from the running ranges; the output domain from 0
            mx = torch.load(f"output_pt/input/input.{i}.max_val.pt")
            mn = 0 if i == 5 else torch.load(f"output_pt/input/input.{i}.min_val.pt")
            s = (mx - mn) / 255
            torch.save(s, f"output_pt/input/input.{i}.scale.pt")
            torch.save(-128 - round(mn / s), f"output_pt/input/input.{i}.zero.pt")
        ld = torch.load
        d, sh = {}, {}
        for f in FRAMES:
            x = torch.from_numpy(fx[f"inp{m}_{f}"])
            with torch.no_grad():
                y = splice(make(sim_cls), 1)(x)
            q0 = ld("output_pt/input/input.0.pt").numpy()
            assert np.all(q0 == np.rint(q0)) and q0.min() >= -128 and q0.max() <= 127
            sh[f"input0_{f}"] = sha(q0.astype(np.int8))
            s5 = np.float32(ld("output_pt/input/input.5.scale.pt"))
            z5 = int(ld("output_pt/input/input.5.zero.pt"))
            yf = y.numpy().astype(np.float32)
            yq = np.rint(yf.astype(np.float64) / np.float64(s5) + z5)
            assert yq.min() >= -128 and yq.max() <= 127
            yq = yq.astype(np.int8)
            assert np.array_equal(((yq.astype(np.float32) - np.float32(z5)) * s5).astype(np.float32), yf)
            sh[f"out_q_{f}"] = sha(yq)
            sh[f"out_{f}"] = sha(yf)
            if m == 6:                     # test.py:148-155: inps_x2[:, :, i::2, j::2] = inps; gfake + inps_x2
                up = torch.zeros(x.shape[0], x.shape[1], x.shape[2] * 2, x.shape[3] * 2)
                up[:, :, 0::2, 0::2] = x; up[:, :, 0::2, 1::2] = x; up[:, :, 1::2, 0::2] = x; up[:, :, 1::2, 1::2] = x
                yf = (y + up).numpy().astype(np.float32)
                sh[f"anchored_{f}"] = sha(yf)
            sh[f"png_rgb_{f}"] = sha(export_bytes(yf, False))
            sh[f"png_bgr_{f}"] = sha(export_bytes(yf, True))
        L = 5
        for k in range(L):
            d[f"Wq{k}"] = ld(f"output_pt/weight/conv.weight.{k}.pt").numpy().astype(np.int8)
            d[f"add_const{k}"] = ld(f"output_pt/bias/conv.bias.quan{k}.pt").numpy().reshape(-1).astype(np.int32)
        names = ["0_1", "1_2", "2_3", "3_4", "4_5"]
        meta = dict(case=net, mflag=m, calibrated_on=f"frame {CAL_FRAME}",
                    scale=[float(ld(f"output_pt/input/input.{k}.scale.pt")) for k in range(6)],
                    zero=[int(ld(f"output_pt/input/input.{k}.zero.pt")) for k in range(6)],
                    M=[int(ld(f"output_pt/requan_factor/requan_{n}.pt")) for n in names],
                    n=[int(ld(f"output_pt/requan_factor/n_{n}.pt")) for n in names],
                    M_res=int(ld("output_pt/requan_factor/requan_res.pt")), n_res=int(ld("output_pt/requan_factor/n_res.pt")),
                    sha=sh)
        d["meta"] = np.array(json.dumps(meta))
        np.savez_compressed(os.path.join(OUT, f"{net}.npz"), **d)
        print(f"[{net}] scale0={meta['scale'][0]} zero={meta['zero']} M={meta['M']} n={meta['n']}", flush=True)


if __name__ == "__main__":
    main()
