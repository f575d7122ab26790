#!/usr/bin/env python3
"""Raw-frame fixtures made by the reference.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference's sources).

The reference feeds its denoise / demosaic nets (MFLAG 1-4) from 12-bit RGGB raw files through its own dataset class
(self_dataset.py TestDataset.__getitem__): a uint16 ``<name>_<rows>_<cols>.raw`` frame is spread into a sparse 3-channel mosaic,
divided by 4095 in fp32 and clamped; the ground truth is a 16-bit PNG, BGR -> RGB, / 4095, clamped.  This script writes synthetic raw
files into a scratch directory (no '_' in its path other than the two size fields: the reference splits the whole path), puts stub
``cv2`` / ``h5py`` modules in ``sys.modules`` (neither is installed; the ``imread`` stub hands back a synthetic uint16 BGR ground truth),
and calls the reference's own ``TestDataset.__getitem__`` (noise off) on an instance made with ``object.__new__``.  It harvests ``inp``
and ``gt``, calibrates ``nrdm_3_raw_G.pth`` and ``nrdm_3_qat_G.pth`` on frame (b) with the reference's mode-0 pass (as the *_nat cases of
make_golden.py do), runs the reference's integer simulation on every frame and harvests ``input.0`` and the output.

Frames: (a) 132 x 128 with every code 0 .. 4095 at every Bayer phase plus 4095, 4096, 4097 and 65535; (b) a natural-ish 12-bit frame
(natural.py x 4095, mosaicked) of 80 x 960; (c) an odd-size 75 x 101 crop of another one.

Output (tests/golden/raw/, never the top level: every tests/golden/*.npz is taken as a net fixture).  Only what cannot be
regenerated is stored; every frame and every result is pinned by SHA-256:
  frames.npz      raw_a (H, W) uint16 and gt16_a (1, 3, H, W) uint16 RGB (frames b and c: natural_raw(), regenerated);
                  levels_inp / levels_gt: the fp32 value the reference gave each code 0 .. 4095 in inp / gt, read off frame (a);
                  meta.sha: SHA-256 of raw_<f>, gt16_<f> and of the reference's inp_<f> (1, 3, H, W) fp32 and gt_<f> (1, 3, H, W) fp32
  <net>.npz       the calibrated net (Bundle.load reads it), input0_a (1, 3, H, W) int8; meta.sha: SHA-256 of input0_<f>, of the
                  int8 output out_q_<f> (recovered from the fp32 output exactly) and of the fp32 output out_<f>

Usage:  python tests/golden/make_raw_golden.py
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
OUT = os.path.join(HERE, "raw")
NETS = {"nrdm_3": dict(ckpt="model_params/nrdm_3_raw_G.pth", qat=False),
        "nrdm_3_qat": dict(ckpt="model_params/nrdm_3_qat_G.pth", qat=True)}
FRAMES = ("a", "b", "c")
CAL_FRAME = "b"


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sites(H, W):
    """Site channel of every pixel: (0,0) R, (0,1) / (1,0) G, (1,1) B."""
    yy, xx = np.meshgrid(np.arange(H) & 1, np.arange(W) & 1, indexing="ij")
    return yy + xx


def mosaic(rgb):
    """(3, H, W) -> (H, W): the value at the RGGB site of every pixel."""
    return np.take_along_axis(rgb, sites(*rgb.shape[1:])[None], 0)[0]


NATURAL = {"b": (80, 960, 3101), "c": (75, 101, 3102)}     # frame -> (H, W, natural_frame seed)


def natural_raw(f):
    """Frames (b) and (c): (raw (H, W) uint16, ground truth (3, H, W) uint16 RGB), regenerated the same anywhere (natural.py)."""
    sys.path.insert(0, HERE)
    from natural import natural_frame
    h, w, seed = NATURAL[f]
    gt = np.rint(natural_frame(3, h, w, seed)[0].astype(np.float64) * 4095).astype(np.uint16)
    return mosaic(gt), gt


def make_frames():
    """{name: (raw (H, W) uint16, ground truth (3, H, W) uint16 RGB)}"""
    rng = np.random.default_rng(4095)
    H, W = 132, 128
    raw = np.zeros((H, W), np.uint16)
    for py in (0, 1):
        for px in (0, 1):
            n = (H // 2) * (W // 2)
            codes = np.concatenate([np.arange(4096), [4095, 4096, 4097, 65535],
                                    rng.integers(0, 65536, n - 4100)]).astype(np.uint16)
            raw[py::2, px::2] = rng.permutation(codes).reshape(H // 2, W // 2)
    gt_a = rng.integers(0, 4096, (3, H, W)).astype(np.uint16)
    gt_a.reshape(-1)[:4096] = np.arange(4096)                  # every code once in the ground truth as well
    gt_a[:, :2, :3] = [[[4095, 4096, 65535]]]          # the ground truth's clamp too
    out = {"a": (raw, gt_a)}
    for name in NATURAL:
        out[name] = natural_raw(name)
    return out


def per_code(codes, values):
    """The value the reference gave each code 0 .. 4095 (codes above 4095 clamp to 4095's); every code must occur, consistently."""
    c = np.minimum(codes, 4095).ravel()
    v = values.ravel()
    lv = np.full(4096, np.nan, np.float32)
    lv[c] = v
    assert not np.isnan(lv).any() and np.array_equal(lv[c], v)
    return lv


def main():
    sys.dont_write_bytecode = True
    frames = make_frames()
    scratch = os.path.join(tempfile.gettempdir(), f"rawgolden{os.getpid()}")
    assert "_" not in scratch, "the reference splits the whole path at '_'"
    os.makedirs(os.path.join(scratch, "noisy"))
    os.makedirs(os.path.join(scratch, "png"))
    cwd = os.getcwd()
    os.chdir(scratch)
    try:
        run(frames, scratch)
    finally:
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)


def run(frames, scratch):
    # ---- the reference's dataset class on stub cv2 / h5py
    gts_bgr = {}
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2RGB = 4
    cv2.imread = lambda path, flag=None: gts_bgr[path].copy()
    cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[:, :, ::-1]) if code == cv2.COLOR_BGR2RGB else None
    sys.modules["cv2"] = cv2
    sys.modules["h5py"] = types.ModuleType("h5py")
    sys.path.insert(0, REF)
    import torch
    import define
    define.MFLAG = 3
    assert define.TEST_RAW_ADD_NOISE is False
    import self_dataset
    assert self_dataset.TEST_RAW_ADD_NOISE is False

    paths = {}
    for f, (raw, gt) in frames.items():
        H, W = raw.shape
        p = os.path.join(scratch, "noisy", f"frame{f}_{H}_{W}.raw")
        raw.astype("<u2").tofile(p)
        paths[f] = p
        gts_bgr[os.path.join(scratch, "png", f"frame{f}.png")] = np.ascontiguousarray(gt.transpose(1, 2, 0)[:, :, ::-1])
    ds = object.__new__(self_dataset.TestDataset)
    ds.rggb, ds.ps, ds.mflag = [paths[f] for f in FRAMES], 128, 3
    fx, fsha = {}, {}
    for i, f in enumerate(FRAMES):
        inp, gt = ds[i]
        assert inp.dtype == torch.float32 and gt.dtype == torch.float32
        fx[f"raw_{f}"] = frames[f][0]
        fx[f"inp_{f}"] = inp.numpy()[None]
        fx[f"gt16_{f}"] = frames[f][1][None]
        fx[f"gt_{f}"] = gt.numpy()[None]
        fsha.update({f"{k}_{f}": sha(fx[f"{k}_{f}"]) for k in ("raw", "gt16", "inp", "gt")})
    # stored: frame (a) itself and the reference's value of every code, read off frame (a)'s inp and gt; every frame is pinned by SHA-256
    raw_a = fx["raw_a"]
    keep = dict(raw_a=raw_a, gt16_a=fx["gt16_a"], levels_inp=per_code(raw_a, mosaic(fx["inp_a"][0])),
                levels_gt=per_code(fx["gt16_a"], fx["gt_a"]))
    keep["meta"] = np.array(json.dumps(dict(natural=NATURAL, sha=fsha)))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "frames.npz"), **keep)
    print("[frames]", {f: fx[f"raw_{f}"].shape for f in FRAMES}, flush=True)

    # ---- the nets: calibrated on frame (b) by the reference's mode-0 pass, then its integer simulation on every frame
    from torch import nn
    from myQL import quan_func as qf
    from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
    from myQL.graph_modify import insert_before, insert_bias_bypass, insert_after
    from models import nrdm_3, nrdm_3_sim

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
        shutil.rmtree("output_pt", ignore_errors=True)

        def make(cls):
            m = cls()
            m.train()
            if cfg["qat"]:
                from models import quantize_utils_pt as quantize
                quantize.prepare(m, inplace=True, a_bits=8, w_bits=8, q_type=0, q_level="C")
            m.load_state_dict(torch.load(os.path.join(REF, cfg["ckpt"]), weights_only=True, map_location="cpu"), strict=False)
            m = m.float()
            m.collapse()
            return m

        x_cal = torch.from_numpy(fx[f"inp_{CAL_FRAME}"])
        with torch.no_grad():
            splice(make(nrdm_3.nr), 0)(x_cal)
        for i in range(6):                 # test.py:185-217: (scale, zero) from the running ranges; the output domain from 0
            mx = torch.load(f"output_pt/input/input.{i}.max_val.pt")
            mn = 0 if i == 5 else torch.load(f"output_pt/input/input.{i}.min_val.pt")
            s = (mx - mn) / 255
            torch.save(s, f"output_pt/input/input.{i}.scale.pt")
            torch.save(-128 - round(mn / s), f"output_pt/input/input.{i}.zero.pt")
        ld = torch.load
        d, sh = {}, {}
        for f in FRAMES:
            with torch.no_grad():
                y = splice(make(nrdm_3_sim.nr), 1)(torch.from_numpy(fx[f"inp_{f}"]))
            q0 = ld("output_pt/input/input.0.pt").numpy()
            assert np.all(q0 == np.rint(q0)) and q0.min() >= -128 and q0.max() <= 127
            sh[f"input0_{f}"] = sha(q0.astype(np.int8))
            if f == "a":
                d["input0_a"] = q0.astype(np.int8)
            s5 = np.float32(ld("output_pt/input/input.5.scale.pt"))
            z5 = int(ld("output_pt/input/input.5.zero.pt"))
            yf = y.numpy().astype(np.float32)
            yq = np.rint(yf.astype(np.float64) / np.float64(s5) + z5)
            assert yq.min() >= -128 and yq.max() <= 127
            yq = yq.astype(np.int8)
            assert np.array_equal(((yq.astype(np.float32) - np.float32(z5)) * s5).astype(np.float32), yf)
            sh[f"out_q_{f}"] = sha(yq)
            sh[f"out_{f}"] = sha(yf)
        L = 5
        for k in range(L):
            d[f"Wq{k}"] = ld(f"output_pt/weight/conv.weight.{k}.pt").numpy().astype(np.int8)
            d[f"add_const{k}"] = ld(f"output_pt/bias/conv.bias.quan{k}.pt").numpy().reshape(-1).astype(np.int32)
        names = ["0_1", "1_2", "2_3", "3_4", "4_5"]
        meta = dict(case=net, mflag=3, calibrated_on=f"frame {CAL_FRAME}",
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
