#!/usr/bin/env python3
"""Fixtures of the reference's calibration loop over the dataset frames.  RUNS ONLY WHERE THE REFERENCE'S SOURCES ARE (REF below).

The reference's test.py runs its mode-0 (fake-quantised float) graph over the dataset, frame by frame, prints each frame's PSNR and the
mean PSNR / SSIM of that output, and derives the activation domains from the running min/max the graph leaves under output_pt/.  This
script re-drives that graph (the reference's own quan_func / graph_modify / models, spliced as test.py:79-106 splices them, on the CPU
in a scratch directory, as make_golden.py does) over the committed dataset frames (a), (b), (c):

  nrdm_3        (MFLAG 3)  the 12-bit RGGB raw frames of tests/golden/raw/frames.npz (self_dataset.py TestDataset's inp / gt)
  sesr_x4       (MFLAG 5)  the 8-bit images of tests/golden/image/frames.npz (self_dataset_sr.py TestDataset: float64 luma)
  sesr_x2_rand  (MFLAG 6)  the same images in RGB; scored on gfake + up2(inps) (test.py:148-155)

The network inputs are the reference's own inp of each frame: rebuilt from the per-code values its dataset classes gave (levels_inp of
the raw fixture; the image decode restated in tests/image_oracle.py) and checked against the SHA-256 recorded when the reference made
them.  The weights are the ones tests/golden/<case>.params.npz holds (checked).

Writes tests/golden/calib/<case>.npz:
  out_<f>   (1, C, h, w) float32: the upper-left crop of frame f's mode-0 output (the whole output: meta.out_sha)
  meta      JSON: frames, crop, the running min / max of every quantiser input after the three frames, the final scale / zero
            (test.py:185-217), and per frame the expected (mse, psnr, ssim) of the mode-0 output.  skimage is not installed where the
            fixtures are made: the metrics are tests/quality_oracle.py (a restatement of the reference's metric forms, pinned in
            tests/test_quality.py) applied to the reference's full mode-0 outputs and its ground truths.

Usage:  python tests/golden/make_calib_golden.py                 # all three cases (one process each: define.MFLAG binds at import)
        python tests/golden/make_calib_golden.py --case nrdm_3
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(HERE, "calib")
FRAMES = ("a", "b", "c")
CROP = (48, 128)          # rows, columns of the output kept per frame
CASES = {"nrdm_3": dict(mflag=3, kind="raw", ckpt="model_params/nrdm_3_raw_G.pth"),
         "sesr_x4": dict(mflag=5, kind="image", ckpt="model_params/x4sesr.pth"),
         # x2sesr.pth.tar is refused by torch.load(weights_only=True): the reference's own random init, seeded (make_golden.py)
         "sesr_x2_rand": dict(mflag=6, kind="image", ckpt=None, seed=1234)}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dataset(case):
    """[(f, inp (1, C, H, W) float32, gt (1, C', H', W') float32)]: the reference's inp and gt of frames a, b, c, checked by SHA-256."""
    cfg = CASES[case]
    sys.path.insert(0, HERE)
    sys.path.insert(0, TESTS)
    out = []
    if cfg["kind"] == "raw":
        from make_raw_golden import natural_raw
        F = np.load(os.path.join(HERE, "raw", "frames.npz"), allow_pickle=False)
        shas = json.loads(str(F["meta"]))["sha"]
        for f in FRAMES:
            raw, gt16 = (F["raw_a"], F["gt16_a"][0]) if f == "a" else natural_raw(f)
            H, W = raw.shape
            yy, xx = np.meshgrid(np.arange(H) & 1, np.arange(W) & 1, indexing="ij")
            inp = np.zeros((3, H, W), np.float32)          # the value of its code at the pixel's site channel, 0 elsewhere
            np.put_along_axis(inp, (yy + xx)[None], F["levels_inp"][np.minimum(raw, 4095)][None], 0)
            inp = inp[None]
            gt = F["levels_gt"][np.minimum(gt16, 4095)][None]
            assert sha(inp) == shas[f"inp_{f}"] and sha(gt) == shas[f"gt_{f}"], f
            out.append((f, inp, gt))
    else:
        import image_oracle as IO
        from make_image_golden import natural_image
        F = np.load(os.path.join(HERE, "image", "frames.npz"), allow_pickle=False)
        shas = json.loads(str(F["meta"]))["sha"]
        m = cfg["mflag"]
        form = "y" if m == 5 else "rgb"
        for f in FRAMES:
            lr, hr = (F["lr_a"], F[f"hr{m}_a"]) if f == "a" else natural_image(f, m)
            inp, gt = IO.decode(lr, form), IO.decode(hr, form)
            assert sha(inp) == shas[f"inp{m}_{f}"] and sha(gt) == shas[f"gt{m}_{f}"], (f, m)
            out.append((f, inp, gt))
    return out


def run_case(case):
    cfg = CASES[case]
    frames = dataset(case)
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import torch
    from torch import nn
    import define
    define.MFLAG = cfg["mflag"]            # bound by value inside quan_func at import time
    from myQL import quan_func as qf
    from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
    from myQL.graph_modify import insert_before, insert_bias_bypass
    from models import sesr, sesr_sim, nrdm_3, nrdm_3_sim, sesr_arch, sesr_arch_sim
    import quality_oracle as Q
    float_cls, sim_cls = {5: (sesr.sesr, sesr_sim.sesr), 3: (nrdm_3.nr, nrdm_3_sim.nr), 6: (sesr_arch.sesr, sesr_arch_sim.sesr)}[cfg["mflag"]]

    proto_sd = None
    if cfg["ckpt"] is None:
        torch.manual_seed(cfg["seed"])
        proto_sd = {k: v.clone() for k, v in float_cls().state_dict().items()}

    def make(cls):
        m = cls()
        if proto_sd is not None:
            m.load_state_dict(proto_sd, strict=False)
        m.train()
        if cfg["ckpt"] is not None:
            m.load_state_dict(torch.load(os.path.join(REF, cfg["ckpt"]), weights_only=True, map_location="cpu"), strict=False)
        m = m.float()
        m.collapse()
        return m

    # the weights are those of tests/golden/<case>.params.npz (what the tests build their calibrators from)
    params = np.load(os.path.join(HERE, f"{case}.params.npz"), allow_pickle=False)
    fm = make(sim_cls)
    convs = [fm.conv_first.conv_expand] + [b.conv_expand for b in fm.residual_block] + [fm.conv_last.conv_expand]
    for k, c in enumerate(convs):
        assert np.array_equal(c.weight.detach().numpy(), params[f"Wf{k}"]) and np.array_equal(c.bias.detach().numpy(), params[f"bf{k}"]), k

    def pack(fn, kw):
        mp = NodeInsertMapping()
        mp.add_config(NodeInsertMappingElement(nn.Conv2d, FunctionPackage(fn, kw)))
        return mp

    def splice(model):                     # test.py:79-106, qmode 0
        model = qf.quantize_model_weight(model, define.QUAN_BIT, 0)
        mp = NodeInsertMapping()
        fp = FunctionPackage(qf.quantize_asymmetrical_by_tensor, {"width": define.QUAN_BIT, "exe_mode": 0})
        mp.add_config(NodeInsertMappingElement(nn.Conv2d, fp))
        mp.add_config(NodeInsertMappingElement(nn.PixelShuffle, fp))
        model = insert_before(model_input=model, insert_mapping=mp, has_func_id=True)
        model = insert_before(model_input=model, insert_mapping=pack(qf.reshape_input_for_hardware_pe, {"pe_num": define.PE}))
        return insert_bias_bypass(model_input=model, insert_mapping=pack(
            qf.PEs_and_bias_adder, {"pe_add_width": define.PE_ADD_BIT, "pe_acc_width": define.PE_ACC_BIT,
                                    "bias_width": define.BIAS_BIT, "pe_num": define.PE, "exe_mode": 0}))

    os.makedirs(os.path.join(TESTS, "..", ".scratch"), exist_ok=True)
    scratch = tempfile.mkdtemp(prefix="calibgolden", dir=os.path.join(TESTS, "..", ".scratch"))
    cwd = os.getcwd()
    os.chdir(scratch)
    try:
        cal = splice(make(float_cls))
        d, per_frame, out_sha = {}, {}, {}
        for f, inp, gt in frames:           # test.py:141-183: one frame per batch, the running ranges accumulate
            x = torch.from_numpy(inp)
            with torch.no_grad():
                y = cal(x)
            y = y.numpy().astype(np.float32)
            out_sha[f] = sha(y)
            d[f"out_{f}"] = np.ascontiguousarray(y[:, :, :CROP[0], :CROP[1]])
            pred = y
            if cfg["mflag"] == 6:           # test.py:148-155: gfake + nearest-upsampled inps, in fp32
                pred = (torch.from_numpy(y) + x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)).numpy()
            mse, psnr, ssim = Q.frame_metrics(pred[0], gt[0], cfg["mflag"])
            per_frame[f] = dict(mse=mse, psnr=psnr, ssim=ssim, out_shape=list(y.shape))
        mins, maxs, scale, zero = [], [], [], []
        for i in range(6):                  # test.py:185-217
            mx = torch.load(f"output_pt/input/input.{i}.max_val.pt")
            mn = torch.load(f"output_pt/input/input.{i}.min_val.pt")
            mins.append(float(mn))
            maxs.append(float(mx))
            mn = 0 if i == 5 else mn
            s = (mx - mn) / (2 ** define.QUAN_BIT - 1)
            scale.append(float(s))
            zero.append(int(-(2 ** (define.QUAN_BIT - 1)) - round(mn / s)))
    finally:
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)
    meta = dict(case=case, mflag=cfg["mflag"], kind=cfg["kind"], frames=list(FRAMES), crop=list(CROP), quan_bit=int(define.QUAN_BIT),
                min=mins, max=maxs, scale=scale, zero=zero, per_frame=per_frame, out_sha=out_sha,
                metrics="tests/quality_oracle.py on the reference's full mode-0 outputs (skimage is not installed where fixtures are made)")
    d["meta"] = np.array(json.dumps(meta))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"{case}.npz"), **d)
    print(f"[{case}] zero={zero} psnr={[round(per_frame[f]['psnr'], 4) for f in FRAMES]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
    else:
        for c in CASES:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--case", c], check=True)


if __name__ == "__main__":
    main()
