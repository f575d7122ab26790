#!/usr/bin/env python3
"""Fixtures of the reference's calibration loop over the dataset frames for its QAT checkpoints.  RUNS ONLY WHERE THE REFERENCE'S
SOURCES ARE (REF below).

A QAT checkpoint is calibrated on the QAT-prepared model: quantize.prepare() wraps the convs and replaces the long skip's AddOp by a
fake-quantising QuantAdd (reference models/quantize_utils_pt.py:654-711), and test.py's mode-0 graph is traced from that model while it
is in training mode.  This script re-drives that graph as make_calib_golden.py does for the plain nets (the reference's own quan_func /
graph_modify / models on the CPU in a scratch directory; the model prepared and loaded as make_golden.py's load_into does) over the
committed dataset frames (a), (b), (c) -- the frames make_calib_golden.py uses:

  nrdm_3_qat   (MFLAG 3, nrdm_3_qat_G.pth)  the 12-bit RGGB raw frames of tests/golden/raw/frames.npz
  sesr_x4_qat  (MFLAG 5, sr_qat_G.pth)      the 8-bit images of tests/golden/image/frames.npz (float64 luma)

Three frames settle whether the QuantAdd's moving-average observers are live in that graph: were they, frames (b) and (c) would be
merged at scales that depend on the frames before them.

Writes
  tests/golden/calib/<case>.npz     meta (JSON): the running min / max of every quantiser input after the three frames, the final
                                    scale / zero (test.py:185-217), the SHA-256 of every frame's mode-0 output
  tests/golden/calib/qat_add.json   per QAT checkpoint: the four observer extrema of add_residual and the scale it stores (data of
                                    the checkpoint); the scale the traced graph's QuantAdd holds (traced_scale: the tensor constant its
                                    nodes divide and multiply by) and the four extrema read back from the model after the loop (the
                                    observers do move; nothing reads them)

Usage:  python tests/golden/make_qat_calib_golden.py                 # both cases (one process each: define.MFLAG binds at import)
        python tests/golden/make_qat_calib_golden.py --case nrdm_3_qat
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import make_calib_golden as MC                 # dataset(): the reference's inp / gt of frames a, b, c, checked by SHA-256

REF = MC.REF
OUT = MC.OUT
CASES = {"nrdm_3_qat": dict(mflag=3, frames="nrdm_3", ckpt="model_params/nrdm_3_qat_G.pth"),
         "sesr_x4_qat": dict(mflag=5, frames="sesr_x4", ckpt="model_params/sr_qat_G.pth")}
OBSERVERS = ("observer_res.min_val", "observer_res.max_val", "observer_shortcut.min_val", "observer_shortcut.max_val")


def run_case(case):
    cfg = CASES[case]
    frames = MC.dataset(cfg["frames"])
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import torch
    from torch import nn
    import define
    define.MFLAG = cfg["mflag"]            # bound by value inside quan_func at import time
    from myQL import quan_func as qf
    from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
    from myQL.graph_modify import insert_before, insert_bias_bypass
    from models import sesr, sesr_sim, nrdm_3, nrdm_3_sim
    from models import quantize_utils_pt as quantize
    float_cls, sim_cls = {5: (sesr.sesr, sesr_sim.sesr), 3: (nrdm_3.nr, nrdm_3_sim.nr)}[cfg["mflag"]]
    sd = torch.load(os.path.join(REF, cfg["ckpt"]), weights_only=True, map_location="cpu")

    def make(cls):                         # make_golden.py load_into, qat
        m = cls()
        m.train()
        quantize.prepare(m, inplace=True, a_bits=8, w_bits=8, q_type=0, q_level="C")
        m.load_state_dict(sd, strict=False)
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
    scratch = tempfile.mkdtemp(prefix="qatcalibgolden", dir=os.path.join(TESTS, "..", ".scratch"))
    cwd = os.getcwd()
    os.chdir(scratch)
    try:
        cal = splice(make(float_cls))
        d, out_sha, out_shape = {}, {}, {}
        for f, inp, _ in frames:            # test.py:141-183: one frame per batch, the running ranges accumulate
            with torch.no_grad():
                y = cal(torch.from_numpy(inp))
            y = y.numpy().astype(np.float32)
            out_sha[f], out_shape[f] = MC.sha(y), list(y.shape)
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
        # the traced graph divides and multiplies by tensor constants: the clones of the scale update_qparams formed at trace time
        consts = {float(getattr(cal, n)) for n in dir(cal) if n.startswith("_tensor_constant")}
        assert len(consts) == 1, consts
        traced = consts.pop()
        after = {k: float(v) for k, v in cal.state_dict().items() if k.startswith("add_residual.") and k.endswith(OBSERVERS)}
    finally:
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)
    meta = dict(case=case, mflag=cfg["mflag"], frames=list(MC.FRAMES), quan_bit=int(define.QUAN_BIT),
                min=mins, max=maxs, scale=scale, zero=zero, out_sha=out_sha, out_shape=out_shape)
    d["meta"] = np.array(json.dumps(meta))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"{case}.npz"), **d)
    # the QuantAdd's state: data of the checkpoint, float32 values written as the doubles that equal them
    path = os.path.join(OUT, "qat_add.json")
    rec = json.load(open(path)) if os.path.isfile(path) else {}
    rec[case] = dict(checkpoint=os.path.basename(cfg["ckpt"]),
                     **{k: float(sd["add_residual." + k]) for k in OBSERVERS},
                     stored_scale=float(sd["add_residual.activation_quantizer.scale"]), traced_scale=traced,
                     observers_after_loop={k[len("add_residual."):]: v for k, v in sorted(after.items())})
    json.dump(rec, open(path, "w"), indent=1, sort_keys=True)
    print(f"[{case}] zero={zero} max={maxs}", flush=True)


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
