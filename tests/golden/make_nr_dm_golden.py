#!/usr/bin/env python3
"""Fixtures of the reference's nr (MFLAG 1, denoise) and dm (MFLAG 2, demosaic) tasks.  RUNS ONLY WHERE THE REFERENCE'S SOURCES ARE
(REF below).

What "the integer path of MFLAG 1 / 2" means.  The reference's sim.py builds nr.nr() / dm.dm() for these flags: the float-skip classes
(the class body of models/nrdm_3.py), whose AddOp stays in the traced graph, so its four integer rewrites leave a float add in the
middle; its authors note "we only use 3 and 5".  The integer net of these tasks is therefore the nrdm_3_sim graph -- the same class
without the AddOp, the long skip merged in the integer domain by requan_conv2d_output, as for MFLAG 3 -- with the task's own weights
(nr_G.pth / dm_G.pth and their QAT counterparts) and the task's own calibrated domains.  Likewise quan_func's observer of the output
domain (input.5, the bias adder of conv 4) is keyed on ``MFLAG == 3``: under MFLAG 1 / 2 the reference records no input.5 range and
its test.py stops at the torch.load of it.  quan_func is therefore bound with MFLAG 3 here -- the nrdm_3 pipeline on the nr / dm
classes; nothing else in it reads the flag.

Per case (nr, dm, nr_qat, dm_qat), with the reference's own quan_func / graph_modify / models on the CPU in a scratch directory, as
make_golden.py and make_calib_golden.py drive them:

  1  mode 0: the calibration graph (test.py:79-106) of nr.nr() / dm.dm() loaded from the checkpoint (a QAT checkpoint on the
     quantize.prepare()d model, whose long skip is then a QuantAdd: make_qat_calib_golden.py) over the raw dataset frames (a), (b), (c)
     of tests/golden/raw/frames.npz, frame by frame; the domains by test.py:185-217.
  2  mode 1: the integer pipeline (sim.py:82-114) on nrdm_3_sim.nr() with the same weights and those domains, on a 24 x 40 crop of
     frame (b)'s network input (the crop size of nrdm_3.crop.npz; even offsets keep the RGGB phase).

Writes into tests/golden/nr_dm/ (a directory of its own: the top level of tests/golden is globbed for the nets calibrated on the
reference's random frames).  In every meta, ``mflag`` is 3 -- the pipeline the tensors were made by, which is what the oracles and
Bundle.load read it for -- and ``task_mflag`` is the task's own flag, 1 or 2:
  <case>.params.npz   collapsed float convs Wf{k} / bf{k}; meta: the running min / max and the scale / zero of step 1
  <case>.crop.npz     every tensor the reference dumped in step 2 (the layout of make_golden.py's crops)
  <case>.calib.npz    the calibration record of step 1: meta as make_calib_golden.py writes it (per-frame metrics: nr by
                      tests/mosaic_oracle.py, dm by tests/quality_oracle.py's RGB form, on the reference's full mode-0 outputs;
                      skimage is not installed where fixtures are made); out_<f> crops for the plain checkpoints; for a QAT
                      checkpoint the four observer extrema of add_residual and the scale its traced QuantAdd holds (meta.qat_add)
Only data is written; no reference source goes into the repository.

Usage:  python tests/golden/make_nr_dm_golden.py                 # all four cases (one process each: define.MFLAG binds at import)
        python tests/golden/make_nr_dm_golden.py --case nr_qat
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
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
import make_calib_golden as MC                 # dataset(): the reference's inp / gt of frames a, b, c, checked by SHA-256

REF = MC.REF
OUT = os.path.join(HERE, "nr_dm")
CASES = {"nr": dict(mflag=1, cls="nr", ckpt="model_params/nr_G.pth", qat=False),
         "dm": dict(mflag=2, cls="dm", ckpt="model_params/dm_G.pth", qat=False),
         "nr_qat": dict(mflag=1, cls="nr", ckpt="model_params/nr_qat_G.pth", qat=True),
         "dm_qat": dict(mflag=2, cls="dm", ckpt="model_params/dm_qat_G.pth", qat=True)}
CROP_H, CROP_W = 24, 40                       # make_golden.py
CROP_AT = (8, 100)                            # rows, columns into frame (b): both even
OBSERVERS = ("observer_res.min_val", "observer_res.max_val", "observer_shortcut.min_val", "observer_shortcut.max_val")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(case):
    cfg = CASES[case]
    frames = MC.dataset("nrdm_3")
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import torch
    from torch import nn
    import define
    define.MFLAG = 3                       # bound by value inside quan_func at import time: the input.5 observer (module docstring)
    from myQL import quan_func as qf
    from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
    from myQL.graph_modify import insert_before, insert_bias_bypass, insert_after
    from models import nr, dm, nrdm_3_sim
    from models import quantize_utils_pt as quantize
    import mosaic_oracle as M
    import quality_oracle as Q
    float_cls, sim_cls = {"nr": nr.nr, "dm": dm.dm}[cfg["cls"]], nrdm_3_sim.nr
    sd = torch.load(os.path.join(REF, cfg["ckpt"]), weights_only=True, map_location="cpu")

    def make(cls):                         # make_golden.py load_into
        m = cls()
        m.train()
        if cfg["qat"]:
            quantize.prepare(m, inplace=True, a_bits=8, w_bits=8, q_type=0, q_level="C")
        m.load_state_dict(sd, strict=False)
        m = m.float()
        m.collapse()
        return m

    def pack(fn, kw):
        mp = NodeInsertMapping()
        mp.add_config(NodeInsertMappingElement(nn.Conv2d, FunctionPackage(fn, kw)))
        return mp

    def splice(model, qmode):              # test.py:79-106 (qmode 0), sim.py:82-114 (qmode 1)
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

    # the float and the sim class fold to the same convs: one class body, one checkpoint
    fm, ff = make(sim_cls), make(float_cls)
    convs_of = lambda m: [m.conv_first.conv_expand] + [b.conv_expand for b in m.residual_block] + [m.conv_last.conv_expand]
    Wf = [c.weight.detach().numpy().copy() for c in convs_of(fm)]
    bf = [c.bias.detach().numpy().copy() for c in convs_of(fm)]
    for k, c in enumerate(convs_of(ff)):
        assert np.array_equal(c.weight.detach().numpy(), Wf[k]) and np.array_equal(c.bias.detach().numpy(), bf[k]), k

    os.makedirs(os.path.join(TESTS, "..", ".scratch"), exist_ok=True)
    scratch = tempfile.mkdtemp(prefix="nrdmgolden", dir=os.path.join(TESTS, "..", ".scratch"))
    cwd = os.getcwd()
    os.chdir(scratch)
    try:
        # ------------------------------------------------------------------ 1: mode 0 over frames a, b, c
        cal = splice(ff, 0)
        rec, per_frame, out_sha = {}, {}, {}
        for f, inp, gt in frames:           # test.py:141-183: one frame per batch, the running ranges accumulate
            with torch.no_grad():
                y = cal(torch.from_numpy(inp))
            y = y.numpy().astype(np.float32)
            out_sha[f] = sha(y)
            if not cfg["qat"]:
                rec[f"out_{f}"] = np.ascontiguousarray(y[:, :, :MC.CROP[0], :MC.CROP[1]])
            mse, psnr, ssim = M.frame_metrics(y[0], gt[0]) if cfg["mflag"] == 1 else Q.frame_metrics(y[0], gt[0], 3)
            per_frame[f] = dict(mse=mse, psnr=psnr, ssim=ssim, out_shape=list(y.shape))
        mins, maxs, scale, zero = [], [], [], []
        for i in range(6):                  # test.py:185-217
            mx = torch.load(f"output_pt/input/input.{i}.max_val.pt")
            mn = torch.load(f"output_pt/input/input.{i}.min_val.pt")
            mins.append(float(mn))
            maxs.append(float(mx))
            mn = 0 if i == 5 else mn
            s = (mx - mn) / (2 ** define.QUAN_BIT - 1)
            z = -(2 ** (define.QUAN_BIT - 1)) - round(mn / s)
            torch.save(s, f"output_pt/input/input.{i}.scale.pt")
            torch.save(z, f"output_pt/input/input.{i}.zero.pt")
            scale.append(float(s))
            zero.append(int(z))
        qat_add = None
        if cfg["qat"]:                      # make_qat_calib_golden.py: the scale the traced QuantAdd divides and multiplies by
            consts = {float(getattr(cal, n)) for n in dir(cal) if n.startswith("_tensor_constant")}
            assert len(consts) == 1, consts
            qat_add = dict(checkpoint=os.path.basename(cfg["ckpt"]), **{k: float(sd["add_residual." + k]) for k in OBSERVERS},
                           stored_scale=float(sd["add_residual.activation_quantizer.scale"]), traced_scale=consts.pop())

        # ------------------------------------------------------------------ 2: mode 1 on the nrdm_3_sim graph, a crop of frame (b)
        x_b = torch.from_numpy(dict((f, inp) for f, inp, _ in frames)["b"])
        x = x_b[:, :, CROP_AT[0]:CROP_AT[0] + CROP_H, CROP_AT[1]:CROP_AT[1] + CROP_W].contiguous()
        with torch.no_grad():
            y = splice(fm, 1)(x)
        ld = torch.load
        d, L = {}, 5
        for k in range(L):
            d[f"Wq{k}"] = ld(f"output_pt/weight/conv.weight.{k}.pt").numpy().astype(np.int8)
            d[f"add_const{k}"] = ld(f"output_pt/bias/conv.bias.quan{k}.pt").numpy().reshape(-1).astype(np.int32)
        names = ["0_1", "1_2", "2_3", "3_4", "4_5"]
        meta = dict(case=case, tag="crop", mflag=3, task_mflag=cfg["mflag"], graph="nrdm_3_sim",
                    wscale=[float(ld(f"output_pt/weight/conv.weight.{k}.scale.pt")) for k in range(L)],
                    scale=[float(ld(f"output_pt/input/input.{k}.scale.pt")) for k in range(6)],
                    zero=[int(ld(f"output_pt/input/input.{k}.zero.pt")) for k in range(6)],
                    M=[int(ld(f"output_pt/requan_factor/requan_{n}.pt")) for n in names],
                    n=[int(ld(f"output_pt/requan_factor/n_{n}.pt")) for n in names],
                    M_res=int(ld("output_pt/requan_factor/requan_res.pt")), n_res=int(ld("output_pt/requan_factor/n_res.pt")),
                    H=CROP_H, W=CROP_W, out_shape=list(y.shape), frame="b", crop_at=list(CROP_AT), sha={})
        assert meta["scale"] == scale and meta["zero"] == zero
        acts = {f"input{k}": ld(f"output_pt/input/input.{k}.pt").numpy() for k in range(6)}
        acts["input4_special"] = ld("output_pt/input/input.4.spcial.pt").numpy()
        for k, v in acts.items():
            assert np.all(v == np.rint(v)) and v.min() >= -128 and v.max() <= 127, k
            acts[k] = v.astype(np.int8)
        acts["shortcut"] = ld("output_pt/residual/shortcut_tensor.pt").numpy().astype(np.float32)
        for k in range(L):
            v = ld(f"output_pt/pe_add/pe_add_output{k}.pt").numpy()
            assert np.all(v == np.rint(v))
            acts[f"pe_add{k}"] = v.astype(np.int32)
            pes = np.stack([ld(f"output_pt/pe_out/pe_output{k}_{p}.pt").numpy() for p in range(4)])
            assert np.all(pes == np.rint(pes))
            acts[f"pe_out{k}"] = pes.astype(np.int32)
        acts["out"] = y.detach().numpy().astype(np.float32)
        for k, v in acts.items():
            meta["sha"][k] = sha(v)
        d.update(acts)
        d["x"] = x.numpy().astype(np.float32)
        d["meta"] = np.array(json.dumps(meta))
    finally:
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)

    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"{case}.crop.npz"), **d)
    np.savez_compressed(os.path.join(OUT, f"{case}.params.npz"),
                        meta=np.array(json.dumps(dict(case=case, mflag=3, task_mflag=cfg["mflag"], frames=list(MC.FRAMES), min=mins, max=maxs,
                                                      scale=scale, zero=zero))),
                        **{f"Wf{k}": Wf[k] for k in range(5)}, **{f"bf{k}": bf[k] for k in range(5)})
    cmeta = dict(case=case, mflag=3, task_mflag=cfg["mflag"], kind="raw", frames=list(MC.FRAMES), crop=list(MC.CROP), quan_bit=int(define.QUAN_BIT),
                 min=mins, max=maxs, scale=scale, zero=zero, per_frame=per_frame, out_sha=out_sha, qat_add=qat_add,
                 metrics=("tests/mosaic_oracle.py" if cfg["mflag"] == 1 else "tests/quality_oracle.py (RGB form)") +
                 " on the reference's full mode-0 outputs (skimage is not installed where fixtures are made)")
    rec["meta"] = np.array(json.dumps(cmeta))
    np.savez_compressed(os.path.join(OUT, f"{case}.calib.npz"), **rec)
    print(f"[{case}] zero={zero} M={meta['M']} n={meta['n']} res=({meta['M_res']},{meta['n_res']}) "
          f"psnr={[round(per_frame[f]['psnr'], 4) for f in MC.FRAMES]}", flush=True)


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
