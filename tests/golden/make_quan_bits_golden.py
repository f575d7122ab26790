#!/usr/bin/env python3
"""Golden vectors of the integer path at a narrow width QUAN_BIT = b < 8.  RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).

Same method as make_golden.py: the reference's own functions (myQL.quan_func / myQL.graph_modify / models.*) run on CPU in a scratch
working directory, with define.QUAN_BIT set to b BEFORE myQL.quan_func is imported (it binds QUAN_BIT by value: the output requant,
quan_func.py:585, and the weight text writer, :110, read the module global) and width = weight_width = b passed to every quantiser.
The activation domains are calibrated at that width on the reference's random inputs, as test.py:185-217 does (scale = range /
(2^b - 1), zero = -2^(b-1) - round(min / scale), min := 0 for the output domain).

Per (case, b), under tests/golden/quan_bits/:
  <case>.q<b>.params.npz  the collapsed float convs Wf{k}/bf{k} + the calibration, in the format of <case>.params.npz (sim.py --params)
  <case>.q<b>.crop.npz    a 24 x 40 crop with every stage of output_pt/** (input0..5, input4_special, shortcut, pe_out, pe_add, out), the
                          int weights / add constants, the reference's weight text files, and in meta["full"] the SHA-256 of the full
                          80 x 960 frame's q_out (input.5.pt, after PixelShuffle) and y
  <case>.q<b>.zeros.npz   the same crop with zero[1] != -2^(b-1) (layer 0 then writes a separate residual operand) and zero[L] moved

Widths: b = 3, 4, 6 and 7 for sesr_x4, nrdm_3 and sesr_x2_rand, b = 2 and 5 for nrdm_3; the reference's own calibration runs at every
one of these (case, b) pairs.

  <case>.q<b>.trace.npz   (--trace; TRACES) where the reference's own mode-0 run on the full frame and oracle/calib_oracle.py first
                          round a quantiser input to different codes: the layer, the positions, both codes, the reference's fp32
                          input values there and the oracle's, and the reference's per-layer extrema

Usage:  python tests/golden/make_quan_bits_golden.py                  # every case (one process each)
        python tests/golden/make_quan_bits_golden.py --case sesr_x4 --bits 4
        python tests/golden/make_quan_bits_golden.py --trace                # TRACES
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
sys.path.insert(0, HERE)
from make_golden import CASES, CROP_H, CROP_W, REF, sha  # noqa: E402

OUT = os.path.join(HERE, "quan_bits")
TRACES = [("sesr_x4", 3)]      # the (case, b) whose calibration the oracle does not reproduce within the bar (test_calib_oracle.py)
RUNS = [("sesr_x4", 4), ("sesr_x4", 6), ("nrdm_3", 4), ("nrdm_3", 2), ("nrdm_3", 6), ("sesr_x2_rand", 4), ("sesr_x2_rand", 6),
        ("sesr_x4", 3), ("sesr_x4", 7), ("nrdm_3", 3), ("nrdm_3", 5), ("nrdm_3", 7), ("sesr_x2_rand", 3), ("sesr_x2_rand", 7)]


def run_case(name: str, b: int) -> None:
    cfg = CASES[name]
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import torch
    from torch import nn
    import define
    define.MFLAG = cfg["mflag"]
    define.QUAN_BIT = b                      # bound by value inside quan_func at import time
    from myQL import quan_func as qf
    assert qf.QUAN_BIT == b
    from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
    from myQL.graph_modify import insert_before, insert_bias_bypass, insert_after
    from models import sesr, sesr_sim, nrdm_3, nrdm_3_sim, sesr_arch, sesr_arch_sim

    QMIN, QMAX = -(2 ** (b - 1)), 2 ** (b - 1) - 1
    torch.manual_seed(0)
    scratch = tempfile.mkdtemp(prefix="golden_q_", dir=os.path.join(HERE, "..", "..", ".scratch"))
    os.chdir(scratch)
    float_cls, sim_cls = {5: (sesr.sesr, sesr_sim.sesr), 3: (nrdm_3.nr, nrdm_3_sim.nr),
                          6: (sesr_arch.sesr, sesr_arch_sim.sesr)}[cfg["mflag"]]

    if cfg["ckpt"] is None:
        torch.manual_seed(cfg["seed"])
        proto_sd = {k: v.clone() for k, v in float_cls().state_dict().items()}

    def make(cls):
        m = cls()
        if cfg["ckpt"] is None:
            m.load_state_dict(proto_sd, strict=False)
        m.train()
        if cfg["ckpt"] is not None:
            m.load_state_dict(torch.load(os.path.join(REF, cfg["ckpt"]), weights_only=True, map_location="cpu"), strict=False)
        m = m.float()
        m.collapse()
        return m

    def pack(fn, kw):
        mp = NodeInsertMapping()
        mp.add_config(NodeInsertMappingElement(nn.Conv2d, FunctionPackage(fn, kw)))
        return mp

    def splice(model, qmode):
        model = qf.quantize_model_weight(model, b, qmode)
        mp = NodeInsertMapping()
        fp = FunctionPackage(qf.quantize_asymmetrical_by_tensor, {"width": b, "exe_mode": qmode})
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

    x_full = torch.load(os.path.join(REF, cfg["inp"]), weights_only=True, map_location="cpu").float()
    fm = make(sim_cls)
    convs = [fm.conv_first.conv_expand] + [blk.conv_expand for blk in fm.residual_block] + [fm.conv_last.conv_expand]
    Wf = [c.weight.detach().numpy().copy() for c in convs]
    bf = [c.bias.detach().numpy().copy() for c in convs]

    # ---- mode 0 on the full random input, finaliser at width b (test.py:185-217 with QUAN_BIT = b)
    cal = splice(make(float_cls), 0)
    with torch.no_grad():
        y_cal = cal(x_full)
    mins, maxs, scales, zeros = [], [], [], []
    for i in range(6):
        mx = torch.load(f"output_pt/input/input.{i}.max_val.pt")
        mn = torch.load(f"output_pt/input/input.{i}.min_val.pt")
        mins.append(mn); maxs.append(mx)
        if i == 5:
            mn = 0
        s = (mx - mn) / (QMAX - QMIN)
        z = QMIN - round(mn / s)
        torch.save(s, f"output_pt/input/input.{i}.scale.pt")
        torch.save(z, f"output_pt/input/input.{i}.zero.pt")
        scales.append(float(s)); zeros.append(int(z))
    tag = f"{name}.q{b}"
    np.savez_compressed(os.path.join(OUT, f"{tag}.params.npz"),
                        meta=np.array(json.dumps(dict(case=name, mflag=cfg["mflag"], quan_bits=b, min=mins, max=maxs, scale=scales,
                                                      zero=zeros, cal_out_sha=sha(y_cal.numpy().astype(np.float32))))),
                        **{f"Wf{k}": Wf[k] for k in range(5)}, **{f"bf{k}": bf[k] for k in range(5)})

    def sim_run(x):
        m = qf.quantize_model_weight(make(sim_cls), b, 1)
        mp = NodeInsertMapping()
        mp.add_config(NodeInsertMappingElement(nn.Conv2d, FunctionPackage(qf.quantize_asymmetrical_by_tensor, {"width": b, "exe_mode": 1})))
        m = insert_before(model_input=m, insert_mapping=mp, has_func_id=True)
        m = insert_before(model_input=m, insert_mapping=pack(qf.reshape_input_for_hardware_pe, {"pe_num": define.PE}))
        m = insert_after(model_input=m, insert_mapping=pack(qf.requan_conv2d_output, {"exe_mode": 1}))
        m = insert_bias_bypass(model_input=m, insert_mapping=pack(
            qf.PEs_and_bias_adder, {"pe_add_width": define.PE_ADD_BIT, "pe_acc_width": define.PE_ACC_BIT,
                                    "bias_width": define.BIAS_BIT, "pe_num": define.PE, "exe_mode": 1}))
        with torch.no_grad():
            return m(x)

    ld = torch.load
    ps = {5: 4, 6: 2, 3: 1}[cfg["mflag"]]

    def q_out_of(y):
        """input.5.pt is the int tensor before PixelShuffle; q_out is what the device returns: after it"""
        return torch.nn.functional.pixel_shuffle(ld("output_pt/input/input.5.pt"), ps).numpy()

    def harvest(x, y, kind, full):
        L = 5
        d = {}
        for k in range(L):
            d[f"Wq{k}"] = ld(f"output_pt/weight/conv.weight.{k}.pt").numpy().astype(np.int8)
            d[f"add_const{k}"] = ld(f"output_pt/bias/conv.bias.quan{k}.pt").numpy().reshape(-1).astype(np.int32)
            d[f"wtxt{k}"] = np.frombuffer(open(f"output_txt/weight/conv.weight.{k}.txt", "rb").read(), dtype=np.uint8)
        names = ["0_1", "1_2", "2_3", "3_4", "4_5"]
        meta = dict(case=name, tag=kind, mflag=cfg["mflag"], quan_bits=b,
                    wscale=[float(ld(f"output_pt/weight/conv.weight.{k}.scale.pt")) for k in range(L)],
                    scale=[float(ld(f"output_pt/input/input.{k}.scale.pt")) for k in range(6)],
                    zero=[int(ld(f"output_pt/input/input.{k}.zero.pt")) for k in range(6)],
                    M=[int(ld(f"output_pt/requan_factor/requan_{n}.pt")) for n in names],
                    n=[int(ld(f"output_pt/requan_factor/n_{n}.pt")) for n in names],
                    M_res=int(ld("output_pt/requan_factor/requan_res.pt")), n_res=int(ld("output_pt/requan_factor/n_res.pt")),
                    H=int(x.shape[2]), W=int(x.shape[3]), out_shape=list(y.shape))
        acts = {f"input{k}": ld(f"output_pt/input/input.{k}.pt").numpy() for k in range(6)}
        acts["input4_special"] = ld("output_pt/input/input.4.spcial.pt").numpy()
        for k, v in acts.items():
            assert np.all(v == np.rint(v)) and v.min() >= QMIN and v.max() <= QMAX, k
            acts[k] = v.astype(np.int8)
        acts["shortcut"] = ld("output_pt/residual/shortcut_tensor.pt").numpy().astype(np.float32)
        for k in range(L):
            acts[f"pe_add{k}"] = ld(f"output_pt/pe_add/pe_add_output{k}.pt").numpy().astype(np.int32)
            acts[f"pe_out{k}"] = np.stack([ld(f"output_pt/pe_out/pe_output{k}_{p}.pt").numpy() for p in range(4)]).astype(np.int32)
        acts["out"] = y.detach().numpy().astype(np.float32)
        acts["q_out"] = q_out_of(y).astype(np.int8)
        if full:
            return dict(q_out=sha(acts["q_out"]), y=sha(acts["out"]), shape=list(y.shape), x_sha256=sha(x.numpy().astype(np.float32)))
        d.update(acts)
        d["x"] = x.numpy().astype(np.float32)
        return d, meta

    full = harvest(x_full, sim_run(x_full), "full", True)
    x_crop = x_full[:, :, 8:8 + CROP_H, 100:100 + CROP_W].contiguous()
    d, meta = harvest(x_crop, sim_run(x_crop), "crop", False)
    meta["full"] = full
    np.savez_compressed(os.path.join(OUT, f"{tag}.crop.npz"), meta=np.array(json.dumps(meta)), **d)
    print(f"[{tag}] M={meta['M']} n={meta['n']} res=({meta['M_res']},{meta['n_res']}) zero={meta['zero']} full={full['q_out'][:12]}", flush=True)

    # zero points moved: zero[1] != -2^(b-1) (separate residual operand), zero[2] below the range, zero[5] inside it
    moved = {1: QMIN + 1, 2: QMIN - 3, 5: min(QMIN + 2, QMAX)}
    for k, v in moved.items():
        torch.save(int(v), f"output_pt/input/input.{k}.zero.pt")
    d, meta = harvest(x_crop, sim_run(x_crop), "zeros", False)
    np.savez_compressed(os.path.join(OUT, f"{tag}.zeros.npz"), meta=np.array(json.dumps(meta)), **d)
    print(f"[{tag}.zeros] zero={meta['zero']}", flush=True)
    os.chdir(HERE)
    shutil.rmtree(scratch, ignore_errors=True)


def trace_case(name: str, b: int) -> None:
    """The reference's mode-0 run with every quantiser's input and output recorded, layer by layer against calib_oracle: at the
    first quantiser input k whose codes differ, the positions and values (the upstream codes all agree, so the oracle's input there is
    its conv of the reference's own codes)."""
    cfg = CASES[name]
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    import torch
    from torch import nn
    import define
    define.MFLAG = cfg["mflag"]
    define.QUAN_BIT = b
    from myQL import quan_func as qf
    from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
    from myQL.graph_modify import insert_before, insert_bias_bypass
    from models import sesr, nrdm_3, sesr_arch
    from oracle import calib_oracle as CO

    torch.manual_seed(0)
    scratch = tempfile.mkdtemp(prefix="golden_t_", dir=os.path.join(HERE, "..", "..", ".scratch"))
    os.chdir(scratch)
    float_cls = {5: sesr.sesr, 3: nrdm_3.nr, 6: sesr_arch.sesr}[cfg["mflag"]]
    if cfg["ckpt"] is None:
        torch.manual_seed(cfg["seed"])
        proto_sd = {k: v.clone() for k, v in float_cls().state_dict().items()}
    m = float_cls()
    if cfg["ckpt"] is None:
        m.load_state_dict(proto_sd, strict=False)
    m.train()
    if cfg["ckpt"] is not None:
        m.load_state_dict(torch.load(os.path.join(REF, cfg["ckpt"]), weights_only=True, map_location="cpu"), strict=False)
    m = m.float()
    m.collapse()
    convs = [m.conv_first.conv_expand] + [blk.conv_expand for blk in m.residual_block] + [m.conv_last.conv_expand]
    Wf = [c.weight.detach().numpy().copy() for c in convs]
    bf = [c.bias.detach().numpy().copy() for c in convs]

    seen = {}

    def recorder(*a, **kw):
        t = kw["tensor_input"] if "tensor_input" in kw else a[0]
        out = qf.quantize_asymmetrical_by_tensor(*a, **kw)
        fid = kw["func_id"]
        seen[fid] = (t.detach().numpy().copy(), out.detach().numpy().copy(),
                     torch.load(f"output_pt/input/input.{fid}.scale.pt"), torch.load(f"output_pt/input/input.{fid}.zero.pt"))
        return out

    def pack(fn, kw):
        mp = NodeInsertMapping()
        mp.add_config(NodeInsertMappingElement(nn.Conv2d, FunctionPackage(fn, kw)))
        return mp

    model = qf.quantize_model_weight(m, b, 0)
    mp = NodeInsertMapping()
    fp = FunctionPackage(recorder, {"width": b, "exe_mode": 0})
    mp.add_config(NodeInsertMappingElement(nn.Conv2d, fp))
    mp.add_config(NodeInsertMappingElement(nn.PixelShuffle, fp))
    model = insert_before(model_input=model, insert_mapping=mp, has_func_id=True)
    model = insert_before(model_input=model, insert_mapping=pack(qf.reshape_input_for_hardware_pe, {"pe_num": define.PE}))
    model = insert_bias_bypass(model_input=model, insert_mapping=pack(
        qf.PEs_and_bias_adder, {"pe_add_width": define.PE_ADD_BIT, "pe_acc_width": define.PE_ACC_BIT,
                                "bias_width": define.BIAS_BIT, "pe_num": define.PE, "exe_mode": 0}))
    x_full = torch.load(os.path.join(REF, cfg["inp"]), weights_only=True, map_location="cpu").float()
    with torch.no_grad():
        model(x_full)
    L = 5
    ps = {5: 4, 6: 2, 3: 1}[cfg["mflag"]]
    mins = [float(seen[k][0].min()) for k in range(L + 1)]
    maxs = [float(seen[k][0].max()) for k in range(L + 1)]
    # the reference's codes r = rint(out / scale) + zero (out = (r - zero) * scale in fp32: |out / scale - (r - zero)| << 0.5)
    rcode = {k: np.rint(seen[k][1].astype(np.float64) / seen[k][2]).astype(np.int64) + seen[k][3] for k in range(L)}
    orc = CO.forward(Wf, bf, ps, [x_full.numpy()], b, keep_inputs=True)
    for k in range(L):
        ocode = CO.codes(orc.inputs[0][k], orc.domains[0][k], b)
        diff = np.argwhere(ocode != rcode[k])
        if len(diff):
            break
    else:
        raise SystemExit(f"{name} b={b}: the reference's codes and the oracle's agree at every layer")
    idx = tuple(diff.T)
    tag = f"{name}.q{b}"
    np.savez_compressed(os.path.join(OUT, f"{tag}.trace.npz"),
                        meta=np.array(json.dumps(dict(case=name, mflag=cfg["mflag"], quan_bits=b, layer=int(k), ref_min=mins,
                                                      ref_max=maxs, ref_scale=float(seen[k][2]), ref_zero=int(seen[k][3])))),
                        pos=diff.astype(np.int32), ref_code=rcode[k][idx].astype(np.int32), oracle_code=ocode[idx].astype(np.int32),
                        ref_x=seen[k][0][idx].astype(np.float32), oracle_x=orc.inputs[0][k][idx].astype(np.float32))
    print(f"[{tag}.trace] layer {k}: {len(diff)} codes differ, first at {diff[0].tolist()}: ref {rcode[k][idx][0]} oracle "
          f"{ocode[idx][0]}; ref x {seen[k][0][idx][0]!r} oracle x {orc.inputs[0][k][idx][0]!r}", flush=True)
    os.chdir(HERE)
    shutil.rmtree(scratch, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    ap.add_argument("--bits", type=int, default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    os.makedirs(os.path.join(HERE, "..", "..", ".scratch"), exist_ok=True)
    os.makedirs(OUT, exist_ok=True)
    if args.trace and args.case:
        trace_case(args.case, args.bits)
    elif args.trace:
        for c, b in TRACES:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--trace", "--case", c, "--bits", str(b)], check=True)
    elif args.case:
        run_case(args.case, args.bits)
    else:
        for c, b in RUNS:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--case", c, "--bits", str(b)], check=True)


if __name__ == "__main__":
    main()
