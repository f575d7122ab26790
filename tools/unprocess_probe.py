#!/usr/bin/env python3
"""Unprocess measurements (sesrq.unprocess, libsesrq_unprocess.so) on one GPU; profiles/unprocess_probe.txt is its --report.

  python tools/unprocess_probe.py --report OUT
  python tools/unprocess_probe.py --resources    # no GPU: compile the library's source for gfx950 with
                                                 # -Rpass-analysis=kernel-resource-usage and print registers, scratch and occupancy

Everything runs in one process, the candidates of a size alternating, several repetitions (HIP events around REPS back-to-back
launches after a warm-up, so a figure is time per launch on a busy stream, not a kernel trace):
1. the fused kernel at 540p and 1080p writing q0 only, raw + gt, and all four outputs; bytes per launch from the shapes, the share
   of 8 TB/s;
2. the torch route it replaces (table, matrix, mean, mask, maximum, clamp, round, strided scatter into the mosaic, divide), to raw + gt;
3. develop.export of the same frame size from fp32: the nearest kernel by bytes and shape, as the floor;
4. host-fed nrdm_3 540p frames/s: Engine.forward_srgb from pinned uint8 images against Engine.forward_raw from pinned raw frames.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sesr-pytorch-quantize_amd"))

PEAK = 8.0e12
SIZES = {"540p": (540, 960), "1080p": (1080, 1920)}
XYZ2CAM = ((1.0234, -0.2969, -0.2266), (-0.5625, 1.6328, -0.0469), (-0.0703, 0.2188, 0.6406))
WARM, REPS, ROUNDS = 20, 200, 5
SETS = {"q0": ("q0",), "raw+gt": ("raw", "gt"), "all four": ("raw", "gt", "q0", "spread")}
BYTES = dict(raw=2, gt=12, q0=3, spread=12)          # per pixel


def timed(fn, dev):
    """Median over ROUNDS of the time per call (us) of REPS back-to-back calls."""
    import torch
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        out.append(a.elapsed_time(b) * 1e3 / REPS)
    return statistics.median(out), min(out), max(out)


def torch_route(img, p, D=4095):
    import torch
    L = torch.from_numpy(p.curve.copy()).to(img.device)
    m = torch.from_numpy(p.rgb2cam.copy()).to(img.device)
    d = torch.from_numpy(p.inv_gains.copy()).to(img.device)
    N, H, W, _ = img.shape
    raw = torch.empty((N, H, W), dtype=torch.int32, device=img.device)

    def run():
        c = L[img.long()] @ m.T
        k = ((c.mean(-1, keepdim=True) - 0.9).clamp(min=0) / 0.1) ** 2
        s = torch.maximum(k + (1 - k) * d, d)
        q = ((c * s).clamp(0, 1) * D).round()
        raw[:, 0::2, 0::2], raw[:, 0::2, 1::2] = q[:, 0::2, 0::2, 0], q[:, 0::2, 1::2, 1]
        raw[:, 1::2, 0::2], raw[:, 1::2, 1::2] = q[:, 1::2, 0::2, 1], q[:, 1::2, 1::2, 2]
        return raw.to(torch.uint16), (q / D).permute(0, 3, 1, 2).contiguous()
    return run


def resources():
    """Registers, scratch and occupancy of every instantiation of sesrq_unprocess.hip as the library's Makefile compiles it."""
    csrc = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(csrc, "sesrq_unprocess.hip"), "-o", os.path.join(tmp, "u.o")], capture_output=True, text=True, check=True)
    rows, cur = [], {}
    for ln in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", ln)
        if m and m.group(1) == "Function Name":
            cur = {"mask": int(re.search(r"ILi(\d+)ELb([01])E", m.group(2)).group(1)), "lds": "Lb1E" in m.group(2)}
            rows.append(cur)
        elif m:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    assert len(rows) == 23 and all(r["ScratchSize"] == 0 for r in rows), "an instantiation is missing or uses scratch"
    names = ("raw", "gt", "q0", "spread")
    lines = ["compiled for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage:"]
    for r in sorted(rows, key=lambda r: (r["mask"], not r["lds"])):
        outs = "+".join(n for i, n in enumerate(names) if r["mask"] >> i & 1)
        home = (", lds" if r["lds"] else ", global") if r["mask"] & 4 else ""
        lines.append(f"   unprocess<{outs}{home}>".ljust(42) + f" VGPRs {r['VGPRs']:3d}  scratch 0 B/lane  occupancy {r['Occupancy']} waves/SIMD")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--report")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        return print("\n".join(resources()))
    if not a.report:
        ap.error("--report OUT or --resources")
    import numpy as np
    import torch
    import sesrq
    from sesrq import develop, sensor, unprocess
    from sesrq.bundle import Bundle
    assert torch.cuda.is_available(), "the probe measures on a GPU"
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    p = unprocess.from_colormatrix(XYZ2CAM, 2.1, 1.6)
    dp = develop.from_colormatrix(XYZ2CAM, 2.1, 1.6)
    fmt = sensor.REFERENCE
    dt = dict(raw=torch.uint16, gt=torch.float32, q0=torch.int8, spread=torch.float32)
    lines = [f"{torch.cuda.get_device_name(dev)}; time per launch in us: median (min .. max) of {ROUNDS} rounds of {REPS} back-to-back launches"]
    for size, (H, W) in SIZES.items():
        img = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev)
        cands = {}
        for name, wants in SETS.items():
            out = {k: torch.empty((1, H, W) if k == "raw" else (1, 3, H, W), dtype=dt[k], device=dev) for k in wants}
            cands[f"unprocess {name}"] = (lambda out=out: unprocess.launch(p, fmt, 1 / 255, -128, 0, img, "rgb", out.get("raw"), out.get("gt"),
                                                                           out.get("q0"), out.get("spread"), st),
                                          H * W * (3 + sum(BYTES[k] for k in wants)))
        cands["torch route (raw + gt)"] = (torch_route(img, p), None)
        pred = torch.rand((1, 3, H, W), device=dev)
        o8 = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
        cands["develop.export fp32 (floor)"] = (lambda: develop.launch(dp, pred, 0.0, 0, "rgb", o8, st), H * W * 15)
        for name, (fn, nb) in cands.items():
            med, lo, hi = timed(fn, dev)
            share = f"  {nb / 1e6:6.1f} MB  {nb / (med * 1e-6) / PEAK * 100:4.1f} % of 8 TB/s" if nb else ""
            lines.append(f"  {size:6s} {name:30s} {med:8.2f} ({lo:.2f} .. {hi:.2f}){share}")
    # host-fed frames per second, nrdm_3 at 540p
    e = sesrq.Engine(Bundle.load(os.path.join(ROOT, "tests", "golden", "raw", "nrdm_3.npz")), dev)
    H, W = SIZES["540p"]
    himg = [torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(4)]
    hraw = [torch.randint(0, 4096, (1, H, W), dtype=torch.int32).to(torch.uint16).pin_memory() for _ in range(4)]
    for name, fn in (("forward_srgb from uint8 images", lambda i: e.forward_srgb(himg[i % 4].to(dev, non_blocking=True), p, want_f=False)),
                     ("forward_raw from .raw frames", lambda i: e.forward_raw(hraw[i % 4].to(dev, non_blocking=True), want_f=False))):
        rates = []
        for _ in range(ROUNDS):
            for i in range(WARM):
                fn(i)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(REPS):
                fn(i)
            torch.cuda.synchronize(dev)
            rates.append(REPS / (time.perf_counter() - t0))
        lines.append(f"  host-fed nrdm_3 540p, {name:32s} {statistics.median(rates):8.0f} frames/s ({min(rates):.0f} .. {max(rates):.0f})")
    lines += ["", *resources()]            # needs hipcc beside the GPU; the same block --resources prints
    os.makedirs(os.path.dirname(os.path.abspath(a.report)), exist_ok=True)
    with open(a.report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
