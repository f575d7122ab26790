#!/usr/bin/env python3
"""Free-size export measurements (sesrq.resize, libsesrq_resize.so) on one GPU; profiles/resize_probe.txt is its --report.

  python tools/resize_probe.py --report OUT [--resources-file FILE]
  python tools/resize_probe.py --resources        # no GPU: compile the library's source for gfx950 with
                                                  # -Rpass-analysis=kernel-resource-usage and print registers, scratch and LDS

1. one process, HIP events around back-to-back launches, the candidates of one case alternating inside a repetition, median of the
   repetitions: the x2 net's 2560 x 1440 int8 output -> 1920 x 1080 (720p in, 1080p out), and a 3840 x 2160 prediction -> 2560 x 1440
   from int8 and from fp32 --
     the fused kernel (what resize.export and Engine.forward_resized launch), its bytes checked against Pillow's at that size;
     image.export of the same prediction: the floor for reading the prediction once (it writes the full-size bytes, not the resized);
     the torch route it replaces: fp32 F.interpolate(mode="bicubic", antialias=True), clamp, * 255, byte cast, permute;
2. registers, scratch, LDS and occupancy of every instantiation.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sesr-pytorch-quantize_amd"))

CASES = {"2560x1440 -> 1920x1080, int8 (x2 net, 720p in)": (1440, 2560, 1080, 1920, "i8"),
         "3840x2160 -> 2560x1440, int8": (2160, 3840, 1440, 2560, "i8"),
         "3840x2160 -> 2560x1440, fp32": (2160, 3840, 1440, 2560, "f32")}
OUT_SCALE, OUT_ZERO = 0.0043, -120
HBM = 8.0                                        # TB/s, the MI355X's peak


def resources():
    """Registers, scratch and LDS of every kernel of sesrq_resize.hip as the library's Makefile compiles it (no GPU needed)."""
    csrc = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sesrq_resize.hip"), "-o",
                            os.path.join(tmp, "resize.o")], capture_output=True, text=True, check=True)
    out, cur = [], {}
    for ln in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if m and m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            out.append(cur)
        elif m:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    assert len(out) == 6 and all(k["ScratchSize"] == 0 for k in out), "an instantiation is missing or uses scratch"
    lines = ["compiled for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage, 6 instantiations resize<source, C>:"]
    for k in out:
        m = re.search(r"ILi(\d)ELi(\d)E", k["name"])
        nice = f"resize<{('u8', 'f32', 'i8')[int(m.group(1))]},C{m.group(2)}>"
        lines.append(f"   {nice:16s} VGPRs {k['VGPRs']:3d}  scratch {k['ScratchSize']} B/lane  LDS {k['LDS']:5d} B/block  occupancy "
                     f"{k['Occupancy']} waves/SIMD")
    return lines


def window(fn, calls):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def candidates(dev, H, W, Ho, Wo, kind):
    """({name: (callable, calls a window, bytes moved)}, whether the fused kernel's bytes equal Pillow's) of one case."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from PIL import Image
    from sesrq import image, resize
    g = torch.Generator(device=dev).manual_seed(H + Wo)
    if kind == "i8":
        pred = torch.randint(-128, 128, (1, 3, H, W), dtype=torch.int8, device=dev, generator=g)
        dom = dict(scale=OUT_SCALE, zero=OUT_ZERO)
        fp = (pred.float() - OUT_ZERO) * OUT_SCALE
    else:
        pred = torch.rand((1, 3, H, W), device=dev, generator=g) * 1.2 - 0.1
        dom, fp = {}, pred
    plan = resize.plan(H, W, Ho, Wo, dev)
    out = torch.empty((1, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    resize.run(plan, pred, out=out, **dom)
    full = image.export(pred, **dom)
    torch.cuda.synchronize()
    equal = np.array_equal(out[0].cpu().numpy(), np.asarray(Image.fromarray(full[0].cpu().numpy()).resize((Wo, Ho), Image.BICUBIC)))

    def torch_route():
        return (F.interpolate(fp, size=(Ho, Wo), mode="bicubic", antialias=True, align_corners=False).clamp(0, 1) * 255).to(torch.uint8) \
            .permute(0, 2, 3, 1).contiguous()
    esz = pred.element_size()
    return {f"resize: fused, tile 192 B x {plan.tile[1]} rows": (lambda: resize.run(plan, pred, out=out, **dom), 100, 3 * H * W * esz + 3 * Ho * Wo),
            "image.export of the prediction (full-size bytes)": (lambda: image.export(pred, **dom), 100, 3 * H * W * esz + 3 * H * W),
            "torch: F.interpolate(bicubic, antialias), clamp, * 255, cast, permute": (torch_route, 10, 0)}, equal


def report(path, reps, res_file):
    import torch
    dev = torch.device("cuda:0")
    lines = ["Free-size export (libsesrq_resize.so, sesrq.resize), one MI355X.  Every number below is MEASURED by",
             "tools/resize_probe.py --report.", "",
             f"1. One process, HIP events around back-to-back launches (100 a window; 10 calls of the torch route), {reps} repetitions, the",
             "   candidates of a case alternating inside a repetition; median (min .. max) us per call.  MB: the prediction read once and",
             f"   the output written once; its rate over {HBM:.0f} TB/s is the share of HBM peak the call reaches.", ""]
    for s, (H, W, Ho, Wo, kind) in CASES.items():
        cands, equal = candidates(dev, H, W, Ho, Wo, kind)
        for fn, _, _ in cands.values():
            for _ in range(5):
                fn()
        got = {k: [] for k in cands}
        for _ in range(reps):
            for k, (fn, calls, _) in cands.items():
                got[k].append(window(fn, calls))
        lines.append(f"   {s}; bytes equal Pillow's resize of image.export: {'yes' if equal else 'NO'}")
        med = {k: statistics.median(v) for k, v in got.items()}
        for k, us in got.items():
            mb = cands[k][2] / 1e6
            lines.append(f"      {k:72s} {med[k]:9.2f} ({min(us):.2f} .. {max(us):.2f})" +
                         (f"   {mb:5.1f} MB, {mb / med[k]:.2f} TB/s, {100 * mb / med[k] / HBM:.0f} % of peak" if mb else ""))
        a, b, t = med.values()
        lines.append(f"      the fused kernel takes {a / b:.2f}x the time of image.export; the torch route takes {t / a:.1f}x the time of the fused kernel")
    lines += ["", "2. Registers, scratch, LDS:"] + ["   " + ln for ln in (open(res_file).read().splitlines() if res_file else resources())]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-file", help="the output of an earlier --resources run to include instead of compiling again")
    ap.add_argument("--report", metavar="OUT")
    args = ap.parse_args()
    if args.resources:
        print("\n".join(resources()))
    elif args.report:
        report(args.report, args.reps, args.resources_file)
    else:
        ap.error("one of --report, --resources")


if __name__ == "__main__":
    main()
