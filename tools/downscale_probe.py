#!/usr/bin/env python3
"""Measurements of the fused bicubic downscale + decode (sesrq.downscale, libsesrq_downscale.so) on one GPU;
profiles/downscale_probe.txt is its --report.

  python tools/downscale_probe.py --report OUT     # everything below into OUT (the kernel-time run is a child process under rocprofv3)
  python tools/downscale_probe.py --kernels-only   # only the kernel launches (what the `rocprofv3 --kernel-trace --stats -- ...` child runs)
  python tools/downscale_probe.py --resources      # no GPU: compile the library's source for gfx950 with
                                                   # -Rpass-analysis=kernel-resource-usage and print registers, scratch and LDS per kernel

1. kernel time, from a rocprofv3 kernel trace of its own (launches after warm-up; duration = end - start): one 2160 x 3840 HR frame ->
   1080p RGB (r = 2) and -> 540p Y (r = 4); lr only, q0 only, all three outputs; bytes per launch from the shapes; the distance to
   (b), the HR frame's 24.9 MB at 8 TB/s;
2. without the profiler, alternating in one process (HIP events around back-to-back calls, several repetitions): the fused kernel
   against (a) the torch route it replaces -- fp32 permute, F.interpolate(mode="bicubic", antialias=True), round, clamp, cast, then
   image.decode;
3. (c) the scored loop in frames/s: quality.evaluate_image with uploaded LR files against quality.evaluate_hr, 4K ground truths.
"""
import argparse
import csv
import glob
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
H, W = 2160, 3840
SCALE, ZERO = 0.0039, -128
WARM = 20
# name -> (r, form, outputs): in launch order
CASES = {"4K -> 1080p RGB r=2, lr only": (2, "rgb", ("lr",)), "4K -> 1080p RGB r=2, q0 only": (2, "rgb", ("q0",)),
         "4K -> 1080p RGB r=2, lr + q0 + x": (2, "rgb", ("lr", "q0", "x")), "4K -> 540p Y r=4, lr only": (4, "y", ("lr",)),
         "4K -> 540p Y r=4, q0 only": (4, "y", ("q0",)), "4K -> 540p Y r=4, lr + q0 + x": (4, "y", ("lr", "q0", "x"))}


def instance(r, form, outs):
    return f"downscale<r{r},{'lr' if outs == ('lr',) else 'Y' if form == 'y' else 'RGB'}>"


def nbytes(r, form, outs):
    px, ch = (H // r) * (W // r), 1 if form == "y" else 3
    return 3 * H * W, sum({"lr": 3 * px, "q0": ch * px, "x": 4 * ch * px}[o] for o in outs)


def resources():
    """Registers, scratch and LDS of every kernel of sesrq_downscale.hip as the library's Makefile compiles it (no GPU needed)."""
    csrc = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sesrq_downscale.hip"), "-o",
                            os.path.join(tmp, "downscale.o")], capture_output=True, text=True, check=True)
    out, cur = [], {}
    for ln in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            out.append(cur)
        else:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    names = {f"ILi{r}ELi{c}E": f"downscale<r{r},{f}>" for r in (2, 4) for c, f in (("n1", "lr"), ("0", "Y"), ("1", "RGB"))}
    lines = ["compiled for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage:"]
    for k in out:
        nice = next((v for s, v in names.items() if s in k["name"]), k["name"])
        lines.append(f"   {nice:20s} VGPRs {k.get('VGPRs'):>3s}  scratch {k.get('ScratchSize')} B/lane  LDS {k.get('LDS'):>5s} B/block  "
                     f"occupancy {k.get('Occupancy')} waves/SIMD")
    assert len(out) == 6 and all(k.get("ScratchSize") == "0" for k in out), "an instantiation uses scratch"
    lines.append("   no scratch in any instantiation")
    return lines


def buffers(dev):
    import numpy as np
    import torch
    hr = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1, H, W, 3), dtype=np.uint8)).to(dev)
    b = {}
    for name, (r, form, outs) in CASES.items():
        ch = 1 if form == "y" else 3
        b[name] = (hr, torch.empty((1, H // r, W // r, 3), dtype=torch.uint8, device=dev) if "lr" in outs else None,
                   torch.empty((1, ch, H // r, W // r), dtype=torch.int8, device=dev) if "q0" in outs else None,
                   torch.empty((1, ch, H // r, W // r), dtype=torch.float32, device=dev) if "x" in outs else None)
    return b


def fused(dev, st, name, hr, lr, q0, x):
    from sesrq import downscale
    r, form, _ = CASES[name]
    return lambda: downscale.launch(dev, SCALE, ZERO, 0, hr, "rgb", r, form, lr, q0, x, st)


def torch_route(dev, st, name, hr, lr, q0, x):
    """(a): the route the fused kernel replaces -- fp32 permute, antialiased bicubic interpolate, round, clamp, cast, then image.decode."""
    import torch.nn.functional as F
    from sesrq import image
    r, form, _ = CASES[name]

    def run():
        f = F.interpolate(hr.permute(0, 3, 1, 2).float(), size=(H // r, W // r), mode="bicubic", antialias=True, align_corners=False)
        u8 = f.round().clamp(0, 255).to(hr.dtype).permute(0, 2, 3, 1).contiguous()
        if q0 is not None or x is not None:
            image.launch(dev, SCALE, ZERO, 0, u8, form, "rgb", q0, x, st)
        return u8
    return run


def window(fn, calls):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def kernels_only(iters):
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    for name, args in buffers(dev).items():
        fn = fused(dev, st, name, *args)
        for _ in range(WARM + iters):
            fn()
        torch.cuda.synchronize()


def summarise(trace_dir, iters):
    """{case: [us]} of the last `iters` launches of each case: an instantiation's launches in start order are its cases' blocks of
    WARM + iters launches, in the order of CASES."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    per = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            m = re.search(r"downscale<\s*(\d)\s*,\s*(-?\d)\s*>", row["Kernel_Name"])
            if m:
                key = f"downscale<r{m.group(1)},{ {'-1': 'lr', '0': 'Y', '1': 'RGB'}[m.group(2)] }>"
                per.setdefault(key, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    out, used = {}, {}
    for name, (r, form, outs) in CASES.items():
        key = instance(r, form, outs)
        us = [d for _, d in sorted(per[key])]
        k = used.get(key, 0)
        block = us[k * (WARM + iters):(k + 1) * (WARM + iters)]
        assert len(block) == WARM + iters, (name, key, len(us))
        out[name] = block[-iters:]
        used[key] = k + 1
    return out


def loop_rates(dev, frames, reps):
    """(c): frames/s of the scored loop with uploaded LR files (evaluate_image) and from the HR image alone (evaluate_hr); host arrays in,
    host scores out, so uploads, kernels and the final synchronisation are all inside the window."""
    import numpy as np
    import sesrq
    from sesrq import downscale, quality
    from sesrq.bundle import Bundle
    import torch
    img = os.path.join(ROOT, "tests", "golden", "image")
    lines = []
    rng = np.random.default_rng(1)
    hrs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(frames)]
    for mflag, net, kw in ((5, "sesr_x4", {}), (6, "sesr_x2_rand", {"anchor_add": True})):
        e = sesrq.Engine(Bundle.load(os.path.join(img, net + ".npz")), dev, **kw)
        r = downscale.factor_of(mflag)
        lrs = [downscale.downscale(torch.from_numpy(h).to(dev), r)[0].cpu().numpy() for h in hrs]
        got = {"evaluate_image (LR + HR uploaded)": [], "evaluate_hr (HR uploaded)": []}
        same = None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            a = quality.evaluate_image(e, lrs, hrs, mflag)
            t1 = time.perf_counter()
            b = quality.evaluate_hr(e, hrs, mflag)
            t2 = time.perf_counter()
            same = bool((a == b).all())
            if rep:                     # the first repetition warms every shape up
                got["evaluate_image (LR + HR uploaded)"].append(frames / (t1 - t0))
                got["evaluate_hr (HR uploaded)"].append(frames / (t2 - t1))
        lines.append(f"   MFLAG {mflag} ({net}), {frames} frames of {H} x {W} a pass, {reps} passes alternating; scores identical: {same}")
        for k, v in got.items():
            lines.append(f"      {k:36s} {statistics.median(v):8.1f} frames/s ({min(v):.1f} .. {max(v):.1f})")
        a, b = (statistics.median(v) for v in got.values())
        lines.append(f"      evaluate_hr / evaluate_image: {b / a:.3f}")
        e.close()
    return lines


def report(path, iters, reps, frames, res_file):
    import torch
    lines = ["Fused bicubic downscale + decode (libsesrq_downscale.so, sesrq.downscale), one MI355X.  Every number below is MEASURED;",
             "tools/downscale_probe.py --report made this file.", ""]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-only", "--iters", str(iters)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        per = summarise(tmp, iters)
    floor = 3 * H * W / PEAK * 1e6
    lines += [f"1. Kernel time.  Durations come from one `rocprofv3 --kernel-trace --stats` run of its own (tools/downscale_probe.py",
              f"   --kernels-only --iters {iters}; {iters} launches per row after {WARM} warm-up launches; duration = end - start timestamp).  Every",
              f"   case reads one {H} x {W} x 3 HR frame.  (b) = {3 * H * W / 1e6:.1f} MB / 8 TB/s = {floor:.2f} us.", "",
              "   case                               kernel               median     min     in + out MB     x (b)   share of 8 TB/s (median)"]
    for name, (r, form, outs) in CASES.items():
        us = per[name]
        a, b = nbytes(r, form, outs)
        m = statistics.median(us)
        lines.append(f"   {name:34s} {instance(r, form, outs):18s} {m:7.2f} us {min(us):7.2f} us  {a / 1e6:5.1f} + {b / 1e6:4.1f}   "
                     f"{m / floor:6.2f}   {100 * (a + b) / (m * 1e-6) / PEAK:5.1f} %")
    lines.append("")

    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    bufs = buffers(dev)
    lines += [f"2. Without the profiler, one process, HIP events around back-to-back calls: {reps} repetitions, the candidates alternating inside",
              f"   a repetition ({iters} launches of the kernel, 20 calls of the torch route); median (min .. max) us per call.", ""]
    for name, args in bufs.items():
        cands = {"fused downscale + decode": (fused(dev, st, name, *args), iters),
                 "(a) torch: permute, interpolate(bicubic, antialias), round, clamp, cast, image.decode": (torch_route(dev, st, name, *args), 20)}
        for fn, _ in cands.values():
            for _ in range(5):
                fn()
        got = {k: [] for k in cands}
        for _ in range(reps):
            for k, (fn, calls) in cands.items():
                got[k].append(window(fn, calls))
        lines.append(f"   {name}")
        for k, us in got.items():
            lines.append(f"      {k:88s} {statistics.median(us):9.2f} ({min(us):.2f} .. {max(us):.2f})")
        f_us, t_us = (statistics.median(got[k]) for k in cands)
        assert f_us < t_us, f"{name}: the fused kernel ({f_us:.2f} us) is not faster than the torch route ({t_us:.2f} us)"
        lines.append(f"      fused vs (a): {t_us / f_us:.1f}x faster; fused per call = {f_us / floor:.2f} x (b)")
    lines += ["", "3. (c) The scored loop, host images in, host scores out (wall clock around the whole call):", ""]
    lines += loop_rates(dev, frames, reps)
    lines += ["", "4. Registers, scratch, LDS:"] + ["   " + ln for ln in (open(res_file).read().splitlines() if res_file else resources())]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8, help="frames a pass of the scored loop")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-file", help="the output of an earlier --resources run to include instead of compiling again")
    ap.add_argument("--report", metavar="OUT")
    args = ap.parse_args()
    if args.resources:
        print("\n".join(resources()))
    elif args.kernels_only:
        kernels_only(args.iters)
    elif args.report:
        report(args.report, args.iters, args.reps, args.frames, args.resources_file)
    else:
        ap.error("one of --report, --kernels-only, --resources")


if __name__ == "__main__":
    main()
