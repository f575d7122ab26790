#!/usr/bin/env python3
"""Colour-export measurements (sesrq.colour, libsesrq_colour.so) on one GPU; profiles/colour_probe.txt is its --report.

  python tools/colour_probe.py --report OUT     # everything below into OUT (the kernel-time run is a child process under rocprofv3)
  python tools/colour_probe.py --kernels-only   # only the export launches (what the `rocprofv3 --kernel-trace --stats -- ...` child runs)
  python tools/colour_probe.py --resources      # no GPU: compile the library's source for gfx950 with
                                                # -Rpass-analysis=kernel-resource-usage and print registers, scratch and LDS per kernel

1. kernel time of the fused export, from a rocprofv3 kernel trace of its own (200 launches after warm-up; duration = end - start):
   540p -> 4K at r = 4 and 1080p -> 4K at r = 2, int8 and fp32 Y; bytes per launch from the shapes, the share of 8 TB/s;
2. without the profiler, alternating in one process (HIP events around back-to-back launches, several repetitions): the fused export
   against the torch route it replaces (fp32 chroma, F.interpolate(mode="bicubic"), the 3 x 3 matrix, clamp, byte cast, permute) and
   against image_export<i8,C3> at 4K, the existing kernel that writes the same bytes.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sesr-pytorch-quantize_amd"))

PEAK = 8.0e12
# name -> (LR H, LR W, r, Y dtype): all give a 2160 x 3840 output
CASES = {"540p -> 4K r=4 int8 Y": (540, 960, 4, "i8"), "540p -> 4K r=4 fp32 Y": (540, 960, 4, "f32"),
         "1080p -> 4K r=2 int8 Y": (1080, 1920, 2, "i8"), "1080p -> 4K r=2 fp32 Y": (1080, 1920, 2, "f32")}
SCALE, ZERO = 0.0047, -119


def nbytes(H, W, r, dt):
    hr = r * H * r * W
    return hr * (1 if dt == "i8" else 4), 3 * H * W, 3 * hr


def instance(r, dt):
    return f"colour_export<{dt},r{r}>"


def resources():
    """Registers, scratch and LDS of every kernel of sesrq_colour.hip as the library's Makefile compiles it (no GPU needed)."""
    csrc = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sesrq_colour.hip"), "-o",
                            os.path.join(tmp, "colour.o")], capture_output=True, text=True, check=True)
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
    names = {"13colour_chroma": "colour_chroma", "ILi1ELi2E": "colour_export<i8,r2>", "ILi1ELi4E": "colour_export<i8,r4>",
             "ILi0ELi2E": "colour_export<f32,r2>", "ILi0ELi4E": "colour_export<f32,r4>"}
    lines = ["compiled for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage:"]
    for k in out:
        nice = next((v for s, v in names.items() if s in k["name"]), k["name"])
        lines.append(f"   {nice:24s} VGPRs {k.get('VGPRs'):>3s}  scratch {k.get('ScratchSize')} B/lane  LDS {k.get('LDS'):>5s} B/block  "
                     f"occupancy {k.get('Occupancy')} waves/SIMD")
    assert len(out) == 5 and all(k.get("ScratchSize") == "0" for k in out), "an instantiation uses scratch"
    lines.append("   no scratch in any instantiation")
    return lines


def buffers(dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    out = torch.empty((1, 2160, 3840, 3), dtype=torch.uint8, device=dev)
    b = {}
    for name, (H, W, r, dt) in CASES.items():
        img = torch.from_numpy(rng.integers(0, 256, (1, H, W, 3)).astype(np.uint8)).to(dev)
        y = torch.randint(-128, 128, (1, 1, r * H, r * W), dtype=torch.int8, device=dev) if dt == "i8" else \
            torch.rand((1, 1, r * H, r * W), device=dev) * 1.2 - 0.1
        b[name] = (y, img, r, out)
    return b


def fused(st, y, img, r, out):
    from sesrq import colour
    return lambda: colour.launch(y, SCALE, ZERO, img, "rgb", r, out, st)


def torch_route(y, img, r):
    """The route the fused kernel replaces, in torch: fp32 chroma of the LR image, two bicubic upscales (one call on two planes), the
    inverse matrix, clamp, byte cast, permute to (N, H, W, 3)."""
    import torch
    import torch.nn.functional as F
    fwd = torch.tensor([[-37.797, -74.203, 112.0], [112.0, -93.786, -18.214]], device=img.device) / 255.0
    inv = torch.tensor([[1.16438356, 0.0, 1.59602679], [1.16438356, -0.39176229, -0.81296765], [1.16438356, 2.01723214, 0.0]],
                       device=img.device)

    def run():
        p = (y.float() - ZERO) * SCALE if y.dtype == torch.int8 else y
        Y = p.clamp(0, 1) * 255.0 - 16.0
        x = img.permute(0, 3, 1, 2).float()
        c = torch.einsum("kc,nchw->nkhw", fwd, x)                            # Cb - 128, Cr - 128
        up = F.interpolate(c, scale_factor=r, mode="bicubic", align_corners=False)
        rgb = torch.einsum("kc,nchw->nkhw", inv, torch.cat([Y, up], 1))
        return rgb.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
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
        fn = fused(st, *args)
        for _ in range(20 + iters):
            fn()
        torch.cuda.synchronize()


def summarise(trace_dir, iters):
    """{instantiation: [us]} of the last `iters` launches of each colour_export instantiation in a rocprofv3 kernel-trace CSV."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    per = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            m = re.search(r"colour_export<\s*(\d)\s*,\s*(\d)\s*>", row["Kernel_Name"])
            if m:
                key = instance(int(m.group(2)), "i8" if m.group(1) == "1" else "f32")
                per.setdefault(key, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    return {k: [d for _, d in sorted(v)][-iters:] for k, v in per.items()}


def report(path, iters, reps, res_file):
    import torch
    from sesrq import image as I
    lines = ["Colour export (libsesrq_colour.so, sesrq.colour.export), one MI355X.  Every number below is MEASURED; tools/colour_probe.py",
             "--report made this file.", ""]
    # 1. kernel time: a child process under the profiler
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-only", "--iters", str(iters)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        per = summarise(tmp, iters)
    lines += [f"1. Kernel time.  Durations come from one `rocprofv3 --kernel-trace --stats` run of its own (tools/colour_probe.py --kernels-only",
              f"   --iters {iters}; {iters} launches per row after 20 warm-up launches; duration = end - start timestamp).  Every case writes one",
              "   2160 x 3840 x 3 image; bytes per launch = Y + LR image + output, from the shapes.", "",
              "   case                      kernel                   median     min      Y + img + out MB      share of 8 TB/s (median)"]
    med = {}
    for name, (H, W, r, dt) in CASES.items():
        us = per[instance(r, dt)]
        assert len(us) == iters, (name, len(us))
        a, b, c = nbytes(H, W, r, dt)
        med[name] = statistics.median(us)
        lines.append(f"   {name:25s} {instance(r, dt):22s} {med[name]:7.2f} us {min(us):7.2f} us   {a / 1e6:5.1f} + {b / 1e6:4.1f} + {c / 1e6:4.1f} = "
                     f"{(a + b + c) / 1e6:5.1f}   {100 * (a + b + c) / (med[name] * 1e-6) / PEAK:5.1f} %")
    lines.append("")

    # 2. alternating, without the profiler
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    bufs = buffers(dev)
    pq = torch.randint(-128, 128, (1, 3, 2160, 3840), dtype=torch.int8, device=dev)
    out = bufs[next(iter(bufs))][3]
    lib = I.lib()
    grey = lambda: lib.sesrq_image_export(pq.data_ptr(), I.PRED_I8, SCALE, ZERO, 3, 0, out.data_ptr(), 1, 2160, 3840, st.cuda_stream)  # noqa: E731
    lines += [f"2. Without the profiler, one process, HIP events around back-to-back launches: {reps} repetitions, the candidates alternating",
              f"   inside a repetition ({iters} launches of a kernel, 20 calls of the torch route); median (min .. max) us per call.", ""]
    for name, (y, img, r, o) in bufs.items():
        H, W, _, dt = CASES[name]
        cands = {"fused colour export": (fused(st, y, img, r, o), iters), "image_export<i8,C3> at 4K (same output bytes)": (grey, iters),
                 "torch route (chroma, bicubic, matrix, clamp, cast, permute)": (torch_route(y, img, r), 20)}
        for fn, _ in cands.values():
            for _ in range(5):
                fn()
        got = {k: [] for k in cands}
        for _ in range(reps):
            for k, (fn, calls) in cands.items():
                got[k].append(window(fn, calls))
        lines.append(f"   {name}")
        for k, us in got.items():
            lines.append(f"      {k:62s} {statistics.median(us):9.2f} ({min(us):.2f} .. {max(us):.2f})")
        f_us, g_us, t_us = (statistics.median(got[k]) for k in cands)
        a, b, c = nbytes(H, W, r, dt)
        lines.append(f"      fused vs torch: {t_us / f_us:.1f}x faster; per output byte the fused export takes {f_us / g_us:.2f}x the time of "
                     f"image_export<i8,C3> ({(a + b + c) / 1e6:.1f} MB against 49.8 MB moved)")
    peak = torch.cuda.max_memory_allocated(dev)
    lines += ["", f"   Peak device memory of the process, torch route included: {peak / 1e6:.0f} MB (the fused export allocates nothing).", ""]
    lines += ["3. Registers, scratch, LDS:"] + ["   " + ln for ln in (open(res_file).read().splitlines() if res_file else resources())]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
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
        report(args.report, args.iters, args.reps, args.resources_file)
    else:
        ap.error("one of --report, --kernels-only, --resources")


if __name__ == "__main__":
    main()
