#!/usr/bin/env python3
"""Develop-export measurements (sesrq.develop, libsesrq_develop.so) on one GPU; profiles/develop_probe.txt is its --report.

  python tools/develop_probe.py --report OUT     # everything below into OUT (the kernel-time run is a child process under rocprofv3)
  python tools/develop_probe.py --kernels-only   # only the launches (what the `rocprofv3 --kernel-trace --stats -- ...` child runs)
  python tools/develop_probe.py --resources      # no GPU: compile the library's source for gfx950 with
                                                 # -Rpass-analysis=kernel-resource-usage and print registers, scratch and LDS per kernel

1. kernel time from a rocprofv3 kernel trace of its own (launches after warm-up; duration = end - start): (a) develop_export from int8
   and from fp32 at 540p and 1080p, per built-in curve, and with the plain 8-step search (SESRQ_DEVELOP_SEARCH=full) on the gamma
   table; (b) image_export<.,C3> of the same frames -- the floor: the same bytes in and out, no arithmetic; bytes per launch from the
   shapes, the share of 8 TB/s;
2. without the profiler, alternating in one process (HIP events around back-to-back launches, several repetitions): (a), (b) and
   (c) the torch route the kernel replaces: clamp, mul, clamp, matmul over channels, clamp, pow, x 255, round, cast, permute;
3. host-fed nrdm_3 540p frames/s: Engine.forward_develop against forward_raw + the torch route.
"""
import argparse
import csv
import ctypes as C
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
SIZES = {"540p": (540, 960), "1080p": (1080, 1920)}
CURVES = ("gamma", "srgb", "trunc255")
SCALE, ZERO = 0.0047, -119
GAINS = (2.1, 1.0, 1.6)
CCM = ((1.2622719, -0.4579577, 0.1956858), (-0.1505005, 1.1334672, 0.0170333), (-0.0106436, -0.3623454, 1.372989))
WARM = 20


def nbytes(H, W, dt):
    return 3 * H * W * (1 if dt == "i8" else 4), 3 * H * W


def resources():
    """Registers, scratch and LDS of every kernel of sesrq_develop.hip as the library's Makefile compiles it (no GPU needed)."""
    csrc = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sesrq_develop.hip"), "-o",
                            os.path.join(tmp, "develop.o")], capture_output=True, text=True, check=True)
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
    names = {"ILi0E": "develop_export<f32>", "ILi1E": "develop_export<i8>"}
    lines = ["compiled for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage:"]
    for k in out:
        nice = next((v for s, v in names.items() if s in k["name"]), k["name"])
        lines.append(f"   {nice:22s} VGPRs {k.get('VGPRs'):>3s}  scratch {k.get('ScratchSize')} B/lane  LDS {k.get('LDS'):>5s} B/block  "
                     f"occupancy {k.get('Occupancy')} waves/SIMD")
    assert len(out) == 2 and all(k.get("ScratchSize") == "0" for k in out), "an instantiation uses scratch"
    lines.append("   no scratch in either instantiation")
    return lines


def full_context(profile):
    """A context of `profile` whose search index is empty: the plain 8-step binary search."""
    from sesrq import develop
    h = C.c_void_p()
    os.environ["SESRQ_DEVELOP_SEARCH"] = "full"
    try:
        rc = develop.lib().sesrq_develop_create(profile.gains.ctypes.data, profile.ccm.ctypes.data, profile.curve.ctypes.data, C.byref(h))
    finally:
        del os.environ["SESRQ_DEVELOP_SEARCH"]
    assert rc == 0, develop.last_error()
    return h


def cases(dev):
    """[(label, kind of kernel, size, dtype, callable)] in launch order: the develop exports per curve, the 8-step search, image.export."""
    import torch
    from sesrq import develop, image
    st = torch.cuda.current_stream(dev)
    lib, ilib = develop.lib(), image.lib()
    out = []
    for size, (H, W) in SIZES.items():
        o = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
        for dt in ("i8", "f32"):
            pred = torch.randint(-128, 128, (1, 3, H, W), dtype=torch.int8, device=dev) if dt == "i8" else \
                torch.rand((1, 3, H, W), device=dev) ** 2 * 1.3 - 0.15
            code = 1 if dt == "i8" else 0

            def dev_call(h, pred=pred, code=code, o=o, H=H, W=W):
                return lambda: lib.sesrq_develop_export(h, pred.data_ptr(), code, SCALE, ZERO, 0, o.data_ptr(), 1, H, W, st.cuda_stream)
            for kind in CURVES:
                p = develop.Profile(GAINS, CCM, kind)
                out.append((f"develop {kind}", "develop", size, dt, dev_call(develop.context(p, dev)), pred))
            out.append(("develop gamma, 8-step search", "develop", size, dt, dev_call(full_context(develop.Profile(GAINS, CCM, "gamma"))), pred))
            out.append(("image.export (floor)", "image", size, dt,
                        lambda pred=pred, code=code, o=o, H=H, W=W: ilib.sesrq_image_export(pred.data_ptr(), code, SCALE, ZERO, 3, 0, o.data_ptr(), 1,
                                                                                           H, W, st.cuda_stream), pred))
    return out


def torch_route(pred):
    """The route the fused kernel replaces, in torch, with the gamma curve."""
    import torch
    g = torch.tensor(GAINS, device=pred.device).view(1, 3, 1, 1)
    m = torch.tensor(CCM, device=pred.device)

    def run():
        p = (pred.float() - ZERO) * SCALE if pred.dtype == torch.int8 else pred
        w = (p.clamp(0, 1) * g).clamp(max=1)
        o = torch.einsum("kc,nchw->nkhw", m, w).clamp(0, 1)
        return (o.clamp(min=1e-8).pow(1 / 2.2) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
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
    for _, _, _, _, fn, _ in cases(dev):
        for _ in range(WARM + iters):
            assert fn() == 0
        torch.cuda.synchronize()


def summarise(trace_dir, iters, n_cases):
    """[[us]] of the last `iters` launches of each case, in launch order: the export kernels of the trace sorted by start time and cut
    into runs of WARM + iters."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    rows = []
    for f in files:
        for row in csv.DictReader(open(f)):
            if re.search(r"develop_export|image_export", row["Kernel_Name"]):
                rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3, row["Kernel_Name"]))
    rows.sort()
    per = WARM + iters
    assert len(rows) == per * n_cases, (len(rows), per, n_cases)
    out = []
    for k in range(n_cases):
        run = rows[k * per:(k + 1) * per]
        assert len({r[2] for r in run}) == 1, "a run of launches mixes kernels"
        out.append([d for _, d, _ in run][-iters:])
    return out


def host_fed(dev, frames):
    """Frames a second of 540p nrdm_3, each frame uploaded from pinned host memory and its bytes copied back: forward_develop against
    forward_raw + the torch route."""
    import time
    import numpy as np
    import torch
    import sesrq
    from sesrq import develop
    from sesrq.bundle import Bundle
    e = sesrq.Engine(Bundle.load(os.path.join(ROOT, "tests", "golden", "raw", "nrdm_3.npz")), dev)
    b = e.bundle
    H, W = SIZES["540p"]
    host = torch.from_numpy(np.random.default_rng(0).integers(0, 4096, (1, 1, H, W)).astype(np.uint16)).pin_memory()
    back = torch.empty((1, H, W, 3), dtype=torch.uint8).pin_memory()
    p = develop.Profile(GAINS, CCM, "gamma")
    g = torch.tensor(GAINS, device=dev).view(1, 3, 1, 1)
    m = torch.tensor(CCM, device=dev)

    def fused():
        back.copy_(e.forward_develop(host.to(dev, non_blocking=True), p), non_blocking=True)

    def torch_way():
        q, _ = e.forward_raw(host.to(dev, non_blocking=True), want_f=False)
        w = (((q.float() - b.zero[b.L]) * float(np.float32(b.scale[b.L]))).clamp(0, 1) * g).clamp(max=1)
        o = torch.einsum("kc,nchw->nkhw", m, w).clamp(0, 1)
        back.copy_((o.clamp(min=1e-8).pow(1 / 2.2) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous(), non_blocking=True)
    res = {}
    for name, fn in (("forward_develop", fused), ("forward_raw + torch route", torch_way)):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        rates = []
        for _ in range(3):
            t = time.perf_counter()
            for _ in range(frames):
                fn()
            torch.cuda.synchronize()
            rates.append(frames / (time.perf_counter() - t))
        res[name] = rates
    return res


def report(path, iters, reps, res_file):
    import torch
    dev = torch.device("cuda:0")
    lines = ["Develop export (libsesrq_develop.so, sesrq.develop.export), one MI355X.  Every number in sections 1 - 4 is MEASURED;",
             "tools/develop_probe.py --report made them.", ""]
    cs = cases(dev)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-only", "--iters", str(iters)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        per = summarise(tmp, iters, len(cs))
    lines += [f"1. Kernel time.  Durations come from one `rocprofv3 --kernel-trace --stats` run of its own (tools/develop_probe.py --kernels-only",
              f"   --iters {iters}; {iters} launches per row after {WARM} warm-up launches; duration = end - start timestamp).  Gains {GAINS}, a",
              "   camera's cam2rgb as the matrix.  Bytes per launch = prediction + output, from the shapes; (a)/(b) is the row's median over the",
              "   image.export median of the same frame.", "",
              "   frame  pred  case                            median      min     in + out MB    share of 8 TB/s   (a)/(b)"]
    med = {}
    for (label, _, size, dt, _, _), us in zip(cs, per):
        med[(label, size, dt)] = statistics.median(us)
    for (label, kind, size, dt, _, _), us in zip(cs, per):
        a, b = nbytes(*SIZES[size], dt)
        m = statistics.median(us)
        ratio = f"{m / med[('image.export (floor)', size, dt)]:.2f}" if kind == "develop" else "  -"
        lines.append(f"   {size:5s}  {dt:4s}  {label:30s} {m:7.2f} us {min(us):7.2f} us  {a / 1e6:5.1f} + {b / 1e6:4.1f}   {100 * (a + b) / (m * 1e-6) / PEAK:5.1f} %"
                     f"          {ratio}")
    lines.append("")

    lines += [f"2. Without the profiler, one process, HIP events around back-to-back launches: {reps} repetitions, the candidates alternating",
              f"   inside a repetition ({iters} launches of a kernel, 20 calls of the torch route); median (min .. max) us per call; gamma curve.", ""]
    for size in SIZES:
        for dt in ("i8", "f32"):
            mine = {label: (fn, iters) for label, _, s, d, fn, _ in cs if s == size and d == dt and label in
                    ("develop gamma", "develop gamma, 8-step search", "image.export (floor)")}
            pred = next(p for label, _, s, d, _, p in cs if s == size and d == dt)
            mine["torch route (clamp, mul, clamp, matmul, clamp, pow, x 255, round, cast, permute)"] = (torch_route(pred), 20)
            for fn, _ in mine.values():
                for _ in range(5):
                    fn()
            got = {k: [] for k in mine}
            for _ in range(reps):
                for k, (fn, calls) in mine.items():
                    got[k].append(window(fn, calls))
            lines.append(f"   {size} from {dt}")
            for k, us in got.items():
                lines.append(f"      {k:84s} {statistics.median(us):9.2f} ({min(us):.2f} .. {max(us):.2f})")
            d_us, f_us, i_us, t_us = (statistics.median(got[k]) for k in mine)
            lines.append(f"      (a)/(b) = {d_us / i_us:.2f}; (c)/(a) = {t_us / d_us:.1f}; the 8-step search takes {f_us / d_us:.2f}x the indexed one")
    peak = torch.cuda.max_memory_allocated(dev)
    lines += ["", f"   Peak device memory of the process, torch route included: {peak / 1e6:.0f} MB (the fused export allocates nothing).", ""]

    fed = host_fed(dev, 300)
    lines += ["3. Host-fed nrdm_3 at 540p: a 12-bit frame uploaded from pinned memory, the net, the developed bytes copied back to pinned memory;",
              "   300 frames a window, one stream, three windows; frames a second."]
    for k, r in fed.items():
        lines.append(f"      {k:30s} {statistics.median(r):8.1f} ({min(r):.1f} .. {max(r):.1f})")
    a, b = (statistics.median(fed[k]) for k in fed)
    lines += [f"      forward_develop runs {a / b:.2f}x the frames of forward_raw + torch route", ""]
    lines += ["4. Registers, scratch, LDS:"] + ["   " + ln for ln in (open(res_file).read().splitlines() if res_file else resources())]
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
