#!/usr/bin/env python3
"""RGB video route measurements (sesrq.video_rgb, libsesrq_video_rgb.so) on one GPU; profiles/video_rgb_probe.txt is its --report.
Every GPU step is an invocation of its own (run each under its own `timeout`, stop at the first that fails); a step writes its
section into --out DIR, and --report joins the sections without touching a GPU.

  python tools/video_rgb_probe.py --resources --out DIR       # no GPU: compile the library's source for gfx950 with
                                                               # -Rpass-analysis=kernel-resource-usage: registers, scratch, LDS
  python tools/video_rgb_probe.py --step kernels --out DIR     # 1. kernel time of every decode and export instantiation, 1080p in and
                                                               #    4K out, from a rocprofv3 kernel trace of a child process
                                                               #    (--kernels-only) of its own
  python tools/video_rgb_probe.py --step routes --out DIR      # 2. without the profiler, alternating in one process (HIP events around
                                                               #    back-to-back launches): each fused kernel against the torch route
                                                               #    it replaces and against image_decode<rgb> / image_export, the
                                                               #    per-byte yardsticks; asserts fused < torch route
  python tools/video_rgb_probe.py --step hostfed --out DIR     # 3. host-fed SESR-x2 1080p frames/s from pinned NV12 (forward_video_rgb)
                                                               #    against forward_image from pinned RGB bytes
  python tools/video_rgb_probe.py --report OUT --out DIR       # join; everything of an earlier OUT from the line "5. " on is kept
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
LR, HR = (1080, 1920), (2160, 3840)
SCALE, ZERO = 0.0047, -119
IN_SCALE, IN_ZERO = 0.0032141484320163728, -146
FMTS = ("nv12", "i420")
OUTS = {"q0": 1, "x": 2, "q0,x": 3}
DECODES = [(f, o) for f in FMTS for o in OUTS]
EXPORTS = [(d, f) for d in ("i8", "f32") for f in FMTS]
WARM = 20


def dname(f, o):
    return f"vrgb_decode<{f},{o}>"


def ename(d, f):
    return f"vrgb_export<{d},{f}>"


def of_mangled(name):
    """The instantiation's name from a (mangled or demangled) kernel name, or None."""
    m = re.search(r"vrgb_decode(?:ILi(\d)ELi(\d)E|<\s*(\d)\s*,\s*(\d)\s*>)", name)
    if m:
        f, o = (int(v) for v in m.groups() if v is not None)
        return dname(FMTS[f], next(k for k, v in OUTS.items() if v == o))
    m = re.search(r"vrgb_export(?:ILi(\d)ELi(\d)E|<\s*(\d)\s*,\s*(\d)\s*>)", name)
    if m:
        d, f = (int(v) for v in m.groups() if v is not None)
        return ename("i8" if d == 1 else "f32", FMTS[f])
    return None


def decode_bytes(o):
    """(surface read, written) of one 1080p decode."""
    px = LR[0] * LR[1]
    return px * 3 // 2, 3 * px * ((1 if OUTS[o] & 1 else 0) + (4 if OUTS[o] & 2 else 0))


def export_bytes(d):
    px = HR[0] * HR[1]
    return 3 * px * (1 if d == "i8" else 4), px * 3 // 2


def resources():
    """Registers, scratch and LDS of every kernel of sesrq_video_rgb.hip as the library's Makefile compiles it (no GPU needed)."""
    csrc = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sesrq_video_rgb.hip"), "-o",
                            os.path.join(tmp, "video_rgb.o")], capture_output=True, text=True, check=True)
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
    lines = ["4. Registers, scratch, LDS: compiled for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage:"]
    for k in out:
        lines.append(f"   {of_mangled(k['name']) or k['name']:26s} VGPRs {k.get('VGPRs'):>3s}  scratch {k.get('ScratchSize')} B/lane  "
                     f"LDS {k.get('LDS'):>5s} B/block  occupancy {k.get('Occupancy')} waves/SIMD")
    assert len(out) == len(DECODES) + len(EXPORTS) and all(k.get("ScratchSize") == "0" for k in out), "an instantiation uses scratch"
    lines.append("   no scratch in any instantiation")
    return lines


# ----------------------------------------------------------------------------------------------------------------- launches
def buffers(dev):
    """{instantiation: a function that launches it once} on random 1080p surfaces / 4K predictions."""
    import torch
    from sesrq import video, video_rgb
    st = torch.cuda.current_stream(dev)
    fns = {}
    q0 = torch.empty((1, 3, *LR), dtype=torch.int8, device=dev)
    x = torch.empty((1, 3, *LR), dtype=torch.float32, device=dev)
    for f in FMTS:
        s = video.Surface.alloc(f, 1, *LR, dev)
        s.buf.copy_(torch.randint(0, 256, (s.buf.numel(),), dtype=torch.uint8, device=dev))
        for o, bits in OUTS.items():
            fns[dname(f, o)] = (lambda s=s, bits=bits: video_rgb.launch_decode(dev, IN_SCALE, IN_ZERO, 0, s, q0 if bits & 1 else None,
                                                                                x if bits & 2 else None, st))
    preds = {"i8": torch.randint(-128, 128, (1, 3, *HR), dtype=torch.int8, device=dev), "f32": torch.rand((1, 3, *HR), device=dev) * 1.2 - 0.1}
    outs = {f: video.Surface.alloc(f, 1, *HR, dev) for f in FMTS}
    for d, f in EXPORTS:
        fns[ename(d, f)] = (lambda d=d, f=f: video_rgb.launch_export(preds[d], SCALE, ZERO, outs[f], st))
    return fns, preds, outs


def kernels_only(iters):
    import torch
    dev = torch.device("cuda:0")
    fns, _, _ = buffers(dev)
    for fn in fns.values():
        for _ in range(WARM + iters):
            fn()
        torch.cuda.synchronize()


def step_kernels(iters):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-only", "--iters", str(iters)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=420)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert files, "no kernel trace"
        per = {}
        for f in files:
            for row in csv.DictReader(open(f)):
                k = of_mangled(row["Kernel_Name"])
                if k:
                    per.setdefault(k, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    lines = [f"1. Kernel time.  Durations come from one `rocprofv3 --kernel-trace --stats` run of its own (tools/video_rgb_probe.py --kernels-only",
             f"   --iters {iters}; the last {iters} launches per row after {WARM} warm-up launches; duration = end - start timestamp).  A decode reads one",
             "   1080 x 1920 4:2:0 surface (3.1 MB), an export writes one 2160 x 3840 surface (12.4 MB); bytes per launch from the shapes.", "",
             "   kernel                       median      min       read + written MB      share of 8 TB/s (median)"]
    for name, (a, b) in [(dname(f, o), decode_bytes(o)) for f, o in DECODES] + [(ename(d, f), export_bytes(d)) for d, f in EXPORTS]:
        us = [d for _, d in sorted(per[name])][-iters:]
        assert len(us) == iters, (name, len(us))
        med = statistics.median(us)
        lines.append(f"   {name:26s} {med:8.2f} us {min(us):8.2f} us   {a / 1e6:5.1f} + {b / 1e6:5.1f} = {(a + b) / 1e6:6.1f}   "
                     f"{100 * (a + b) / (med * 1e-6) / PEAK:5.1f} %")
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


def torch_decode(dev, s, want_q, want_f):
    """The route the fused decode replaces: float chroma planes, F.interpolate(mode="bicubic"), the matrix, round, clamp, byte cast,
    permute to an interleaved RGB image, then the image decode (forward_image's first launch)."""
    import torch
    import torch.nn.functional as F
    from sesrq import image
    st = torch.cuda.current_stream(dev)
    H, W = s.H, s.W
    q0 = torch.empty((1, 3, H, W), dtype=torch.int8, device=dev) if want_q else None
    x = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev) if want_f else None
    m = torch.tensor([[1.16438356, 0.0, 1.59602679], [1.16438356, -0.39176229, -0.81296765], [1.16438356, 2.01723214, 0.0]], device=dev)

    def run():
        if s.fmt_name == "nv12":
            c = s.c0.view(s.N, s.c0.shape[1], -1, 2).permute(0, 3, 1, 2).float()
        else:
            c = torch.stack([s.c0, s.c1], 1).float()
        up = F.interpolate(c, scale_factor=2, mode="bicubic", align_corners=False)[..., :H, :W]
        ycc = torch.cat([s.y[:, None].float() - 16.0, up - 128.0], 1)
        rgb = torch.einsum("oc,nchw->nhwo", m, ycc).round().clamp(0, 255).to(torch.uint8).contiguous()
        image.launch(dev, IN_SCALE, IN_ZERO, 0, rgb, image.RGB, "rgb", q0, x, st)
    return run


def torch_export(dev, pred, out):
    """The route the fused export replaces: the image export to an interleaved RGB image, float, the matrix, round, byte cast, the
    Y plane copied in; chroma averaged over 2 x 2 blocks, rounded, cast and, for NV12, interleaved."""
    import torch
    import torch.nn.functional as F
    from sesrq import image
    dom = dict(scale=SCALE, zero=ZERO) if pred.dtype == torch.int8 else {}
    m = torch.tensor([[65.481, 128.553, 24.966], [-37.797, -74.203, 112.0], [112.0, -93.786, -18.214]], device=dev) / 255.0
    off = torch.tensor([16.0, 128.0, 128.0], device=dev).view(1, 3, 1, 1)

    def run():
        rgb = image.export(pred, **dom).float()
        ycc = torch.einsum("oc,nhwc->nohw", m, rgb) + off
        out.y.copy_(ycc[:, 0].round().to(torch.uint8))
        c = F.avg_pool2d(ycc[:, 1:], 2).round().to(torch.uint8)
        if out.fmt_name == "nv12":
            out.c0.copy_(c.permute(0, 2, 3, 1).reshape(out.c0.shape))
        else:
            out.c0.copy_(c[:, 0])
            out.c1.copy_(c[:, 1])
    return run


def step_routes(iters, reps):
    import torch
    from sesrq import image as I, video
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    fns, preds, outs = buffers(dev)
    lib = I.lib()
    o3 = torch.empty((1, *HR, 3), dtype=torch.uint8, device=dev)
    rgb_lr = torch.randint(0, 256, (1, *LR, 3), dtype=torch.uint8, device=dev)
    q_lr = torch.empty((1, 3, *LR), dtype=torch.int8, device=dev)
    pq = preds["i8"]
    yard = {"image_decode<rgb,q0> at 1080p (6.2 MB in, 6.2 MB out)": lambda: I.launch(dev, IN_SCALE, IN_ZERO, 0, rgb_lr, I.RGB, "rgb", q_lr, None, st),
            "image_export<i8,C3> at 4K (24.9 MB in, 24.9 MB out)": lambda: lib.sesrq_image_export(pq.data_ptr(), I.PRED_I8, SCALE, ZERO, 3, 0, o3.data_ptr(), 1, *HR, st.cuda_stream),
            "image_export<i8,C1> at 4K (8.3 MB in, 8.3 MB out)": lambda: lib.sesrq_image_export(pq.data_ptr(), I.PRED_I8, SCALE, ZERO, 1, 0, o3.data_ptr(), 1, *HR, st.cuda_stream)}
    lines = [f"2. Without the profiler, one process, HIP events around back-to-back launches: {reps} repetitions, the candidates alternating",
             f"   inside a repetition ({iters} launches of a kernel, 10 calls of the torch route); median (min .. max) us per call.", ""]
    ysticks = {}
    for k, fn in yard.items():
        for _ in range(WARM):
            fn()
        us = [window(fn, iters) for _ in range(reps)]
        ysticks[k] = statistics.median(us)
        lines.append(f"   yardstick {k:58s} {statistics.median(us):9.2f} ({min(us):.2f} .. {max(us):.2f})")
    lines.append("")
    srcs = {}
    for f in FMTS:
        s = video.Surface.alloc(f, 1, *LR, dev)
        s.buf.copy_(torch.randint(0, 256, (s.buf.numel(),), dtype=torch.uint8, device=dev))
        srcs[f] = s
    worst = None
    cases = [(dname(f, o), torch_decode(dev, srcs[f], OUTS[o] & 1, OUTS[o] & 2)) for f, o in DECODES] + \
            [(ename(d, f), torch_export(dev, preds[d], outs[f])) for d, f in EXPORTS]
    for name, route in cases:
        for fn in (fns[name], route):
            for _ in range(5):
                fn()
        got = {"fused": [], "torch": []}
        for _ in range(reps):
            got["fused"].append(window(fns[name], iters))
            got["torch"].append(window(route, 10))
        f_us, t_us = statistics.median(got["fused"]), statistics.median(got["torch"])
        lines.append(f"   {name:26s} fused {f_us:9.2f} ({min(got['fused']):.2f} .. {max(got['fused']):.2f})   replaced torch route {t_us:10.2f} "
                     f"({min(got['torch']):.2f} .. {max(got['torch']):.2f})   {t_us / f_us:5.1f}x")
        assert max(got["fused"]) < min(got["torch"]), f"{name}: the fused kernel is not faster than the torch route it replaces"
        worst = t_us / f_us if worst is None else min(worst, t_us / f_us)
    peak = torch.cuda.max_memory_allocated(dev)
    lines += ["", f"   Every fused kernel is faster than the torch route measured beside it; the smallest ratio is {worst:.1f}x.",
              f"   Peak device memory of the process, torch routes included: {peak / 1e6:.0f} MB (the fused kernels allocate nothing)."]
    return lines


def step_hostfed(frames):
    """SESR-x2 1080p frames per second fed from pinned host memory, int8 output left on the device for the image route (as
    profiles/image_probe.txt measured it) and exported and returned to pinned memory for the video route."""
    import torch
    import sesrq
    from sesrq import video
    from sesrq.bundle import Bundle
    dev = torch.device("cuda:0")
    e = sesrq.Engine(Bundle.load(os.path.join(ROOT, "tests", "golden", "image", "sesr_x2_rand.npz")), dev)
    H, W = LR
    up = torch.randint(0, 256, (video.frame_bytes("nv12", H, W),), dtype=torch.uint8).pin_memory()
    down = torch.empty((video.frame_bytes("nv12", 2 * H, 2 * W),), dtype=torch.uint8).pin_memory()
    dbuf = torch.empty_like(up, device=dev)
    src = video.Surface.views(dbuf, "nv12", 1, H, W)
    out = video.Surface.alloc("nv12", 1, 2 * H, 2 * W, dev)
    rgb_up = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8).pin_memory()
    rgb_d = torch.empty_like(rgb_up, device=dev)
    oq = torch.empty((1, 3, 2 * H, 2 * W), dtype=torch.int8, device=dev)

    def vid_up():
        dbuf.copy_(up, non_blocking=True)
        e.forward_video_rgb(src, out=out)

    def vid():
        vid_up()
        down.copy_(out.buf, non_blocking=True)

    def img():
        rgb_d.copy_(rgb_up, non_blocking=True)
        e.forward_image(rgb_d, want_q=True, want_f=False, out_q=oq)
    res = {}
    for k, fn in (("forward_video_rgb  NV12 up (3.1 MB), exported, NV12 down (12.4 MB)", vid),
                  ("forward_video_rgb  NV12 up (3.1 MB), exported, surface left on the device", vid_up),
                  ("forward_image      RGB up (6.2 MB), int8 output left on the device", img)):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        rates = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(frames):
                fn()
            torch.cuda.synchronize()
            rates.append(frames / (time.perf_counter() - t0))
        res[k] = rates
    lines = [f"3. Host-fed SESR-x2 1080p -> 4K from pinned memory, one stream, {frames} frames a repetition, 3 repetitions (report only):"]
    for k, r in res.items():
        lines.append(f"      {k:76s} {statistics.median(r):8.0f} frames/s ({min(r):.0f} .. {max(r):.0f})")
    return lines


def hand_written(path):
    """The hand-written tail of an earlier report at `path` (from the line that starts "5. " on, with the blank line before it), or []."""
    if not os.path.isfile(path):
        return []
    old = open(path).read().splitlines()
    at = next((i for i, ln in enumerate(old) if ln.startswith("5. ")), None)
    return [] if at is None else [""] + old[at:]


def report(path, out):
    lines = ["RGB video route (libsesrq_video_rgb.so, sesrq.video_rgb), one MI355X.  Every number below is MEASURED.  tools/video_rgb_probe.py made",
             'sections 1 - 4, one GPU step per invocation; sections 5 and 6 are written by hand and kept when --report rewrites this file.', ""]
    for name in ("1_kernels.txt", "2_routes.txt", "3_hostfed.txt", "4_resources.txt"):
        lines += open(os.path.join(out, name)).read().splitlines() + [""]
    lines = lines[:-1] + hand_written(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default="build/video_rgb_probe", help="directory of the sections (build/ is kept out of git)")
    ap.add_argument("--step", choices=("kernels", "routes", "hostfed"))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--report", metavar="OUT")
    args = ap.parse_args()
    if args.kernels_only:
        return kernels_only(args.iters)
    if args.report:
        return report(args.report, args.out)
    if args.resources:
        name, lines = "4_resources.txt", resources()
    elif args.step == "kernels":
        name, lines = "1_kernels.txt", step_kernels(args.iters)
    elif args.step == "routes":
        name, lines = "2_routes.txt", step_routes(args.iters, args.reps)
    elif args.step == "hostfed":
        name, lines = "3_hostfed.txt", step_hostfed(args.frames)
    else:
        ap.error("one of --step, --resources, --report, --kernels-only")
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, name), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
