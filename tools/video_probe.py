#!/usr/bin/env python3
"""Video-route measurements (sesrq.video, libsesrq_video.so) on one GPU; profiles/video_probe.txt is its --report.

  python tools/video_probe.py --report OUT      # everything below into OUT (the kernel-time run is a child process under rocprofv3);
                                                # sections of OUT (or of --keep-from FILE) from the line "5. " on are hand-written and kept
  python tools/video_probe.py --kernels-only    # only the export / decode launches (what the `rocprofv3 --kernel-trace --stats -- ...` child runs)
  python tools/video_probe.py --resources       # no GPU: compile the library's source for gfx950 with
                                                # -Rpass-analysis=kernel-resource-usage and print registers, scratch and LDS per kernel

1. kernel time of the fused export and of the decode, from a rocprofv3 kernel trace of its own (launches after warm-up; duration =
   end - start): 540p -> 4K at r = 4 and 1080p -> 4K at r = 2, int8 and fp32 Y, NV12 and I420 out; decode at 540p and 1080p;
2. without the profiler, alternating in one process (HIP events around back-to-back launches, several repetitions): the fused export
   against the route it replaces (the grey export for Y, then per chroma plane fp32 F.interpolate(mode="bicubic"), round, clamp, byte
   cast, and for NV12 the interleave) and against image_export<i8,C3> / <i8,C1> at 4K, the existing byte-store kernels;
3. host-fed SESR-x4 540p frames per second from pinned memory: forward_video (NV12 up, NV12 down) against forward_colour, which is
   forward_image followed by the colour export (RGB up, RGB down).
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
SIZES = {"540p -> 4K r=4": (540, 960, 4), "1080p -> 4K r=2": (1080, 1920, 2)}
# name -> (LR H, LR W, r, Y dtype, out format): all give a 2160 x 3840 4:2:0 frame
CASES = {f"{s} {dt} Y {of}": (H, W, r, dt, of) for s, (H, W, r) in SIZES.items() for dt in ("i8", "f32") for of in ("nv12", "i420")}
SCALE, ZERO = 0.0047, -119
IN_SCALE, IN_ZERO = 0.0022352789546929153, -214
MANGLED = {"ILi1ELi2ELi0E": "video_export<i8,r2,nv12>", "ILi1ELi2ELi1E": "video_export<i8,r2,i420>", "ILi1ELi4ELi0E": "video_export<i8,r4,nv12>",
           "ILi1ELi4ELi1E": "video_export<i8,r4,i420>", "ILi0ELi2ELi0E": "video_export<f32,r2,nv12>", "ILi0ELi2ELi1E": "video_export<f32,r2,i420>",
           "ILi0ELi4ELi0E": "video_export<f32,r4,nv12>", "ILi0ELi4ELi1E": "video_export<f32,r4,i420>", "decodeILi1E": "video_decode<q0>",
           "decodeILi2E": "video_decode<x>", "decodeILi3E": "video_decode<q0,x>"}


def nbytes(H, W, r, dt):
    """(luma read, LR chroma read, 4:2:0 frame written) of one export."""
    hr = r * H * r * W
    return hr * (1 if dt == "i8" else 4), H * W // 2, hr * 3 // 2


def instance(r, dt, of):
    return f"video_export<{dt},r{r},{of}>"


def resources():
    """Registers, scratch and LDS of every kernel of sesrq_video.hip as the library's Makefile compiles it (no GPU needed)."""
    csrc = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sesrq_video.hip"), "-o",
                            os.path.join(tmp, "video.o")], capture_output=True, text=True, check=True)
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
    lines = ["compiled for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage:"]
    for k in out:
        nice = next((v for s, v in MANGLED.items() if s in k["name"]), k["name"])
        lines.append(f"   {nice:26s} VGPRs {k.get('VGPRs'):>3s}  scratch {k.get('ScratchSize')} B/lane  LDS {k.get('LDS'):>5s} B/block  "
                     f"occupancy {k.get('Occupancy')} waves/SIMD")
    assert len(out) == len(MANGLED) and all(k.get("ScratchSize") == "0" for k in out), "an instantiation uses scratch"
    lines.append("   no scratch in any instantiation")
    return lines


def surfaces(dev, H, W, r):
    """(LR surface with random planes, {format: HR output surface}) on the device."""
    import torch
    from sesrq import video
    lr = video.Surface.alloc("nv12", 1, H, W, dev)
    lr.buf.copy_(torch.randint(0, 256, (lr.buf.numel(),), dtype=torch.uint8, device=dev))
    return lr, {f: video.Surface.alloc(f, 1, r * H, r * W, dev) for f in ("nv12", "i420")}


def buffers(dev):
    import torch
    b, per_size = {}, {}
    for name, (H, W, r, dt, of) in CASES.items():
        if (H, W) not in per_size:
            per_size[(H, W)] = surfaces(dev, H, W, r) + ({"i8": torch.randint(-128, 128, (1, 1, r * H, r * W), dtype=torch.int8, device=dev),
                                                          "f32": torch.rand((1, 1, r * H, r * W), device=dev) * 1.2 - 0.1},)
        lr, outs, ys = per_size[(H, W)]
        b[name] = (ys[dt], lr, r, outs[of])
    return b


def fused(st, y, lr, r, out):
    from sesrq import video
    return lambda: video.launch_export(y, SCALE, ZERO, lr, r, out, st)


def decoder(st, dev, lr):
    import torch
    from sesrq import video
    q0 = torch.empty((1, 1, lr.H, lr.W), dtype=torch.int8, device=dev)
    return lambda: video.launch_decode(dev, IN_SCALE, IN_ZERO, 0, lr, q0, None, st)


def torch_route(y, lr, r, out):
    """The route the fused kernel replaces: the existing grey export for Y, then per chroma plane fp32 F.interpolate(mode="bicubic"),
    round, clamp, byte cast, and for NV12 the interleave into the surface's chroma plane."""
    import torch
    import torch.nn.functional as F
    from sesrq import image
    dom = dict(scale=SCALE, zero=ZERO) if y.dtype == torch.int8 else {}
    H2, W2 = out.H // 2, out.W // 2

    def run():
        out.y.copy_(image.export(y, **dom)[..., 0])
        c = lr.c0.view(lr.N, lr.c0.shape[1], -1, 2).permute(0, 3, 1, 2).float()       # (N, 2, Hc, Wc): Cb, Cr
        up = F.interpolate(c, scale_factor=r, mode="bicubic", align_corners=False)[..., :H2, :W2]
        u8 = up.round().clamp(0, 255).to(torch.uint8)
        if out.fmt_name == "nv12":
            out.c0.copy_(u8.permute(0, 2, 3, 1).reshape(out.c0.shape))
        else:
            out.c0.copy_(u8[:, 0])
            out.c1.copy_(u8[:, 1])
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
    bufs = buffers(dev)
    fns = [fused(st, *args) for args in bufs.values()]
    fns += [decoder(st, dev, surfaces(dev, H, W, r)[0]) for H, W, r in SIZES.values()]
    for fn in fns:
        for _ in range(20 + iters):
            fn()
        torch.cuda.synchronize()


def summarise(trace_dir, iters):
    """({export instantiation: [us]}, [decode us in launch order]) of a rocprofv3 kernel-trace CSV."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    per, dec = {}, []
    for f in files:
        for row in csv.DictReader(open(f)):
            t0, us = int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            m = re.search(r"video_export<\s*(\d)\s*,\s*(\d)\s*,\s*(\d)\s*>", row["Kernel_Name"])
            if m:
                key = instance(int(m.group(2)), "i8" if m.group(1) == "1" else "f32", "nv12" if m.group(3) == "0" else "i420")
                per.setdefault(key, []).append((t0, us))
            elif "video_decode" in row["Kernel_Name"]:
                dec.append((t0, us))
    return {k: [d for _, d in sorted(v)][-iters:] for k, v in per.items()}, [d for _, d in sorted(dec)]


def host_fed(dev, frames):
    """SESR-x4 540p frames per second fed from pinned host memory and returned to it: (forward_video NV12 -> NV12, forward_colour RGB -> RGB)."""
    import torch
    import sesrq
    from sesrq import video
    from sesrq.bundle import Bundle
    e = sesrq.Engine(Bundle.load(os.path.join(ROOT, "tests", "golden", "image", "sesr_x4.npz")), dev)
    H, W, r = 540, 960, 4
    up = torch.randint(0, 256, (video.frame_bytes("nv12", H, W),), dtype=torch.uint8).pin_memory()
    down = torch.empty((video.frame_bytes("nv12", r * H, r * W),), dtype=torch.uint8).pin_memory()
    dbuf = torch.empty_like(up, device=dev)
    src = video.Surface.views(dbuf, "nv12", 1, H, W)
    out = video.Surface.alloc("nv12", 1, r * H, r * W, dev)
    rgb_up = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8).pin_memory()
    rgb_down = torch.empty((1, r * H, r * W, 3), dtype=torch.uint8).pin_memory()
    rgb_d = torch.empty_like(rgb_up, device=dev)
    rgb_o = torch.empty_like(rgb_down, device=dev)

    def vid():
        dbuf.copy_(up, non_blocking=True)
        e.forward_video(src, out=out)
        down.copy_(out.buf, non_blocking=True)

    def col():
        rgb_d.copy_(rgb_up, non_blocking=True)
        e.forward_colour(rgb_d, out=rgb_o)
        rgb_down.copy_(rgb_o, non_blocking=True)
    res = []
    for fn in (vid, col):
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
        res.append(rates)
    return res


def report(path, iters, reps, res_file, frames, keep=None):
    import torch
    from sesrq import image as I
    lines = ["Video route (libsesrq_video.so, sesrq.video), one MI355X.  Every number below is MEASURED.  tools/video_probe.py --report made",
             'sections 1 - 4; sections 5 and 6 are appended by hand, and --report keeps everything from the line "5. " on when it rewrites this file.',
             ""]
    # 1. kernel time: a child process under the profiler
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-only", "--iters", str(iters)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        per, dec = summarise(tmp, iters)
    lines += [f"1. Kernel time.  Durations come from one `rocprofv3 --kernel-trace --stats` run of its own (tools/video_probe.py --kernels-only",
              f"   --iters {iters}; {iters} launches per row after 20 warm-up launches; duration = end - start timestamp).  Every export writes one",
              "   2160 x 3840 4:2:0 frame (12.4 MB); bytes per launch = Y + LR chroma + output, from the shapes.  Two cases share an",
              "   instantiation's launches only if they share r, Y dtype and output format: none do.", "",
              "   case                            kernel                       median     min      Y + chroma + out MB     share of 8 TB/s (median)"]
    for name, (H, W, r, dt, of) in CASES.items():
        us = per[instance(r, dt, of)]
        assert len(us) == iters, (name, len(us))
        a, b, c = nbytes(H, W, r, dt)
        med = statistics.median(us)
        lines.append(f"   {name:31s} {instance(r, dt, of):26s} {med:7.2f} us {min(us):7.2f} us   {a / 1e6:5.1f} + {b / 1e6:4.1f} + {c / 1e6:4.1f} = "
                     f"{(a + b + c) / 1e6:5.1f}   {100 * (a + b + c) / (med * 1e-6) / PEAK:5.1f} %")
    assert len(dec) == 2 * (20 + iters), len(dec)
    for k, (s, (H, W, r)) in enumerate(SIZES.items()):
        us = dec[k * (20 + iters) + 20:(k + 1) * (20 + iters)]
        lines.append(f"   decode {s.split(' ')[0]:24s} {'video_decode<q0>':26s} {statistics.median(us):7.2f} us {min(us):7.2f} us   "
                     f"{H * W / 1e6:.1f} MB read, {H * W / 1e6:.1f} MB of q0 written")
    lines.append("")

    # 2. alternating, without the profiler
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    bufs = buffers(dev)
    pq = torch.randint(-128, 128, (1, 3, 2160, 3840), dtype=torch.int8, device=dev)
    o3 = torch.empty((1, 2160, 3840, 3), dtype=torch.uint8, device=dev)
    lib = I.lib()
    grey3 = lambda: lib.sesrq_image_export(pq.data_ptr(), I.PRED_I8, SCALE, ZERO, 3, 0, o3.data_ptr(), 1, 2160, 3840, st.cuda_stream)  # noqa: E731
    grey1 = lambda: lib.sesrq_image_export(pq.data_ptr(), I.PRED_I8, SCALE, ZERO, 1, 0, o3.data_ptr(), 1, 2160, 3840, st.cuda_stream)  # noqa: E731
    lines += [f"2. Without the profiler, one process, HIP events around back-to-back launches: {reps} repetitions, the candidates alternating",
              f"   inside a repetition ({iters} launches of a kernel, 20 calls of the torch route); median (min .. max) us per call.", ""]
    for name, (y, lr, r, o) in bufs.items():
        H, W, _, dt, of = CASES[name]
        cands = {"fused video export": (fused(st, y, lr, r, o), iters),
                 "image_export<i8,C3> at 4K (24.9 MB out)": (grey3, iters), "image_export<i8,C1> at 4K (8.3 MB out)": (grey1, iters),
                 "replaced route (grey export, 2 x bicubic, round, clamp, cast" + (", interleave)" if of == "nv12" else ")"): (torch_route(y, lr, r, o), 20)}
        for fn, _ in cands.values():
            for _ in range(5):
                fn()
        got = {k: [] for k in cands}
        for _ in range(reps):
            for k, (fn, calls) in cands.items():
                got[k].append(window(fn, calls))
        lines.append(f"   {name}")
        for k, us in got.items():
            lines.append(f"      {k:72s} {statistics.median(us):9.2f} ({min(us):.2f} .. {max(us):.2f})")
        f_us, g3_us, g1_us, t_us = (statistics.median(got[k]) for k in cands)
        a, b, c = nbytes(H, W, r, dt)
        lines.append(f"      fused vs replaced route: {t_us / f_us:.1f}x faster; per output byte the fused export takes {(f_us / c) / (g3_us / 24883200):.2f}x the "
                     f"time of image_export<i8,C3> and {(f_us / c) / (g1_us / 8294400):.2f}x that of image_export<i8,C1> ({(a + b + c) / 1e6:.1f} MB moved)")
    lines.append("")
    for s, (H, W, r) in SIZES.items():
        fn = decoder(st, dev, surfaces(dev, H, W, r)[0])
        for _ in range(20):
            fn()
        us = [window(fn, iters) for _ in range(reps)]
        lines.append(f"   decode {s.split(' ')[0]} (q0): {statistics.median(us):.2f} ({min(us):.2f} .. {max(us):.2f}) us per host-issued call")
    peak = torch.cuda.max_memory_allocated(dev)
    lines += ["", f"   Peak device memory of the process, torch route included: {peak / 1e6:.0f} MB (the fused export allocates nothing).", ""]

    # 3. host-fed
    vid, col = host_fed(dev, frames)
    lines += [f"3. Host-fed SESR-x4 540p -> 4K from pinned memory and back to it, one stream, {frames} frames a repetition, 3 repetitions (report only):",
              f"      forward_video   NV12 up (0.78 MB), NV12 down (12.4 MB)    {statistics.median(vid):8.0f} frames/s ({min(vid):.0f} .. {max(vid):.0f})",
              f"      forward_colour  RGB up (1.56 MB), RGB down (24.9 MB)      {statistics.median(col):8.0f} frames/s ({min(col):.0f} .. {max(col):.0f})",
              "      (forward_colour is forward_image followed by the colour export)", ""]
    lines += ["4. Registers, scratch, LDS:"] + ["   " + ln for ln in (open(res_file).read().splitlines() if res_file else resources())]
    lines += hand_written(keep if keep else path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def hand_written(path):
    """The hand-written tail of an earlier report at `path` (from the line that starts "5. " on, with the blank line before it), or []."""
    if not os.path.isfile(path):
        return []
    old = open(path).read().splitlines()
    at = next((i for i, ln in enumerate(old) if ln.startswith("5. ")), None)
    return [] if at is None else [""] + old[at:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-file", help="the output of an earlier --resources run to include instead of compiling again")
    ap.add_argument("--report", metavar="OUT")
    ap.add_argument("--keep-from", metavar="FILE", help="the earlier report whose hand-written sections (5 on) are kept (default: OUT itself)")
    args = ap.parse_args()
    if args.resources:
        print("\n".join(resources()))
    elif args.kernels_only:
        kernels_only(args.iters)
    elif args.report:
        report(args.report, args.iters, args.reps, args.resources_file, args.frames, args.keep_from)
    else:
        ap.error("one of --report, --kernels-only, --resources")


if __name__ == "__main__":
    main()
