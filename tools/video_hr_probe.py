#!/usr/bin/env python3
"""HR-only video route measurements (sesrq.video_hr, libsesrq_video_hr.so) on one GPU; profiles/video_hr_probe.txt is its --report.

  python tools/video_hr_probe.py --report OUT [--resources-file FILE]
  python tools/video_hr_probe.py --resources      # no GPU: compile the library's source for gfx950 with
                                                  # -Rpass-analysis=kernel-resource-usage and print registers, scratch and LDS

1. one process, HIP events around back-to-back launches, the candidates of one size alternating inside a repetition, median of the
   repetitions: 1080p -> 540p at r = 2 and 2160p -> 540p at r = 4, NV12 and I420 in --
     the fused kernel writing q0 and the LR chroma planes (what forward_video_hr launches);
     the fused kernel writing the whole LR surface (what forward_video_rgb_hr launches);
     the `downscale` kernel of libsesrq_downscale.so on an RGB image of the same HR size (q0 out): 3 B/px read against 1.5, the bar per
     HR pixel;
     the torch route it replaces: per plane fp32 F.interpolate(mode="bicubic", antialias=True), round, clamp, byte cast;
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

SIZES = {"1080p -> 540p r=2": (1080, 1920, 2), "2160p -> 540p r=4": (2160, 3840, 4)}      # HR luma H, W, r
IN_SCALE, IN_ZERO = 0.0022352789546929153, -214


def resources():
    """Registers, scratch and LDS of every kernel of sesrq_video_hr.hip as the library's Makefile compiles it (no GPU needed)."""
    csrc = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sesrq_video_hr.hip"), "-o",
                            os.path.join(tmp, "video_hr.o")], capture_output=True, text=True, check=True)
    out, cur = [], {}
    for ln in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if m and m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            out.append(cur)
        elif m:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    assert len(out) == 44 and all(k["ScratchSize"] == 0 for k in out), "an instantiation is missing or uses scratch"
    lines = ["compiled for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage, 44 instantiations "
             "video_hr<r, input format, LR format, luma outputs>:"]
    fmt = {"0": "nv12", "1": "i420", "n1": "none"}
    for k in out:
        m = re.search(r"ILi(\d)ELi(\d)ELi(n?\d)ELi(\d)E", k["name"])
        nice = f"video_hr<r{m.group(1)},{fmt[m.group(2)]}->{fmt[m.group(3)]},{('none', 'q0', 'x', 'q0,x')[int(m.group(4))]}>"
        lines.append(f"   {nice:34s} VGPRs {k['VGPRs']:3d}  scratch {k['ScratchSize']} B/lane  LDS {k['LDS']:5d} B/block  occupancy "
                     f"{k['Occupancy']} waves/SIMD")
    lines.append(f"   VGPRs {min(k['VGPRs'] for k in out)} .. {max(k['VGPRs'] for k in out)}, LDS {min(k['LDS'] for k in out)} .. "
                 f"{max(k['LDS'] for k in out)} B, occupancy {min(k['Occupancy'] for k in out)} waves/SIMD in every one, no scratch in any")
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


def candidates(dev, st, H, W, r, fmt):
    """{name: (callable, calls a window, bytes moved)} of one HR size and input format."""
    import torch
    import torch.nn.functional as F
    from sesrq import downscale, video, video_hr
    hr = video.Surface.alloc(fmt, 1, H, W, dev)
    hr.buf.copy_(torch.randint(0, 256, (hr.buf.numel(),), dtype=torch.uint8, device=dev))
    h, w = H // r, W // r
    lr = video.Surface.alloc(fmt, 1, h, w, dev)
    q0 = torch.empty((1, 1, h, w), dtype=torch.int8, device=dev)
    img = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev)
    q3 = torch.empty((1, 3, h, w), dtype=torch.int8, device=dev)
    planes = [hr.y] + ([hr.c0[..., 0::2], hr.c0[..., 1::2]] if fmt == "nv12" else [hr.c0, hr.c1])

    def torch_route():
        return [F.interpolate(p[:, None].float(), scale_factor=1 / r, mode="bicubic", antialias=True, align_corners=False)
                .round().clamp(0, 255).to(torch.uint8) for p in planes]
    px = H * W
    return {"video_hr: q0 + LR chroma": (lambda: video_hr.launch(dev, IN_SCALE, IN_ZERO, 0, hr, r, lr, q0, None, st, lr_luma=False), 100,
                                          px * 3 // 2 + h * w * 3 // 2),
            "video_hr: the whole LR surface": (lambda: video_hr.launch(dev, 1.0, 0, 0, hr, r, lr, None, None, st), 100, px * 3 // 2 + h * w * 3 // 2),
            "downscale<RGB> q0, RGB image of the HR size": (lambda: downscale.launch(dev, IN_SCALE, IN_ZERO, 0, img, "rgb", r, "rgb", None, q3, None, st),
                                                            100, px * 3 + h * w * 3),
            "torch: F.interpolate(bicubic, antialias) a plane, round, clamp, cast": (torch_route, 10, 0)}


def report(path, reps, res_file):
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    lines = ["HR-only video route (libsesrq_video_hr.so, sesrq.video_hr), one MI355X.  Every number below is MEASURED by",
             "tools/video_hr_probe.py --report.", "",
             f"1. One process, HIP events around back-to-back launches (100 a window; 10 calls of the torch route), {reps} repetitions, the",
             "   candidates of a size alternating inside a repetition; median (min .. max) us per call.", ""]
    for s, (H, W, r) in SIZES.items():
        for fmt in ("nv12", "i420"):
            cands = candidates(dev, st, H, W, r, fmt)
            for fn, _, _ in cands.values():
                for _ in range(5):
                    fn()
            got = {k: [] for k in cands}
            for _ in range(reps):
                for k, (fn, calls, _) in cands.items():
                    got[k].append(window(fn, calls))
            lines.append(f"   {s}, {fmt} in ({H * W / 1e6:.2f} M HR pixels)")
            med = {k: statistics.median(v) for k, v in got.items()}
            for k, us in got.items():
                mb = cands[k][2] / 1e6
                lines.append(f"      {k:70s} {med[k]:9.2f} ({min(us):.2f} .. {max(us):.2f})" + (f"   {mb:5.1f} MB, {mb / med[k]:.2f} TB/s" if mb else ""))
            a, b, d, t = med.values()
            lines.append(f"      per HR pixel: q0 + chroma takes {a / d:.2f}x, the whole surface {b / d:.2f}x the time of the downscale kernel; the torch "
                         f"route takes {t / a:.1f}x / {t / b:.1f}x the time of the fused kernel")
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
