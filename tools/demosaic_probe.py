#!/usr/bin/env python3
"""Demosaic baseline measurements (sesrq.demosaic, libsesrq_demosaic.so) on one GPU; profiles/demosaic_probe.txt is its --report.

  python tools/demosaic_probe.py --report OUT [--resources-file FILE]
  python tools/demosaic_probe.py --resources      # no GPU: compile the library's source for gfx950 with
                                                  # -Rpass-analysis=kernel-resource-usage and print registers, scratch and LDS

1. one process, HIP events around back-to-back launches after a warm-up, the candidates of one case alternating inside a repetition,
   median of the repetitions: RGGB frames of 960 x 540, 1920 x 1080 and 3840 x 2160 in uint16 and in RAW12, both methods, from the
   packed frame and from its fp32 spread frame --
     the fused kernel (what demosaic.run / run_spread launch), its words checked against the torch route's to 1e-6;
     sensor.unpack of the same frame to the spread frame alone: the floor, it reads the same bytes and writes the same 12 B/px;
     the torch route it replaces: unpack, the mosaic plane, one F.conv2d with the method's four 5 x 5 filters on a reflect-padded
     frame, torch.where by CFA phase, clamp;
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

SIZES = {"540p": (540, 960), "1080p": (1080, 1920), "2160p": (2160, 3840)}      # 2160p: where no candidate is bound by its enqueue rate
PACKINGS = ("u16", "raw12")
IN_BYTES = {"u16": 2.0, "raw12": 1.5, "spread": 8.0}      # per pixel; spread: the two planes that have sites in a row
HBM = 8.0                                                  # TB/s, the MI355X's peak


def resources():
    """Registers, scratch and LDS of every kernel of sesrq_demosaic.hip as the library's Makefile compiles it (no GPU needed)."""
    csrc = os.path.join(ROOT, "sesr-pytorch-quantize_amd", "csrc")
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "sesrq_demosaic.hip"), "-o",
                            os.path.join(tmp, "demosaic.o")], capture_output=True, text=True, check=True)
    out, cur = [], {}
    for ln in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if m and m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            out.append(cur)
        elif m:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    assert len(out) == 16 and all(k["ScratchSize"] == 0 for k in out), "an instantiation is missing or uses scratch"
    lines = ["compiled for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage, 16 instantiations "
             "demosaic<method, input, green diagonal>:"]
    for k in out:
        m = re.search(r"ILi(\d)ELb(\d)ELi(\d)E", k["name"])
        nice = (f"demosaic<{('bilinear', 'malvar')[int(m.group(3))]},{('u16', 'raw10', 'raw12', 'spread')[int(m.group(1))]},"
                f"{('rggb|bggr', 'grbg|gbrg')[int(m.group(2))]}>")
        lines.append(f"   {nice:38s} VGPRs {k['VGPRs']:3d}  scratch {k['ScratchSize']} B/lane  LDS {k['LDS']:5d} B/block  occupancy "
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


def filters(method, dev):
    """(4, 1, 5, 5) fp32 / 16: G at a chroma site, chroma at a G site in its row, in its column, the other chroma at a chroma site."""
    import torch
    k = torch.zeros(4, 5, 5)
    plus, diag = ((1, 2), (3, 2), (2, 1), (2, 3)), ((1, 1), (1, 3), (3, 1), (3, 3))
    far_v, far_h = ((0, 2), (4, 2)), ((2, 0), (2, 4))
    def put(i, cells, v):
        for c in cells:
            k[i][c] = v
    if method == "malvar":
        put(0, ((2, 2),), 8), put(0, plus, 4), put(0, far_v + far_h, -2)
        put(1, ((2, 2),), 10), put(1, ((2, 1), (2, 3)), 8), put(1, diag, -2), put(1, far_h, -2), put(1, far_v, 1)
        put(2, ((2, 2),), 10), put(2, ((1, 2), (3, 2)), 8), put(2, diag, -2), put(2, far_v, -2), put(2, far_h, 1)
        put(3, ((2, 2),), 12), put(3, diag, 4), put(3, far_v + far_h, -3)
    else:
        put(0, plus, 4), put(1, ((2, 1), (2, 3)), 8), put(2, ((1, 2), (3, 2)), 8), put(3, diag, 4)
    return (k / 16).unsqueeze(1).to(dev)


def candidates(dev, H, W, packing, method):
    """({name: (callable, calls a window, bytes moved)}, the largest difference between the fused kernel and the torch route)."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from sesrq import demosaic, sensor
    fmt = sensor.Format(packing=packing)
    codes = np.random.default_rng(H).integers(0, 4096, (1, H, W)).astype(np.uint16)
    raw = torch.from_numpy(codes if packing == "u16" else sensor.pack(codes, fmt)).to(dev)
    _, spread = sensor.unpack(None, raw, fmt, want_q=False, want_spread=True)
    out, out2 = (torch.empty((1, 3, H, W), dtype=torch.float32, device=dev) for _ in range(2))
    k = filters(method, dev)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev) & 1, torch.arange(W, device=dev) & 1, indexing="ij")
    red, blue, g_r = (yy == 0) & (xx == 0), (yy == 1) & (xx == 1), (yy == 0) & (xx == 1)     # RGGB; g_r: a G site in a red row

    def torch_route():
        _, sp = sensor.unpack(None, raw, fmt, want_q=False, want_spread=True)
        m = sp.sum(1, keepdim=True)
        c = F.conv2d(F.pad(m, (2, 2, 2, 2), mode="reflect"), k)[0]
        r = torch.where(red, m[0, 0], torch.where(blue, c[3], torch.where(g_r, c[1], c[2])))
        b = torch.where(blue, m[0, 0], torch.where(red, c[3], torch.where(g_r, c[2], c[1])))
        g = torch.where(red | blue, c[0], m[0, 0])
        return torch.stack([r, g, b]).clamp(0, 1)[None]
    demosaic.run(raw, fmt, method, out=out)
    torch.cuda.synchronize()
    diff = float((out - torch_route()).abs().max())
    px = H * W
    return {f"demosaic.run, {packing}": (lambda: demosaic.run(raw, fmt, method, out=out), 100, px * (IN_BYTES[packing] + 12)),
            "demosaic.run_spread": (lambda: demosaic.run_spread(spread, "rggb", method, out=out2), 100, px * (IN_BYTES["spread"] + 12)),
            f"sensor.unpack to spread, {packing} (the floor)": (lambda: sensor.unpack(None, raw, fmt, want_q=False, want_spread=True), 100,
                                                               px * (IN_BYTES[packing] + 12)),
            "torch: unpack, sum, pad, conv2d, where, clamp": (torch_route, 10, 0)}, diff


def report(path, reps, res_file):
    import torch
    dev = torch.device("cuda:0")
    lines = ["Demosaic baseline (libsesrq_demosaic.so, sesrq.demosaic), one MI355X.  Every number below is MEASURED by",
             "tools/demosaic_probe.py --report.", "",
             f"1. One process, HIP events around back-to-back launches (100 a window; 10 calls of the torch route), {reps} repetitions after",
             "   5 warm-up calls, the candidates of a case alternating inside a repetition; median (min .. max) us per call.  MB: the input",
             "   read once (a spread frame: the two planes with sites in each row) and the 12 B/px written once; its rate over",
             f"   {HBM:.0f} TB/s is the share of HBM peak the call reaches.  The python wrapper's host time is inside every number.", ""]
    for size, (H, W) in SIZES.items():
        for packing in PACKINGS:
            for method in ("malvar", "bilinear"):
                cands, diff = candidates(dev, H, W, packing, method)
                for fn, _, _ in cands.values():
                    for _ in range(5):
                        fn()
                got = {k: [] for k in cands}
                for _ in range(reps):
                    for k, (fn, calls, _) in cands.items():
                        got[k].append(window(fn, calls))
                lines.append(f"   {size} ({W} x {H}) rggb {packing}, {method}; largest |fused - torch route|: {diff:.2e}")
                med = {k: statistics.median(v) for k, v in got.items()}
                for k, us in got.items():
                    mb = cands[k][2] / 1e6
                    lines.append(f"      {k:52s} {med[k]:9.2f} ({min(us):.2f} .. {max(us):.2f})" +
                                 (f"   {mb:5.1f} MB, {mb / med[k]:.2f} TB/s, {100 * mb / med[k] / HBM:.0f} % of peak" if mb else ""))
                a, s, f, t = med.values()
                lines.append(f"      the fused kernel takes {a / f:.2f}x the floor's time (from the spread frame {s / f:.2f}x); the torch route takes "
                             f"{t / a:.1f}x the fused kernel's")
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
