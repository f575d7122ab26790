#!/usr/bin/env python3
"""Denoise baseline measurements (sesrq.denoise, libsesrq_denoise.so) on one GPU; profiles/denoise_probe.txt is its --report.

  python tools/denoise_probe.py --build           # no GPU: the side builds under lib/probe/ (direct 25 terms; inner loop rolled)
  python tools/denoise_probe.py --resources       # no GPU: registers, scratch, LDS and occupancy of every build
  python tools/denoise_probe.py --report OUT [--resources-file FILE]

One process, HIP events around back-to-back launches after a warm-up, the candidates of a size alternating inside a repetition, median
of the repetitions: an RGGB spread frame of 960 x 540, 1920 x 1080 and 3840 x 2160 with the model's noise --
  the shipped kernel (denoise.run_spread), and the same frame as packed uint16 (denoise.run);
  the side builds of the same source, whose words must equal the shipped kernel's;
  demosaic.run_spread of the same frame: the HBM-traffic floor (it reads and writes the same bytes);
  a torch unfold route of the same filter at 540p (its words differ by rounding: the sums are in another order).
"""
import argparse
import ctypes as C
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sesr-pytorch-quantize_amd")
sys.path.insert(0, PKG)
CSRC, PROBE = os.path.join(PKG, "csrc"), os.path.join(PKG, "lib", "probe")
BUILDS = {"shipped": [], "direct 25 terms": ["-DSESRQ_DENOISE_DIRECT"], "inner loop rolled": ["-DSESRQ_DENOISE_UNROLL_I=1"]}
SIZES = {"540p": (540, 960), "1080p": (1080, 1920), "2160p": (2160, 3840)}
LEVELS = (0.01, 5e-4)
LANE_INSTR = 49 / 7 * 1521 / 8          # vector instructions per pixel: the unrolled loop body's count (read off the ISA), 8 pixels a lane
ISSUE = 256 * 64 * 2.4e9                # lane-instructions a second the MI355X's vector units issue at their peak clock


def oracle_rounding():
    """Largest |float32 - float64| of tests/denoise_oracle.py on the synthetic frame of tests/test_denoise.py (no GPU)."""
    import numpy as np
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import denoise_oracle as NO
    y, x = np.mgrid[0:96, 0:128]
    gain = np.array([0.8, 1.0, 0.6])[(y & 1) + (x & 1)]
    clean = ((0.5 + 0.3 * np.sin(2 * np.pi * x / 64) * np.cos(2 * np.pi * y / 48)) * (0.6 + 0.4 * ((y // 16 + x // 24) & 1)) * gain)[None]
    noisy = np.clip(clean + np.sqrt(clean * LEVELS[0] + LEVELS[1]) * np.random.default_rng(0).standard_normal(clean.shape), 0, 1)
    noisy = noisy.astype(np.float32)
    return float(np.abs(NO.nlm(noisy, LEVELS) - NO.nlm(noisy, LEVELS, dtype=np.float64)).max())


def flags():
    return subprocess.run(["make", "-s", "-C", CSRC, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.split()


def side_path(name):
    return os.path.join(PROBE, "libsesrq_denoise_" + re.sub(r"\W+", "_", name) + ".so")


def build():
    os.makedirs(PROBE, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for name, extra in BUILDS.items():
        if extra:
            subprocess.run([hipcc, *flags(), *extra, "-shared", os.path.join(CSRC, "sesrq_denoise.hip"), "-o", side_path(name)], check=True)
            print("built", side_path(name))


def resources():
    """Registers, scratch, LDS and occupancy of one instantiation (spread, scalars, wide; the others differ in staging only) per build."""
    hipcc, lines = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), []
    for name, extra in BUILDS.items():
        with tempfile.TemporaryDirectory() as tmp:
            p = subprocess.run([hipcc, *flags(), *extra, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "sesrq_denoise.hip"),
                                "-o", os.path.join(tmp, "d.o")], capture_output=True, text=True, check=True)
        got, on = {}, False
        for ln in p.stderr.splitlines():
            m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
            if m and m.group(1) == "Function Name":
                on = "ILi3ELb0ELb1E" in m.group(2)
            elif m and on:
                got[m.group(1).split(" ")[0]] = int(m.group(2))
        lines.append(f"   {name:24s} VGPRs {got['VGPRs']:3d}  scratch {got['ScratchSize']} B/lane  LDS {got['LDS']} B/block  occupancy "
                     f"{got['Occupancy']} waves/SIMD")
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


def unfold_route(m, shot, read, h=1.0):
    """The same filter with torch.nn.functional.unfold on the (1, 1, H, W) mosaic: 49 candidate planes of 25-term patch distances."""
    import torch
    import torch.nn.functional as F
    c = m.clamp(0, 1)
    g = 1 / (2 * (c * shot + read)).clamp_min(2.0 ** -100)
    H, W = c.shape[2:]
    cp, gp = F.pad(c, (8, 8, 8, 8), mode="reflect"), F.pad(g, (2, 2, 2, 2), mode="reflect")
    cen, gw = F.unfold(cp[:, :, 6:-6, 6:-6], 5), F.unfold(gp, 5)          # (1, 25, H W)
    num, den = torch.zeros_like(c), torch.zeros_like(c)
    for j in range(-3, 4):
        for i in range(-3, 4):
            q = cp[:, :, 6 + 2 * j:6 + 2 * j + H + 4, 6 + 2 * i:6 + 2 * i + W + 4]
            Dp = (((cen - F.unfold(q, 5)) ** 2) * gw).sum(1).view(1, 1, H, W)
            w = (1 - (Dp * 0.04 - 1).clamp_min(0) / h).clamp_min(0) ** 2
            num, den = num + w * q[:, :, 2:-2, 2:-2], den + w
    return num / den


def report(path, reps, res_file):
    import numpy as np
    import torch
    from sesrq import demosaic, denoise, sensor
    dev = torch.device("cuda:0")
    sides = {n: C.CDLL(side_path(n)) for n, x in BUILDS.items() if x}
    for l in sides.values():
        l.sesrq_denoise_spread.argtypes = denoise.SYMBOLS["sesrq_denoise_spread"][1]
    lines = ["Denoise baseline (libsesrq_denoise.so, sesrq.denoise), one MI355X.  Every number below is MEASURED by",
             "tools/denoise_probe.py --report.", "",
             f"1. One process, HIP events around back-to-back launches (20 a window; 2 of the torch route), {reps} repetitions after 3 warm-up",
             "   calls, the candidates of a size alternating inside a repetition; median (min .. max) us per call.  The python wrapper's host",
             "   time is inside every number.  The side builds are checked word for word against the shipped kernel first.", ""]
    for size, (H, W) in SIZES.items():
        y, x = np.mgrid[0:H, 0:W]
        clean = 0.5 + 0.3 * np.sin(2 * np.pi * x / 64) * np.cos(2 * np.pi * y / 48)
        s = np.clip(clean + np.sqrt(clean * LEVELS[0] + LEVELS[1]) * np.random.default_rng(H).standard_normal(clean.shape), 0, 1)
        sp = np.zeros((1, 3, H, W), np.float32)
        for c, (py, px) in ((0, (0, 0)), (1, (0, 1)), (1, (1, 0)), (2, (1, 1))):
            sp[0, c, py::2, px::2] = s[py::2, px::2]
        spread = torch.from_numpy(sp).to(dev)
        raw = torch.from_numpy(np.rint(s * 4095).astype(np.uint16)[None]).to(dev)
        outs = [torch.empty_like(spread) for _ in range(4)]
        p, st = denoise.Params(*LEVELS), torch.cuda.current_stream(dev).cuda_stream
        cands = {"denoise.run_spread (shipped)": (lambda: denoise.run_spread(spread, "rggb", p, out=outs[0]), 20),
                 "denoise.run, uint16 (shipped)": (lambda: denoise.run(raw, sensor.Format(), p, out=outs[1]), 20)}
        for n, l in sides.items():
            cands[f"side build: {n}"] = (lambda l=l: l.sesrq_denoise_spread(0, spread.data_ptr(), *LEVELS, None, 1.0, outs[2].data_ptr(), 1, H, W, st), 20)
        cands["demosaic.run_spread, malvar (the traffic floor)"] = (lambda: demosaic.run_spread(spread, "rggb", "malvar", out=outs[3]), 20)
        if size == "540p":
            m = spread.sum(1, keepdim=True)
            cands["torch: pad, unfold x 50, sums, weights"] = (lambda: unfold_route(m, *LEVELS), 2)
        denoise.run_spread(spread, "rggb", p, out=outs[0])
        for n, l in sides.items():
            assert cands[f"side build: {n}"][0]() == 0
            torch.cuda.synchronize()
            assert torch.equal(outs[2].view(torch.int32), outs[0].view(torch.int32)), n
        note = ""
        if size == "540p":
            note = f"; largest |shipped - torch route|: {float((outs[0].sum(1, keepdim=True) - unfold_route(m, *LEVELS)).abs().max()):.2e}"
        for fn, _ in cands.values():
            for _ in range(3):
                fn()
        got = {k: [] for k in cands}
        for _ in range(reps):
            for k, (fn, calls) in cands.items():
                got[k].append(window(fn, calls))
        lines.append(f"   {size} ({W} x {H}) rggb, levels {LEVELS}, h = 1{note}")
        med = {k: statistics.median(v) for k, v in got.items()}
        rate = H * W / med["denoise.run_spread (shipped)"] / 1e3          # Gpx/s; the last size's is quoted in section 4
        for k, us in got.items():
            lines.append(f"      {k:52s} {med[k]:10.1f} ({min(us):.1f} .. {max(us):.1f})   {H * W / med[k] / 1e3:7.2f} Gpx/s   "
                         f"{med[k] / med['denoise.run_spread (shipped)']:.2f}x the shipped kernel")
    lines += ["", "2. Registers, scratch, LDS (instantiation <spread, scalars, wide> of each build):"]
    lines += open(res_file).read().splitlines() if res_file else resources()
    lines += ["", "3. The numpy restatement (tests/denoise_oracle.py) in float32 against the same formulas in float64, on the 96 x 128 synthetic",
              f"   frame of tests/test_denoise.py at levels {LEVELS}, seed 0: largest difference {oracle_rounding():.3e} (the test's bound is 4 x).",
              "", "4. Alternatives.  Measured above: the direct 25-term evaluation (no sharing of e and r between a lane's pixels) and the rolled",
              "   inner loop.  Weighed on paper and not built: a 4 x 4 block (4 e per pixel and candidate instead of 6, but 2 x 64 footprint VGPRs",
              "   and 16 accumulator pairs: past 256 VGPRs, one wave per SIMD); a row-major LDS plane (candidate shifts of 2 mod 4 columns",
              "   then need 8-byte reads or three 16-byte reads a row for two rows' worth of data, and vertical pairs cost moves).",
              "   What bounds the kernel is an inference, not a counter reading.  The unrolled loop body (7 candidates) holds 1521 vector",
              "   instructions (588 v_pk_add_f32, 448 v_pk_mul_f32) and 30 ds_read_b128 -- neighbouring shifts share their words -- so a pixel",
              f"   costs 49 / 7 x 1521 / 8 = {LANE_INSTR:.0f} lane-instructions.  256 CUs x 64 lanes x 2.4 GHz issue {ISSUE / 1e12:.1f}e12 of them a second:",
              f"   {ISSUE / LANE_INSTR / 1e9:.1f} Gpx/s.  The shipped kernel reaches {rate:.1f} Gpx/s at 2160p, {100 * rate * 1e9 * LANE_INSTR / ISSUE:.0f} % of that, while its LDS reads are",
              "   about a sixth of what a CU's LDS delivers at 128 B a clock in the same time: vector issue is taken to bound it."]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-file", help="the output of an earlier --resources run to include instead of compiling again")
    ap.add_argument("--report", metavar="OUT")
    args = ap.parse_args()
    if args.build:
        build()
    elif args.resources:
        print("\n".join(resources()))
    elif args.report:
        report(args.report, args.reps, args.resources_file)
    else:
        ap.error("one of --build, --resources, --report")


if __name__ == "__main__":
    main()
