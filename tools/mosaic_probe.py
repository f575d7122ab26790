"""Times the MFLAG 1 (nr) mosaic metric on a 1080x1920 fp32 pair (GPU only; no fallback).

    python tools/mosaic_probe.py [--runs 30] [--calls 20]

Three routes on the same frames, in the same process, alternating: A  quality.score(pred, gt, 1) (libsesrq_mosaic.so); B  the only
route without the mosaic form -- two torch gathers into mono frames and quality.score(mono, mono_gt, 5), whose kernel clips;
C  quality.score(pred, gt, 3), the RGB form, for context.  Device events around `calls` back-to-back calls, after a warm-up of every
route; the median, minimum and maximum over `runs` windows, per call.  The algorithmic bytes of A are the two planes a row selects
from, of pred and gt: 2/3 of the pair.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sesr-pytorch-quantize_amd"), os.path.join(ROOT, "tests", "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 8.0e12          # B/s, MI355X peak


def window_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mosaic_probe: needs a HIP device")
    from sesrq import quality
    from natural import natural_frame
    dev = torch.device("cuda:0")
    H, W = 1080, 1920
    rng = np.random.default_rng(1)
    gt = torch.from_numpy(natural_frame(3, H, W, 11)).to(dev)
    pred = (gt + torch.from_numpy(rng.normal(0, 0.02, gt.shape).astype(np.float32)).to(dev)).contiguous()
    yy, xx = np.meshgrid(np.arange(H) & 1, np.arange(W) & 1, indexing="ij")
    idx = torch.from_numpy((yy + xx)[None, None]).to(dev)

    def gathered():
        return quality.score(torch.gather(pred, 1, idx), torch.gather(gt, 1, idx), 5)
    routes = {"A mosaic form, score(pred, gt, 1)": lambda: quality.score(pred, gt, 1),
              "B two gathers + score(mono, mono_gt, 5)": gathered,
              "C RGB form, score(pred, gt, 3)": lambda: quality.score(pred, gt, 3)}
    a, b = routes["A mosaic form, score(pred, gt, 1)"](), gathered()
    torch.cuda.synchronize()
    assert torch.equal(a[:, 2], b[:, 2]) and torch.equal(65025.0 * a[:, 0], b[:, 0]), "routes A and B disagree"
    for fn in routes.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(args.runs):
        for k, fn in routes.items():
            times[k].append(window_us(fn, args.calls))
    print(f"device: {torch.cuda.get_device_name(0)}; 1x3x{H}x{W} fp32 pair; {args.runs} windows of {args.calls} calls per route, alternating")
    for k, t in times.items():
        print(f"{k:42s} median {np.median(t):8.1f} us/call   min {min(t):8.1f}   max {max(t):8.1f}")
    nbytes = 2 * 2 * H * W * 4
    ta = float(np.median(times["A mosaic form, score(pred, gt, 1)"]))
    print(f"A: algorithmic bytes {nbytes / 1e6:.1f} MB (two of three planes of pred and gt)  floor at 8 TB/s {nbytes / HBM * 1e6:.1f} us  "
          f"share of 8 TB/s {nbytes / HBM * 1e6 / ta:.0%}")
    print("scores (mse, psnr, ssim):", a.cpu().numpy().tolist())


if __name__ == "__main__":
    main()
