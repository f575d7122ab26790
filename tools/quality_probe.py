"""Times sesrq.quality on 4K frames (GPU only; no fallback).

    python tools/quality_probe.py [--iters 50]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/quality_probe.py      (kernel times: eval_tile / eval_finish)

1. score() of one 2160x3840 pair: fp32 RGB (MFLAG 3 form) and int8 single-channel (MFLAG 5 form, the x4 net's int8 output);
   device-event time per call, the algorithmic bytes (pred + gt read once) and their share of 8 TB/s.
2. evaluate() on the two 4K workloads: SESR x4 540p -> 2160x3840 (int8 output scored) and SESR x2 1080p -> 2160x3840
   (anchored fp32 output scored); forward + score per frame, one synchronisation per call.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sesr-pytorch-quantize_amd"), os.path.join(ROOT, "tests", "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 8.0e12          # B/s, MI355X peak


def events_us(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quality_probe: needs a HIP device")
    import sesrq
    from sesrq import quality
    from sesrq.bundle import Bundle
    from natural import natural_frame
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    H, W = 2160, 3840

    gt3 = torch.from_numpy(natural_frame(3, H, W, 11)).to(dev)
    p3 = (gt3 + torch.from_numpy(rng.normal(0, 0.02, gt3.shape).astype(np.float32)).to(dev)).contiguous()
    t = events_us(lambda: quality.score(p3, gt3, 3), args.iters)
    nbytes = 2 * p3.numel() * 4
    print(f"score fp32 RGB 1x3x{H}x{W}: {t:8.1f} us/call  bytes {nbytes / 1e6:.1f} MB  floor {nbytes / HBM * 1e6:.1f} us  "
          f"share of 8 TB/s {nbytes / HBM * 1e6 / t:.0%}")

    gt1 = torch.from_numpy(natural_frame(1, H, W, 12)).to(dev)
    q1 = torch.from_numpy(rng.integers(-128, 100, (1, 1, H, W), dtype=np.int8)).to(dev)
    t = events_us(lambda: quality.score(q1, gt1, 5, scale=1.0 / 220, zero=-110), args.iters)
    nbytes = q1.numel() * (1 + 4)
    print(f"score int8 Y 1x1x{H}x{W}:   {t:8.1f} us/call  bytes {nbytes / 1e6:.1f} MB  floor {nbytes / HBM * 1e6:.1f} us  "
          f"share of 8 TB/s {nbytes / HBM * 1e6 / t:.0%}")

    gold = os.path.join(ROOT, "tests", "golden")
    for name, mflag, shape, kw in (("x4 540p->4K", 5, (1, 1, 540, 960), {}),
                                   ("x2 1080p->4K", 6, (1, 3, 1080, 1920), {"anchor_add": True})):
        case = "sesr_x4_nat.crop" if mflag == 5 else "sesr_x2_rand.crop"
        e = sesrq.Engine(Bundle.load(os.path.join(gold, case + ".npz")), dev, **kw)
        frames = [torch.from_numpy(natural_frame(shape[1], shape[2], shape[3], 20 + k)).to(dev) for k in range(4)]
        gts = [torch.from_numpy(natural_frame(shape[1], H, W, 30 + k)).to(dev) for k in range(4)]
        quality.evaluate(e, frames, gts, mflag)
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        reps = max(1, args.iters // 4)
        t0.record()
        for _ in range(reps):
            res = quality.evaluate(e, frames, gts, mflag)
        t1.record()
        torch.cuda.synchronize()
        per = t0.elapsed_time(t1) * 1e3 / (reps * len(frames))
        print(f"evaluate {name}: {per:8.1f} us/frame (forward + score, host loop, one sync per {len(frames)} frames)  "
              f"psnr {res[:, 1].mean():.3f} ssim {res[:, 2].mean():.4f}")


if __name__ == "__main__":
    main()
