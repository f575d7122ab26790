#!/usr/bin/env python3
"""PSNR / SSIM of the INT8 nr and nrdm_3 paths over the shot noise level (GPU only; no fallback).

    python tools/noise_sweep.py > profiles/noise_sweep.txt

Clean 12-bit RGGB raw frames are cut from natural frames (tests/golden/natural.py: an RGB frame in [0, 1], coded as round(4095 x), its
RGGB mosaic the raw frame, the RGB codes the 16-bit ground truth) and scored by quality.evaluate_raw with noise=NoiseModel(shot, read,
seed): the noise is added on the device while the frames are unpacked (libsesrq_noise.so).  read follows the reference's line at its
centre, ln read = 2.18 ln shot + 1.20 (random_noise_levels with g = 0).  nr (tests/golden/nr_dm/nr.crop.npz) is MFLAG 1, scored on the
Bayer mosaic of its output; nrdm_3 (tests/golden/nrdm_3.crop.npz) is MFLAG 3, scored on RGB.  Both nets come from the reference's
checkpoints as the fixtures hold them.  Neither reconstructs these frames (their outputs average about 0.1 where the frames average
0.48, on the CPU oracle as well: 7 - 10 dB without any noise), so the table shows how the scores move with the level, not what a
denoiser can reach.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sesr-pytorch-quantize_amd"), os.path.join(ROOT, "tests", "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHOTS = (1e-4, 1e-3, 3e-3, 0.012)
NETS = (("nr", os.path.join("tests", "golden", "nr_dm", "nr.crop.npz"), 1), ("nrdm_3", os.path.join("tests", "golden", "nrdm_3.crop.npz"), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--size", type=int, nargs=2, default=(540, 960), metavar=("H", "W"))
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_sweep: needs a HIP device")
    import sesrq
    from natural import natural_frame
    from sesrq import noise, quality
    from sesrq.bundle import Bundle
    dev = torch.device("cuda:0")
    H, W = args.size
    raws, gts = [], []
    for k in range(args.frames):
        rgb = np.rint(np.clip(natural_frame(3, H, W, 100 + k)[0], 0, 1) * 4095).astype(np.uint16)
        raw = np.empty((H, W), np.uint16)
        raw[0::2, 0::2], raw[0::2, 1::2], raw[1::2, 0::2], raw[1::2, 1::2] = rgb[0, 0::2, 0::2], rgb[1, 0::2, 1::2], rgb[1, 1::2, 0::2], rgb[2, 1::2, 1::2]
        raws.append(raw)
        gts.append(rgb)
    print(f"device: {torch.cuda.get_device_name(dev)}; {args.frames} natural frames of {H} x {W} (seeds 100 ...), noise seed {args.seed}; "
          "mean over the frames of quality.evaluate_raw's per-frame (psnr, ssim)")
    print(f"{'net':8s} {'mflag':>5s} {'shot':>8s} {'read':>10s} {'psnr dB':>9s} {'ssim':>8s}")
    for name, path, mflag in NETS:
        e = sesrq.Engine(Bundle.load(os.path.join(ROOT, path)), dev)
        rows = [("clean", None, quality.evaluate_raw(e, raws, gts, mflag))]
        for shot in SHOTS:
            read = float(noise.levels_from(np.log(shot), 0.0)[1])
            rows.append((f"{shot:g}", read, quality.evaluate_raw(e, raws, gts, mflag, noise=noise.NoiseModel(shot, read, seed=args.seed))))
        for shot, read, r in rows:
            print(f"{name:8s} {mflag:5d} {shot:>8s} {'-' if read is None else format(read, '.3e'):>10s} {r[:, 1].mean():9.3f} {r[:, 2].mean():8.5f}")


if __name__ == "__main__":
    main()
