#!/usr/bin/env python3
"""Narrow-width (define.py QUAN_BIT = b < 8) measurements on one GPU.

  python tools/quan_bits_probe.py [--iters 300]

A net with b < 8 runs every layer on the dot4 kernels (sesrq_create_q).  For nrdm_3 and SESR-x4 at 540p and SESR-x2 at 1080p (int8 out,
fp32 frame in, device-resident) it prints frames/s of
  - the b = 4 net (tests/golden/quan_bits/<case>.q4.crop.npz),
  - the b = 8 net of the same weights on the dot4 engine (ENGINE_DOT4: the same kernels with the 8-bit clamps -- the cost of the width
    as such),
  - the b = 8 net on the default engine (MFMA kernels + fused trio: what the width costs against the production path),
and the per-launch kernel times of the b = 4 forward (sesrq_forward_timed).
"""
import argparse
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sesr-pytorch-quantize_amd"))

import sesrq  # noqa: E402
from sesrq import _lib  # noqa: E402
from sesrq.bundle import Bundle  # noqa: E402

CASES = [("nrdm_3", 540, 960), ("sesr_x4", 540, 960), ("sesr_x2_rand", 1080, 1920)]


def timed(fn, iters, warm=20):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters          # us per frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(dev)}; measured, HIP events around {args.iters} back-to-back forwards per number, "
          "fp32 frame in, int8 frame out, device-resident")
    for case, H, W in CASES:
        b4 = Bundle.load(os.path.join(ROOT, "tests", "golden", "quan_bits", f"{case}.q4.crop.npz"))
        cin = b4.in_channels
        x = torch.rand((1, cin, H, W), generator=torch.Generator().manual_seed(1)).to(dev)
        engines = {"b=4 (dot4)": sesrq.Engine(b4, dev),
                   "b=8 dot4": sesrq.Engine(dataclasses.replace(b4, quan_bits=8), dev, engine=_lib.ENGINE_DOT4),
                   "b=8 default (MFMA)": sesrq.Engine(dataclasses.replace(b4, quan_bits=8), dev)}
        for name, e in engines.items():
            oq = torch.empty(e.out_shape(1, H, W), dtype=torch.int8, device=dev)
            us = timed(lambda: e.forward(x, want_f=False, out_q=oq), args.iters)
            print(f"{case} {H}p {name}: {us:.1f} us/frame = {1e6 / us:.0f} frames/s")
        e = engines["b=4 (dot4)"]
        ms, fwd = e.forward_timed(x, iters=50)
        print(f"{case} {H}p b=4 kernels (us): " + ", ".join(f"{n} {1e3 * t:.1f}" for n, t in zip(e.layer_engines(), ms)) +
              f"; forward {1e3 * fwd:.1f}")


if __name__ == "__main__":
    main()
