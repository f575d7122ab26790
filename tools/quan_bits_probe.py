#!/usr/bin/env python3
"""Narrow-width (define.py QUAN_BIT = b < 8) measurements on one GPU.

  python tools/quan_bits_probe.py [--iters 300] [--repeats 3]

A net with b < 8 runs every layer on the dot4 kernels (sesrq_create_q) unless it is created with ENGINE_MFMA_Q, which gives its layers
their MFMA kinds on the width-aware kernel flavours.  For nrdm_3 and SESR-x4 at 540p and SESR-x2 at 1080p (int8 out, fp32 frame in,
device-resident) it prints frames/s -- median of --repeats runs and their min .. max -- of
  - the b = 4 and b = 6 nets (tests/golden/quan_bits/<case>.q<b>.crop.npz) on the dot4 kernels and on ENGINE_MFMA_Q,
  - the b = 8 net of the b = 4 weights on the dot4 engine (the cost of the width as such on those kernels),
  - the b = 8 net on the default engine (MFMA kernels + fused trio, every proven reduced form),
  - the b = 8 net on the MFMA engine with reduced_forms = 0: the generic epilogues, i.e. the instruction mix of the width-aware flavours
    -- the yardstick for "the narrow engine runs at the MFMA rate",
and the per-launch kernel times (sesrq_forward_timed) of the b = 4 forwards and of that yardstick.
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
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(dev)}; measured, HIP events around {args.iters} back-to-back forwards per run, "
          f"{args.repeats} runs per number (median, min .. max), fp32 frame in, int8 frame out, device-resident")
    for case, H, W in CASES:
        b4 = Bundle.load(os.path.join(ROOT, "tests", "golden", "quan_bits", f"{case}.q4.crop.npz"))
        b6 = Bundle.load(os.path.join(ROOT, "tests", "golden", "quan_bits", f"{case}.q6.crop.npz"))
        b8 = dataclasses.replace(b4, quan_bits=8)
        cin = b4.in_channels
        x = torch.rand((1, cin, H, W), generator=torch.Generator().manual_seed(1)).to(dev)
        engines = {"b=4 dot4": sesrq.Engine(b4, dev),
                   "b=4 mfma-q": sesrq.Engine(b4, dev, engine=_lib.ENGINE_MFMA_Q),
                   "b=6 dot4": sesrq.Engine(b6, dev),
                   "b=6 mfma-q": sesrq.Engine(b6, dev, engine=_lib.ENGINE_MFMA_Q),
                   "b=8 dot4": sesrq.Engine(b8, dev, engine=_lib.ENGINE_DOT4),
                   "b=8 default (MFMA)": sesrq.Engine(b8, dev),
                   "b=8 MFMA reduced_forms=0": sesrq.Engine(b8, dev, engine=_lib.ENGINE_MFMA, reduced_forms=0)}
        for name, e in engines.items():
            oq = torch.empty(e.out_shape(1, H, W), dtype=torch.int8, device=dev)
            us = sorted(timed(lambda: e.forward(x, want_f=False, out_q=oq), args.iters) for _ in range(args.repeats))
            med = us[len(us) // 2]
            print(f"{case} {H}p {name}: {med:.1f} us/frame = {1e6 / med:.0f} frames/s ({1e6 / us[-1]:.0f} .. {1e6 / us[0]:.0f})")
        for name in ("b=4 dot4", "b=4 mfma-q", "b=8 MFMA reduced_forms=0"):
            e = engines[name]
            ms, fwd = e.forward_timed(x, iters=50)
            names = e.layer_engines()
            print(f"{case} {H}p {name} kernels (us): " + ", ".join(f"{names[k]} {1e3 * t:.1f}" for (k, _), t in zip(e.launch_plan(), ms)) +
                  f"; forward {1e3 * fwd:.1f}")


if __name__ == "__main__":
    main()
