#!/usr/bin/env python3
"""Raw-route measurements (sesrq.raw, Engine.forward_raw) on one GPU.

  python tools/raw_probe.py                 # everything below, one line per number
  python tools/raw_probe.py --unpack-only   # only the unpack launches (for a `rocprofv3 --kernel-trace --stats -- ...` run of its own)

1. unpack kernel time at 540p and 1080p (q0 alone, q0 + fp32 frame): HIP events around `--iters` back-to-back launches, with the bytes
   a frame moves and the resulting share of 8 TB/s;
2. device-resident frames/s of nrdm_3 at 540p: forward_raw (uint16 frame) vs forward on the int8 q0 vs forward on the fp32 frame;
3. host-fed frames/s: a pinned uint16 frame uploaded + forward_raw vs a pinned fp32 frame uploaded + forward.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sesr-pytorch-quantize_amd"))

import sesrq  # noqa: E402
from sesrq import raw as R  # noqa: E402
from sesrq.bundle import Bundle  # noqa: E402

SIZES = {"540p": (540, 960), "1080p": (1080, 1920)}
PEAK = 8.0e12


def timed(fn, iters, warm=20):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--unpack-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b = Bundle.load(os.path.join(ROOT, "tests", "golden", "raw", "nrdm_3.npz"))
    e = sesrq.Engine(b, dev)
    st = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(0)
    print(f"device: {torch.cuda.get_device_name(dev)}; measured, HIP events, {args.iters} calls per number")
    for name, (H, W) in SIZES.items():
        x = torch.from_numpy(rng.integers(0, 4096, (1, H, W)).astype(np.uint16)).to(dev)
        q0 = torch.empty((1, 3, H, W), dtype=torch.int8, device=dev)
        sp = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
        for what, q, f, bpp in (("q0", q0, None, 5), ("q0+spread", q0, sp, 17)):
            us = timed(lambda: R.launch(dev, b.scale[0], b.zero[0], 0, x, q, f, st), args.iters)
            nbytes = bpp * H * W
            print(f"unpack {name} {what}: {us:.2f} us/launch (host-issued back to back), {nbytes / 1e6:.2f} MB/frame, "
                  f"{nbytes / (us * 1e-6) / 1e12:.2f} TB/s = {100 * nbytes / (us * 1e-6) / PEAK:.1f} % of 8 TB/s")
    if args.unpack_only:
        return
    H, W = SIZES["540p"]
    x = torch.from_numpy(rng.integers(0, 4096, (1, H, W)).astype(np.uint16)).to(dev)
    q0, sp = R.unpack(e, x, want_q=True, want_spread=True)
    oq = torch.empty(e.out_shape(1, H, W), dtype=torch.int8, device=dev)
    ws = e.workspace(1, H, W)
    del ws
    routes = {
        "forward_raw(uint16)": lambda: e.forward_raw(x, want_f=False, out_q=oq),
        "forward(int8 q0)": lambda: e.forward(q0, want_f=False, out_q=oq),
        "forward(fp32 spread)": lambda: e.forward(sp, want_f=False, out_q=oq),
    }
    for k, fn in routes.items():
        us = timed(fn, args.iters)
        print(f"device-resident nrdm_3 540p {k}: {us:.1f} us/frame = {1e6 / us:.0f} frames/s")
    raw_h = torch.from_numpy(rng.integers(0, 4096, (1, H, W)).astype(np.uint16)).pin_memory()
    sp_h = sp.cpu().pin_memory()
    xd = torch.empty_like(x)
    spd = torch.empty_like(sp)
    fed = {
        "pinned uint16 upload + forward_raw": lambda: (xd.copy_(raw_h, non_blocking=True), e.forward_raw(xd, want_f=False, out_q=oq)),
        "pinned fp32 upload + forward": lambda: (spd.copy_(sp_h, non_blocking=True), e.forward(spd, want_f=False, out_q=oq)),
    }
    for k, fn in fed.items():
        us = timed(fn, args.iters)
        print(f"host-fed nrdm_3 540p {k}: {us:.1f} us/frame = {1e6 / us:.0f} frames/s")


if __name__ == "__main__":
    main()
