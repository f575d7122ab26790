#!/usr/bin/env python3
"""Sensor-format raw route measurements (sesrq.sensor, libsesrq_sensor.so) on one GPU, against libsesrq_raw.so in the same process.

  python tools/sensor_probe.py > profiles/sensor_probe.txt
  python tools/sensor_probe.py --unpack-only   # (a)-(d) alone, for a `rocprofv3 --kernel-trace -d DIR -o sensor -- ...` run of its own
  python tools/sensor_probe.py --summarise DIR/sensor_results.db >> profiles/sensor_probe.txt    # kernel durations of that trace

One box, one process, HIP events.  Every number is the median of `--reps` repetitions of `--calls` back-to-back calls after a warm-up,
printed with the repetitions' own min and max.  At 540 x 960 and 1080 x 1920, q0 alone (what Engine.forward_raw asks for):
  (a) libsesrq_raw.so's kernel: the yardstick (12-bit RGGB, uint16);
  (b) libsesrq_sensor.so at the default format: the same bytes in and out; said to be "slower" / "faster" only when its median lies
      outside (a)'s own min - max;
  (c) uint16 frames at (64, 1023) -- the LDS table -- and at (4096, 65535) -- the deep-sensor step search;
  (d) RAW10 and RAW12 rows;
  (e) host-fed nrdm_3 540p frames/s from pinned host memory: upload + forward_raw for uint16 (libsesrq_raw.so), RAW10 and RAW12
      (tools/raw_probe.py's loop with the fmt= entry point), and the upload alone.
(a)-(d) alternate within each repetition, so drift of the box shows in every row alike.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sesr-pytorch-quantize_amd"))

import sesrq  # noqa: E402
from sesrq import raw as R, sensor as S  # noqa: E402
from sesrq.bundle import Bundle  # noqa: E402

SIZES = {"540p": (540, 960), "1080p": (1080, 1920)}


def window(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / calls          # us per call


def measure(fns, calls, reps, warm=50):
    """{name: [us per call of each repetition]}: the candidates alternate inside every repetition."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(window(fn, calls))
    return out


def line(name, us):
    return f"{name}: median {statistics.median(us):.2f} us/call (min {min(us):.2f}, max {max(us):.2f})"


def summarise(db):
    """Median, min and max duration per (kernel, grid) of a rocprofv3 kernel trace: the time on the device, without the host's issue."""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, grid_x, start, end from kernels order by start").fetchall()
    agg = {}
    for name, grid, start, end in rows:
        agg.setdefault((name.split("(")[0], grid), []).append((end - start) / 1e3)
    print("kernel trace (rocprofv3 --kernel-trace, a run of its own): duration on the device per launch, warm-up launches included;\n"
          "sensor_unpack<outputs (1: q0), map (0: table, 1: steps), packing (0: u16, 1: raw10, 2: raw12)>; 540p grids come first")
    for (name, grid), us in agg.items():
        if len(us) >= 100:
            print(f"{name} grid {grid}: {len(us)} launches, median {statistics.median(us):.2f} us (min {min(us):.2f}, max {max(us):.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--unpack-only", action="store_true")
    ap.add_argument("--summarise", metavar="DB", help="print the kernel durations of a rocprofv3 --kernel-trace result database")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    dev = torch.device("cuda:0")
    b = Bundle.load(os.path.join(ROOT, "tests", "golden", "raw", "nrdm_3.npz"))
    e = sesrq.Engine(b, dev)
    st = torch.cuda.current_stream(dev)
    s0, z0 = b.scale[0], b.zero[0]
    rng = np.random.default_rng(0)
    print(f"device: {torch.cuda.get_device_name(dev)}; measured, HIP events, one process; {args.reps} repetitions of {args.calls} calls per "
          f"number, candidates alternating inside a repetition")
    f10 = S.Format(black=64, white=1023, packing="raw10")
    f12 = S.Format(black=256, white=4095, packing="raw12")
    for name, (H, W) in SIZES.items():
        q0 = torch.empty((1, 3, H, W), dtype=torch.int8, device=dev)
        codes = rng.integers(0, 4096, (1, H, W)).astype(np.uint16)
        deep = rng.integers(0, 65536, (1, H, W)).astype(np.uint16)
        x, xd = torch.from_numpy(codes).to(dev), torch.from_numpy(deep).to(dev)
        x10 = torch.from_numpy(S.pack(codes & 1023, f10)).to(dev)
        x12 = torch.from_numpy(S.pack(codes, f12)).to(dev)

        def sensor(fmt, t):
            return lambda: S.launch(dev, fmt, s0, z0, 0, t, W, t.shape[2] * t.element_size(), q0, None, st)
        fns = {
            "(a) libsesrq_raw q0": lambda: R.launch(dev, s0, z0, 0, x, q0, None, st),
            "(b) sensor default format q0": sensor(S.Format(), x),
            "(c) sensor u16 (64, 1023) table q0": sensor(S.Format(black=64, white=1023), x),
            "(c) sensor u16 (4096, 65535) steps q0": sensor(S.Format(black=4096, white=65535), xd),
            "(d) sensor raw10 (64, 1023) q0": sensor(f10, x10),
            "(d) sensor raw12 (256, 4095) q0": sensor(f12, x12),
        }
        got = measure(fns, args.calls, args.reps)
        for k, us in got.items():
            print(line(f"unpack {name} {k}", us))
        a, bm = got["(a) libsesrq_raw q0"], statistics.median(got["(b) sensor default format q0"])
        verdict = "slower than" if bm > max(a) else "faster than" if bm < min(a) else "inside"
        print(f"unpack {name} (b) median {bm:.2f} us is {verdict} (a)'s own min - max {min(a):.2f} - {max(a):.2f} us")
    if args.unpack_only:
        return
    # (e) host-fed: pinned upload + forward_raw, nrdm_3 540p, q output only
    H, W = SIZES["540p"]
    codes = rng.integers(0, 4096, (1, H, W)).astype(np.uint16)
    oq = torch.empty(e.out_shape(1, H, W), dtype=torch.int8, device=dev)
    hosts = {"uint16 (libsesrq_raw)": (torch.from_numpy(codes).pin_memory(), None),
             "raw10": (torch.from_numpy(S.pack(codes & 1023, f10)).pin_memory(), f10),
             "raw12": (torch.from_numpy(S.pack(codes, f12)).pin_memory(), f12)}
    fed, up = {}, {}
    for k, (h, fmt) in hosts.items():
        d = torch.empty(h.shape, dtype=h.dtype, device=dev)
        nb = h.numel() * h.element_size()
        up[f"host-fed 540p {k} upload alone ({nb / 1e6:.2f} MB)"] = lambda d=d, h=h: d.copy_(h, non_blocking=True)
        fed[f"host-fed nrdm_3 540p {k} upload + forward_raw"] = \
            lambda d=d, h=h, fmt=fmt: (d.copy_(h, non_blocking=True), e.forward_raw(d, want_f=False, out_q=oq, fmt=fmt))
    dq = torch.from_numpy(codes).to(dev)
    fed["device-resident nrdm_3 540p uint16 forward_raw (no upload)"] = lambda: e.forward_raw(dq, want_f=False, out_q=oq)
    for group in (fed, up):
        for k, us in measure(group, args.calls, args.reps).items():
            print(line(k, us) + f" = {1e6 / statistics.median(us):.0f} /s")


if __name__ == "__main__":
    main()
