#!/usr/bin/env python3
"""Noise route measurements (sesrq.noise, libsesrq_noise.so) on one GPU, against the routes it stands beside, in the same process.

  python tools/noise_probe.py > profiles/noise_probe.txt

T_z: the largest |z_dev - z_oracle| over the frames of tests/test_noise.py (SHAPES there), z_oracle the float64 restatement
(tests/noise_oracle.py) rounded to fp32.  tests/test_noise.py asserts four times this value rounded up to a power of two.

Timings: one box, one process, HIP events.  Every number is the median of `--reps` repetitions of `--calls` back-to-back calls after a
warm-up, printed with the repetitions' own min and max; the candidates alternate inside each repetition, so drift of the box shows in
every row alike.  At 540 x 960 and 1080 x 1920, 12-bit RGGB uint16 frames:
  (a) sesrq_sensor_unpack, q0 alone: the clean unpack, the stream this kernel shares;
  (b) sesrq_noise_unpack, q0 alone, and (c) q0 + spread;
  (d) sesrq_noise_deviates alone: the generator and the Box-Muller without the combine;
  (e) the route (b) replaces, up to the net's input: sensor unpack to fp32, torch.randn_like + the elementwise combine and clamp
      in torch (the forward then quantises the fp32 frame itself).
Then nrdm_3 at 540p, device-resident frames: forward_raw without noise, forward_raw(noise=...), and route (e) + forward from fp32; and
host-fed from pinned memory (upload + forward_raw), frames/s with and without noise.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sesr-pytorch-quantize_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import sesrq  # noqa: E402
from sesrq import noise as NZ, sensor as S  # noqa: E402
from sesrq.bundle import Bundle  # noqa: E402
from sensor_probe import line, measure  # noqa: E402

SIZES = {"540p": (540, 960), "1080p": (1080, 1920)}


def t_z(dev):
    import noise_oracle as NO
    import test_noise as T
    worst = 0.0
    for nhw, frame0 in [(s[1], 3) for s in T.SHAPES] + [((3, 5, 37), T.FRAME_HI)]:
        z = NZ.deviates(nhw, T.SEED, frame0, dev).cpu().numpy()
        want = NO.deviates(T.SEED, frame0, *nhw).astype(np.float32)
        err = float(np.abs(z.astype(np.float64) - want).max())
        i = np.unravel_index(np.abs(z.astype(np.float64) - want).argmax(), z.shape)
        print(f"T_z frame {nhw} frame0 {frame0}: max |z_dev - z_oracle| = {err:.3e} at z = {float(want[i]):+.4f}; max |z| = {np.abs(z).max():.3f}, "
              f"{int((z != want).sum())} of {z.size} samples differ from the rounded oracle")
        worst = max(worst, err)
    p = int(np.ceil(np.log2(4 * worst)))
    print(f"T_z = {worst:.3e}; 4 T_z rounded up to a power of two = 2^{p} = {2.0 ** p:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b = Bundle.load(os.path.join(ROOT, "tests", "golden", "raw", "nrdm_3.npz"))
    e = sesrq.Engine(b, dev)
    st = torch.cuda.current_stream(dev)
    s0, z0 = b.scale[0], b.zero[0]
    rng = np.random.default_rng(0)
    print(f"device: {torch.cuda.get_device_name(dev)}; measured, HIP events, one process; {args.reps} repetitions of {args.calls} calls per "
          f"number, candidates alternating inside a repetition")
    t_z(dev)
    fmt = S.Format()
    m = NZ.NoiseModel(0.003, 1e-5, seed=3)
    shot, read = 0.003, 1e-5

    def torch_route(x, sp, W):
        S.launch(dev, fmt, s0, z0, 0, x, W, 2 * W, None, sp, st)
        return (sp + torch.sqrt(sp * shot + read) * torch.randn_like(sp)).clamp_(0.0, 1.0)

    for name, (H, W) in SIZES.items():
        q0 = torch.empty((1, 3, H, W), dtype=torch.int8, device=dev)
        sp = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
        x = torch.from_numpy(rng.integers(0, 4096, (1, H, W)).astype(np.uint16)).to(dev)
        fns = {
            "(a) sensor unpack q0": lambda: S.launch(dev, fmt, s0, z0, 0, x, W, 2 * W, q0, None, st),
            "(b) noise unpack q0": lambda: NZ.launch(dev, fmt, s0, z0, 0, x, W, 2 * W, q0, None, st, m),
            "(c) noise unpack q0 + spread": lambda: NZ.launch(dev, fmt, s0, z0, 0, x, W, 2 * W, q0, sp, st, m),
            "(d) noise deviates alone": lambda: NZ.deviates((1, H, W), 3, 0, dev),
            "(e) sensor unpack fp32 + torch.randn_like + elementwise": lambda: torch_route(x, sp, W),
        }
        got = measure(fns, args.calls, args.reps, warm=20)
        for k, us in got.items():
            print(line(f"{name} {k}", us))
        px = H * W
        bm = statistics.median(got["(b) noise unpack q0"])
        print(f"{name} (b): {bm * 1e3 / px:.3f} ns per pixel, {5 * px / bm / 1e6:.3f} TB/s of its 5 B/px; "
              f"(b) / (a) = {bm / statistics.median(got['(a) sensor unpack q0']):.1f}, "
              f"(b) / (e) = {bm / statistics.median(got['(e) sensor unpack fp32 + torch.randn_like + elementwise']):.2f}")

    H, W = SIZES["540p"]
    codes = rng.integers(0, 4096, (1, H, W)).astype(np.uint16)
    oq = torch.empty(e.out_shape(1, H, W), dtype=torch.int8, device=dev)
    dq = torch.from_numpy(codes).to(dev)
    sp = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
    h = torch.from_numpy(codes).pin_memory()
    d = torch.empty(h.shape, dtype=h.dtype, device=dev)
    fed = {
        "device-resident nrdm_3 540p forward_raw": lambda: e.forward_raw(dq, want_f=False, out_q=oq),
        "device-resident nrdm_3 540p forward_raw(noise)": lambda: e.forward_raw(dq, want_f=False, out_q=oq, noise=m),
        "device-resident nrdm_3 540p unpack fp32 + torch noise + forward(fp32)": lambda: e.forward(torch_route(dq, sp, W), want_f=False, out_q=oq),
        "host-fed nrdm_3 540p upload + forward_raw": lambda: (d.copy_(h, non_blocking=True), e.forward_raw(d, want_f=False, out_q=oq)),
        "host-fed nrdm_3 540p upload + forward_raw(noise)": lambda: (d.copy_(h, non_blocking=True),
                                                                      e.forward_raw(d, want_f=False, out_q=oq, noise=m)),
    }
    for k, us in measure(fed, args.calls, args.reps, warm=20).items():
        print(line(k, us) + f" = {1e6 / statistics.median(us):.0f} /s")


if __name__ == "__main__":
    main()
