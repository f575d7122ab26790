"""Calibration rate, frames/s, of the host-driven pass (Calibrator.observe: one host round trip per quantiser) and the device-resident
pass (Calibrator.enqueue: one synchronisation at the end) on one net at one frame size.

    python tools/calib_rate.py --params tests/golden/nrdm_3.params.npz --ps 1 --H 540 --W 960 --frames 50 [--out FILE]
    python tools/calib_rate.py --params tests/golden/nrdm_3_qat.params.npz ... --skip-quant-scale 0.004919898   # + the QAT nets' merge

Frames are fp32 (1, Cin, H, W) already on the device (natural-ish, tests/golden/natural.py); each pass calibrates the same frames from
a reset, after one untimed warm-up pass; the wall time from the first call to the synchronisation after the last is the run."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sesr-pytorch-quantize_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--params", required=True)
    ap.add_argument("--ps", type=int, default=1)
    ap.add_argument("--H", type=int, default=540)
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-quant-scale", type=float, default=None,
                    help="also time both passes with the long skip merged through the QuantAdd at this scale (same box, same frames)")
    ap.add_argument("--out")
    a = ap.parse_args()
    from sesrq.calibrate import Calibrator
    from natural import natural_frame
    p = np.load(a.params, allow_pickle=False)
    dev = torch.device("cuda:0")
    cals = [("", Calibrator([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], a.ps, dev))]
    if a.skip_quant_scale is not None:
        cals.append((f", quantised merge s={a.skip_quant_scale!r}",
                     Calibrator([p[f"Wf{k}"] for k in range(5)], [p[f"bf{k}"] for k in range(5)], a.ps, dev,
                                skip_quant_scale=a.skip_quant_scale)))
    cin = cals[0][1].in_channels
    xs = [torch.from_numpy(natural_frame(cin, a.H, a.W, 7000 + i)).to(dev) for i in range(a.frames)]
    torch.cuda.synchronize()

    def run(cal, fn):
        cal.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for x in xs:
            fn(x)
        cal.finalize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    lines = [f"# {os.path.basename(a.params)}  {a.frames} frames (1, {cin}, {a.H}, {a.W}) fp32 on the device, "
             f"best of {a.repeats} runs after one warm-up; {torch.cuda.get_device_name(dev)}"]
    for tag, cal in cals:
        for name, fn in (("host pass (observe)", cal.observe), ("device pass (enqueue)", cal.enqueue)):
            run(cal, fn)
            best = min(run(cal, fn) for _ in range(a.repeats))
            lines.append(f"{name + tag:24s} {a.frames / best:9.1f} frames/s   ({best * 1e3 / a.frames:.3f} ms/frame)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
