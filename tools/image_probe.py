#!/usr/bin/env python3
"""Image-route measurements (sesrq.image, Engine.forward_image) on one GPU.

  python tools/image_probe.py                  # everything below, one line per number
  python tools/image_probe.py --kernels-only   # only the decode / export launches (for a `rocprofv3 --kernel-trace --stats -- ...` run)

1. decode kernel time at 540p and 1080p (Y and RGB form, q0 alone and q0 + fp32 frame) and export kernel time for a 4K x2 output
   (fp32 anchored, int8): HIP events around `--iters` back-to-back launches, with the bytes a launch moves and its share of 8 TB/s;
2. host-fed frames/s of SESR-x2 at 1080p (int8 output): a pinned uint8 image uploaded + forward_image vs a pinned fp32 frame
   uploaded + forward vs the host's numpy conversion (the reference's u8 / 255. in float64) + fp32 upload + forward; and the host
   conversion alone for both forms;
3. device -> host: the exported uint8 4K frame vs the fp32 4K frame, pinned, bytes and time.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sesr-pytorch-quantize_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sesrq  # noqa: E402
from sesrq import image as I  # noqa: E402
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


def line(what, us, nbytes):
    print(f"{what}: {us:.2f} us/launch (host-issued back to back), {nbytes / 1e6:.2f} MB, "
          f"{nbytes / (us * 1e-6) / 1e12:.2f} TB/s = {100 * nbytes / (us * 1e-6) / PEAK:.1f} % of 8 TB/s")


def host_y(img):
    """The reference's MFLAG 5 conversion on the host (self_dataset_sr.py), float64."""
    g = img / 255.
    return np.clip((65.481 * g[:, :, 0] + 128.553 * g[:, :, 1] + 24.966 * g[:, :, 2] + 16.) / 255.0, 0, 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    img_dir = os.path.join(ROOT, "tests", "golden", "image")
    b2 = Bundle.load(os.path.join(img_dir, "sesr_x2_rand.npz"))
    b4 = Bundle.load(os.path.join(img_dir, "sesr_x4.npz"))
    st = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(0)
    print(f"device: {torch.cuda.get_device_name(dev)}; measured, HIP events, {args.iters} calls per number")
    for name, (H, W) in SIZES.items():
        x = torch.from_numpy(rng.integers(0, 256, (1, H, W, 3)).astype(np.uint8)).to(dev)
        for form, b in (("y", b4), ("rgb", b2)):
            C = I.CHANNELS[I.FORMS[form]]
            q0 = torch.empty((1, C, H, W), dtype=torch.int8, device=dev)
            xf = torch.empty((1, C, H, W), dtype=torch.float32, device=dev)
            for what, q, f, bpp in (("q0", q0, None, 3 + C), ("q0+x", q0, xf, 3 + 5 * C)):
                us = timed(lambda: I.launch(dev, b.scale[0], b.zero[0], 0, x, form, "rgb", q, f, st), args.iters)
                line(f"decode {form} {name} {what}", us, bpp * H * W)
    H4, W4 = 2160, 3840
    pf = torch.rand((1, 3, H4, W4), device=dev) * 1.2 - 0.1
    pq = torch.randint(-128, 128, (1, 3, H4, W4), dtype=torch.int8, device=dev)
    out = torch.empty((1, H4, W4, 3), dtype=torch.uint8, device=dev)
    L = b2.L
    s, z = float(np.float32(b2.scale[L])), int(b2.zero[L])
    lib = I.lib()
    ex_f = lambda: lib.sesrq_image_export(pf.data_ptr(), I.PRED_F32, 0.0, 0, 3, 0, out.data_ptr(), 1, H4, W4, st.cuda_stream)  # noqa: E731
    ex_q = lambda: lib.sesrq_image_export(pq.data_ptr(), I.PRED_I8, s, z, 3, 0, out.data_ptr(), 1, H4, W4, st.cuda_stream)  # noqa: E731
    line("export 4K x2 from fp32", timed(ex_f, args.iters), 15 * H4 * W4)
    line("export 4K x2 from int8", timed(ex_q, args.iters), 6 * H4 * W4)
    if args.kernels_only:
        return

    # 2. host-fed SESR-x2 1080p, int8 output
    H, W = SIZES["1080p"]
    e = sesrq.Engine(b2, dev)
    img_h = torch.from_numpy(rng.integers(0, 256, (1, H, W, 3)).astype(np.uint8)).pin_memory()
    x_h = torch.from_numpy((img_h.numpy()[0] / 255.).astype(np.float32).transpose(2, 0, 1).copy()[None]).pin_memory()
    img_d, x_d = torch.empty_like(img_h, device=dev), torch.empty_like(x_h, device=dev)
    oq = torch.empty(e.out_shape(1, H, W), dtype=torch.int8, device=dev)
    fed = {
        "pinned uint8 upload (6.22 MB) + forward_image": lambda: (img_d.copy_(img_h, non_blocking=True),
                                                                  e.forward_image(img_d, want_f=False, out_q=oq)),
        "pinned fp32 upload (24.9 MB) + forward": lambda: (x_d.copy_(x_h, non_blocking=True), e.forward(x_d, want_f=False, out_q=oq)),
    }
    for k, fn in fed.items():
        us = timed(fn, max(50, args.iters // 5))
        print(f"host-fed SESR-x2 1080p {k}: {us:.1f} us/frame = {1e6 / us:.0f} frames/s")
    img_np = img_h.numpy()[0]
    n = 10
    t0 = time.perf_counter()
    for _ in range(n):
        xx = torch.from_numpy((img_np / 255.).astype(np.float32).transpose(2, 0, 1).copy()[None]).pin_memory()
        x_d.copy_(xx, non_blocking=True)
        e.forward(x_d, want_f=False, out_q=oq)
    torch.cuda.synchronize(dev)
    us = (time.perf_counter() - t0) * 1e6 / n
    print(f"host-fed SESR-x2 1080p host numpy u8 / 255. (float64) + pinned fp32 upload + forward: {us:.0f} us/frame = "
          f"{1e6 / us:.0f} frames/s (wall clock, {n} frames)")
    for form, fn in (("rgb", lambda: (img_np / 255.).astype(np.float32)), ("y", lambda: host_y(img_np))):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        print(f"host numpy conversion alone, 1080p {form}: {(time.perf_counter() - t0) * 1e3 / n:.1f} ms/frame")

    # 3. device -> host: the exported uint8 4K frame vs the fp32 4K frame
    u8_h = torch.empty((1, H4, W4, 3), dtype=torch.uint8).pin_memory()
    f_h = torch.empty((1, 3, H4, W4), dtype=torch.float32).pin_memory()
    us_u8 = timed(lambda: (ex_f(), u8_h.copy_(out, non_blocking=True)), 50, warm=5)
    us_f = timed(lambda: f_h.copy_(pf, non_blocking=True), 50, warm=5)
    print(f"device->host 4K x2: export + uint8 copy ({u8_h.numel() / 1e6:.1f} MB) {us_u8:.0f} us vs fp32 copy "
          f"({4 * f_h.numel() / 1e6:.1f} MB) {us_f:.0f} us per frame (pinned)")


if __name__ == "__main__":
    main()
