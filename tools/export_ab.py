#!/usr/bin/env python3
"""The A/B behind profiles/upscale_refactor_ab.txt, kept so that its command lines can be run again; it has no other use.  HIP-event
timing of the 4 colour and 8 video export cases of TREE's probes (the buffers and fused launches of tools/colour_probe.py and
tools/video_probe.py) on TREE's libraries, one process; run once per checkout and turn, the checkouts alternating in one job:
   python tools/export_ab.py TREE OUT.json [--iters N --reps R]
Per case one untimed window of N launches, then R timed windows back to back, then the sha256 of the case's output (seeded inputs),
to compare two checkouts' results: nothing but launches lies between the warm-up and the last timed window."""
import argparse
import hashlib
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("tree")
ap.add_argument("out")
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path[:0] = [os.path.join(tree, "tools"), os.path.join(tree, "sesr-pytorch-quantize_amd")]
import colour_probe as CP  # noqa: E402
import video_probe as VP  # noqa: E402
import torch  # noqa: E402
from sesrq import colour, video  # noqa: E402

assert os.path.abspath(colour.LIB_PATH).startswith(tree + os.sep), colour.LIB_PATH
assert os.path.abspath(video.LIB_PATH).startswith(tree + os.sep), video.LIB_PATH
dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev)
torch.manual_seed(0)
res = {"tree": tree, "iters": args.iters, "reps": args.reps, "cases": {}}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def window(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def run(name, fn, outs):
    window(fn, args.iters)
    us = [window(fn, args.iters) for _ in range(args.reps)]
    digest = sha(*outs)
    res["cases"][name] = {"us": us, "median": statistics.median(us), "min": min(us), "max": max(us), "sha256": digest}
    print(f"{name:40s} median {statistics.median(us):7.2f}  min {min(us):7.2f}  max {max(us):7.2f} us   {digest[:12]}", flush=True)


for name, (y, img, r, out) in CP.buffers(dev).items():
    run("colour " + name, CP.fused(st, y, img, r, out), [out])
for name, (y, lr, r, out) in VP.buffers(dev).items():
    run("video " + name, VP.fused(st, y, lr, r, out), [out.buf])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
