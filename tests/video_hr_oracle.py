"""numpy restatement of include/sesrq_video_hr.h: every plane of an HR 4:2:0 frame is an image of its own and goes through the two
passes of tests/downscale_oracle.py (vertical first); the LR luma is decoded by tests/video_oracle.py.  No arithmetic of its own.

A frame is video_oracle's dict of planes {"y": (N, H, W), "cb": (N, H / 2, W / 2), "cr": likewise} uint8."""
import os
import re

import numpy as np

import downscale_oracle as DO
import video_oracle as VO

HEADER = os.path.join(os.path.dirname(VO.HEADER), "sesrq_video_hr.h")


def tile(r):
    """The kernel's tile (w, h) in LR luma pixels at factor r: the header's HR tile over r."""
    src = open(HEADER).read()
    w, h = (int(re.search(rf"#define SESRQ_VIDEO_HR_TILE_HR_{d}\s+(\d+)", src).group(1)) for d in "WH")
    assert w % (2 * r) == 0 and h % (2 * r) == 0
    return w // r, h // r


def plane(p, r):
    """(N, H, W) uint8 -> (N, H / r, W / r) uint8."""
    return np.ascontiguousarray(DO.one_pass(DO.one_pass(p, r, 1), r, 2))


def downscale(hr, r):
    """The HR frames -> the LR frames; the HR luma must be a multiple of 2 r each way."""
    assert hr["y"].shape[1] % (2 * r) == 0 and hr["y"].shape[2] % (2 * r) == 0
    return {k: plane(v, r) for k, v in hr.items()}


def run(hr, r, scale_in=None, zero_in=None, exact_div=0):
    """(LR frames, q0 int8 (N, 1, H, W) | None without a domain, x fp32 (N, 1, H, W))."""
    lr = downscale(hr, r)
    return (lr,) + VO.decode(lr["y"], scale_in, zero_in, exact_div)
