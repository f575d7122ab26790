"""Writes tests/golden/quality/quality.npz (a directory of its own: every tests/golden/*.npz is a net fixture): (pred, gt) pairs with their PSNR / SSIM, for tests/test_quality.py.  Build container only.

PSNR of the srx4 (MFLAG 5) and srx2 (MFLAG 6) forms is reference-run: the reference's own ``compute_psnr`` and ``rgb_to_yuv`` are
taken out of its test.py by ``ast`` (the module itself cannot be imported: it needs cv2 and the dataset) and called exactly as its
loop calls them (test.py:157-169), on float64 copies of the stored float32 frames (HWC, the prediction clipped).
SSIM of every form and the skimage PSNR of the RGB form (MFLAG 3 / 4) are a float64 restatement of skimage's defaults
(tests/quality_oracle.py); skimage is not installed, so those values are not reference-run.

    python tests/golden/make_quality_golden.py /path/to/reference
Only data is written; no reference source goes into the repository.
"""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import quality_oracle as Q  # noqa: E402

# int8 output domain the int8 predictions are written in: (q - ZERO) * SCALE spans [-0.082, 1.06], so the clip is exercised
SCALE, ZERO = np.float32(1.0 / 220.0), -110


def reference_functions(ref_root):
    src = open(os.path.join(ref_root, "test.py")).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("compute_psnr", "rgb_to_yuv")]
    assert len(keep) == 2, "compute_psnr / rgb_to_yuv not found in the reference's test.py"
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "reference test.py", "exec"), ns)
    return ns["compute_psnr"], ns["rgb_to_yuv"]


def smooth(rng, N, C, H, W):
    yy = np.linspace(0.0, 1.0, H)[:, None]
    xx = np.linspace(0.0, 1.0, W)[None, :]
    out = np.empty((N, C, H, W), np.float64)
    for n in range(N):
        for c in range(C):
            a, b, d = rng.uniform(0.1, 0.6, 3)
            out[n, c] = 0.2 + a * xx + b * yy * yy + 0.1 * np.where(xx + d * yy > 0.6, 1.0, 0.0)
    return out


def dequant(q):
    return ((q.astype(np.int32) - ZERO).astype(np.float32) * SCALE).astype(np.float32)


def make_case(rng, mflag, N, H, W, identical=False):
    C = 1 if mflag == 5 else 3
    gt = smooth(rng, N, C, H, W) + rng.normal(0.0, 0.02, (N, C, H, W))
    gt[..., 0, :3] += 0.2                      # a few ground-truth values outside [0, 1]: never clipped
    gt = gt.astype(np.float32)
    if identical:                              # an int8-representable frame inside [0, 1]: pred == gt after the clip
        q = np.clip(np.rint(gt / SCALE) + ZERO, ZERO, 100).astype(np.int8)
        pred = dequant(q)
        gt = pred.copy()
    elif mflag == 6:                           # the anchored float output: not on an int8 grid
        q = np.zeros(gt.shape, np.int8)
        pred = (gt + rng.normal(0.0, 0.06, gt.shape)).astype(np.float32)
        pred[..., -1, :5] = 1.3                # clipped
        pred[..., 1, -4:] = -0.2
    else:
        noisy = gt.astype(np.float64) + rng.normal(0.0, 0.05, gt.shape)
        noisy[..., -1, :5] = 1.2
        noisy[..., 1, -4:] = -0.2
        q = np.clip(np.rint(noisy / float(SCALE)) + ZERO, -128, 127).astype(np.int8)
        pred = dequant(q)
    return pred, gt, q


def main(ref_root):
    compute_psnr, rgb_to_yuv = reference_functions(ref_root)
    rng = np.random.default_rng(20261015)
    cases = [("rgb_67x101", 3, 2, 67, 101, False), ("rgb_7x7", 3, 3, 7, 7, False), ("rgb_same", 3, 1, 9, 12, True),
             ("y255_67x101", 5, 2, 67, 101, False), ("y255_7x7", 5, 3, 7, 7, False), ("y255_same", 5, 1, 9, 12, True),
             ("x2_67x101", 6, 2, 67, 101, False), ("x2_7x7", 6, 3, 7, 7, False), ("x2_same", 6, 1, 9, 12, True)]
    out, meta = {}, {"scale": float(SCALE), "zero": ZERO, "cases": {}}
    for name, mflag, N, H, W, same in cases:
        pred, gt, q = make_case(rng, mflag, N, H, W, same)
        oracle = Q.metrics(pred, gt, mflag)
        psnr_ref = np.full(N, np.nan)
        for n in range(N):                     # the reference's loop body, HWC, on float64 copies
            g = gt[n].astype(np.float64).transpose(1, 2, 0)
            p = np.clip(pred[n].astype(np.float64).transpose(1, 2, 0), 0, 1)
            if mflag == 5:
                psnr_ref[n] = compute_psnr(g[:, :, 0] * 255., p[:, :, 0] * 255.)
            elif mflag == 6:
                psnr_ref[n] = compute_psnr(rgb_to_yuv(g), rgb_to_yuv(p))
        out[name + ".pred"], out[name + ".gt"], out[name + ".q"] = pred, gt, q
        out[name + ".psnr_ref"] = psnr_ref
        out[name + ".psnr_restated"] = oracle[:, 1]
        out[name + ".ssim_restated"] = oracle[:, 2]
        meta["cases"][name] = {"mflag": mflag, "int8": mflag != 6, "identical": same}
    meta["psnr_ref"] = "reference-run: compute_psnr / rgb_to_yuv of the reference's test.py (MFLAG 5 and 6; NaN for MFLAG 3)"
    meta["psnr_restated"] = ("restatement of skimage defaults; skimage is not installed, so not reference-run "
                             "(peak_signal_noise_ratio, data_range 1, for MFLAG 3; the compute_psnr form otherwise)")
    meta["ssim_restated"] = "restatement of skimage defaults; skimage is not installed, so not reference-run"
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.join(HERE, "quality"), exist_ok=True)
    dst = os.path.join(HERE, "quality", "quality.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, sorted(meta["cases"]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SESRQ_REFERENCE", "../reference"))
