"""Writes tests/golden/quality/mosaic.npz: (pred, gt) pairs with their reference-run Bayer mosaics and the MFLAG 1 (nr) PSNR / SSIM,
for tests/test_mosaic_quality.py.  Build container only.

The mosaics are reference-run: the reference's own ``three2one`` is taken out of its test.py by ``ast`` (the module itself cannot be
imported: it needs cv2 and the dataset) and called exactly as its loop calls it (test.py:156-160), on the HWC fp32 frames, the
prediction clipped by np.clip first.  PSNR and SSIM are a float64 restatement of skimage's defaults (tests/mosaic_oracle.py on
tests/quality_oracle.py); skimage is not installed, so those values are not reference-run.

    python tests/golden/make_mosaic_golden.py /path/to/reference
Only data is written; no reference source goes into the repository.
"""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mosaic_oracle as M  # noqa: E402
from make_quality_golden import SCALE, ZERO, make_case  # noqa: E402  the int8 domain and the frames of the existing fixture


def reference_three2one(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, "test.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "three2one"]
    assert len(keep) == 1, "three2one not found in the reference's test.py"
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "reference test.py", "exec"), ns)
    return ns["three2one"]


def main(ref_root):
    three2one = reference_three2one(ref_root)
    rng = np.random.default_rng(20261019)
    # name, N, H, W, identical
    cases = [("mosaic_67x101", 2, 67, 101, False), ("mosaic_7x7", 3, 7, 7, False), ("mosaic_same", 1, 9, 12, True),
             ("mosaic_8x9", 2, 8, 9, False), ("mosaic_9x8", 2, 9, 8, False)]
    out, meta = {}, {"scale": float(SCALE), "zero": ZERO, "cases": {}}
    for name, N, H, W, same in cases:
        pred, gt, q = make_case(rng, 3, N, H, W, same)          # 3-channel frames; pred is the dequantised int8 frame q
        assert ((pred > 1).any() and (pred < 0).any()) or same, name
        mp = np.empty((N, H, W), np.float64)
        mg = np.empty((N, H, W), np.float64)
        for n in range(N):                     # the reference's loop body, HWC
            gfake = np.clip(pred[n].transpose(1, 2, 0), 0, 1)
            mp[n] = three2one(gfake)
            mg[n] = three2one(gt[n].transpose(1, 2, 0))
        oracle = M.metrics(pred, gt)
        out[name + ".pred"], out[name + ".gt"], out[name + ".q"] = pred, gt, q
        out[name + ".mosaic_pred_ref"], out[name + ".mosaic_gt_ref"] = mp, mg
        out[name + ".mse_restated"] = oracle[:, 0]
        out[name + ".psnr_restated"] = oracle[:, 1]
        out[name + ".ssim_restated"] = oracle[:, 2]
        meta["cases"][name] = {"identical": same}
    meta["mosaic_ref"] = "reference-run: three2one of the reference's test.py on the clipped prediction and on the ground truth (float64)"
    meta["restated"] = ("mse / psnr / ssim: restatement of skimage defaults (peak_signal_noise_ratio, data_range 1; single-channel "
                        "structural_similarity); skimage is not installed, so not reference-run")
    out["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.join(HERE, "quality"), exist_ok=True)
    dst = os.path.join(HERE, "quality", "mosaic.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, sorted(meta["cases"]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SESRQ_REFERENCE", "../reference"))
