#!/usr/bin/env python3
"""Colour-metadata fixtures made by the reference.  Needs the reference's sources: python make_develop_golden.py <reference dir>.

Imports the reference's own ``metadata2tensor`` (self_dataset.py, on stub cv2 / h5py as make_noise_golden.py does) and records, into
tests/golden/develop/metadata.npz, for a handful of well-conditioned camera matrices (the four xyz2cam matrices of the unprocessing
paper's pipeline and two synthetic ones) with white-balance gains:

  xyz2cam      (K, 3, 3) float64   the inputs
  red_gain, blue_gain   (K,) float64
  ref_cam2rgb  (K, 3, 3) fp32      what metadata2tensor returned (fp32 throughout: torch.mm, a row division, torch.inverse)
  ref_red, ref_blue     (K,) fp32
  cam2rgb      (K, 3, 3) float64   the same map in float64 with a closed-form inverse (tests/develop_oracle.py cam2rgb_f64)
  e_ref        (K,) float64        max |ref_cam2rgb - cam2rgb| of the case

A case whose e_ref exceeds 1e-4 of its largest entry is refused: that is far above the error of an fp32 LU inverse at these condition
numbers and far below what a misreading (a transpose, a missing row normalisation) moves."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
XYZ2CAM = (
    ((1.0234, -0.2969, -0.2266), (-0.5625, 1.6328, -0.0469), (-0.0703, 0.2188, 0.6406)),
    ((0.4913, -0.0541, -0.0202), (-0.613, 1.3513, 0.2906), (-0.1564, 0.2151, 0.7183)),
    ((0.838, -0.263, -0.0639), (-0.2887, 1.0725, 0.2496), (-0.0627, 0.1427, 0.5438)),
    ((0.6596, -0.2079, -0.0562), (-0.4782, 1.3016, 0.1933), (-0.097, 0.1581, 0.5181)),
    ((0.9, -0.1, -0.05), (-0.3, 1.2, 0.1), (-0.02, 0.15, 0.7)),
    ((0.75, -0.2, -0.1), (-0.45, 1.4, 0.05), (-0.08, 0.2, 0.6)),
)
GAINS = ((2.1, 1.6), (1.9, 1.5), (2.4, 1.9), (1.95, 2.05), (1.0, 1.0), (2.25, 1.55))


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "self_dataset.py")):
        raise SystemExit("usage: make_develop_golden.py <directory of the reference's self_dataset.py>")
    sys.dont_write_bytecode = True
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.modules["h5py"] = types.ModuleType("h5py")
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    import self_dataset
    import develop_oracle as DO

    fx = {k: [] for k in ("xyz2cam", "red_gain", "blue_gain", "ref_cam2rgb", "ref_red", "ref_blue", "cam2rgb", "e_ref")}
    for x, (rg, bg) in zip(XYZ2CAM, GAINS):
        ccm, r, b = self_dataset.metadata2tensor({"colormatrix": [list(row) for row in x], "red_gain": [rg], "blue_gain": [bg]})
        assert ccm.dtype == torch.float32 and tuple(ccm.shape) == (3, 3) and tuple(r.shape) == tuple(b.shape) == (1,)
        ref = ccm.numpy().copy()
        want = DO.cam2rgb_f64(x)
        e = float(np.abs(ref.astype(np.float64) - want).max())
        if e > 1e-4 * np.abs(want).max():
            raise SystemExit(f"case {len(fx['e_ref'])}: the reference and the float64 closed form differ by {e}")
        print(f"case {len(fx['e_ref'])}: e_ref = {e:.3e}, largest entry {np.abs(want).max():.4f}, cond = {np.linalg.cond(want):.2f}")
        for k, v in (("xyz2cam", np.array(x, np.float64)), ("red_gain", rg), ("blue_gain", bg), ("ref_cam2rgb", ref), ("ref_red", float(r)),
                     ("ref_blue", float(b)), ("cam2rgb", want), ("e_ref", e)):
            fx[k].append(v)
    out = {k: np.array(v, np.float32 if k.startswith("ref_") else np.float64) for k, v in fx.items()}
    out["meta"] = np.array(json.dumps({"torch": torch.__version__, "source": "self_dataset.metadata2tensor",
                                       "bound": "e_ref <= 1e-4 * max |cam2rgb| per case"}))
    out_dir = os.path.join(HERE, "develop")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "metadata.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
