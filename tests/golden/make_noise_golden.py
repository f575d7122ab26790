#!/usr/bin/env python3
"""Noise fixtures made by the reference.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference's sources).

Imports the reference's own ``add_noise`` and ``random_noise_levels`` (self_dataset.py, on stub cv2 / h5py as make_raw_golden.py does)
and records, into tests/golden/noise/add_noise.npz (fp32):

  x            (8192,)  a ramp of all 4096 codes / 4095 (the reference's fp32 quotient), then 4096 zeros (the non-sites)
  levels       (P, 2)   (shot, read) pairs, shot = 0 and read = 0 among them (read = 0: recorded with the argument validation of
                        torch.distributions off, since the reference's Normal refuses the zero variance at x = 0)
  seeds        (P,)     torch.manual_seed of each pair
  eps_<p>      (8192,)  what torch.normal(zeros, ones) yields under that seed: the standard normal add_noise scales
  out_<p>      (8192,)  add_noise(x, shot, read) under the same seed
  sigma_<p>    (8192,)  the reference's own torch.sqrt(x * shot + read), the scale of its Normal
  log_shot, g  (K,)     the two draws of random_noise_levels under seeds level_seeds: the uniform log shot level and the N(0, 0.26)
                        offset of the log read level
  shot, read   (K,)     what random_noise_levels returned under the same seeds

torch's CPU normal sampler fills a tensor with standard normals and then scales it by the std tensor, so the same-seed eps is the draw
behind out.  One step of the reference is not IEEE arithmetic: torch's vectorised CPU sqrt (the AVX-512 build this fixture was made
with) is off by one ulp for about 0.4 % of its arguments, where numpy's, the C library's and the device's sqrtf are correctly
rounded.  So the generator asserts, before it writes anything (tests/noise_oracle.py):
  - x * shot + read as combine forms it is the reference's variance, bit for bit;
  - sigma_<p> is within one ulp of the correctly rounded root of that variance;
  - combine(x, shot, read, eps, sigma=sigma_<p>) == out bit for bit, everywhere -- every other step of combine is the reference's;
  - combine(x, shot, read, eps) == out bit for bit wherever sigma_<p> is the correctly rounded root.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
PAIRS = ((0.01, 0.0005), (1e-4, 1e-8), (0.012, 1e-3), (0.0, 1e-4), (3e-3, 0.0), (0.0, 0.0))
LEVEL_SEEDS = tuple(range(100, 164))


def main():
    sys.dont_write_bytecode = True
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.modules["h5py"] = types.ModuleType("h5py")
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    import torch.distributions as tdist
    import self_dataset
    import noise_oracle as NO

    codes = torch.arange(4096, dtype=torch.float32)
    x = torch.cat([codes / (2 ** 12 - 1), torch.zeros(4096)])
    assert x.dtype == torch.float32
    fx = {"x": x.numpy().copy(), "levels": np.array(PAIRS, np.float32), "seeds": np.arange(len(PAIRS), dtype=np.int64) + 7}
    for p, (shot, read) in enumerate(PAIRS):
        seed = int(fx["seeds"][p])
        torch.manual_seed(seed)
        # read = 0 leaves zero variance wherever x = 0, which the reference's Normal refuses when it validates its arguments; the
        # arithmetic is the same without the validation, and a zero level must leave the frame as it is
        tdist.Distribution.set_default_validate_args(read > 0)
        out = self_dataset.add_noise(x, shot, read)
        tdist.Distribution.set_default_validate_args(True)
        torch.manual_seed(seed)
        eps = torch.normal(torch.zeros_like(x), torch.ones_like(x))
        assert out.dtype == torch.float32 and eps.dtype == torch.float32
        var = x * shot + read
        sigma = torch.sqrt(var).numpy()
        bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
        v = NO.variance(fx["x"], shot, read)
        assert np.array_equal(bits(v), bits(var.numpy())), f"variance differs at pair {p}"
        root = np.sqrt(v.astype(np.float64)).astype(np.float32)
        assert np.abs(bits(sigma).astype(np.int64) - bits(root)).max() <= 1, f"the reference's sqrt is more than an ulp off at pair {p}"
        got = NO.combine(fx["x"], shot, read, eps.numpy(), sigma=sigma)
        assert np.array_equal(bits(got), bits(out.numpy())), f"combine on the reference's sigma differs from add_noise at pair {p}"
        same = sigma == root
        got = NO.combine(fx["x"], shot, read, eps.numpy())
        assert np.array_equal(bits(got)[same], bits(out.numpy())[same]), f"combine differs from add_noise at pair {p}"
        print(f"pair {p}: sigma off by an ulp at {int((~same).sum())} of {same.size}")
        fx[f"eps_{p}"], fx[f"out_{p}"], fx[f"sigma_{p}"] = eps.numpy().copy(), out.numpy().copy(), sigma.copy()

    rec = {k: [] for k in ("log_shot", "g", "shot", "read")}
    for seed in LEVEL_SEEDS:
        torch.manual_seed(seed)
        shot, read = self_dataset.random_noise_levels()
        torch.manual_seed(seed)          # the same two draws, in the reference's order
        log_shot = torch.FloatTensor(1).uniform_(np.log(0.0001), np.log(0.012))
        g = tdist.Normal(loc=torch.tensor([0.0]), scale=torch.tensor([0.26])).sample()
        assert torch.equal(torch.exp(log_shot), shot), "the replayed uniform draw is not random_noise_levels'"
        assert torch.equal(torch.exp(2.18 * log_shot + 1.20 + g), read), "the replayed normal draw is not random_noise_levels'"
        for k, v in (("log_shot", log_shot), ("g", g), ("shot", shot), ("read", read)):
            rec[k].append(float(v))
    for k, v in rec.items():
        fx[k] = np.array(v, np.float32)
    fx["level_seeds"] = np.array(LEVEL_SEEDS, np.int64)
    fx["meta"] = np.array(json.dumps({"torch": torch.__version__, "eps": "same-seed torch.normal(zeros, ones); combine(x, shot, read, eps, "
                                      "sigma=sigma_p) == add_noise(x, shot, read) bit for bit; sigma_p is torch's CPU sqrt, within "
                                      "one ulp of the correctly rounded root"}))
    out_dir = os.path.join(HERE, "noise")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "add_noise.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
