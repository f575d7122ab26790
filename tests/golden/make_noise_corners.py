#!/usr/bin/env python3
"""Where the Box-Muller stage of include/sesrq_noise.h reaches its corners: tests/golden/noise/corners.json.

Uses tests/noise_oracle.py alone.  Searches frames 0 .. 15 of 2048 x 2048 of the stream SEED = 0x0123456789ABCDEF for pixels whose
words hit

  w0 >> 9, w2 >> 9   0 and 2^23 - 1: u_r = 2^-24 (|z| up to Z_MAX) and 1 - 2^-24 (rho = 3.5e-4)
  w1 >> 8, w3 >> 8   0, 1, 2^22, 2^23, 3 * 2^22 and 2^24 - 1: the angle 2 pi u_t on the quadrant boundaries 0, pi / 2, pi, 3 pi / 2,
                     where cospif / sincospif must return exact 0 and +-1, and next to the boundary at 0 from both sides

and writes up to KEEP hits per (word, target), in scan order: {"seed", "frames", "H", "W", "hits": [[frame, y, x, word, target]]}.
About 16 s.  tests/test_noise_limits.py checks the list against the oracle and the device's deviates at those pixels."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED = 0x0123456789ABCDEF
FRAMES, H, W = 16, 2048, 2048
KEEP = 3
R_TARGETS = (0, 2 ** 23 - 1)
T_TARGETS = (0, 1, 2 ** 22, 2 ** 23, 3 * 2 ** 22, 2 ** 24 - 1)
TARGETS = [(k, t) for k in (0, 2) for t in R_TARGETS] + [(k, t) for k in (1, 3) for t in T_TARGETS]


def main():
    import noise_oracle as NO
    hits = {kt: [] for kt in TARGETS}
    for f in range(FRAMES):
        w = NO.words(SEED, f, H, W)
        for k in range(4):
            v = w[k] >> np.uint64(9 if k % 2 == 0 else 8)
            for t in (R_TARGETS if k % 2 == 0 else T_TARGETS):
                for y, x in np.argwhere(v == np.uint64(t)):
                    hits[k, t].append([f, int(y), int(x), k, t])
    missing = [kt for kt in TARGETS if not hits[kt]]
    assert not missing, f"no pixel for (word, target) {missing}"
    for kt in TARGETS:
        print(f"w{kt[0]} >> {9 if kt[0] % 2 == 0 else 8} = {kt[1]}: {len(hits[kt])} hits, first {hits[kt][0][:3]}")
    out = dict(seed=SEED, frames=FRAMES, H=H, W=W, hits=[h for kt in TARGETS for h in hits[kt][:KEEP]])
    path = os.path.join(HERE, "noise", "corners.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print("wrote", path, len(out["hits"]), "hits")


if __name__ == "__main__":
    main()
