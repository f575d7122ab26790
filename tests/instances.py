"""What the instance-coverage modules share -- TEST INFRASTRUCTURE (not collected): the tracker that attributes launched kernel
instantiations to a tier, the reference crops and the selection options they run under.  tests/test_instances.py drives the matrix and
judges the coverage; tests/test_launch_trace.py adds its launches to the same record."""
from conftest import golden_files
from oracle import sesrq_oracle as O
from sesrq import _lib

REF_PINNED = set()       # instances launched by a case whose expected result came from the reference
ORACLE_ONLY = set()      # ... by a case checked against the oracle only


class Track:
    """Attributes the instances launched inside the block to a tier."""

    def __init__(self, pinned):
        self.pinned = pinned

    def __enter__(self):
        self.before = _lib.instances()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            import torch
            torch.cuda.synchronize()
            after = _lib.instances()
            hit = {k for k, v in after.items() if v > self.before.get(k, 0)}
            (REF_PINNED if self.pinned else ORACLE_ONLY).update(hit)
        return False


def shuffle(q5, r):
    return O.pixel_shuffle(q5, r)


OUT_KINDS = [(True, False), (False, True), (True, True)]      # (want_q, want_f): the three output kinds of the boundary


RF_ALL = 63
# reduced_forms masks: trio modes 0 / 1 / 3 / 7 / 15 (bits 1, 2, 4, 8) and the last layer's forms 1 / 2 / none (bits 16, 32)
RF_MASKS = [0, 1, RF_ALL & ~4 & ~8, RF_ALL & ~8, RF_ALL, RF_ALL & ~16, RF_ALL & ~16 & ~32]

CROPS = [f for f in golden_files() if f.endswith((".crop.npz", ".zeros.npz", ".satw.npz", ".satw_zeros.npz", ".stim.npz"))]


def plan_variants():
    v = [dict(), dict(fuse_hidden=0), dict(engine=_lib.ENGINE_DOT4), dict(force_general=True)]
    v += [dict(reduced_forms=m) for m in RF_MASKS] + [dict(reduced_forms=m, fuse_hidden=0) for m in (0, RF_ALL & ~16)]
    return v
