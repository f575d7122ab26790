"""Seeded synthetic checkpoints for the --ckpt path of the host tests (tests/test_host_mirror.py).

The trained checkpoints of the reference are not part of this repository, so the load -> fold -> weight-quantiser path is pinned
on state dicts of the same nets with seeded conv weights instead: the tests write them to a .pth and load it like a reference
checkpoint; make_golden.py --case synth_ckpt ran the reference's own fold and weight quantiser on the very same state dicts
(tests/golden/ckpt/synthetic_folds.npz).  Only the tensors the fold reads are generated (the convs' weights and biases); every other
entry (PReLU slopes, a QAT checkpoint's quantiser buffers, which the fold does not read) keeps the value of the model it is made
for.  Every tensor is drawn from its own generator, keyed by the seed and the entry's name, so that the values do not depend on
which other entries a model has.  Pure numpy: no import of either implementation."""
import zlib

import numpy as np

CASES = {          # name: (MFLAG, QAT checkpoint layout, seed)
    "sesr_x4": (5, False, 11),
    "nrdm_3": (3, False, 12),
    "sesr_x4_qat": (5, True, 13),
    "nrdm_3_qat": (3, True, 14),
    "nrdm_6_qat": (4, True, 15),
}
STD = 0.05          # about the spread of the trained convs' weights (0.04-0.16)
CONV_KEYS = ("conv_expand.weight", "conv_expand.bias", "conv_squeeze.weight", "conv_squeeze.bias")
# what a reference QAT checkpoint carries besides the convs: the quantiser state of its two long-skip adds (QuantAdd), which the
# loader drops; a few entries of that kind
QUANT_ADD_KEYS = tuple(f"{m}.{o}.{v}" for m in ("add_residual", "add_upsampled_input")
                       for o in ("observer_res", "observer_shortcut") for v in ("min_val", "max_val"))


def synthetic_state_dict(model_sd, case):
    """model_sd: {name: tensor or array} of the (prepared, for a QAT case) model the checkpoint is made for -> {name: float32 array}."""
    mflag, qat, seed = CASES[case]
    out = {}
    for k, v in model_sd.items():
        a = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)
        if k.endswith(CONV_KEYS):
            rng = np.random.default_rng([seed, zlib.crc32(k.encode())])
            a = (rng.standard_normal(a.shape) * STD).astype(np.float32)
        out[k] = a
    if qat:
        for k in QUANT_ADD_KEYS:
            out.setdefault(k, np.zeros(1, np.float32))
    return out
