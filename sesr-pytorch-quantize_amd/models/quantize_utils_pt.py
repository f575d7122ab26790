"""``quantize.prepare()`` for the integer path: what a ``*_qat_G.pth`` checkpoint needs to be folded.

The reference consumes its QAT checkpoints by wrapping every conv in a ``QuantConv2d`` (reference
models/quantize_utils_pt.py:331-512, ``prepare`` :801-835, called at sim.py:64-66 with ``a_bits=8, w_bits=8,
q_type=0, q_level="C"``) and then calling ``collapse()`` while the net is in training mode (sim.py:63,76).  The
fold therefore runs the block's two convs on a delta image THROUGH their fake-quantisers, and because a fresh
observer takes its first range from the tensor it sees (MinMaxObserver / MovingAverageMinMaxObserver
``num_flag == 0``, :68-81, :107-120) the observer state stored in the checkpoint plays no part: the collapsed
weights depend on the conv weights alone.  Per conv, for its input x and weight w (Quantizer.forward :220-246,
SymmetricQuantizer.update_qparams :299-312, Round :150-166; ``q_level="C"`` is not the integer 0 the layer
constructor tests for, so both quantisers are per-TENSOR, :376-404):

    fq(t, lo, hi):  s = max(max(|min t|, |max t|) / ((hi - lo) / 2), eps_f32)
                    q = clamp(sign(t/s) * floor(|t/s| + 0.5), lo, hi)          # round half away from zero
                    return q * s
    y = conv2d(fq(x, -128, 127), fq(w, -127, 127), bias)

Only this inference-time fold and the QuantAdd's constant scale (below) are implemented -- observers' running averages,
the straight-through backward, the asymmetric / histogram / per-channel variants, QuantReLU and BN fusing are training
machinery outside the hot path ("out of scope").

QuantAdd (:654-711): ``prepare`` also replaces the long skip's ``AddOp`` by a ``QuantAdd`` (``add_residual``), and the
reference's calibration pass (test.py, mode 0) therefore adds two fake-quantised tensors.  test.py traces the prepared
model with torch.fx while it is in training mode; buffers are not proxied, so the union of the two observers' ranges
(:700-707) and ``update_qparams`` (:299-312) run once, at trace time, on the observer state the checkpoint holds, and the
scale enters the graph as a constant -- the moving-average updates of the observers are dead writes nothing reads back.
``skip_quant_scale`` recomputes that constant from a state_dict (the ``activation_quantizer.scale`` the checkpoint stores
differs from it in the last digits and is not what the trace uses); sesrq.calibrate.Calibrator(skip_quant_scale=...)
applies it.  The integer path merges the skip in the integer domain and never evaluates the QuantAdd, so the loader
(sim.py) still drops the ``add_residual.*`` / ``add_upsampled_input.*`` entries before ``load_state_dict``; the second add
is commented out of the reference's forward.
"""
import copy

import torch
import torch.nn.functional as F
from torch import nn

def fake_quantize(t, lo, hi):
    """Symmetric per-tensor fake quantisation with the range taken from ``t`` itself (first call of a fresh observer)."""
    eps = torch.tensor(torch.finfo(torch.float32).eps, dtype=torch.float32)
    span = torch.max(torch.abs(torch.min(t)), torch.abs(torch.max(t)))
    s = torch.max(span / (float(hi - lo) / 2), eps)
    u = t / s
    q = torch.clamp(torch.sign(u) * torch.floor(torch.abs(u) + 0.5), lo, hi)
    return q * s


class _QuantizerState(nn.Module):
    """Holds the buffers a reference Quantizer saves, so a QAT state_dict loads key for key.  Values are not used."""

    def __init__(self, lo, hi):
        super().__init__()
        self.register_buffer("scale", torch.ones(1))
        self.register_buffer("zero_point", torch.zeros(1))
        self.register_buffer("eps", torch.tensor(torch.finfo(torch.float32).eps))
        self.register_buffer("quant_min_val", torch.tensor(float(lo)))
        self.register_buffer("quant_max_val", torch.tensor(float(hi)))
        self.observer = nn.Module()
        self.observer.register_buffer("min_val", torch.zeros(1))
        self.observer.register_buffer("max_val", torch.zeros(1))


class QuantConv2d(nn.Conv2d):
    """A conv whose forward fake-quantises its input (8-bit activations: [-128, 127]) and its weight ([-127, 127])
    per tensor, ranges observed on the spot -- the training-mode first call of the reference's layer."""

    def __init__(self, conv: nn.Conv2d, a_bits=8, w_bits=8):
        super().__init__(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, conv.dilation,
                         conv.groups, conv.bias is not None, conv.padding_mode)
        self.weight = conv.weight
        self.bias = conv.bias
        self.a_range = (-(1 << (a_bits - 1)), (1 << (a_bits - 1)) - 1)
        self.w_range = (-((1 << (w_bits - 1)) - 1), (1 << (w_bits - 1)) - 1)
        self.activation_quantizer = _QuantizerState(*self.a_range)
        self.weight_quantizer = _QuantizerState(*self.w_range)

    def forward(self, x):
        return F.conv2d(fake_quantize(x, *self.a_range), fake_quantize(self.weight, *self.w_range), self.bias, self.stride,
                        self.padding, self.dilation, self.groups)


def prepare(model, inplace=False, a_bits=8, w_bits=8, q_type=0, q_level=0, **unsupported):
    """Wrap every ``nn.Conv2d`` of ``model`` for the QAT fold (reference prepare(), :801-835).  Only the
    configuration the reference's integer path uses is accepted: symmetric (``q_type=0``), 8/8 bits, per-tensor
    weight ranges (``q_level`` anything but the integer 0)."""
    if unsupported:
        raise ValueError(f"prepare(): options {sorted(unsupported)} belong to QAT training, which this package does not implement")
    if q_type != 0:
        raise ValueError("prepare(): only symmetric quantisers (q_type=0, reference sim.py:66) are implemented")
    if isinstance(q_level, int) and q_level == 0:
        raise ValueError("prepare(): per-channel weight ranges (q_level=0) are not implemented; the reference's integer "
                         "path passes q_level=\"C\", which selects per-tensor ranges (quantize_utils_pt.py:376-404)")
    if a_bits == 32 or w_bits == 32 or a_bits < 2 or w_bits < 2:
        raise ValueError("prepare(): a_bits / w_bits must be integer widths below 32")
    if not inplace:
        model = copy.deepcopy(model)

    def wrap(module):
        for name, child in list(module.named_children()):
            if isinstance(child, QuantConv2d):
                continue
            if isinstance(child, nn.Conv2d):
                setattr(module, name, QuantConv2d(child, a_bits, w_bits))
            else:
                wrap(child)
    wrap(model)
    return model


SKIP_ADD = "add_residual."
SKIP_OBSERVER_KEYS = tuple(SKIP_ADD + k for k in ("observer_res.min_val", "observer_res.max_val", "observer_shortcut.min_val",
                                                  "observer_shortcut.max_val"))


def skip_quant_scale(sd):
    """The constant scale of the long skip's QuantAdd, from the four observer extrema of a QAT state_dict (reference
    QuantAdd.forward :700-707, SymmetricQuantizer.update_qparams :299-312, a_bits = 8: test.py:62), in fp32 as the reference
    forms it:  s = max(max(|min(res.min, shortcut.min)|, |max(res.max, shortcut.max)|) / 127.5, eps_f32).
    None for a state_dict without ``add_residual.*`` entries (not a QAT checkpoint); ValueError when some of the four are missing."""
    if not any(k.startswith(SKIP_ADD) for k in sd):
        return None
    missing = [k for k in SKIP_OBSERVER_KEYS if k not in sd]
    if missing:
        raise ValueError(f"QAT state_dict: the QuantAdd's observer state is incomplete, missing {missing}")
    r_min, r_max, s_min, s_max = (torch.as_tensor(sd[k], dtype=torch.float32).reshape(-1)[0] for k in SKIP_OBSERVER_KEYS)
    lo, hi = torch.min(r_min, s_min), torch.max(r_max, s_max)
    eps = torch.tensor(torch.finfo(torch.float32).eps, dtype=torch.float32)
    s = torch.max(torch.max(torch.abs(lo), torch.abs(hi)) / 127.5, eps)
    return float(s)


def is_qat_state_dict(sd):
    return any("_quantizer." in k for k in sd)
