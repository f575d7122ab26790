"""ctypes binding of libsesrq.so (C ABI declared in include/sesrq.h), and the host plumbing every binding in the package shares:
the loader (bind, Library), the stream entry of a launch, the host-array conversion, the input domain of the front ends and the
luma arguments of the colour and the video export.

The library is the product: if it is missing or a symbol cannot be resolved this module
raises immediately -- there is no CPU or PyTorch fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SESRQ_LIB selects another build of the same ABI (A/B kernel experiments); never a fallback.
LIB_PATH = os.environ.get("SESRQ_LIB") or os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq.so"))

MAX_LAYERS = 16
MAX_CH = 16
F32, I8 = 0, 1
ENGINE_AUTO, ENGINE_DOT4, ENGINE_MFMA, ENGINE_MFMA_Q = 0, 1, 2, 3
ENGINE_NAMES = {"auto": ENGINE_AUTO, "dot4": ENGINE_DOT4, "mfma": ENGINE_MFMA, "mfma-q": ENGINE_MFMA_Q}      # the --engine flag of sim.py / test.py
VERDICT_SATURATION_FREE, VERDICT_BIASED_OK = 1, 2
ABI_VERSION = 4


class LayerDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("ic", C.c_int32), ("oc", C.c_int32),
                ("w", C.POINTER(C.c_int8)), ("add_const", C.POINTER(C.c_int32)),
                ("M", C.c_uint32), ("n", C.c_uint32), ("relu", C.c_int32),
                ("M_oc", C.POINTER(C.c_uint32)), ("n_oc", C.POINTER(C.c_uint32))]


class NetDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("layers", C.POINTER(LayerDesc)), ("zero", C.POINTER(C.c_int32)),
                ("scale_in", C.c_float), ("scale_out", C.c_float), ("M_res", C.c_uint32), ("n_res", C.c_uint32),
                ("pixel_shuffle", C.c_int32), ("pe_num", C.c_int32), ("pe_acc_bits", C.c_int32),
                ("pe_add_bits", C.c_int32)]


class Options(C.Structure):
    _fields_ = [("engine", C.c_int32), ("force_general", C.c_int32), ("exact_div", C.c_int32),
                ("anchor_add", C.c_int32), ("fuse_hidden", C.c_int32), ("wg_budget", C.c_int32),
                ("i8_in_scale", C.c_float), ("i8_in_zero", C.c_int32), ("reduced_forms", C.c_int32)]


class CalibConvDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("ic", C.c_int32), ("oc", C.c_int32), ("w", C.c_void_p), ("qbias", C.c_void_p),
                ("in_scale", C.c_float), ("in_zero", C.c_int32), ("ss", C.c_float), ("acc_lo", C.c_float),
                ("acc_hi", C.c_float), ("add_lo", C.c_float), ("add_hi", C.c_float), ("relu", C.c_int32)]


class CalibSlot(C.Structure):
    """sesrq_calib_slot: one quantiser input's state in the device-resident calibration pass (include/sesrq.h)."""
    _fields_ = [("ord", C.c_uint32 * 2), ("min", C.c_float), ("max", C.c_float), ("run_min", C.c_float), ("run_max", C.c_float),
                ("scale", C.c_double), ("zero", C.c_int32), ("degenerate", C.c_int32), ("batches", C.c_int32),
                ("scale32", C.c_float), ("zero32", C.c_float), ("ss", C.c_float), ("acc_lo", C.c_float), ("acc_hi", C.c_float),
                ("add_lo", C.c_float), ("add_hi", C.c_float), ("qbias", C.c_float * MAX_CH)]


class CalibDomainDesc(C.Structure):
    _fields_ = [("quan_bits", C.c_int32), ("oc", C.c_int32), ("bias", C.c_void_p), ("sw", C.c_double), ("acc_bits", C.c_int32),
                ("add_bits", C.c_int32), ("bias_bits", C.c_int32)]


class FrameIO(C.Structure):
    _fields_ = [("inp", C.c_void_p), ("out_q", C.c_void_p), ("out_f", C.c_void_p)]


class Taps(C.Structure):
    _fields_ = [("act", C.c_void_p * MAX_LAYERS), ("pe_out", C.c_void_p * MAX_LAYERS),
                ("pe_add", C.c_void_p * MAX_LAYERS), ("overflow", C.c_void_p), ("shortcut", C.c_void_p), ("ic", C.c_void_p)]


# every symbol include/sesrq.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_default_options": (None, [C.POINTER(Options)]),
    "sesrq_create": (C.c_int, [C.POINTER(NetDesc), C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "sesrq_create_q": (C.c_int, [C.POINTER(NetDesc), C.POINTER(Options), C.c_int, C.POINTER(C.c_void_p)]),
    "sesrq_net_quan_bits": (C.c_int, [C.c_void_p]),
    "sesrq_destroy": (None, [C.c_void_p]),
    "sesrq_launch_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sesrq_fast_division_proven": (C.c_int, [C.c_void_p]),
    "sesrq_layer_one_fma": (C.c_int, [C.c_void_p, C.c_int]),
    "sesrq_requant_form": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int]),
    "sesrq_saturation_verdict": (C.c_int, [C.POINTER(C.c_int8), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sesrq_net_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sesrq_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "sesrq_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                C.c_void_p, C.c_size_t, C.c_void_p]),
    "sesrq_forward_many": (C.c_int, [C.c_void_p, C.POINTER(FrameIO), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "sesrq_submit_selftest": (C.c_int, [C.c_int, C.c_int]),
    "sesrq_instance_count": (C.c_int, []),
    "sesrq_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_narrow_instance_count": (C.c_int, []),
    "sesrq_narrow_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_narrow_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_qadd_instance_count": (C.c_int, []),
    "sesrq_qadd_instance_name": (C.c_char_p, [C.c_int]),
    "sesrq_qadd_instance_launches": (C.c_longlong, [C.c_int]),
    "sesrq_forward_debug": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Taps)]),
    "sesrq_forward_timed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_float),
                                      C.POINTER(C.c_float)]),
    "sesrq_layer_engine": (C.c_char_p, [C.c_void_p, C.c_int]),
    "sesrq_calib_conv": (C.c_int, [C.POINTER(CalibConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p]),
    "sesrq_calib_conv_q": (C.c_int, [C.POINTER(CalibConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p]),
    "sesrq_calib_minmax": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sesrq_calib_fakequant": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_void_p]),
    "sesrq_calib_fakequant_q": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_int, C.c_void_p]),
    "sesrq_calib_histogram": (C.c_int, [C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "sesrq_calib_slot_bytes": (C.c_size_t, []),
    "sesrq_calib_slots_init": (C.c_int, [C.POINTER(CalibSlot), C.c_int]),
    "sesrq_calib_observe_slot": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(CalibDomainDesc), C.c_void_p]),
    "sesrq_calib_conv_slot": (C.c_int, [C.POINTER(CalibConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p]),
    "sesrq_calib_conv_qadd": (C.c_int, [C.POINTER(CalibConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_float, C.c_void_p]),
    "sesrq_calib_conv_slot_qadd": (C.c_int, [C.POINTER(CalibConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "sesrq_calib_fakequant_slot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p]),
    "sesrq_requant_const": (C.c_int, [C.c_double, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "sesrq_quantize_weight": (C.c_int, [C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(C.c_int8),
                                        C.POINTER(C.c_double)]),
    "sesrq_quantize_weight_per_channel": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_int8),
                                                    C.POINTER(C.c_double)]),
    "sesrq_add_const": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_int8), C.c_int, C.c_int, C.c_double, C.c_int,
                                  C.c_double, C.c_int, C.POINTER(C.c_int32)]),
    "sesrq_calib_scale_zero": (C.c_int, [C.c_double, C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "sesrq_last_error": (C.c_char_p, []),
    "sesrq_version": (C.c_int, []),
}


def bind(path: str, symbols: dict, who: str = "sesrq") -> C.CDLL:
    """Load the library at `path` and bind every symbol of `symbols` (name -> (restype, argtypes)); raise loudly when it is absent."""
    if not os.path.isfile(path):
        raise RuntimeError(f"{who}: native library not found at {path}. Build it with "
                           "`make -C sesr-pytorch-quantize_amd/csrc` (or __graft_entry__.build()); there is no fallback path.")
    # PyTorch-ROCm wheels bundle their own libamdhip64 (SONAME libamdhip64.so.7, needed by torch as
    # "libamdhip64.so").  Loading a library of ours first would pull /opt/rocm's copy in and torch would then
    # load a SECOND runtime; importing torch first makes the loader satisfy our NEEDED entry by SONAME
    # with the runtime torch already mapped -> one HIP runtime per process, shared streams/pointers.
    try:
        import torch  # noqa: F401
    except ImportError:  # standalone C/C++ use of the library: system runtime only
        pass
    handle = C.CDLL(path)
    for name, (res, args) in symbols.items():
        fn = getattr(handle, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    return handle


class Library:
    """One native library, loaded and bound on first use.  `prefix` names its C entry points: <prefix>_last_error, the launch
    counters <prefix>_<counters>_{count,name,launches} and, for the raw / image front ends, <prefix>_create of a device context."""

    def __init__(self, path: str, symbols: dict, who: str, prefix: str, counters: str = "instance"):
        self.path, self.symbols, self.who, self.prefix, self.counters = path, symbols, who, prefix, counters
        self._handle = None
        self._ctx = {}          # (device index, f32 scale bits, zero, exact_div) -> context handle; lives as long as the process

    def lib(self) -> C.CDLL:
        """The library, loaded once with every declared symbol bound; raises loudly when it is absent."""
        if self._handle is None:
            self._handle = bind(self.path, self.symbols, self.who)
        return self._handle

    def last_error(self) -> str:
        return (getattr(self.lib(), self.prefix + "_last_error")() or b"").decode()

    def instances(self):
        """{name: launches so far} of every kernel instantiation the library can launch."""
        l, p = self.lib(), f"{self.prefix}_{self.counters}"
        name, launches = getattr(l, p + "_name"), getattr(l, p + "_launches")
        return {name(i).decode(): int(launches(i)) for i in range(getattr(l, p + "_count")())}

    def context(self, device, scale_in, zero_in, exact_div):
        """The device context (<prefix>_create) of one input domain on `device`, created once."""
        import numpy as np
        import torch
        key = (device.index, np.float32(scale_in).tobytes(), int(zero_in), int(exact_div))
        h = self._ctx.get(key)
        if h is None:
            h, create = C.c_void_p(), getattr(self.lib(), self.prefix + "_create")
            with torch.cuda.device(device):
                if create(float(np.float32(scale_in)), int(zero_in), int(exact_div), C.byref(h)) != 0:
                    raise ValueError(self.last_error())
            self._ctx[key] = h
        return h


_core = Library(LIB_PATH, SYMBOLS, "sesrq", "sesrq")
lib, last_error, instances = _core.lib, _core.last_error, _core.instances


def narrow_instances():
    """{name: launches so far} of the width-aware kernels of ENGINE_MFMA_Q at quan_bits < 8: a list of their own."""
    l = lib()
    return {l.sesrq_narrow_instance_name(i).decode(): int(l.sesrq_narrow_instance_launches(i))
            for i in range(l.sesrq_narrow_instance_count())}


def qadd_instances():
    """{name: launches so far} of the calibration convs with the quantised long-skip merge: a list of their own."""
    l = lib()
    return {l.sesrq_qadd_instance_name(i).decode(): int(l.sesrq_qadd_instance_launches(i)) for i in range(l.sesrq_qadd_instance_count())}


def check(rc: int, exc=RuntimeError) -> None:
    if rc != 0:
        raise exc("sesrq: " + last_error())


def enter_stream(device, stream, *tensors):
    """The stream to launch on: the current stream of `device` when `stream` is None or is that stream.  Any other stream is
    ordered after the work already queued on the current stream (which may still be producing an input, or own the memory of
    freshly allocated outputs), and every tensor the launch touches (None entries are skipped) is recorded on it so that the
    caching allocator does not recycle it while the kernels run."""
    import torch
    cur = torch.cuda.current_stream(device)
    if stream is None or stream == cur:
        return cur
    stream.wait_stream(cur)
    for t in tensors:
        if t is not None:
            t.record_stream(stream)
    return stream


def host_tensor(a):
    """A numpy array as a torch tensor over its (contiguous) bytes; anything else as it is."""
    import numpy as np
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a


FACTORS = (2, 4)                    # what the chroma upscale of the colour and the video export takes
Y_F32, Y_I8 = 0, 1                  # SESRQ_COLOUR_F32 / _I8 = SESRQ_VIDEO_F32 / _I8: the luma dtype of both exports


def chroma_factor(r, what: str) -> int:
    """r of the `what` ("colour" / "video") export."""
    if r not in FACTORS:
        raise ValueError(f"scale factor {r!r}: the {what} export upscales chroma by 2 or 4")
    return int(r)


def luma_domain(y, shape, device, scale, zero, noun: str):
    """(scale, zero) an export passes on with the net's luma `y`: a tensor of `shape` = (N, 1, r H, r W) on the device of the LR `noun`
    ("image" / "surface"), fp32 -- (0.0, 0) -- or int8 with the net's output domain."""
    import torch
    if not isinstance(y, torch.Tensor) or tuple(y.shape) != tuple(shape):
        raise ValueError(f"export: the luma is a (N, 1, r H, r W) = {tuple(shape)} tensor, got "
                         f"{tuple(y.shape) if isinstance(y, torch.Tensor) else type(y).__name__}")
    if y.device != device:
        raise ValueError(f"export: the luma is on {y.device}, the {noun} on {device}")
    if y.dtype == torch.float32:
        return 0.0, 0
    if y.dtype != torch.int8:
        raise ValueError("export: the luma must be float32 or int8")
    if scale is None or zero is None:
        raise ValueError("export: an int8 luma needs the output domain: scale and zero")
    return scale, zero


def input_domain(engine_or_bundle, want_q: bool, who: str):
    """(bundle, scale_in, zero_in, exact_div, device) of a front end's q0 (raw.unpack, image.decode).  An Engine fixes all of them;
    a Bundle all but the device (None) and exact_div (0); None only allows the fp32 frame: (None, 1.0, 0, 0, None)."""
    from .bundle import Bundle
    if engine_or_bundle is None:          # the fp32 frame alone: no input domain involved
        if want_q:
            raise ValueError(f"{who}: q0 needs the net's input domain (an Engine or a Bundle)")
        return None, 1.0, 0, 0, None
    if isinstance(engine_or_bundle, Bundle):
        b, exact_div, dev = engine_or_bundle, 0, None
    else:
        b, exact_div, dev = engine_or_bundle.bundle, engine_or_bundle.exact_div, engine_or_bundle.device
    return b, b.scale[0], b.zero[0], exact_div, dev
