"""PSNR / SSIM of output frames on the device: the reference's evaluation loop (test.py:141-183).

ctypes bindings of libsesrq_eval.so (C ABI declared in include/sesrq_eval.h) and libsesrq_mosaic.so (include/sesrq_mosaic.h),
``score()`` for a batch of frames already on the device, and ``evaluate()``: forward + score over a set of frames, one synchronisation at the end.  There is no CPU path: scoring
needs the device, as the forward does.

The metric form follows the network (MFLAG, reference sim.py ``MODELS``):
  1     nr                     MOSAIC skimage PSNR (data_range 1) and single-channel SSIM of three2one(pred), three2one(gt): the
                               Bayer mosaics, channel (row & 1) + (column & 1) of each pixel (libsesrq_mosaic.so)
  2     dm                     RGB   as 3, 4
  3, 4  nrdm_small / nrdm_big  RGB   skimage PSNR (data_range 1), SSIM = mean over the three channels
  5     srx4                   Y255  compute_psnr(255 gt, 255 pred) (eps 1e-8), single-channel SSIM
  6     srx2                   X2    compute_psnr(rgb_to_yuv(gt), rgb_to_yuv(pred)) on the anchored output, SSIM as RGB
The prediction is clipped to [0, 1] first; the ground truth is not.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_eval.so"))
MOSAIC_LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libsesrq_mosaic.so"))

FORM_RGB, FORM_Y255, FORM_X2 = 0, 1, 2
FORM_MOSAIC = 3                     # scored by libsesrq_mosaic.so: not a form of sesrq_eval
PRED_F32, PRED_I8 = 0, 1
FORMS = {1: FORM_MOSAIC, 2: FORM_RGB, 3: FORM_RGB, 4: FORM_RGB, 5: FORM_Y255, 6: FORM_X2}
CHANNELS = {FORM_RGB: 3, FORM_Y255: 1, FORM_X2: 3, FORM_MOSAIC: 3}
RAW_MFLAGS = (1, 2, 3, 4)           # the denoise / demosaic nets: what 12-bit RGGB raw frames feed
TASKS = {1: "nr", 2: "dm", 3: "nrdm_small", 4: "nrdm_big", 5: "srx4", 6: "srx2"}     # reference test.py:182


class EvalDesc(C.Structure):
    _fields_ = [("form", C.c_int32), ("pred_dtype", C.c_int32), ("pred_scale", C.c_float), ("pred_zero", C.c_int32)]


# every symbol include/sesrq_eval.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sesrq_eval_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sesrq_eval": (C.c_int, [C.POINTER(EvalDesc), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                             C.c_void_p, C.c_size_t, C.c_void_p]),
    "sesrq_eval_kernel_count": (C.c_int, []),
    "sesrq_eval_kernel_name": (C.c_char_p, [C.c_int]),
    "sesrq_eval_kernel_launches": (C.c_longlong, [C.c_int]),
    "sesrq_eval_last_error": (C.c_char_p, []),
}

# what include/sesrq_eval_anchor.h declares (the same library)
ANCHOR_SYMBOLS = {
    "sesrq_eval_anchored": (C.c_int, [C.POINTER(EvalDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

_so = _lib.Library(LIB_PATH, SYMBOLS, "sesrq.quality", "sesrq_eval", counters="kernel")
lib, last_error, kernels = _so.lib, _so.last_error, _so.instances


class MosaicDesc(C.Structure):
    _fields_ = [("pred_dtype", C.c_int32), ("pred_scale", C.c_float), ("pred_zero", C.c_int32)]


# every symbol include/sesrq_mosaic.h declares: name -> (restype, argtypes)
MOSAIC_SYMBOLS = {
    "sesrq_mosaic_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sesrq_mosaic_score": (C.c_int, [C.POINTER(MosaicDesc), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "sesrq_mosaic_kernel_count": (C.c_int, []),
    "sesrq_mosaic_kernel_name": (C.c_char_p, [C.c_int]),
    "sesrq_mosaic_kernel_launches": (C.c_longlong, [C.c_int]),
    "sesrq_mosaic_last_error": (C.c_char_p, []),
}

_mosaic_so = _lib.Library(MOSAIC_LIB_PATH, MOSAIC_SYMBOLS, "sesrq.quality", "sesrq_mosaic", counters="kernel")
mosaic_lib, mosaic_last_error, mosaic_kernels = _mosaic_so.lib, _mosaic_so.last_error, _mosaic_so.instances


_anchor_bound = False


def anchored_lib():
    """The library with the entry points of include/sesrq_eval_anchor.h bound too (once)."""
    global _anchor_bound
    h = lib()
    if not _anchor_bound:
        for name, (res, args) in ANCHOR_SYMBOLS.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        _anchor_bound = True
    return h


def form_of(mflag: int) -> int:
    if mflag not in FORMS:
        raise ValueError(f"MFLAG {mflag}: only 1 (nr, mosaic), 2, 3, 4 (RGB), 5 (srx4) and 6 (srx2) have a metric on the integer path")
    return FORMS[mflag]


def _check_pair(pred, gt, mflag: int, scale=None, zero=None):
    """The refusals every scorer shares: pred and gt are (N, C, H, W) tensors of one shape on one HIP device, of the MFLAG's channel
    count, at least one frame of at least 7x7, gt float32.  Returns ((N, C, H, W), (pred_dtype, pred_scale, pred_zero)); an int8
    prediction takes its domain from `scale` and `zero`."""
    import torch
    form = form_of(mflag)
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise ValueError("pred and gt must be torch tensors")
    if pred.dim() != 4 or tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must both be (N, C, H, W) of one shape")
    N, Ch, H, W = pred.shape
    if Ch != CHANNELS[form]:
        raise ValueError(f"MFLAG {mflag} scores {CHANNELS[form]}-channel frames, got {Ch}")
    if H < 7 or W < 7:
        raise ValueError(f"frame {H}x{W} is smaller than the 7x7 SSIM window")
    if N < 1:
        raise ValueError("no frames")
    if pred.device.type != "cuda" or gt.device != pred.device:
        raise ValueError(f"pred ({pred.device}) and gt ({gt.device}) must be on one HIP device")
    if gt.dtype != torch.float32:
        raise ValueError("gt must be float32")
    domain = PRED_F32, 0.0, 0
    if pred.dtype == torch.int8:
        if scale is None or zero is None:
            raise ValueError("an int8 prediction needs the output domain: scale and zero")
        if form == FORM_X2:
            raise ValueError("MFLAG 6 scores the anchored float output; the anchor does not exist in the int8 output")
        domain = PRED_I8, float(scale), int(zero)
    elif pred.dtype != torch.float32:
        raise ValueError("pred must be float32 or int8")
    return (N, Ch, H, W), domain


def _run(so, fn, desc, tensors, dims, stream):
    """Enqueue scorer `fn` of library `so` on `stream`: `tensors` (made contiguous) are its frames in the order of its arguments,
    `dims` its frame counts and sizes, which are also those of the library's workspace.  The (N, 3) float64 device result."""
    import torch
    dev = tensors[0].device
    with torch.cuda.device(dev):
        tensors = [t.contiguous() for t in tensors]
        out = torch.empty((dims[0], 3), dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, getattr(so.lib(), so.prefix + "_workspace_bytes")(*dims)), dtype=torch.uint8, device=dev)
        st = _lib.enter_stream(dev, stream, *tensors, out, ws)
        rc = fn(C.byref(desc), *(t.data_ptr() for t in tensors), *dims, out.data_ptr(), ws.data_ptr(), ws.numel(), st.cuda_stream)
    if rc != 0:
        raise ValueError(f"{fn.__name__}: " + so.last_error())
    return out


def score(pred, gt, mflag: int, scale=None, zero=None, stream=None):
    """(mse, psnr, ssim) per frame as a device float64 tensor of shape (N, 3), enqueued on `stream` (default: current), not synchronised.

    pred: (N, C, H, W) float32 output frames, or int8 output frames with the net's output domain (scale = f32(input.L.scale),
    zero = zero[L]), dequantised on the device to the bits of the float output; gt: float32 of the same shape and device.
    For MFLAG 6, pred is the anchored float output (Engine(..., anchor_add=True)).  MFLAG 1 scores the Bayer mosaics of the two
    3-channel frames (libsesrq_mosaic.so); mse is then the mosaic's, over H W."""
    (N, Ch, H, W), (dtype, pscale, pzero) = _check_pair(pred, gt, mflag, scale, zero)
    if FORMS[mflag] == FORM_MOSAIC:
        md = MosaicDesc(pred_dtype=dtype, pred_scale=pscale, pred_zero=pzero)
        return _run(_mosaic_so, mosaic_lib().sesrq_mosaic_score, md, (pred, gt), (N, H, W), stream)
    d = EvalDesc(form=FORMS[mflag], pred_dtype=dtype, pred_scale=pscale, pred_zero=pzero)
    return _run(_so, lib().sesrq_eval, d, (pred, gt), (N, Ch, H, W), stream)


def score_anchored(pred, lr, gt, stream=None):
    """MFLAG 6 scores of fl32(pred + up2(lr)) without forming that frame: pred (N, 3, 2H, 2W) float32 -- an output without the fused
    anchor, such as the calibration pass's mode-0 output --, lr (N, 3, H, W) float32, the net's input, gt (N, 3, 2H, 2W) float32, all on
    one device.  The bits of score(pred + up2(lr), gt, 6).  A device float64 (N, 3) tensor of (mse, psnr, ssim), not synchronised."""
    import torch
    for name, t in (("pred", pred), ("lr", lr)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a (N, C, H, W) float32 tensor")
    (N, Ch, H, W), _ = _check_pair(pred, gt, 6)
    if tuple(lr.shape) != (N, Ch, H // 2, W // 2) or H % 2 or W % 2:
        raise ValueError(f"lr {tuple(lr.shape)} is not the half-size input of a {tuple(pred.shape)} prediction")
    if lr.device != pred.device:
        raise ValueError("pred, lr and gt must be on one HIP device")
    d = EvalDesc(form=FORM_X2, pred_dtype=PRED_F32, pred_scale=0.0, pred_zero=0)
    return _run(_so, anchored_lib().sesrq_eval_anchored, d, (pred, lr, gt), (N, Ch, H, W), stream)


KINDS = ("f32", "raw", "image", "hr")


def check_mosaic_format(mflag: int, fmt):
    """The MFLAG 1 metric selects channel (r & 1) + (c & 1) of every pixel, which is the RGGB mosaic: with a sensor format of another
    CFA order it would score the wrong sites, so it is refused ("Not covered": a CFA-aware mosaic metric)."""
    if fmt is not None and mflag in FORMS and FORMS[mflag] == FORM_MOSAIC and fmt.cfa != "rggb":
        raise ValueError(f"MFLAG {mflag}: the mosaic metric scores the RGGB sites; a {fmt.cfa} frame cannot be scored with it")


def check_calibration_input(calibrator, mflag: int, kind: str, scored: bool = True):
    """The refusals of evaluate_calibration, before any device work: the input kind must fit the MFLAG (raw frames: 1 ... 4, images:
    5 / 6) and the net's input channels, and the calibrator must be on the min/max rule (the device pass has no entropy variant).
    The scored loop has no MFLAG 1 ("Not covered"); scored=False is the calibration pass alone (test.py without
    --gt), whose domains do not depend on the metric."""
    form_of(mflag)
    if scored and FORMS[mflag] == FORM_MOSAIC:
        raise ValueError(f"MFLAG {mflag}: the scored calibration loop has no mosaic form; calibrate without ground truths and score "
                         "the integer path's output (evaluate, evaluate_raw, sim.py --gt)")
    if kind not in KINDS:
        raise ValueError(f"kind {kind!r}: one of {KINDS}")
    cin = calibrator.in_channels
    if kind == "raw":
        if mflag not in RAW_MFLAGS:
            raise ValueError(f"MFLAG {mflag}: raw RGGB frames feed the denoise / demosaic nets (MFLAG 1, 2, 3, 4)")
        if cin != 3:
            raise ValueError(f"a raw RGGB frame feeds 3-channel nets; this one takes {cin}")
    if kind in ("image", "hr"):
        from . import image as imgmod
        f = imgmod.form_of(mflag)
        if imgmod.CHANNELS[imgmod._form(f)] != cin:
            raise ValueError(f"MFLAG {mflag} images give {imgmod.CHANNELS[imgmod._form(f)]} channel(s); this net takes {cin}")
    if kind == "hr":           # the HR image is the input's source: downscaled by the MFLAG's factor, which must be the net's
        from . import downscale
        r = getattr(calibrator, "pixel_shuffle", None)
        if r is not None and r != downscale.factor_of(mflag):
            raise ValueError(f"MFLAG {mflag} downscales the HR image by {downscale.factor_of(mflag)}; this net upscales by {r}")
    if calibrator.method != "minmax":
        raise ValueError("evaluate_calibration: the device-resident calibration pass computes the reference's min/max ranges only; "
                         "method='entropy' runs on the host pass (Calibrator.observe)")


def evaluate_calibration(calibrator, frames, gts, mflag: int, kind: str = "f32", order: str = "rgb", fmt=None, noise=None):
    """The reference's calibration loop (test.py:141-183) on the device: per frame the mode-0 forward (Calibrator.enqueue /
    enqueue_raw / enqueue_image, which also accumulates the running ranges) and the metrics of its output in the form the MFLAG uses
    -- MFLAG 6 the anchored output fl32(gfake + up2(inps)), formed inside the scoring kernel (score_anchored).  One synchronisation at
    the end; calibrator.finalize() then gives the activation domains.

    kind "f32": frames (1, Cin, H, W) float32 (or one (N, Cin, H, W) tensor, taken frame by frame); "raw": (1, 1, H, W) / (1, H, W) /
    (H, W) uint16 RGGB frames; "image": (H, W, 3) / (1, H, W, 3) uint8 LR images in `order`.  gts, numpy or torch, by dtype: float32
    frames of the output shape, uint16 RGB frames (3, H, W) / (1, 3, H, W) (sesrq.raw.load_gt), or uint8 HR images in `order`
    (sesrq.image.load_gt); "hr": (H, W, 3) / (1, H, W, 3) uint8 HR images in `order`, sizes multiples of the net's factor -- each is
    its own ground truth and the source of its input (Calibrator.enqueue_hr; the matching entry of gts is not read).
    fmt: the sesrq.sensor.Format of "raw" frames and uint16 ground truths (default: 12-bit RGGB, sesrq.raw).
    noise: a sesrq.noise.NoiseModel for "raw" frames -- shot and read noise added on the device, consecutive frames getting
    consecutive frame numbers from the model's frame0 (the reference's TEST_RAW_ADD_NOISE).
    Returns a host float64 array (frames, 3) of (mse, psnr, ssim)."""
    import torch
    check_calibration_input(calibrator, mflag, kind)
    if fmt is not None and kind != "raw":
        raise ValueError("a sensor format belongs to raw frames (kind='raw')")
    if noise is not None and kind != "raw":
        raise ValueError("noise belongs to raw frames (kind='raw')")
    done = 0             # raw frames so far
    dev = calibrator.device
    form = FORMS[mflag]
    rows = []
    for x, g in zip(frames, gts):
        x = _lib.host_tensor(x).to(dev, non_blocking=True)
        if kind == "f32":
            y = calibrator.enqueue(x.float() if x.dim() == 4 else x.float().unsqueeze(0))
        elif kind == "raw":
            if noise is None:
                y = calibrator.enqueue_raw(x, fmt=fmt)
            else:
                y = calibrator.enqueue_raw(x, fmt=fmt, noise=noise.advance(done))
                done += y.shape[0]
        elif kind == "hr":     # one upload: the HR image is downscaled and decoded on the device, and is the ground truth
            y = calibrator.enqueue_hr(x, order=order)
            g = x
        else:
            y = calibrator.enqueue_image(x, order=order)
        g = _lib.host_tensor(g)
        if g.dtype == torch.uint8:           # an 8-bit HR image: the reference's gt formed on the device
            from . import image as imgmod
            g = imgmod.load_gt(g, mflag, dev, order=order)
        elif g.dtype == torch.uint16:        # a 16-bit RGB frame: / 4095, clamped (self_dataset.py:235-243)
            from . import sensor
            g = sensor.load_gt(g, fmt, dev)
        else:
            g = (g if g.dim() == 4 else g.unsqueeze(0)).to(dev, dtype=torch.float32, non_blocking=True)
        rows.append(score_anchored(y, calibrator.last_input, g) if form == FORM_X2 else score(y, g, mflag))
    if not rows:
        raise ValueError("no frames")
    res = torch.cat(rows)
    torch.cuda.synchronize(dev)
    return res.cpu().numpy()


def _evaluate(engine, mflag: int, pairs, step):
    """The loop of evaluate, evaluate_raw and evaluate_image: per (input, gt) of `pairs`, step(input, gt, fp32) runs the forward and
    returns (prediction, device fp32 gt).  MFLAG 6 scores the anchored fp32 output (fp32 True), every other MFLAG the int8 output
    in the net's output domain (MFLAG 1: its Bayer mosaic).  One synchronisation at the end; a host float64 array (frames, 3) of (mse, psnr, ssim)."""
    import torch
    form = form_of(mflag)
    if form == FORM_X2 and not getattr(engine, "anchor_add", False):
        raise ValueError("MFLAG 6 is scored on the anchored output: create the engine with anchor_add=True")
    b = engine.bundle
    scale, zero = float(b.scale[b.L]), int(b.zero[b.L])
    rows = []
    for x, g in pairs:
        pred, gt = step(x, g, form == FORM_X2)
        rows.append(score(pred, gt, mflag) if form == FORM_X2 else score(pred, gt, mflag, scale=scale, zero=zero))
    if not rows:
        raise ValueError("no frames")
    res = torch.cat(rows)
    torch.cuda.synchronize(engine.device)
    return res.cpu().numpy()


def evaluate(engine, frames, gts, mflag: int):
    """The reference's dataset loop on the device: per frame a forward and its metrics; one synchronisation at the end.

    frames: iterable of (1, Cin, H, W) float32 input frames (or one (N, Cin, H, W) tensor, taken frame by frame); gts: the matching
    ground truths of the output shape.  MFLAG 1 ... 5: the forward writes only the int8 output, which is scored in the net's output
    domain (bundle.scale[L], bundle.zero[L]).  MFLAG 6: the forward writes only the anchored float output; the engine must have
    been created with anchor_add=True.  Returns a host float64 array (frames, 3) of (mse, psnr, ssim)."""
    import torch
    dev = engine.device

    def step(x, g, fp32):
        x = x if x.dim() == 4 else x.unsqueeze(0)
        g = g if g.dim() == 4 else g.unsqueeze(0)
        x, g = x.to(dev, non_blocking=True), g.to(dev, dtype=torch.float32, non_blocking=True)
        q, y = engine.forward(x, want_q=not fp32, want_f=fp32)
        return (y if fp32 else q), g
    return _evaluate(engine, mflag, zip(frames, gts), step)


def evaluate_raw(engine, raws, gts_u16, mflag: int, fmt=None, noise=None):
    """The reference's MFLAG 1 ... 4 loop from raw frames to scores (test.py:30-55 with self_dataset.py TestDataset): per frame the
    12-bit RGGB raw frame is unpacked on the device into the net's q0 and run forward (Engine.forward_raw), its 16-bit RGB ground
    truth is mapped to / 4095 and clamped on the device (sesrq.raw.load_gt), and the int8 output is scored as evaluate() scores it.

    raws: iterable of (1, 1, H, W) / (1, H, W) / (H, W) uint16 frames (numpy or torch; uploaded at 2 B/px), or one (N, 1, H, W)
    tensor taken frame by frame; gts_u16: the matching (3, H, W) / (1, 3, H, W) uint16 RGB frames.  One synchronisation at the end;
    returns a host float64 array (frames, 3) of (mse, psnr, ssim).

    fmt: a sesrq.sensor.Format -- the frames are unpadded frames of that sensor format (uint16, or uint8 rows of RAW10 / RAW12) and the
    ground truths are mapped with its levels.  MFLAG 1 scores the RGGB mosaic and refuses every other CFA order.

    noise: a sesrq.noise.NoiseModel -- the frames are clean and the model's shot and read noise is added on the device (the reference's
    TEST_RAW_ADD_NOISE).  The pass's first frame is the model's frame0 and consecutive frames get consecutive frame numbers, so the
    scores follow from the model alone, whatever the batch split."""
    from . import sensor
    form_of(mflag)
    if mflag not in RAW_MFLAGS:
        raise ValueError(f"MFLAG {mflag}: raw RGGB frames feed the denoise / demosaic nets (MFLAG 1, 2, 3, 4)")
    check_mosaic_format(mflag, fmt)
    dev = engine.device
    if noise is not None:
        from . import noise as noisemod
        noisemod._model(noise)
    done = [0]           # frames so far

    def step(r, g, fp32):
        if noise is None:
            q, _ = engine.forward_raw(_lib.host_tensor(r).to(dev, non_blocking=True), want_q=True, want_f=False, fmt=fmt)
        else:
            q, _ = engine.forward_raw(_lib.host_tensor(r).to(dev, non_blocking=True), want_q=True, want_f=False, fmt=fmt,
                                      noise=noise.advance(done[0]))
            done[0] += q.shape[0]
        return q, sensor.load_gt(g, fmt, dev)
    return _evaluate(engine, mflag, zip(raws, gts_u16), step)


def evaluate_image(engine, lr_imgs, hr_imgs, mflag: int, order: str = "rgb"):
    """The reference's MFLAG 5 / 6 loop from 8-bit images to scores (self_dataset_sr.py TestDataset): per frame the uint8 LR image is
    uploaded at 3 B/px, decoded on the device and run forward (Engine.forward_image), its uint8 HR image is decoded into the
    reference's fp32 gt (sesrq.image.load_gt), and the output is scored as evaluate() scores it -- MFLAG 5 the int8 output, MFLAG 6
    the anchored fp32 output (the engine must have been created with anchor_add=True).

    lr_imgs / hr_imgs: iterables of (H, W, 3) / (1, H, W, 3) uint8 images (numpy or torch), in `order`.  One synchronisation at the
    end; returns a host float64 array (frames, 3) of (mse, psnr, ssim)."""
    from . import image as imgmod
    form_of(mflag)
    imgmod.form_of(mflag)
    dev = engine.device

    def step(lr, hr, fp32):
        lr = _lib.host_tensor(lr).to(dev, non_blocking=True)
        g = imgmod.load_gt(hr, mflag, dev, order=order)
        q, y = engine.forward_image(lr, order=order, want_q=not fp32, want_f=fp32)
        return (y if fp32 else q), g
    return _evaluate(engine, mflag, zip(lr_imgs, hr_imgs), step)


def evaluate_video(engine, lr_surfaces, hr_surfaces, mflag: int = 5):
    """evaluate_image for YUV 4:2:0 video (sesrq.video): per LR Surface (a frame or a batch, host or device) its Y plane is uploaded
    with the surface at 1.5 B/px, decoded on the device into the net's q0 and run forward from int8; the ground truth is the HR
    Surface's Y plane decoded to fp32 by the same per-code table, and the int8 output is scored as evaluate() scores it.  The luma
    net only (MFLAG 5).  One synchronisation at the end; returns a host float64 array (frames, 3) of (mse, psnr, ssim)."""
    from . import video
    if mflag != 5:
        raise ValueError(f"MFLAG {mflag}: video surfaces feed the luma net (MFLAG 5: SESR-x4, Y in, Y out); MFLAG 6 is "
                         "evaluate_video_rgb's")
    dev = engine.device

    def step(lr, hr, fp32):
        q0, _ = video.decode(engine, video.to_device(lr, dev))
        _, g = video.decode(None, video.to_device(hr, dev), want_q=False, want_f=True)
        q, _ = engine.forward(q0, want_q=True, want_f=False)
        return q, g
    return _evaluate(engine, mflag, zip(lr_surfaces, hr_surfaces), step)


def evaluate_video_rgb(engine, lr_surfaces, hr_surfaces, mflag: int = 6):
    """evaluate_image for YUV 4:2:0 video into the RGB net (sesrq.video_rgb): per LR Surface (a frame or a batch, host or device)
    the surface is uploaded at 1.5 B/px, decoded on the device into the net's input and run forward (the fp32 frame and the anchored
    fp32 output: the engine must have been created with anchor_add=True); the ground truth is the HR Surface decoded to fp32 RGB by
    the same decode, and the output is scored as evaluate_image scores MFLAG 6.  One synchronisation at the end; returns a host
    float64 array (frames, 3) of (mse, psnr, ssim)."""
    from . import video_rgb
    if mflag != 6:
        raise ValueError(f"MFLAG {mflag}: the RGB video route feeds the RGB net (MFLAG 6: SESR-x2); MFLAG 5 is evaluate_video's")
    if engine.bundle.in_channels != 3:
        raise ValueError(f"MFLAG 6 takes an RGB net (3 channels in); this net takes {engine.bundle.in_channels}")
    dev = engine.device

    def step(lr, hr, fp32):
        _, x = video_rgb.decode(None, video_rgb.to_device(lr, dev), want_q=False, want_f=True)
        _, g = video_rgb.decode(None, video_rgb.to_device(hr, dev), want_q=False, want_f=True)
        _, y = engine.forward(x, want_q=False, want_f=True)
        return y, g
    return _evaluate(engine, mflag, zip(lr_surfaces, hr_surfaces), step)


def evaluate_hr(engine, hr_imgs, mflag: int, order: str = "rgb"):
    """evaluate_image without the LR files: per frame ONE upload, the uint8 HR image, which is both the ground truth
    (sesrq.image.load_gt) and, downscaled bicubically by the net's factor and decoded in one kernel, the input
    (Engine.forward_hr, sesrq.downscale); the output is scored as evaluate_image scores it -- MFLAG 5 the int8 output, MFLAG 6 the
    anchored fp32 output (the engine must have been created with anchor_add=True).

    hr_imgs: an iterable of (H, W, 3) / (1, H, W, 3) uint8 images (numpy or torch), in `order`, H and W multiples of the factor
    (sesrq.downscale.modcrop).  One synchronisation at the end; returns a host float64 array (frames, 3) of (mse, psnr, ssim)."""
    from . import downscale, image as imgmod
    form_of(mflag)
    imgmod.form_of(mflag)
    r = downscale.factor_of(mflag)
    if engine.bundle.pixel_shuffle != r:
        raise ValueError(f"MFLAG {mflag} downscales the HR image by {r}; this net upscales by {engine.bundle.pixel_shuffle}")
    dev = engine.device

    def step(hr, _, fp32):
        hr = _lib.host_tensor(hr).to(dev, non_blocking=True)
        q, y = engine.forward_hr(hr, order=order, want_q=not fp32, want_f=fp32)
        return (y if fp32 else q), imgmod.load_gt(hr, mflag, dev, order=order)
    return _evaluate(engine, mflag, ((h, None) for h in hr_imgs), step)
