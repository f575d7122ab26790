"""Calibration entry point -- the counterpart of the reference's ``test.py`` (:79-113 graph build with
qmode = 0, :141-183 loop over calibration frames, :185-217 scale/zero derivation).  The reference's
dataset is private; frames come from ``--frames`` (.npy / .pt, (N,C,H,W) float32, one batch per N), or from ``--input``: what
sim.py reads -- 12-bit RGGB raw frames (``*.raw``, MFLAG 1 ... 4), 8-bit images (``.png``, or uint8 ``.npy`` with ``--image``; MFLAG
5 / 6) or fp32 ``.npy`` / ``.pt`` frames -- decoded on the device and calibrated frame by frame without a host round trip
(Calibrator.enqueue*), or from ``--hr``: 8-bit HR images alone, downscaled on the device.  With ``--gt`` every frame's mode-0 output is scored as the reference's loop scores it (each frame's PSNR, then
the mean line) before the domains are printed -- not for MFLAG 1 (nr), whose mosaic metric the scored loop does not have: ``--mflag 1``
calibrates without ``--gt``.

    python test.py --mflag 5 --params tests/golden/sesr_x4.params.npz --frames tests/golden/rand_SR_Input_80x960.npy \\
                   --save-bundle x4.bundle.npz
    python test.py --mflag 3 --params tests/golden/nrdm_3.params.npz --input a_132_128.raw b_132_128.raw --gt gt16.npy
    python test.py --mflag 6 --params ... --input lr0.png lr1.png --gt hr0.png hr1.png
    python test.py --mflag 3 --ckpt nrdm_3_qat_G.pth --input a_132_128.raw          # a QAT checkpoint: the long skip is its QuantAdd

A QAT checkpoint (``*_qat_G.pth``) decides for itself, as it does for the fold: quantize.prepare() puts a fake-quantising QuantAdd in
place of the long skip's add, and the pass merges the skip through it at the scale the checkpoint's observer state gives
(models/quantize_utils_pt.skip_quant_scale; one line names the scale used).  ``--params`` files carry no such state:
``--skip-quant-scale S`` gives it by hand, ``--float-skip`` forces the float add.
"""
import argparse
import types

import numpy as np
import torch

import define
from define import PE, BIAS_BIT, PE_ACC_BIT, PE_ADD_BIT
from myQL.quan_func import quantize_model_weight, quantize_asymmetrical_by_tensor, reshape_input_for_hardware_pe, PEs_and_bias_adder
from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
from myQL.graph_modify import insert_before, insert_bias_bypass
from sesrq.store import STORE
from sesrq.calibrate import finish_calibration
import sim


def splice_calibration(model):
    """The three graph rewrites of the reference's calibration script, qmode = 0 (test.py:79-106)."""
    qmode = 0
    model = quantize_model_weight(model, define.QUAN_BIT, qmode)
    mapping = NodeInsertMapping()
    quan = FunctionPackage(quantize_asymmetrical_by_tensor, {"width": define.QUAN_BIT, "exe_mode": qmode})
    mapping.add_config(NodeInsertMappingElement(torch.nn.Conv2d, quan))
    mapping.add_config(NodeInsertMappingElement(torch.nn.PixelShuffle, quan))
    model = insert_before(model_input=model, insert_mapping=mapping, has_func_id=True)
    m2 = NodeInsertMapping()
    m2.add_config(NodeInsertMappingElement(torch.nn.Conv2d, FunctionPackage(reshape_input_for_hardware_pe, {"pe_num": PE})))
    model = insert_before(model_input=model, insert_mapping=m2)
    m3 = NodeInsertMapping()
    m3.add_config(NodeInsertMappingElement(torch.nn.Conv2d, FunctionPackage(
        PEs_and_bias_adder, {"pe_add_width": PE_ADD_BIT, "pe_acc_width": PE_ACC_BIT, "bias_width": BIAS_BIT, "pe_num": PE,
                             "exe_mode": qmode})))
    return insert_bias_bypass(model_input=model, insert_mapping=m3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mflag", type=int, default=define.MFLAG)
    ap.add_argument("--ckpt")
    ap.add_argument("--params")
    ap.add_argument("--frames", help="(N,C,H,W) float32 frames, .npy / .pt: calibrated on the host-driven pass (without --gt)")
    ap.add_argument("--input", nargs="+", help="dataset frames as sim.py reads them: *.raw 12-bit RGGB frames <name>_<rows>_<cols>.raw "
                                              "(MFLAG 1 ... 4), 8-bit images .png (or uint8 .npy with --image; MFLAG 5 / 6), or fp32 "
                                              ".npy / .pt (N,C,H,W); calibrated on the device-resident pass")
    ap.add_argument("--gt", nargs="+", help="ground truths, one per --input file (or one batch .npy / .pt): score every frame's mode-0 "
                                           "output and print its PSNR and the mean line, as the reference's test.py does.  fp32 or "
                                           "uint16 RGB (N,3,H,W) .npy / .pt, or 8-bit HR images (.png, uint8 .npy with --image)")
    ap.add_argument("--hr", nargs="+", help="MFLAG 5 / 6, in place of --input and --gt: 8-bit HR images (.png, or uint8 .npy with --image), "
                                           "each both the ground truth and, downscaled bicubically by the net's factor on the device, "
                                           "the input (sesrq.downscale); calibrated on the device-resident pass and scored")
    ap.add_argument("--modcrop", action=argparse.BooleanOptionalAction, default=True,
                    help="crop every --hr image to multiples of 12 each way first (top left), as the datasets' GTmod12 folders were made")
    ap.add_argument("--image", action="store_true", help="--input / --gt .npy files are uint8 (H, W, 3) or (N, H, W, 3) images")
    ap.add_argument("--order", choices=("rgb", "bgr"), default="rgb", help="byte order of uint8 .npy images (PNGs are read as RGB)")
    ap.add_argument("--method", default="minmax", choices=["minmax", "entropy"],
                    help="minmax: the reference's running min/max (default); entropy: KL-minimising clipping ranges from a second "
                         "pass over the frames (no reference counterpart, parity unpinned)")
    ap.add_argument("--bins", type=int, default=2048, help="histogram bins of --method entropy")
    ap.add_argument("--save-bundle")
    ap.add_argument("--save-output-pt", help="directory to write input.K.{min_val,max_val,scale,zero}.pt like the reference")
    ap.add_argument("--quan-bit", type=int, default=None, help="define.py QUAN_BIT for this run (2..8; default: define.QUAN_BIT): "
                                                               "the width the activation domains are calibrated for")
    ap.add_argument("--engine", choices=("auto", "dot4", "mfma", "mfma-q"), default="auto",
                    help="kernel family (sesrq_options.engine) the calibrated net is created with once its domains are known: other than "
                         "auto, the net is built on the device and the kernels its layers resolve to are printed (mfma-q with --quan-bit "
                         "below 8: the width-aware MFMA kernels, what sim.py --engine mfma-q then runs)")
    ap.add_argument("--skip-quant-scale", type=float, default=None, metavar="S",
                    help="merge the long skip through the QAT nets' QuantAdd at scale S (positive, finite): for --params files, which "
                         "carry no QuantAdd state; a QAT --ckpt gives its own")
    ap.add_argument("--float-skip", action="store_true", help="add the long skip in float even for a QAT checkpoint")
    sim.add_sensor_flags(ap)
    sim.add_noise_flags(ap)
    args = ap.parse_args(argv)
    args.fmt = sim.sensor_format(args, "test.py", args.input)
    args.noise = sim.noise_model(args, "test.py", args.input)
    if args.quan_bit is not None:
        define.QUAN_BIT = args.quan_bit
    define.check()
    print("QUAN_BIT:", define.QUAN_BIT)
    STORE.clear()
    if args.hr is not None:
        if args.frames is not None or args.input is not None or args.gt is not None:
            raise SystemExit("test.py: --hr images are the inputs' source and the ground truths; give none of --frames, --input and --gt "
                             "with them")
    elif (args.frames is None) == (args.input is None):
        raise SystemExit("test.py: give the frames with --frames or with --input (one of them)")
    if args.float_skip and args.skip_quant_scale is not None:
        raise SystemExit("test.py: --float-skip and --skip-quant-scale exclude each other")
    if args.skip_quant_scale is not None and not (np.isfinite(args.skip_quant_scale) and args.skip_quant_scale > 0):
        raise SystemExit("test.py: --skip-quant-scale must be positive and finite")
    fmodel = sim.float_model(args.mflag, args.ckpt, args.params)
    skip_s = None if args.float_skip else args.skip_quant_scale if args.skip_quant_scale is not None else \
        fmodel.__dict__.get("sesrq_skip_quant_scale")
    if isinstance(skip_s, Exception):
        raise SystemExit(f"test.py: {skip_s}; give the scale with --skip-quant-scale or add the skip in float with --float-skip")
    if skip_s is not None:
        skip_s = float(np.float32(skip_s))
    print("skip_quant_scale:", skip_s if skip_s is not None else "none (float long skip)")
    model = splice_calibration(fmodel)
    model.__dict__["sesrq_skip_quant_scale"] = skip_s         # read by sesrq.lowering.lower_calibration
    if args.input is not None or args.gt is not None or args.hr is not None:
        return dataset_pass(args, model)
    frames = torch.load(args.frames, weights_only=True, map_location="cpu") if args.frames.endswith(".pt") else torch.from_numpy(np.load(args.frames))
    if not torch.cuda.is_available():
        raise SystemExit("test.py: calibration runs on a HIP device (no CPU fallback)")
    with torch.no_grad():
        for i in range(frames.shape[0]):
            model(frames[i:i + 1].float().cuda())
    print("calibrate start")
    cal = model._sesrq_cal
    if args.method == "entropy":
        cal.set_method("entropy", args.bins)
        cal.begin_histogram_pass()
        with torch.no_grad():
            for i in range(frames.shape[0]):
                model(frames[i:i + 1].float().cuda())
        scale, zero = cal.finalize()
        STORE.set_activation_domains(scale, zero)
    else:
        scale, zero = finish_calibration(STORE, cal.L)
    return report(args, model, scale, zero)


def report(args, model, scale, zero):
    for s, z in zip(scale, zero):
        print("scale:", s)
        print("zero:", z)
    print("calibrate end")
    print("bit:", define.QUAN_BIT)
    if args.save_output_pt:
        STORE.save_output_pt(args.save_output_pt)
    if args.save_bundle:
        model._sesrq_cal.bundle(name=f"mflag{args.mflag}").save(args.save_bundle)
    if args.engine != "auto":
        from sesrq import Engine, _lib
        cal = model._sesrq_cal
        print("engines:", Engine(cal.bundle(name=f"mflag{args.mflag}"), cal.device, engine=_lib.ENGINE_NAMES[args.engine]).layer_engines())
    return scale, zero


def _frames_of(a, image):
    """A file's frames: one frame, or a batch of them along a leading axis.  Images (H, W, 3) uint8; other frames (1, C, H, W)."""
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4:
        raise SystemExit(f"test.py: expected a frame or a batch of frames, got shape {a.shape}")
    return [a[i] if image else a[i:i + 1] for i in range(a.shape[0])]


def load_inputs(paths, image_flag, fmt=None):
    """(kind, [host frame]) of the --input files: "raw" (H, W) uint16, "image" (H, W, 3) uint8, "f32" (1, C, H, W) float32."""
    kinds = {"raw" if p.endswith(".raw") else "image" if sim.is_image(p, image_flag) else "f32" for p in paths}
    if len(kinds) != 1:
        raise SystemExit("test.py: --input files must all be of one kind (raw frames, images or fp32 frames)")
    kind = kinds.pop()
    frames = []
    for p in paths:
        if kind == "raw":
            from sesrq import sensor
            frames.append(sensor.load_raw(p, fmt))
        elif kind == "image":
            from sesrq import image
            frames += _frames_of(image.load_image(p), True)
        else:
            frames += [f.astype(np.float32) for f in _frames_of(sim.load_frames(p), False)]
    return kind, frames


def load_gts(paths, kind, image_flag):
    gts = []
    for p in paths:
        if sim.is_image(p, image_flag):
            from sesrq import image
            gts += _frames_of(image.load_image(p), True)
        else:
            gts += _frames_of(sim.load_frames(p), False)
    return gts


def dataset_pass(args, model):
    """--input / --gt: the reference's calibration loop (test.py:141-183) on the device-resident pass: every frame decoded and
    calibrated on the device, scored with --gt; one synchronisation at the end."""
    from sesrq import quality
    from sesrq.lowering import lower_calibration
    if args.method != "minmax":
        raise SystemExit("test.py: --input / --gt run the device-resident pass, which computes the reference's min/max ranges only; "
                         "use --frames for --method entropy")
    if args.hr is not None:
        from sesrq import downscale
        kind, frames = load_inputs(args.hr, args.image)
        try:
            if kind != "image":
                raise ValueError("--hr takes 8-bit HR images (.png, or uint8 .npy with --image)")
            kind, frames = "hr", [downscale.modcrop(f, 12) if args.modcrop else f for f in frames]
            for f in frames:       # the size refusal, before any device work
                downscale.hr_images(torch.from_numpy(np.ascontiguousarray(f)), downscale.factor_of(args.mflag), who="--hr")
        except ValueError as e:
            raise SystemExit(f"test.py: {e}") from None
    elif args.frames is not None:
        kind, frames = "f32", [f.astype(np.float32) for f in _frames_of(sim.load_frames(args.frames), False)]
    else:
        kind, frames = load_inputs(args.input, args.image, args.fmt)
    cin = next(m for m in model.modules() if isinstance(m, torch.nn.Conv2d)).in_channels
    try:       # the refusals of forward_raw / forward_image, before any device work
        quality.check_calibration_input(types.SimpleNamespace(in_channels=cin, method=args.method), args.mflag, kind,
                                        scored=args.gt is not None or args.hr is not None)
    except ValueError as e:
        raise SystemExit(f"test.py: {e}") from None
    gts = frames if kind == "hr" else load_gts(args.gt, kind, args.image) if args.gt else None
    if gts is not None and len(gts) != len(frames):
        raise SystemExit(f"test.py: {len(frames)} input frames, {len(gts)} ground truths")
    if not torch.cuda.is_available():
        raise SystemExit("test.py: calibration runs on a HIP device (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    cal = lower_calibration(model, dev)
    model.__dict__["_sesrq_cal"] = cal
    if gts is not None:
        res = quality.evaluate_calibration(cal, frames, gts, args.mflag, kind=kind, order=args.order, fmt=args.fmt, noise=args.noise)
        totalpsnr = totalssim = 0.0
        for _, psnr, ssim in res:
            print(float(psnr))
            totalpsnr += float(psnr)
            totalssim += float(ssim)
        print(quality.TASKS[args.mflag] + ' mean psnr is: ', totalpsnr / len(res), ' ssim is: ', totalssim / len(res))
    else:
        for i, f in enumerate(frames):
            t = torch.from_numpy(np.ascontiguousarray(f)).to(dev)
            if kind == "raw":          # --add-noise: frame i of the pass is frame i of the noise stream
                cal.enqueue_raw(t, fmt=args.fmt, noise=args.noise.advance(i) if args.noise is not None else None)
            elif kind == "image":
                cal.enqueue_image(t, order=args.order)
            else:
                cal.enqueue(t)
    cal.sync()
    for k in range(cal.L + 1):
        STORE[f"input/input.{k}.min_val"] = cal.run_min[k]
        STORE[f"input/input.{k}.max_val"] = cal.run_max[k]
        STORE[f"input/input.{k}.scale"] = cal.last_scale[k]
        STORE[f"input/input.{k}.zero"] = cal.last_zero[k]
    print("calibrate start")
    scale, zero = finish_calibration(STORE, cal.L)
    return report(args, model, scale, zero)


if __name__ == "__main__":
    main()
