"""Integer-inference entry point -- the counterpart of the reference's ``sim.py``.

Behaviour reproduced (reference sim.py:29-114, :197-213): pick the network by ``define.MFLAG``
(1 = nr, 2 = dm, 3 = nrdm_3, 5 = SESR x4, 6 = SESR x2), load float weights, ``collapse()``, quantise the weights
(mode 1), splice the four stage callables around every conv in the reference's order, run ONE
forward on the frame and print the bit-width banner.  Here the forward is a single fused device
call; activation domains (input.K.scale / input.K.zero) come from a calibration the reference's
test.py produced (an ``output_pt`` directory) or from a bundle/fixture file.

    python sim.py --mflag 5 --ckpt x4sesr.pth --calib output_pt --input rand_SR_Input_80x960.pt
    python sim.py --mflag 5 --params tests/golden/sesr_x4.params.npz --input tests/golden/rand_SR_Input_80x960.npy
    python sim.py --mflag 6 --params ... --input LR.png --gt HR.png --save-png SR.png      # 8-bit images (MFLAG 5 / 6)
    python sim.py --mflag 5 --params ... --input LR.png --colour --save-png SR.png         # the x4 luma net's output in colour
    python sim.py --mflag 6 --params ... --hr HR.png --save-lr LR.png                      # the HR image alone: input and ground truth
    python sim.py --mflag 5 --params ... --yuv LR.yuv --size 960x540 --pix-fmt nv12 --save-yuv SR.yuv     # YUV 4:2:0 video in and out
    python sim.py --mflag 6 --params ... --yuv LR.yuv --size 1920x1080 --pix-fmt nv12 --save-yuv SR.yuv   # ... of the RGB net (YCbCr <-> RGB)
    python sim.py --mflag 1 --ckpt nr_G.pth --calib output_pt --input a_132_128.raw --gt gt16.npy     # nr: scored on the Bayer mosaic
    python sim.py --mflag 3 --params ... --input a_132_128.raw --develop --colormatrix ... --red-gain 2.1 --blue-gain 1.6 --save-png OUT.png
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

import define
from define import QUAN_BIT, PE, BIAS_BIT, PE_ACC_BIT, PE_ADD_BIT, REQUAN_BIT, REQUAN_N_MAX
from myQL.quan_func import (quantize_model_weight, quantize_asymmetrical_by_tensor, reshape_input_for_hardware_pe,
                            PEs_and_bias_adder, requan_conv2d_output)
from myQL.quan_classes import NodeInsertMapping, FunctionPackage, NodeInsertMappingElement
from myQL.graph_modify import insert_before, insert_bias_bypass, insert_after
from models import sesr_sim, nrdm_3_sim, sesr_arch_sim, nrdm_6, nr, dm
from models import quantize_utils_pt as quantize
from sesrq.store import STORE

# MFLAG -> net, as the reference's test_float.py:25-48 numbers them.  4 (nrdm_6, 8 convs) has no integer path in the
# reference: roles generalise by position here, parity unpinned.  1 (nr) and 2 (dm) have the class body of nrdm_3: their
# integer net is the nrdm_3_sim graph with that task's weights and domains.
MODELS = {1: nr.nr, 2: dm.dm, 3: nrdm_3_sim.nr, 4: nrdm_6.nr, 5: sesr_sim.sesr, 6: sesr_arch_sim.sesr}


def float_model(mflag, ckpt=None, params=None):
    """Float net, collapsed.  ckpt: a reference state_dict (.pth, loaded with weights_only=True);
    params: an .npz holding already-collapsed convs Wf{k}/bf{k} (tests/golden/*.params.npz)."""
    if mflag not in MODELS:
        raise ValueError(f"MFLAG {mflag}: only 1 (nr), 2 (dm), 3 (nrdm_3), 4 (nrdm_6), 5 (SESR x4) and 6 (SESR x2) have an integer path")
    model = MODELS[mflag]()
    model.train()
    skip_s = load_checkpoint(model, ckpt, mflag) if ckpt is not None else None
    model.collapse()
    # a QAT checkpoint's QuantAdd scale, for the calibration pass (test.py); the integer path does not read it
    model.__dict__["sesrq_skip_quant_scale"] = skip_s
    if params is not None:
        z = np.load(params, allow_pickle=False)
        convs = [model.conv_first.conv_expand] + [b.conv_expand for b in model.residual_block] + [model.conv_last.conv_expand]
        with torch.no_grad():
            for k, c in enumerate(convs):
                c.weight.copy_(torch.from_numpy(z[f"Wf{k}"]))
                c.bias.copy_(torch.from_numpy(z[f"bf{k}"]))
        meta = json.loads(str(z["meta"]))
        if "scale" in meta:
            STORE.set_activation_domains(meta["scale"], meta["zero"])
    return model


QAT_SKIP_ADDS = ("add_residual.", "add_upsampled_input.")


def load_checkpoint(model, ckpt, mflag):
    """Load a reference checkpoint into the collapsible net -- strictly.

    A ``*_qat_G.pth`` (it carries ``*_quantizer.*`` entries) is only meaningful after ``quantize.prepare()`` has wrapped
    every conv in a fake-quantising conv (reference sim.py:64-66): ``collapse()`` then folds THROUGH the quantisers, and
    the folded weights differ from a fold of the raw conv weights by tens to hundreds of INT8 weights per net.  The
    reference selects this with its ``qatf`` switch; here the checkpoint itself decides (models/quantize_utils_pt.py).
    Entries of the two long-skip adds' quantisers (``add_residual.*``, ``add_upsampled_input.*``: QuantAdd state) are
    dropped: the integer path merges the skip in the integer domain and never evaluates them.  Returns the constant scale of
    ``add_residual``'s QuantAdd (quantize.skip_quant_scale; None for a checkpoint without one), which the calibration pass
    of a QAT net needs (test.py); for an incomplete observer state the ValueError of skip_quant_scale is returned in its
    place, not raised -- the integer path has no use for the scale and loads such a checkpoint as before, test.py raises it
    when it needs the scale.  Any other key mismatch (a checkpoint of another net / --mflag) is refused -- nothing may leave
    random-init weights behind."""
    sd = torch.load(ckpt, weights_only=True, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"{ckpt}: not a state_dict")
    try:
        skip_s = quantize.skip_quant_scale(sd)
    except ValueError as e:     # an incomplete QuantAdd state: no obstacle here, the integer path never evaluates it
        skip_s = e
    if quantize.is_qat_state_dict(sd):
        quantize.prepare(model, inplace=True, a_bits=QUAN_BIT, w_bits=QUAN_BIT, q_type=0, q_level="C")
        sd = {k: v for k, v in sd.items() if not k.startswith(QAT_SKIP_ADDS)}
    try:
        res = model.load_state_dict(sd, strict=False)
    except RuntimeError as e:           # tensor shape mismatch
        raise ValueError(f"{ckpt} does not fit the MFLAG {mflag} net ({type(model).__module__}): {e}") from None
    if res.missing_keys or res.unexpected_keys:
        raise ValueError(f"{ckpt} does not fit the MFLAG {mflag} net ({type(model).__module__}): missing "
                         f"{res.missing_keys[:3]}{'...' if len(res.missing_keys) > 3 else ''}, unexpected "
                         f"{res.unexpected_keys[:3]}{'...' if len(res.unexpected_keys) > 3 else ''}")
    return skip_s


def splice(model, qmode=1):
    """The four graph rewrites of the reference, in the reference's order (sim.py:85-114)."""
    model = quantize_model_weight(model, define.QUAN_BIT, qmode)

    def one(fn, kw):
        m = NodeInsertMapping()
        m.add_config(NodeInsertMappingElement(torch.nn.Conv2d, FunctionPackage(fn, kw)))
        return m
    model = insert_before(model_input=model, insert_mapping=one(quantize_asymmetrical_by_tensor, {"width": define.QUAN_BIT, "exe_mode": qmode}),
                          has_func_id=True)
    model = insert_before(model_input=model, insert_mapping=one(reshape_input_for_hardware_pe, {"pe_num": PE}))
    model = insert_after(model_input=model, insert_mapping=one(requan_conv2d_output, {"exe_mode": qmode}))
    model = insert_bias_bypass(model_input=model, insert_mapping=one(
        PEs_and_bias_adder, {"pe_add_width": PE_ADD_BIT, "pe_acc_width": PE_ACC_BIT, "bias_width": BIAS_BIT, "pe_num": PE,
                             "exe_mode": qmode}))
    return model


def banner(mflag):
    print("SIM_mflag:", mflag)
    print("QUAN_BIT:", define.QUAN_BIT)
    print("BIAS_BIT:", BIAS_BIT)
    print("PE_ACC_BIT:", PE_ACC_BIT)
    print("PE_ADD_BIT:", PE_ADD_BIT)
    print("REQUAN_BIT:", REQUAN_BIT)
    print("REQUAN_N_MAX:", REQUAN_N_MAX)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mflag", type=int, default=define.MFLAG)
    ap.add_argument("--ckpt", help="reference float checkpoint (.pth state_dict)")
    ap.add_argument("--params", help=".npz with collapsed float convs (+ calibrated domains)")
    ap.add_argument("--calib", help="output_pt directory written by the reference's test.py")
    ap.add_argument("--input", help="frame tensor: .pt (torch) or .npy, shape (N,C,H,W) float32; or a 12-bit RGGB raw frame "
                                                   "<name>_<rows>_<cols>.raw (uint16), spread on the device into the reference's "
                                                   "3-channel input (self_dataset.py TestDataset); or an 8-bit LR image (.png, or a "
                                                   "uint8 .npy with --image), decoded on the device as self_dataset_sr.py does "
                                                   "(MFLAG 5: luma, 6: RGB)")
    ap.add_argument("--image", action="store_true", help="--input / --gt .npy files are uint8 (H, W, 3) or (N, H, W, 3) images, taken "
                                                         "as *.png inputs are (MFLAG 5 / 6)")
    ap.add_argument("--order", choices=("rgb", "bgr"), default="rgb", help="byte order of uint8 .npy images (PNGs are read as RGB)")
    ap.add_argument("--save-png", help="write the output as an 8-bit PNG here (the reference's export: clip to [0, 1], * 255, "
                                       "truncate; MFLAG 6 the anchored output); frame k of a batch goes to <stem>_<k>.png")
    ap.add_argument("--colour", action="store_true", help="MFLAG 5 with an 8-bit LR image and --save-png: write the COLOUR image -- the "
                                                          "net's luma, the LR image's Cb / Cr upscaled bicubically, back to RGB "
                                                          "(sesrq.colour); without the flag the PNG is the grey luma, as the reference's")
    ap.add_argument("--hr", help="MFLAG 5 / 6, in place of --input and --gt: an 8-bit HR image (.png, or a uint8 .npy with --image) that is "
                                 "both the ground truth and, downscaled bicubically by the net's factor on the device, the input "
                                 "(sesrq.downscale); the output is scored against it")
    ap.add_argument("--modcrop", action=argparse.BooleanOptionalAction, default=True,
                    help="crop the --hr image to multiples of 12 each way first (top left), as the datasets' GTmod12 folders were made "
                         "(the default; --no-modcrop takes it as it is, its size must then be a multiple of the factor)")
    ap.add_argument("--save-lr", help="with --hr: write the device-made LR image as an 8-bit PNG here")
    ap.add_argument("--save", help="write the float result here (.npy)")
    ap.add_argument("--gt", help="ground truth of the output shape (N,Cout,H*r,W*r) float32, .npy or .pt: score the output with the "
                                 "reference's PSNR / SSIM on the device (test.py:141-183) and print them as its loop does; a uint16 "
                                 "(N,3,H,W) RGB ground truth is taken / 4095 and clamped, as the reference's TestDataset does (at --black / --white with those levels); an "
                                 "8-bit HR image (.png, or a uint8 .npy with --image) is formed as self_dataset_sr.py forms its gt")
    ap.add_argument("--dump", help="write the parameter store as an output_pt-compatible tree here (what the define.py *_W_FLG "
                                   "switches select, plus weights and activation domains); all dump switches are turned on")
    ap.add_argument("--quan-bit", type=int, default=None, help="define.py QUAN_BIT for this run (2..8; default: define.QUAN_BIT): "
                                                               "the width of weights and activations")
    ap.add_argument("--engine", choices=("auto", "dot4", "mfma", "mfma-q"), default="auto",
                    help="kernel family of the integer path (sesrq_options.engine).  With --quan-bit below 8, auto, dot4 and mfma run the "
                         "dot4 kernels; mfma-q runs the width-aware MFMA kernels and the fused trio (same bits, several times the rate)")
    add_sensor_flags(ap)
    add_noise_flags(ap)
    add_video_flags(ap)
    add_develop_flags(ap)
    args = ap.parse_args(argv)
    profile = develop_profile(ap, args)
    yuv = video_args(args)
    if yuv is not None:                     # --yuv stands in place of --input / --hr (video_args has refused them beside it)
        if args.save_lr:
            raise SystemExit("sim.py: --save-lr writes the LR image made from --hr")
    elif args.hr is None:
        if args.input is None:
            ap.error("the following arguments are required: --input")
        if args.save_lr:
            raise SystemExit("sim.py: --save-lr writes the LR image made from --hr")
    else:
        if args.input is not None or args.gt is not None:
            raise SystemExit("sim.py: --hr is the input's source and the ground truth; give neither --input nor --gt with it")
        if args.mflag not in (5, 6) or not is_image(args.hr, args.image):
            raise SystemExit("sim.py: --hr takes an 8-bit HR image (.png, or a uint8 .npy with --image) for the super-resolution nets "
                             "(--mflag 5 or 6)")
    fmt = sensor_format(args, "sim.py", [args.input] if args.input else [])
    noise_m = noise_model(args, "sim.py", [args.input] if args.input else [])
    if fmt is not None and args.gt:
        from sesrq import quality
        try:
            quality.check_mosaic_format(args.mflag, fmt)
        except ValueError as e:
            raise SystemExit(str(e)) from None
    if args.quan_bit is not None:
        define.QUAN_BIT = args.quan_bit
    define.check()
    if args.dump:
        for n in ("WEIGHT_W_FLG", "INPUT_W_FLG", "BIAS_W_FLG", "BIAS_QUAN_W_FLG", "OUTPUT_PE_W_FLG", "OUTPUT_PE_ADD_W_FLG", "REQUAN_FACTOR_W_FLG"):
            setattr(define, n, True)
    if args.calib:
        STORE.load_output_pt(args.calib)
    model = splice(float_model(args.mflag, args.ckpt, args.params))
    from sesrq import _lib
    model.__dict__["sesrq_engine_option"] = _lib.ENGINE_NAMES[args.engine]
    if yuv is not None:                     # a raw .yuv sequence: decoded, run and exported batch by batch
        if not torch.cuda.is_available():
            raise SystemExit("sim.py: the integer path needs a HIP device (no CPU fallback)")
        return run_yuv(args, yuv, model, keep=argv is not None)
    as_image = args.hr is not None or is_image(args.input, args.image)
    if args.colour and not (args.mflag == 5 and as_image and args.save_png):
        raise SystemExit("sim.py: --colour rebuilds colour around the luma net: it needs --mflag 5, an 8-bit LR image as --input "
                         "(.png, or a uint8 .npy with --image) and --save-png")
    lr_u8 = hr_u8 = None
    if not as_image and not args.input.endswith(".raw"):
        inps = torch.load(args.input, weights_only=True, map_location="cpu") if args.input.endswith(".pt") else \
            torch.from_numpy(np.load(args.input))
    if not torch.cuda.is_available():
        raise SystemExit("sim.py: the integer path needs a HIP device (no CPU fallback)")
    if args.hr is not None:                 # the HR image alone: its bicubic downscale, decoded in the same kernel -> model(inps)
        from sesrq import downscale, image
        r = downscale.factor_of(args.mflag)
        hr = image.load_image(args.hr)
        try:
            hr_u8 = torch.from_numpy(np.ascontiguousarray(downscale.modcrop(hr, 12) if args.modcrop else hr)).cuda()
            _, inps = downscale.decode(None, hr_u8, r, image.form_of(args.mflag), order=args.order, want_q=False, want_f=True)
            if args.colour or args.save_lr:
                lr_u8 = downscale.downscale(hr_u8, r, order=args.order)
        except ValueError as e:
            raise SystemExit(f"sim.py: {e}") from None
    elif args.input.endswith(".raw"):       # the reference's loop: raw frame -> sparse RGGB mosaic / 4095, clamped -> model(inps)
        from sesrq import sensor           # fmt: a sensor's format (CFA order, levels, MIPI packing), or None for the reference's
        raw = torch.from_numpy(sensor.load_raw(args.input, fmt)).cuda()
        if noise_m is None:
            _, inps = sensor.unpack(None, raw, fmt, want_q=False, want_spread=True)
        else:                               # TEST_RAW_ADD_NOISE: shot and read noise added while the frame is unpacked
            from sesrq import noise
            _, inps = noise.apply(None, raw, fmt, noise_m, want_q=False, want_spread=True)
    elif as_image:                          # self_dataset_sr.py: uint8 LR image / 255 (MFLAG 5: the float64 luma) -> model(inps)
        from sesrq import image
        form = image.form_of(args.mflag)
        lr_u8 = torch.from_numpy(image.load_image(args.input)).cuda()
        _, inps = image.decode(None, lr_u8, form, order=args.order, want_q=False, want_f=True)
    gfake = model(inps.float().cuda())
    torch.cuda.synchronize()
    banner(args.mflag)
    print("output:", tuple(gfake.shape), "engines:", model._sesrq_engine(gfake.device).layer_engines())
    if args.save:
        np.save(args.save, gfake.cpu().numpy())
    if args.dump:
        STORE.save_output_pt(args.dump)
        print("dumped:", args.dump)
    if args.hr is not None:
        from sesrq import image
        score_against(args.hr, gfake, inps, args.mflag, gts=image.load_gt(hr_u8, args.mflag, gfake.device, order=args.order))
        if args.save_lr:
            save_lr_png(args.save_lr, lr_u8, args.order)
    if args.gt:
        gts = None
        if is_image(args.gt, args.image):   # the HR image: the reference's gt formed on the device
            from sesrq import image
            gts = image.load_gt(image.load_image(args.gt), args.mflag, gfake.device, order=args.order)
        score_against(args.gt, gfake, inps, args.mflag, gts=gts, fmt=fmt)
    if args.save_png and args.colour:
        save_colour_png(args.save_png, gfake, lr_u8, args.order)
    elif args.save_png and profile is not None:
        save_develop_png(args.save_png, gfake, profile, args.order)
    elif args.save_png:
        save_png(args.save_png, gfake, inps, args.mflag)
    return gfake


def add_sensor_flags(ap):
    """--cfa / --black / --white / --packing: the sensor format of *.raw inputs (sesrq.sensor.Format).  Without any of them a raw
    frame is the reference's dataset format (uint16, RGGB, black 0, white 4095) and takes the route it always took."""
    ap.add_argument("--cfa", choices=("rggb", "grbg", "gbrg", "bggr"), default=None, help="CFA order of *.raw inputs (default rggb)")
    ap.add_argument("--black", type=int, default=None, help="black level of *.raw inputs (default 0)")
    ap.add_argument("--white", type=int, default=None, help="white level of *.raw inputs and uint16 ground truths (default 4095)")
    ap.add_argument("--packing", choices=("u16", "raw10", "raw12"), default=None,
                    help="how *.raw inputs hold their pixels: uint16 containers (default), MIPI RAW10 (4 px in 5 bytes) or RAW12 "
                         "(2 px in 3 bytes); a file is <rows> x the unpadded row bytes")


def add_develop_flags(ap):
    """--develop / --wb / --ccm / --colormatrix / --red-gain / --blue-gain / --rgb-gain / --curve: the display image of a raw net's
    linear camera-RGB output (sesrq.develop)."""
    nine = lambda s: [float(v) for v in s.replace(",", " ").split()]
    ap.add_argument("--develop", action="store_true", help="MFLAG 2 / 3 / 4 with a *.raw input and --save-png: write the DEVELOPED image -- "
                                                           "white-balance gains, colour-correction matrix, tone curve (sesrq.develop); "
                                                           "without the flag the PNG is the linear camera RGB, as the reference's")
    ap.add_argument("--wb", metavar="R,G,B", type=nine, default=None, help="with --develop: the three gains (default 1,1,1)")
    ap.add_argument("--ccm", metavar="M", type=float, nargs=9, default=None,
                    help="with --develop: the colour-correction matrix (camera RGB -> display RGB), nine numbers row by row (default: "
                         "the identity)")
    ap.add_argument("--colormatrix", metavar="M", type=float, nargs=9, default=None,
                    help="with --develop, in place of --ccm and --wb: the camera's xyz2cam matrix, nine numbers row by row, turned into "
                         "cam2rgb as the reference's metadata2tensor does; gains from --red-gain, --blue-gain and --rgb-gain")
    ap.add_argument("--red-gain", type=float, default=None, help="with --colormatrix: the red white-balance gain (default 1)")
    ap.add_argument("--blue-gain", type=float, default=None, help="with --colormatrix: the blue white-balance gain (default 1)")
    ap.add_argument("--rgb-gain", type=float, default=None, help="with --colormatrix: the exposure gain on all three channels (default 1)")
    ap.add_argument("--curve", choices=("gamma", "srgb", "trunc255"), default=None,
                    help="with --develop: the tone curve -- gamma (o^(1/2.2), the default), srgb, or trunc255 (no curve: * 255, truncated)")


def develop_profile(ap, args):
    """The sesrq.develop.Profile the develop flags describe, or None without --develop; a flag error is an argparse error."""
    rest = [k for k in ("wb", "ccm", "colormatrix", "red_gain", "blue_gain", "rgb_gain", "curve") if getattr(args, k) is not None]
    if not args.develop:
        if rest:
            ap.error("--wb, --ccm, --colormatrix, --red-gain, --blue-gain, --rgb-gain and --curve belong to --develop")
        return None
    if args.mflag not in (2, 3, 4):
        ap.error(f"--develop: MFLAG {args.mflag} does not return a linear camera-RGB image (2: dm, 3: nrdm_3 and 4: nrdm_6 do; the "
                 "output of 1, nr, is a mosaic; 5 and 6 are developed images already)")
    if args.input is None or not args.input.endswith(".raw"):
        ap.error("--develop: the developed image comes from a raw frame: it needs a *.raw file as --input")
    if not args.save_png:
        ap.error("--develop: the developed image is written as a PNG: it needs --save-png")
    if args.colour:
        ap.error("--develop: --colour rebuilds colour around the luma net (--mflag 5)")
    gains = [k for k in ("red_gain", "blue_gain", "rgb_gain") if getattr(args, k) is not None]
    if args.colormatrix is not None and (args.ccm is not None or args.wb is not None):
        ap.error("--develop: either --ccm (with --wb), or --colormatrix (with --red-gain, --blue-gain, --rgb-gain)")
    if args.colormatrix is None and gains:
        ap.error("--develop: --red-gain, --blue-gain and --rgb-gain belong to --colormatrix; with --ccm the gains are --wb R,G,B")
    if args.wb is not None and len(args.wb) != 3:
        ap.error("--develop: --wb takes three gains R,G,B")
    from sesrq import develop
    try:
        if args.colormatrix is not None:
            one = lambda v: 1.0 if v is None else v
            return develop.from_colormatrix(args.colormatrix, one(args.red_gain), one(args.blue_gain), one(args.rgb_gain),
                                            curve=args.curve or "gamma")
        return develop.Profile(args.wb or (1.0, 1.0, 1.0), args.ccm or (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), args.curve or "gamma")
    except ValueError as e:
        ap.error(f"--develop: {e}")


def save_develop_png(path, gfake, profile, order):
    """--develop: the raw net's linear camera RGB with gains, colour matrix and tone curve applied, as an RGB PNG (sesrq.develop.export;
    the fp32 output is the dequantised int8 output, so the bytes are Engine.forward_develop's)."""
    from sesrq import develop, image
    u8 = develop.export(gfake, profile, order="rgb").cpu().numpy()          # PIL takes RGB bytes
    stem, ext = os.path.splitext(path)
    for k in range(u8.shape[0]):
        image.save_png(path if u8.shape[0] == 1 else f"{stem}_{k}{ext or '.png'}", u8[k])
    print("png:", path, tuple(u8.shape))


YUV_BATCH = 8          # frames of a .yuv sequence that go through as one batch


def add_video_flags(ap):
    """--yuv / --size / --pix-fmt / --frames / --save-yuv / --out-pix-fmt / --gt-yuv: YUV 4:2:0 video through the luma net (sesrq.video)
    or the RGB net (sesrq.video_rgb)."""
    ap.add_argument("--yuv", help="MFLAG 5 / 6, in place of --input: a raw .yuv file of unpadded 8-bit 4:2:0 frames (with --size and "
                                  "--pix-fmt), decoded on the device; MFLAG 5: the Y plane is the net's input, MFLAG 6: the frame "
                                  "converted to RGB")
    ap.add_argument("--size", metavar="WxH", help="frame size of --yuv (luma; odd sizes are legal)")
    ap.add_argument("--pix-fmt", choices=("nv12", "i420"), default=None, help="pixel format of --yuv and --gt-yuv")
    ap.add_argument("--frames", metavar="A:B", help="with --yuv: run frames A .. B-1 of the file only (default: all)")
    ap.add_argument("--save-yuv", help="with --yuv: write the super-resolved sequence here as a raw .yuv file -- MFLAG 5: the net's luma "
                                       "as bytes, the input's chroma upscaled bicubically (sesrq.video.export); MFLAG 6: the anchored RGB "
                                       "output converted to YCbCr 4:2:0 (sesrq.video_rgb.export)")
    ap.add_argument("--out-pix-fmt", choices=("nv12", "i420"), default=None, help="pixel format of --save-yuv (default: --pix-fmt)")
    ap.add_argument("--gt-yuv", help="with --yuv: the HR sequence (same frames, r times the size, --pix-fmt); its Y plane (MFLAG 6: the frame "
                                     "converted to RGB) is the ground truth the output is scored against")


def video_args(args):
    """(W, H, (first, end) | None) of a --yuv run, or None without --yuv; a flag error ends the program."""
    rest = [k for k in ("size", "pix_fmt", "frames", "save_yuv", "out_pix_fmt", "gt_yuv") if getattr(args, k) is not None]
    if args.yuv is None:
        if rest:
            raise SystemExit("sim.py: --size, --pix-fmt, --frames, --save-yuv, --out-pix-fmt and --gt-yuv belong to --yuv")
        return None
    if args.mflag not in (5, 6) or args.input is not None or args.hr is not None or args.gt is not None or args.save_png or args.colour:
        raise SystemExit("sim.py: --yuv feeds the luma net (--mflag 5) or the RGB net (--mflag 6) in place of --input / --hr; its ground "
                         "truth is --gt-yuv, its output --save-yuv")
    if args.size is None or args.pix_fmt is None:
        raise SystemExit("sim.py: --yuv needs --size WxH and --pix-fmt")
    try:
        W, H = (int(v) for v in args.size.lower().split("x"))
        span = None
        if args.frames is not None:
            a, b = args.frames.split(":")
            span = (int(a or 0), int(b) if b else None)
    except ValueError:
        raise SystemExit("sim.py: --size is WxH, --frames is A:B") from None
    return W, H, span


def run_yuv(args, yuv, model, keep=False):
    """The --yuv run: the sequence goes through in batches of YUV_BATCH frames -- Y plane decoded on the device -> model(inps) ->
    scored against --gt-yuv's Y plane, exported with the input's chroma to --save-yuv.  Prints what the image path prints.
    MFLAG 6 goes through sesrq.video_rgb instead: the frames decoded to RGB -> model(inps) -> the anchored output scored against
    --gt-yuv decoded to RGB and exported to --save-yuv as YCbCr 4:2:0.
    A batch's fp32 output (33 MB a 4K frame) is dropped once it is scored and saved, so device memory does not grow with the
    sequence: only a caller from Python (keep: main(argv) returns the whole output, on the device) and --save (host copies) hold it."""
    from sesrq import quality, video
    rgb = args.mflag == 6
    if rgb:
        from sesrq import video_rgb
    route = video_rgb if rgb else video
    W, H, span = yuv
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        lr = video.load_yuv(args.yuv, W, H, args.pix_fmt, span)
        r = model._sesrq_engine(dev).bundle.pixel_shuffle
        gt = video.load_yuv(args.gt_yuv, r * W, r * H, args.pix_fmt, span) if args.gt_yuv else None
        if gt is not None and gt.N != lr.N:
            raise ValueError(f"{args.gt_yuv}: {gt.N} frames, {args.yuv} has {lr.N}")
        outs, rows, shape = [], [], None
        for a in range(0, lr.N, YUV_BATCH):
            part = video.to_device(lr[a:a + YUV_BATCH], dev)
            _, inps = route.decode(None, part, want_q=False, want_f=True)
            gfake = model(inps)
            pred = anchored(gfake, inps, args.mflag)        # test.py:149-155: MFLAG 6 + the nearest-upsampled input
            shape = (a + gfake.shape[0],) + tuple(gfake.shape[1:])
            if keep:
                outs.append(gfake)
            elif args.save:
                outs.append(gfake.cpu())
            if gt is not None:
                _, g = route.decode(None, video.to_device(gt[a:a + YUV_BATCH], dev), want_q=False, want_f=True)
                rows.append(quality.score(pred, g, args.mflag))
            if args.save_yuv:
                fmt = args.out_pix_fmt or args.pix_fmt
                sr = video_rgb.export(pred, fmt=fmt) if rgb else video.export(gfake, part, r, fmt=fmt)
                video.save_yuv(args.save_yuv, sr, append=a > 0)
    except ValueError as e:
        raise SystemExit(f"sim.py: {e}") from None
    gfake = torch.cat(outs) if outs else None
    torch.cuda.synchronize()
    banner(args.mflag)
    print("output:", shape, "engines:", model._sesrq_engine(dev).layer_engines())
    if args.save:
        np.save(args.save, gfake.cpu().numpy())
    if rows:
        res = torch.cat(rows).cpu().numpy()
        for _, psnr, _ in res:
            print(float(psnr))
        print(quality.TASKS[args.mflag] + ' mean psnr is: ', float(res[:, 1].sum()) / len(res), ' ssim is: ', float(res[:, 2].sum()) / len(res))
    if args.save_yuv:
        print("yuv:", args.save_yuv, (shape[0], shape[2], shape[3]), args.out_pix_fmt or args.pix_fmt)
    return gfake if keep else None


def add_noise_flags(ap):
    """--add-noise / --shot / --read / --noise-seed: the reference's TEST_RAW_ADD_NOISE on clean *.raw inputs (sesrq.noise)."""
    ap.add_argument("--add-noise", action=argparse.BooleanOptionalAction, default=None,
                    help="add shot and read noise to *.raw inputs on the device while they are unpacked, as the reference's dataset does "
                         "under define.TEST_RAW_ADD_NOISE (the default: without the flag, that constant decides)")
    ap.add_argument("--shot", type=float, default=None, metavar="S", help="shot noise level (with --read; without them a level is drawn "
                                                                          "per frame as the reference's random_noise_levels draws it)")
    ap.add_argument("--read", type=float, default=None, metavar="R", help="read noise level (with --shot)")
    ap.add_argument("--noise-seed", type=int, default=None, metavar="K", help="seed of the noise stream (default 0): frame f of a run "
                                                                              "gets the same noise whenever the seed is the same")


def noise_model(args, who, inputs):
    """The sesrq.noise.NoiseModel the noise flags describe, or None without --add-noise (or, with define.TEST_RAW_ADD_NOISE alone,
    when the inputs are no raw frames: the reference adds noise to raw frames only); a flag error ends the program."""
    given = [k for k in ("shot", "read", "noise_seed") if getattr(args, k) is not None]
    raws = bool(inputs) and all(p.endswith(".raw") for p in inputs)
    explicit = args.add_noise is not None
    if not (args.add_noise if explicit else define.TEST_RAW_ADD_NOISE):
        if given:
            raise SystemExit(f"{who}: --shot, --read and --noise-seed belong to --add-noise")
        return None
    if not raws:
        if given or explicit:
            raise SystemExit(f"{who}: --add-noise adds noise to *.raw inputs")
        return None
    from sesrq import noise
    try:
        return noise.NoiseModel(args.shot, args.read, seed=args.noise_seed or 0)
    except ValueError as e:
        raise SystemExit(f"{who}: {e}") from None


def sensor_format(args, who, inputs):
    """The sesrq.sensor.Format the sensor flags describe, or None when none is given; a flag error ends the program."""
    given = {k: v for k, v in (("cfa", args.cfa), ("black", args.black), ("white", args.white), ("packing", args.packing))
             if v is not None}
    if not given:
        return None
    if not inputs or not all(p.endswith(".raw") for p in inputs):
        raise SystemExit(f"{who}: --cfa, --black, --white and --packing describe *.raw inputs")
    from sesrq import sensor
    try:
        return sensor.Format(**given)
    except ValueError as e:
        raise SystemExit(f"{who}: {e}") from None


def is_image(path, image_flag):
    return path.lower().endswith(".png") or (image_flag and path.endswith(".npy"))


def anchored(gfake, inps, mflag):
    """test.py:149-155: MFLAG 6 is judged (and exported) with the nearest-upsampled input added."""
    if mflag != 6:
        return gfake
    x = inps.float().to(gfake.device)
    return gfake + x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def save_png(path, gfake, inps, mflag):
    """The reference's PNG export (sim.py:163-169) on the device: clip to [0, 1], * 255 in fp32, truncate to uint8; PIL takes RGB
    bytes, so no channel flip."""
    from sesrq import image
    u8 = image.export(anchored(gfake, inps, mflag), order="rgb").cpu().numpy()
    stem, ext = os.path.splitext(path)
    for k in range(u8.shape[0]):
        image.save_png(path if u8.shape[0] == 1 else f"{stem}_{k}{ext or '.png'}", u8[k])
    print("png:", path, tuple(u8.shape))


def save_lr_png(path, lr_u8, order):
    """--save-lr: the LR image the device made from --hr, as an RGB PNG."""
    from sesrq import image
    u8 = (lr_u8.flip(-1) if order == "bgr" else lr_u8).cpu().numpy()          # PIL takes RGB bytes
    stem, ext = os.path.splitext(path)
    for k in range(u8.shape[0]):
        image.save_png(path if u8.shape[0] == 1 else f"{stem}_{k}{ext or '.png'}", u8[k])
    print("lr:", path, tuple(u8.shape))


def save_colour_png(path, gfake, lr_u8, order):
    """--colour: the net's luma with the LR image's chroma, upscaled bicubically, as an RGB PNG (sesrq.colour.export; the fp32 output
    is the dequantised int8 output, so the bytes are Engine.forward_colour's)."""
    from sesrq import colour, image
    lr = lr_u8 if lr_u8.dim() == 4 else lr_u8.unsqueeze(0)
    if order == "bgr":                      # PIL takes RGB bytes
        lr = lr.flip(-1)
    u8 = colour.export(gfake, lr, gfake.shape[2] // lr.shape[1], order="rgb").cpu().numpy()
    stem, ext = os.path.splitext(path)
    for k in range(u8.shape[0]):
        image.save_png(path if u8.shape[0] == 1 else f"{stem}_{k}{ext or '.png'}", u8[k])
    print("png:", path, tuple(u8.shape))


def load_frames(path):
    return torch.load(path, weights_only=True, map_location="cpu") if path.endswith(".pt") else torch.from_numpy(np.load(path))


def score_against(path, gfake, inps, mflag, gts=None, fmt=None):
    """The reference's evaluation loop (test.py:141-183) on the device: anchor for MFLAG 6, clip, PSNR / SSIM per frame; prints each
    frame's PSNR and the mean line.  gts: the ground truth already formed (an 8-bit HR image's), else read from `path`.  Returns the
    (N, 3) float64 host array of (mse, psnr, ssim)."""
    from sesrq import quality
    if gts is None:
        gts = load_frames(path)
    if tuple(gts.shape) != tuple(gfake.shape):
        raise SystemExit(f"sim.py: --gt has shape {tuple(gts.shape)}, the output is {tuple(gfake.shape)}")
    if gts.dtype == torch.uint16:                   # 16-bit RGB ground truth: / 4095, clamped (self_dataset.py:235-243)
        from sesrq import sensor
        gts = sensor.load_gt(gts, fmt, gfake.device)
    pred = anchored(gfake, inps, mflag)             # test.py:149-155: MFLAG 6 + the nearest-upsampled input
    res = quality.score(pred, gts.float().to(gfake.device), mflag).cpu().numpy()
    totalpsnr = totalssim = 0.0
    for _, psnr, ssim in res:
        print(float(psnr))
        totalpsnr += float(psnr)
        totalssim += float(ssim)
    print(quality.TASKS[mflag] + ' mean psnr is: ', totalpsnr / len(res), ' ssim is: ', totalssim / len(res))
    return res


if __name__ == "__main__":
    main()
