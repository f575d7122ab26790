"""Device engine: a Bundle uploaded to one GPU (sesrq_create) + the fused integer forward
(sesrq_forward).  torch is plumbing only: device memory, the current HIP stream."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .bundle import Bundle


class GraphedForward:
    """A forward (or a chain of forwards: nrdm_6 -> SESR-x2) captured as a HIP graph (Engine.capture)."""

    def __init__(self, engine, x, want_q, want_f, slot, downstream):
        if downstream and not want_q:
            raise ValueError("a chain hands the int8 output on: want_q must be True")
        if downstream and any(e.quan_bits != 8 for e in (engine,) + tuple(downstream)):
            raise ValueError("chained engines need 8-bit nets")
        dt = engine._check_in(x)
        del dt
        if not x.is_contiguous():
            raise ValueError("capture needs a contiguous input buffer (it is baked into the graph)")
        self.engines = (engine,) + downstream
        self.x = x
        dev = engine.device
        N, _, H, W = x.shape
        self.outs = []
        cur_shape = (N, H, W)
        for j, e in enumerate(self.engines):
            shp = e.out_shape(*cur_shape)
            last = j == len(self.engines) - 1
            q = torch.empty(shp, dtype=torch.int8, device=dev) if (want_q or not last) else None
            y = torch.empty(shp, dtype=torch.float32, device=dev) if (want_f and last) else None
            self.outs.append((q, y))
            e.workspace(*cur_shape, slot)                 # allocate outside the capture
            cur_shape = (shp[0], shp[2], shp[3])
        self.q, self.y = self.outs[-1]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._issue(side, slot)                       # warm-up: one-time occupancy queries / attribute calls happen here
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self._issue(side, slot)

    def _issue(self, stream, slot):
        cur = self.x
        for e, (q, y) in zip(self.engines, self.outs):
            e.forward(cur, want_q=q is not None, want_f=y is not None, out_q=q, out_f=y, stream=stream, slot=slot,
                      assume_ordered=True)
            cur = q

    def replay(self):
        self.graph.replay()
        return self.q, self.y


class Submission:
    """Frames, buffers and streams of Engine.submission(), laid out once as the C arrays sesrq_forward_many takes."""

    def __init__(self, engine, frames, outs_q, outs_f, streams, group=1):
        if not frames or not streams or (outs_q is None and outs_f is None):
            raise ValueError("submission: frames / outputs / streams do not match")
        for o in (outs_q, outs_f):
            if o is not None and len(o) != len(frames):
                raise ValueError("submission: frames / outputs / streams do not match")
        if len(frames) % len(streams):
            raise ValueError("submission: the frame list must be a multiple of the stream count (frame k runs on stream k % S, cyclically)")
        self.engine, self.n = engine, len(frames)
        self.dt = engine._check_in(frames[0])
        N, _, H, W = frames[0].shape
        self.shape = (N, H, W)
        shp = engine.out_shape(N, H, W)
        for k, x in enumerate(frames):
            if engine._check_in(x) != self.dt or tuple(x.shape) != tuple(frames[0].shape) or not x.is_contiguous():
                raise ValueError("submission: every frame must be a contiguous tensor of the same shape and dtype")
            for o, dtp, what in ((outs_q, torch.int8, "int8"), (outs_f, torch.float32, "fp32")):
                if o is not None and (tuple(o[k].shape) != tuple(shp) or o[k].dtype != dtp or not o[k].is_contiguous()):
                    raise ValueError(f"submission: every {what} output must be a contiguous tensor of the forward's output shape")
        self._keep = (list(frames), list(outs_q) if outs_q is not None else None, list(outs_f) if outs_f is not None else None, list(streams))
        # two periods back to back: any window of up to n frames starting anywhere in the cycle is one contiguous slice
        self.io = (_lib.FrameIO * (2 * self.n))()
        for k in range(2 * self.n):
            j = k % self.n
            self.io[k] = _lib.FrameIO(frames[j].data_ptr(), outs_q[j].data_ptr() if outs_q is not None else None,
                                      outs_f[j].data_ptr() if outs_f is not None else None)
        S = len(streams)
        if group < 1 or (group > 1 and N != 1):
            raise ValueError("submission: group >= 1, and grouping needs single-image frames")
        self.group = int(group)
        if self.group > 1:      # the frames of one launch sequence are written concurrently (the library refuses a shared buffer too)
            for o in (outs_q, outs_f):
                if o is None:
                    continue
                for s_ in range(S):
                    seq = [t.data_ptr() for t in o[s_::S]]
                    g_eff = min(self.group, len(seq))      # one call hands over at most one period: a group never wraps onto its own frames
                    ring = seq + seq[:g_eff - 1]
                    for i in range(len(seq)):
                        win = ring[i:i + g_eff]
                        if len(set(win)) != len(win):
                            raise ValueError("submission: frames that may share a launch sequence (any `group` consecutive frames of a "
                                             "stream) share an output buffer")
        self.ws = [engine.workspace(N * self.group, H, W, s) for s in range(S)]       # room for `group` frames per launch sequence
        self.ws_bytes = self.ws[0].numel()
        # the library maps frame k of a call to streams[k % S]: a window that starts at frame f of the list gets the arrays rotated by f % S
        self.ws_rot = [(C.c_void_p * S)(*[self.ws[(r + i) % S].data_ptr() for i in range(S)]) for r in range(S)]
        self.st_rot = [(C.c_void_p * S)(*[streams[(r + i) % S].cuda_stream for i in range(S)]) for r in range(S)]
        self.S = S

    def enqueue(self, count: int, first: int = 0):
        """Frames first .. first+count-1 (indices taken modulo the list): sesrq_forward_many calls of at most one period each."""
        lib, N, (n, H, W) = _lib.lib(), self.n, self.shape
        k, base, sz = first, C.addressof(self.io), C.sizeof(_lib.FrameIO)
        while count > 0:
            c = min(count, N)
            off = k % N
            _lib.check(lib.sesrq_forward_many(self.engine._h, C.cast(base + off * sz, C.POINTER(_lib.FrameIO)), c, self.dt, n, H, W,
                                              self.ws_rot[off % self.S], self.ws_bytes, self.st_rot[off % self.S], self.S, self.group))
            k += c
            count -= c


class Engine:
    """One immutable net on one device.  forward() is stream-ordered and allocation-free once
    the workspace for a given (N, H, W) exists."""

    def __init__(self, bundle: Bundle, device: Optional[torch.device] = None, engine: int = _lib.ENGINE_AUTO,
                 force_general: bool = False, exact_division: bool = False, anchor_add: bool = False,
                 fuse_hidden=1, wg_budget: int = 0, upstream: Optional[Bundle] = None, reciprocal_division: bool = False,
                 reduced_forms: int = -1):
        """reciprocal_division: form x / s0 of the input quantiser as x * fl(1/s0) -- torch's tensor / scalar on a GPU --
        instead of the true quotient the CPU-run reference and the goldens define (sesrq_options.exact_div = 2).
        upstream: the net whose int8 OUTPUT frames this engine takes as int8 input (chained nets, e.g. nrdm_6 ->
        SESR-x2): they are re-quantised into this net's input domain while the first layer stages them.
        reduced_forms: sesrq_options.reduced_forms -- which of the proven reduced epilogue forms the kernels may select (-1 = all); same
        bits either way, it only picks the kernel instantiation (tests run every one of them on reference-made data)."""
        if not torch.cuda.is_available():
            raise RuntimeError("sesrq.Engine needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback in this package")
        self.bundle = bundle
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        # define.py QUAN_BIT of the bundle: b < 8 is created by sesrq_create_q and runs on the dot4 kernels, or, with
        # engine=_lib.ENGINE_MFMA_Q, on the width-aware MFMA kernels and the fused trio (same bits; grouped submissions work there)
        self.quan_bits = int(getattr(bundle, "quan_bits", 8))
        if self.quan_bits != 8 and upstream is not None:
            raise ValueError(f"chained engines (upstream=) need 8-bit nets; this bundle is {self.quan_bits}-bit")
        if upstream is not None and int(getattr(upstream, "quan_bits", 8)) != 8:
            raise ValueError(f"chained engines (upstream=) need 8-bit nets; the upstream bundle is {upstream.quan_bits}-bit")
        self.anchor_add = bool(anchor_add)          # the fp32 output carries the x2 anchor (sesrq.quality.evaluate checks it)
        L = bundle.L
        self._keep = []
        layers = (_lib.LayerDesc * L)()
        for k, l in enumerate(bundle.layers):
            w = np.ascontiguousarray(l.wq, dtype=np.int8)
            ac = np.ascontiguousarray(l.add_const, dtype=np.int32)
            self._keep += [w, ac]
            layers[k] = _lib.LayerDesc(k=w.shape[2], ic=w.shape[1], oc=w.shape[0],
                                       w=w.ctypes.data_as(C.POINTER(C.c_int8)),
                                       add_const=ac.ctypes.data_as(C.POINTER(C.c_int32)),
                                       M=l.M, n=l.n, relu=int(l.relu))
            if getattr(l, "M_oc", None) is not None:      # per-output-channel requant constants (that layer runs on the dot4 kernels)
                moc = np.ascontiguousarray(l.M_oc, dtype=np.uint32)
                noc = np.ascontiguousarray(l.n_oc, dtype=np.uint32)
                if moc.shape != (w.shape[0],) or noc.shape != (w.shape[0],):
                    raise ValueError("per-channel requant constants: one (M, n) per output channel")
                self._keep += [moc, noc]
                layers[k].M_oc = moc.ctypes.data_as(C.POINTER(C.c_uint32))
                layers[k].n_oc = noc.ctypes.data_as(C.POINTER(C.c_uint32))
        zero = (C.c_int32 * (L + 1))(*bundle.zero)
        desc = _lib.NetDesc(n_layers=L, layers=layers, zero=zero,
                            scale_in=float(np.float32(bundle.scale[0])), scale_out=float(np.float32(bundle.scale[L])),
                            M_res=bundle.M_res, n_res=bundle.n_res, pixel_shuffle=bundle.pixel_shuffle,
                            pe_num=bundle.pe_num, pe_acc_bits=bundle.pe_acc_bits, pe_add_bits=bundle.pe_add_bits)
        # options are part of sesrq_create: the device net is immutable afterwards
        opts = _lib.Options()
        _lib.lib().sesrq_default_options(C.byref(opts))
        opts.engine = int(engine)
        opts.force_general = int(bool(force_general))
        if exact_division and reciprocal_division:
            raise ValueError("exact_division and reciprocal_division exclude each other")
        opts.exact_div = 2 if reciprocal_division else int(bool(exact_division))
        opts.anchor_add = int(bool(anchor_add))
        opts.fuse_hidden = 1 if fuse_hidden is True else int(fuse_hidden)     # 0 per layer, 1 (default) fused hidden trios
        opts.wg_budget = int(wg_budget)
        opts.reduced_forms = int(reduced_forms)
        if upstream is not None:
            opts.i8_in_scale = float(np.float32(upstream.scale[upstream.L]))
            opts.i8_in_zero = int(upstream.zero[upstream.L])
        self.exact_div = int(opts.exact_div)         # how x / s0 is formed: the raw route's q0 table forms it the same way
        self.i8_in_scale = float(opts.i8_in_scale)   # > 0: an int8 input is an upstream net's output, not q0 (forward_raw refuses)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            if self.quan_bits == 8:
                _lib.check(_lib.lib().sesrq_create(C.byref(desc), C.byref(opts), C.byref(handle)), ValueError)
            else:
                _lib.check(_lib.lib().sesrq_create_q(C.byref(desc), C.byref(opts), self.quan_bits, C.byref(handle)), ValueError)
        self._h = handle
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._in: Dict[tuple, torch.Tensor] = {}      # kept input buffers of forward_raw / forward_image

    def close(self):
        if getattr(self, "_op_id", None):      # registered as a torch.ops.sesrq.forward handle: the C++ side drops its pointer first
            from . import torch_op
            torch_op.unregister_engine(self)
        if getattr(self, "_h", None):
            _lib.lib().sesrq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------
    def fast_division_proven(self) -> bool:
        return bool(_lib.lib().sesrq_fast_division_proven(self._h))

    def one_fma_layers(self):
        """Per layer, the form of its requant (sesrq_layer_one_fma, proven per (M, n) at create): 1 = ONE fused multiply-add,
        2 = one fma that also subtracts the 128 plus the add back (output layer only), 0 = the two-step form."""
        return [int(_lib.lib().sesrq_layer_one_fma(self._h, k)) for k in range(self.bundle.L)]

    def layer_engines(self):
        return [(_lib.lib().sesrq_layer_engine(self._h, k) or b"").decode() for k in range(self.bundle.L)]

    def launch_plan(self):
        """[(first_layer, n_layers)] per kernel launch of forward() (n_layers == 3: fused hidden trio)."""
        L = self.bundle.L
        first, count = (C.c_int * L)(), (C.c_int * L)()
        n = _lib.lib().sesrq_launch_plan(self._h, first, count)
        return [(first[i], count[i]) for i in range(n)]

    def out_shape(self, N, H, W):
        r = self.bundle.pixel_shuffle
        return (N, self.bundle.out_channels, H * r, W * r)

    def workspace(self, N, H, W, slot: int = 0) -> torch.Tensor:
        """Device workspace for (N,H,W); `slot` selects an independent copy so that several frames can be
        in flight on different streams (the library itself keeps no per-call state)."""
        key = (N, H, W, slot)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = _lib.lib().sesrq_workspace_bytes(self._h, N, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def _run(self, src, dt, want_q, want_f, out_q, out_f, stream, slot, in_shape=None, decode=None):
        """What every stream-ordered forward shares: the outputs asked for and not given are allocated, the slot's workspace taken
        and the stream entered; then `decode(src, inp, stream)` fills a kept (N, C, H, W) input buffer of dtype `dt` from `src`
        (a front end's launch; without it `src` is the input), and sesrq_forward runs on that input."""
        with torch.cuda.device(self.device):
            if isinstance(src, torch.Tensor):
                src = src.contiguous()
                planes = (src,)
            else:                            # a video surface: planes with pitches, read where they lie
                planes = tuple(src.tensors())
            if decode is None:
                inp, (N, _, H, W) = src, src.shape
            else:
                N, _, H, W = in_shape
                key = (*in_shape, slot, dt)
                inp = self._in.get(key)
                if inp is None:
                    inp = self._in[key] = torch.empty(in_shape, dtype=torch.float32 if dt == _lib.F32 else torch.int8,
                                                      device=self.device)
            shp = self.out_shape(N, H, W)
            self._check_out(out_q, out_f, shp)
            if want_q and out_q is None:
                out_q = torch.empty(shp, dtype=torch.int8, device=self.device)
            if want_f and out_f is None:
                out_f = torch.empty(shp, dtype=torch.float32, device=self.device)
            ws = self.workspace(N, H, W, slot)
            st = _lib.enter_stream(self.device, stream, *planes, inp, out_q, out_f, ws)
            if decode is not None:
                decode(src, inp, st)
            rc = _lib.lib().sesrq_forward(self._h, inp.data_ptr(), dt, out_q.data_ptr() if out_q is not None else None,
                                          out_f.data_ptr() if out_f is not None else None, N, H, W, ws.data_ptr(), ws.numel(),
                                          st.cuda_stream)
        _lib.check(rc)
        return out_q, out_f

    def _check_out(self, out_q, out_f, shp):
        """A caller-supplied output is written through its data_ptr(): anything but a contiguous tensor of the output shape, of its
        dtype, on this device would be a device-memory overrun (or land in the wrong place), so it is refused before any launch."""
        for o, dtp, what in ((out_q, torch.int8, "int8"), (out_f, torch.float32, "fp32")):
            if o is not None and (not isinstance(o, torch.Tensor) or tuple(o.shape) != tuple(shp) or o.dtype != dtp
                                  or o.device != self.device or not o.is_contiguous()):
                raise ValueError(f"forward: every {what} output must be a contiguous tensor of the forward's output shape "
                                 f"{tuple(shp)} on {self.device}")

    def _check_in(self, x: torch.Tensor):
        if x.dim() != 4:
            raise ValueError("Expect input tensor dimension: 4, but get %d" % x.dim())
        if x.device != self.device:
            raise ValueError(f"input is on {x.device}, engine on {self.device}")
        if x.shape[0] < 1 or x.shape[2] < 1 or x.shape[3] < 1:
            raise ValueError("empty frame: N, H and W must be positive")
        if x.shape[1] != self.bundle.in_channels:
            raise ValueError(f"expected {self.bundle.in_channels} input channels, got {x.shape[1]}")
        if x.dtype == torch.float32:
            return _lib.F32
        if x.dtype == torch.int8:
            return _lib.I8
        raise ValueError("input must be float32 (frame) or int8 (already quantised q0)")

    def forward(self, x: torch.Tensor, want_q: bool = True, want_f: bool = True, out_q=None, out_f=None, stream=None,
                slot: int = 0, assume_ordered: bool = False):
        """x: (N, Cin, H, W) float32 | int8 on self.device -> (q int8 | None, y float32 | None).
        stream: torch.cuda.Stream to enqueue on (default: current); slot: workspace copy to use -- give
        concurrent in-flight frames different slots.  A side stream is ordered behind the current stream and the
        tensors are recorded on it (safe default); assume_ordered=True skips that (and the device switch) for a caller
        that owns persistent, contiguous buffers and fences its streams itself -- the throughput harness: the
        bookkeeping costs more host time per call than the three kernel launches."""
        dt = self._check_in(x)
        if assume_ordered:
            if not x.is_contiguous() or (want_q and out_q is None) or (want_f and out_f is None) or stream is None:
                raise ValueError("assume_ordered=True needs a contiguous input, caller-owned output buffers and a stream")
            N, _, H, W = x.shape
            self._check_out(out_q if want_q else None, out_f if want_f else None, self.out_shape(N, H, W))
            ws = self.workspace(N, H, W, slot)
            _lib.check(_lib.lib().sesrq_forward(self._h, x.data_ptr(), dt, out_q.data_ptr() if want_q else None,
                                                out_f.data_ptr() if want_f else None, N, H, W, ws.data_ptr(), ws.numel(),
                                                stream.cuda_stream))
            return (out_q if want_q else None), (out_f if want_f else None)
        return self._run(x, dt, want_q, want_f, out_q, out_f, stream, slot)

    __call__ = forward

    def forward_raw(self, raw: torch.Tensor, want_q: bool = True, want_f: bool = True, out_q=None, out_f=None, stream=None,
                    slot: int = 0, fmt=None, stride=None, width=None, noise=None):
        """raw: (N, 1, H, W) or (N, H, W) torch.uint16 12-bit RGGB frames on self.device -> (q int8 | None, y float32 | None).

        The frames are unpacked on the device (libsesrq_raw.so, sesrq.raw) into this net's q0 -- a per-(N, H, W, slot) buffer the
        engine keeps -- and run through the same forward as an int8 q0 input: the results are those of forward() on the reference's
        fp32 input frame (self_dataset.py TestDataset).  Both launches go to `stream` (default: current), ordered as forward() orders
        them; give concurrent in-flight frames different slots.  Only for nets with 3 input channels whose int8 input is q0 (no
        `upstream`) and without the fp32 anchor.  A net narrower than 8 bits takes the unpack's fp32 frame and the fp32 forward (the
        unpack's q0 is 8-bit): the same bits as forward() on that frame.

        fmt: a sesrq.sensor.Format -- the frames are in that sensor format (any CFA order and levels; torch.uint16, or torch.uint8
        rows of MIPI RAW10 / RAW12; `stride` and `width` as sesrq.sensor.frames takes them) and libsesrq_sensor.so unpacks them.
        Without it nothing changes: 12-bit RGGB through libsesrq_raw.so.

        noise: a sesrq.noise.NoiseModel -- the reference's TEST_RAW_ADD_NOISE: libsesrq_noise.so unpacks the frames (in `fmt`, or the
        reference's format) and adds the model's shot and read noise on the way; frame n of the call is the model's frame0 + n.  The
        results are those of forward() on noise.apply(..., want_spread=True)'s frame.  Without it nothing changes."""
        from . import sensor
        if self.bundle.in_channels != 3:
            raise ValueError(f"forward_raw: a raw RGGB frame feeds 3-channel nets; this one takes {self.bundle.in_channels}")
        if self.i8_in_scale != 0.0:
            raise ValueError("forward_raw: this engine takes an upstream net's int8 output as input (upstream=...), not q0")
        if self.anchor_add:
            raise ValueError("forward_raw: anchor_add needs the fp32 input frame; use raw.unpack(..., want_spread=True) and forward()")
        if not (want_q or want_f):
            raise ValueError("forward_raw: ask for the int8 output, the fp32 output or both")
        narrow = self.quan_bits != 8       # the buffer holds q0, or the fp32 frame of a narrow net
        raw, W, S = sensor.frames(raw, fmt, self.device, stride, width, "forward_raw: ")
        N, H = raw.shape[0], raw.shape[1]

        if noise is not None:
            from . import noise as noisemod
            noisemod._model(noise)

        def unpack(src, buf, st):
            args = (self.device, fmt, self.bundle.scale[0], self.bundle.zero[0], self.exact_div, src, W, S,
                    None if narrow else buf, buf if narrow else None, st)
            if noise is None:
                sensor.launch(*args)
            else:
                noisemod.launch(*args, noise)
        return self._run(raw, _lib.F32 if narrow else _lib.I8, want_q, want_f, out_q if want_q else None, out_f if want_f else None,
                         stream, slot, (N, 3, H, W), unpack)

    def forward_develop(self, raw: torch.Tensor, profile, order: str = "rgb", out=None, stream=None, slot: int = 0, fmt=None, stride=None,
                        width=None, noise=None):
        """raw: sensor frames as forward_raw takes them (with its fmt, stride, width and noise) -> the developed display images
        (N, H, W, 3) torch.uint8 in `order`.

        For the raw nets whose output is a linear camera-RGB image (3 channels out, no PixelShuffle: dm, nrdm_3, nrdm_6): forward_raw
        with the int8 output only, followed by the fused develop export (libsesrq_develop.so, sesrq.develop) from that int8 output with
        the net's output domain -- white-balance gains, colour-correction matrix and tone curve of `profile` (a
        sesrq.develop.Profile), bytes out.  out: a contiguous uint8 tensor of the output shape to write into.  All launches go to
        `stream` (default: current), ordered as forward() orders them; give concurrent in-flight frames different slots.  Everything
        forward_raw refuses is refused by forward_raw.  An nr net (MFLAG 1) has the shape of a dm net but returns a mosaic; a bundle
        does not record its task, so that misuse is the caller's to avoid (sim.py --develop refuses MFLAG 1)."""
        from . import develop, sensor
        b = self.bundle
        if b.out_channels != 3 or b.pixel_shuffle != 1:
            raise ValueError(f"forward_develop: a developed image comes from a net that returns the 3 planes R, G, B at the frame's size; "
                             f"this net gives {b.out_channels} channel(s) at PixelShuffle factor {b.pixel_shuffle} (the SR nets export "
                             "through image.export, forward_colour and forward_video)")
        develop._order(order)
        profile = develop._profile(profile)
        if out is not None:                  # the frame size as forward_raw will read it (what it refuses of `raw`, it refuses here too)
            frames, W, _ = sensor.frames(raw, fmt, self.device, stride, width, "forward_raw: ")
            develop.check_out(out, (frames.shape[0], frames.shape[1], W, 3), self.device, "forward_develop")
        with torch.cuda.device(self.device):
            q, _ = self.forward_raw(raw, want_q=True, want_f=False, stream=stream, slot=slot, fmt=fmt, stride=stride, width=width,
                                    noise=noise)
            N, _, H, W = q.shape
            if out is None:
                out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=self.device)
            st = _lib.enter_stream(self.device, stream, q, out)
            develop.launch(profile, q, b.scale[b.L], b.zero[b.L], order, out, st)
        return out

    def forward_image(self, img_u8: torch.Tensor, form=None, order: str = "rgb", want_q: bool = True, want_f: bool = True, out_q=None,
                      out_f=None, stream=None, slot: int = 0):
        """img_u8: (N, H, W, 3) or (H, W, 3) torch.uint8 images on self.device, interleaved in `order` ("rgb" or "bgr") ->
        (q int8 | None, y float32 | None).

        form: "y" (SESR-x4, MFLAG 5: the float64 luma) or "rgb" (SESR-x2, MFLAG 6); None takes the one that fits the net's input
        channels.  The images are decoded on the device (libsesrq_image.so, sesrq.image) into this net's q0 -- a per-(N, H, W, slot)
        buffer the engine keeps -- and run through the same forward as an int8 q0 input: the results are those of forward() on the
        reference's fp32 input frame (self_dataset_sr.py TestDataset).  An anchor_add engine needs the fp32 frame for its anchor: the
        images are decoded into the fp32 frame instead (a kept buffer too) and run through the fp32 forward.  Both launches go to
        `stream` (default: current), ordered as forward() orders them; give concurrent in-flight frames different slots.  Not for
        engines whose int8 input is an upstream net's output.  A net narrower than 8 bits takes the fp32 frame too (the decoder's q0
        is 8-bit): the same bits as forward() on that frame."""
        from . import image as imgmod
        cin = self.bundle.in_channels
        f = imgmod._form(form if form is not None else ("y" if cin == 1 else "rgb"))
        if imgmod.CHANNELS[f] != cin:
            raise ValueError(f"forward_image: the {'Y' if f == imgmod.Y else 'RGB'} form gives {imgmod.CHANNELS[f]} channel(s); "
                             f"this net takes {cin}")
        if self.i8_in_scale != 0.0:
            raise ValueError("forward_image: this engine takes an upstream net's int8 output as input (upstream=...), not an image")
        if not (want_q or want_f):
            raise ValueError("forward_image: ask for the int8 output, the fp32 output or both")
        imgmod._order(order)
        img = imgmod._images(img_u8, self.device)
        N, H, W, _ = img.shape
        # the buffer holds q0, or the fp32 frame an anchored forward adds back / a narrow net quantises itself
        fp = self.anchor_add or self.quan_bits != 8

        def decode(src, buf, st):
            imgmod.launch(self.device, self.bundle.scale[0], self.bundle.zero[0], self.exact_div, src, f, order, None if fp else buf,
                          buf if fp else None, st)
        return self._run(img, _lib.F32 if fp else _lib.I8, want_q, want_f, out_q if want_q else None, out_f if want_f else None,
                         stream, slot, (N, cin, H, W), decode)

    def forward_hr(self, hr_u8: torch.Tensor, order: str = "rgb", want_q: bool = True, want_f: bool = True, out_q=None, out_f=None,
                   stream=None, slot: int = 0):
        """hr_u8: (N, H, W, 3) or (H, W, 3) torch.uint8 HR images (the ground truths) on self.device, interleaved in `order`, H and W
        multiples of the net's PixelShuffle factor r -> (q int8 | None, y float32 | None) of the output shape (N, C, H, W).

        forward_image of the bicubically downscaled image, without that image: one kernel (libsesrq_downscale.so, sesrq.downscale)
        downscales the HR image by r and decodes the result into this net's kept input buffer, exactly as forward_image decodes an LR
        file -- q0, or the fp32 frame for an anchor_add engine and for a net narrower than 8 bits.  r and the form come from the net:
        x4 luma (1 channel in), x2 RGB (3 channels in).  Launches, streams, slots and the refusals of caller outputs are
        forward_image's."""
        from . import downscale as ds
        cin, r = self.bundle.in_channels, self.bundle.pixel_shuffle
        if cin not in (1, 3):
            raise ValueError(f"forward_hr: an 8-bit image feeds 1- or 3-channel nets; this one takes {cin}")
        if r not in ds.FACTORS:
            raise ValueError(f"forward_hr: the HR image is downscaled by the net's PixelShuffle factor, 2 or 4; this net's is {r}")
        if self.i8_in_scale != 0.0:
            raise ValueError("forward_hr: this engine takes an upstream net's int8 output as input (upstream=...), not an image")
        if not (want_q or want_f):
            raise ValueError("forward_hr: ask for the int8 output, the fp32 output or both")
        ds._order(order)
        f = ds.Y if cin == 1 else ds.RGB
        img = ds.hr_images(hr_u8, r, who="forward_hr")
        ds._on_device(img, self.device, "forward_hr")
        N, H, W, _ = img.shape
        # the buffer holds q0, or the fp32 frame an anchored forward adds back / a narrow net quantises itself
        fp = self.anchor_add or self.quan_bits != 8

        def decode(src, buf, st):
            ds.launch(self.device, self.bundle.scale[0], self.bundle.zero[0], self.exact_div, src, order, r, f, None,
                      None if fp else buf, buf if fp else None, st)
        return self._run(img, _lib.F32 if fp else _lib.I8, want_q, want_f, out_q if want_q else None, out_f if want_f else None,
                         stream, slot, (N, cin, H // r, W // r), decode)

    def forward_colour(self, img_u8: torch.Tensor, order: str = "rgb", out=None, stream=None, slot: int = 0):
        """img_u8: (N, H, W, 3) or (H, W, 3) torch.uint8 colour images on self.device, interleaved in `order` -> the colour
        super-resolved images (N, r H, r W, 3) torch.uint8 in the same order, r the net's PixelShuffle factor.

        For luma nets (1 channel in, 1 channel out: SESR-x4, MFLAG 5): forward_image in the Y form, int8 output only, followed by
        the fused colour export (libsesrq_colour.so, sesrq.colour) from that int8 output and the same LR image -- the net's Y, the
        LR image's Cb and Cr upscaled bicubically, back to RGB bytes.  out: a contiguous uint8 tensor of the output shape to write
        into.  All launches go to `stream` (default: current), ordered as forward() orders them; give concurrent in-flight frames
        different slots."""
        from . import colour, image as imgmod
        b = self.bundle
        if b.in_channels != 1 or b.out_channels != 1:
            raise ValueError(f"forward_colour: colour is rebuilt around a luma net (1 channel in, 1 out); this net takes "
                             f"{b.in_channels} and gives {b.out_channels}: RGB nets export their own colour through "
                             "forward_image and image.export")
        r = colour._factor(b.pixel_shuffle)
        colour._order(order)
        img = imgmod._images(img_u8, self.device)
        N, H, W, _ = img.shape
        shape = (N, r * H, r * W, 3)
        if out is not None:
            colour.check_out(out, shape, self.device, "forward_colour")
        with torch.cuda.device(self.device):
            img = img.contiguous()
            q, _ = self.forward_image(img, form="y", order=order, want_q=True, want_f=False, stream=stream, slot=slot)
            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=self.device)
            st = _lib.enter_stream(self.device, stream, img, q, out)
            colour.launch(q, b.scale[b.L], b.zero[b.L], img, order, r, out, st)
        return out

    def forward_video(self, src, out=None, want_q: bool = False, stream=None, slot: int = 0):
        """src: a sesrq.video.Surface of N YUV 4:2:0 frames (NV12 or I420) on self.device -> the super-resolved frames as a Surface of
        r H x r W, r the net's PixelShuffle factor; with want_q also the net's luma: (surface, luma).

        For luma nets (1 channel in, 1 channel out: SESR-x4, MFLAG 5): the Y plane is decoded through its pitch into this net's kept
        q0 buffer (libsesrq_video.so, sesrq.video) and run through the same forward as an int8 q0 input; the fused export then writes
        the net's luma as bytes and the surface's chroma planes, upscaled bicubically, as a 4:2:0 surface -- no RGB on the way.  The
        luma is the net's int8 output; an anchor_add engine and a net narrower than 8 bits take the fp32 frame and give the fp32
        output, as forward_image does.  out: a Surface of the output size on this device to write into (its pixel format decides;
        without it the output has src's).  All launches go to `stream` (default: current), ordered as forward() orders them; give
        concurrent in-flight frames different slots."""
        from . import video
        b = self.bundle
        if b.in_channels != 1 or b.out_channels != 1:
            raise ValueError(f"forward_video: a video surface feeds a luma net (1 channel in, 1 out); this net takes {b.in_channels} "
                             f"and gives {b.out_channels}: RGB nets take a surface through forward_video_rgb")
        r = video._factor(b.pixel_shuffle)
        if self.i8_in_scale != 0.0:
            raise ValueError("forward_video: this engine takes an upstream net's int8 output as input (upstream=...), not a surface")
        s = video._on_device(src, self.device, "forward_video")
        N, H, W = s.N, s.H, s.W
        if out is not None:
            video.check_out(out, None, N, r * H, r * W, self.device, "forward_video")
        # the buffer holds q0, or the fp32 frame an anchored forward adds back / a narrow net quantises itself
        fp = self.anchor_add or self.quan_bits != 8

        def decode(surf, buf, st):
            video.launch_decode(self.device, b.scale[0], b.zero[0], self.exact_div, surf, None if fp else buf, buf if fp else None, st)
        with torch.cuda.device(self.device):
            q, f = self._run(s, _lib.F32 if fp else _lib.I8, not fp, fp, None, None, stream, slot, (N, 1, H, W), decode)
            luma = f if fp else q
            if out is None:
                out = video.Surface.alloc(s.fmt, N, r * H, r * W, self.device)
            st = _lib.enter_stream(self.device, stream, luma, *s.planes()[1:], *out.planes())
            video.launch_export(luma, b.scale[b.L], b.zero[b.L], s, r, out, st)
        return (out, luma) if want_q else out

    def forward_video_rgb(self, src, out=None, want_q: bool = False, stream=None, slot: int = 0):
        """src: a sesrq.video.Surface of N YUV 4:2:0 frames (NV12 or I420) on self.device -> the super-resolved frames as a Surface of
        r H x r W, r the net's PixelShuffle factor; with want_q also the net's prediction: (surface, prediction).

        For RGB nets (3 channels in, 3 out: SESR-x2, MFLAG 6): one kernel (libsesrq_video_rgb.so, sesrq.video_rgb) upscales the
        surface's chroma to 4:4:4, converts YCbCr to RGB bytes and decodes them into this net's kept q0 buffer -- forward_image on
        the RGB image those bytes are, without that image; the same forward runs from int8, and one kernel exports the int8 output
        to a 4:2:0 surface again (RGB bytes as image.export forms them, BT.601 luma, chroma averaged over 2 x 2 blocks).  An
        anchor_add engine and a net narrower than 8 bits decode into the fp32 frame instead and export the fp32 output, exactly as
        forward_image decides.  out: a Surface of the output size on this device to write into (its pixel format decides; without
        it the output has src's).  All launches go to `stream` (default: current), ordered as forward() orders them; give concurrent
        in-flight frames different slots."""
        from . import video_rgb
        b = self.bundle
        if b.in_channels != 3 or b.out_channels != 3:
            raise ValueError(f"forward_video_rgb: the RGB route feeds an RGB net (3 channels in, 3 out); this net takes {b.in_channels} "
                             f"and gives {b.out_channels}: a luma net takes a surface through forward_video")
        r = b.pixel_shuffle
        if self.i8_in_scale != 0.0:
            raise ValueError("forward_video_rgb: this engine takes an upstream net's int8 output as input (upstream=...), not a surface")
        s = video_rgb._on_device(src, self.device, "forward_video_rgb")
        N, H, W = s.N, s.H, s.W
        if out is not None:
            video_rgb.check_out(out, None, N, r * H, r * W, self.device, "forward_video_rgb")
        # the buffer holds q0, or the fp32 frame an anchored forward adds back / a narrow net quantises itself
        fp = self.anchor_add or self.quan_bits != 8

        def decode(surf, buf, st):
            video_rgb.launch_decode(self.device, b.scale[0], b.zero[0], self.exact_div, surf, None if fp else buf, buf if fp else None, st)
        with torch.cuda.device(self.device):
            q, f = self._run(s, _lib.F32 if fp else _lib.I8, not fp, fp, None, None, stream, slot, (N, 3, H, W), decode)
            pred = f if fp else q
            if out is None:
                out = video_rgb.Surface.alloc(s.fmt, N, r * H, r * W, self.device)
            st = _lib.enter_stream(self.device, stream, pred, *out.planes())
            video_rgb.launch_export(pred, b.scale[b.L], b.zero[b.L], out, st)
        return (out, pred) if want_q else out

    def submission(self, frames, outs_q, streams, outs_f=None, group: int = 1):
        """A prepared batch of independent forwards for sesrq_forward_many: frame k = frames[k] -> outs_q[k] (/ outs_f[k]; either may be None) on
        streams[k % len(streams)] with workspace slot k % len(streams).  Returns a Submission; .enqueue(count, first=0) issues frames
        first .. first+count-1 of the (cyclically repeated) list with ONE call into the library -- for callers whose frames are so small
        that the host's per-call cost bounds the rate.  group = G > 1 (single-image frames only): the per-stream workspaces are sized
        for G frames, and the library then runs up to G consecutive frames of a stream as the images of one launch sequence.
        Caller-owned persistent buffers; the caller fences the streams."""
        return Submission(self, frames, outs_q, outs_f, streams, group)

    def capture(self, x: torch.Tensor, want_q: bool = True, want_f: bool = False, slot: int = 0, downstream=()):
        """Capture one forward on `x` (and then, optionally, the chained `downstream` engines on its int8 output) as a HIP
        graph.  Returns a GraphedForward: `.replay()` re-issues the kernels on the current stream with ONE host call
        (x, q, y are fixed buffers: overwrite x in place -- stream-ordered -- to process another frame).  The kernels and
        their results are exactly those of forward(); what changes is the host cost per frame."""
        return GraphedForward(self, x, want_q, want_f, slot, tuple(downstream))

    def forward_timed(self, x: torch.Tensor, iters: int = 10):
        """Measurement hook (sesrq_forward_timed): average device ms per kernel launch (see launch_plan())
        and per forward, HIP events on the launch stream."""
        dt = self._check_in(x)
        with torch.cuda.device(self.device):
            x = x.contiguous()
            N, _, H, W = x.shape
            shp = self.out_shape(N, H, W)
            out_q = torch.empty(shp, dtype=torch.int8, device=self.device)
            ws = self.workspace(N, H, W)
            st = torch.cuda.current_stream(self.device).cuda_stream
            nl = len(self.launch_plan())
            launch_ms = (C.c_float * nl)()
            fwd = C.c_float()
            _lib.check(_lib.lib().sesrq_forward_timed(self._h, x.data_ptr(), dt, out_q.data_ptr(), None, N, H, W,
                                                      ws.data_ptr(), ws.numel(), st, iters, launch_ms, C.byref(fwd)))
        return list(launch_ms), float(fwd.value)

    def forward_debug(self, x: torch.Tensor, pe: bool = True, overflow: bool = False, acts: bool = True, special: bool = False):
        """Forward with the reference's dump taps (define.py *_W_FLG): returns a dict with
        q_out, y, input{k} (int8 NCHW), pe_out{k} (N,4,OC,H,W int32), pe_add{k} (N,OC,H,W int32) and, with
        overflow=True, `overflow` (L,2) int32: PE sums above / below the accumulator range before saturation --
        the events the reference prints as max_overflow / min_overflow (quan_func.py:358-361).
        On the MFMA engine the PE taps are written by the per-PE MFMA kernels themselves; the quantised-input tap
        (input0), the overflow counters and the pe-split last layer (OC <= 4) run their layer on the dot4 kernels.
        acts=False: no input{k} taps (layer 0 then stays on its MFMA kernel too).
        special=True: also `shortcut` (N, OC_0, H, W) fp32 = the reference's residual/shortcut_tensor.pt (layer 0's un-rounded ReLU'd requant
        output, quan_func.py:529-549) and `input4_special` (N, OC_{L-2}, H, W) int8 = input.4.spcial.pt (ic, quan_func.py:250-254); both are
        taps of the dot4 kernels (layers 0 and L-2 then run there)."""
        dt = self._check_in(x)
        with torch.cuda.device(self.device):
            x = x.contiguous()
            N, _, H, W = x.shape
            L = self.bundle.L
            shp = self.out_shape(N, H, W)
            res = {"q_out": torch.empty(shp, dtype=torch.int8, device=self.device),
                   "y": torch.empty(shp, dtype=torch.float32, device=self.device)}
            taps = _lib.Taps()
            for k, l in enumerate(self.bundle.layers):
                oc, ic = l.wq.shape[0], l.wq.shape[1]
                if acts:
                    res[f"input{k}"] = torch.empty((N, ic, H, W), dtype=torch.int8, device=self.device)
                    taps.act[k] = res[f"input{k}"].data_ptr()
                if pe:
                    res[f"pe_out{k}"] = torch.empty((N, 4, oc, H, W), dtype=torch.int32, device=self.device)
                    res[f"pe_add{k}"] = torch.empty((N, oc, H, W), dtype=torch.int32, device=self.device)
                    taps.pe_out[k] = res[f"pe_out{k}"].data_ptr()
                    taps.pe_add[k] = res[f"pe_add{k}"].data_ptr()
            if special:
                l0, lm = self.bundle.layers[0], self.bundle.layers[L - 2]
                res["shortcut"] = torch.empty((N, l0.wq.shape[0], H, W), dtype=torch.float32, device=self.device)
                res["input4_special"] = torch.empty((N, lm.wq.shape[0], H, W), dtype=torch.int8, device=self.device)
                taps.shortcut = res["shortcut"].data_ptr()
                taps.ic = res["input4_special"].data_ptr()
            if overflow:
                res["overflow"] = torch.zeros((L, 2), dtype=torch.int32, device=self.device)
                taps.overflow = res["overflow"].data_ptr()
            ws = self.workspace(N, H, W)
            st = torch.cuda.current_stream(self.device).cuda_stream
            rc = _lib.lib().sesrq_forward_debug(self._h, x.data_ptr(), dt, res["q_out"].data_ptr(), res["y"].data_ptr(),
                                                N, H, W, ws.data_ptr(), ws.numel(), st, C.byref(taps))
        _lib.check(rc)
        return res
