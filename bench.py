#!/usr/bin/env python3
"""bench.py -- INT8 SESR frames/s on MI355X (BASELINE.json metric), one process per GPU.

    python bench.py [--gpus N] [--steps K] [--warmup W]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path (sesrq_forward: quantise -> first conv -> fused hidden trio -> last conv with
the pixel-shuffle store) over one batch of synthetic frames already resident in HBM.  Workload at N=1 =
BASELINE.json configs[1]: SESR-x2 INT8 1080p -> 4K, one frame per step; the steps rotate over 8 distinct resident
input frames.  Frames shard across ranks with no data-path collective.  Rank 0 prints ONE JSON line.

The timed region is exactly K steps, bracketed by synchronize + barrier on both sides; `value` = frames of those K steps / their
time, MAX over ranks (sesrq/dist.py:run_timed).  Before it, untimed: `--settle` blocks of K steps, each fenced like the timed one
(default: ceil(SETTLE_STEPS / K) blocks, so that the timed block runs in the steady state of a series of blocks), then the W warm-up
steps and the host-enqueue sample.  `--repeats R` (opt-in, A/B scripts) times R blocks and reports the median.

    --dump-outputs DIR   after the timed steps, write what the timed path returned in its last step (the int8 output frame of that step,
                         as float32) to DIR/out_q.npy (DIR/out_q.rank<r>.npy per rank for N > 1): the whole array, or a fixed seeded sample
                         of it where the whole would exceed DUMP_BYTES.  The inputs are seeded: the same arguments give the same arrays.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "sesr-pytorch-quantize_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12            # B/s, MI355X HBM3E spec (/opt/skills/guides/MI355X_MICROARCH.md)
MFMA_I8_PEAK = 5.0e15     # dense int8 MFMA, ops/s (MI355X_MICROARCH.md: twice the bf16 rate of ~2.5 PFLOP/s)
POOL = 8                     # distinct resident input frames the steps rotate over
# untimed steps before the timed block, as blocks of K: block rates climb over the first tens of ms of a series of blocks (round 5, 1080p:
# a first 200-step block at 16.6 k frames/s, the next ones 17.5-18.2 k; 20-step blocks: ~15.0 k for the first eight, median 15.9 k)
SETTLE_STEPS = 1500
DUMP_BYTES = 64_000_000      # --dump-outputs: at most this many bytes of .npy files in all (every rank's file together)

# name: (nets [(bundle fixture, description)], Cin, H, W, frames: ("per_gpu", B) weak | ("total", B) strong, description)
WORKLOADS = {
    "sesr_x2_1080p": (["sesr_x2_rand.crop.npz"], 3, 1080, 1920, ("per_gpu", 1),
                      "SESR-x2 INT8 1080p->4K (3->12ch, PixelShuffle 2)"),                       # BASELINE config 2 (headline)
    # the same net calibrated BY THE REFERENCE on a natural-ish frame (zero_0 = -169), natural-ish frames in the pool (tests/golden/natural.py);
    # pool frame 0 is the very 1080p frame the reference itself ran (sesr_x2_rand_nat.big.json): the last layer's 18-bit PE clamp fires on it
    "sesr_x2_1080p_nat": (["sesr_x2_rand_nat.crop.npz"], 3, 1080, 1920, ("per_gpu", 1),
                          "SESR-x2 INT8 1080p->4K on natural-ish frames, reference-calibrated on a natural frame"),
    "nrdm_3_540p": (["nrdm_3_qat.crop.npz"], 3, 540, 960, ("per_gpu", 1),
                    "nrdm_3 INT8 (nrdm_3_qat_G.pth) 960x540 denoise+demosaic (3->3ch)"),          # config 3 (the QAT checkpoint it names)
    "sesr_x4_540p": (["sesr_x4.crop.npz"], 1, 540, 960, ("per_gpu", 1), "SESR-x4 INT8 540p->4K (1->16ch, PixelShuffle 4)"),
    "sesr_x4_540p_b32": (["sesr_x4.crop.npz"], 1, 540, 960, ("total", 32),
                         "SESR-x4 INT8 540p->4K, batch of 32 frames sharded over the ranks"),   # config 4
    "nrdm6_sesrx2_540p": (["unpinned/nrdm_6.bundle.npz", "sesr_x2_rand.crop.npz"], 3, 540, 960, ("per_gpu", 4),
                          "nrdm_6 (8 convs) -> SESR-x2 end-to-end INT8, 960x540 -> 1920x1080, int8 hand-off"),  # config 5
}


# Launch plan per workload: (streams, wg_budget), chosen by throughput in same-box A/Bs (tools/plan_ab.sh; profiles/README.md, round 3):
# 1080p: 3 streams x 512 slots 14.5 k frames/s vs 2 streams x full chip 14.2 k; anything else: the round-2 plan.
# The budget is counted in workgroup slots PER COMPUTE UNIT (2 = half of the four a CU holds for these kernels) and scaled by the device's
# CU count at run time: 2 x 256 = 512 on an MI355X (not a constant of this chip).
PLAN = {"sesr_x2_1080p": (3, 2), "sesr_x2_1080p_nat": (3, 2), "nrdm_3_540p": (3, 2), "sesr_x4_540p": (3, 2), "nrdm6_sesrx2_540p": (3, 2)}      # (streams, slots per CU): same-box A/Bs, profiles/README.md
PLAN_DEFAULT = (2, 0)
GROUP = {"nrdm_3_540p": 8, "sesr_x4_540p": 8}      # frames per launch sequence in --submit many (profiles/README.md, round 4); 1 elsewhere


def launch_bytes_per_px(bundle, first, count, in_f32):
    """Algorithmic HBM bytes per input pixel of ONE launch covering layers first..first+count-1: what the launch must
    move.  Every NHWC16 int8 activation that crosses a launch boundary is written once and read once; the frame goes in as fp32 (or
    int8) and out as int8.  The residual operand rc (layer 0's output when zero[1] == -128, else a tensor of its own that layer 0
    writes besides) is one more 16 B/px read for the launch that holds layer L-2 -- UNLESS that launch's own input already is that
    tensor (first == 1, zero[1] == -128: the fused trio of the 5-conv nets takes rc out of its LDS input window, sesrq_trio.hip
    instance 15) or layer 0 is in the same launch.  A fused trio of a 5-conv net therefore moves 16 in + 16 out = 32 B/px -- not the
    112 B/px its three layers move one by one."""
    L = bundle.L
    cin = bundle.in_channels
    cout_last = int(bundle.layers[-1].wq.shape[0])
    last = first + count - 1
    rc_separate = int(bundle.zero[1]) != -128
    rd = ((4 * cin) if in_f32 else cin) if first == 0 else 16
    wr = cout_last if last == L - 1 else 16
    holds_merge = first <= L - 2 <= last
    if holds_merge and first > 0 and (rc_separate or first != 1):
        rd += 16
    if first == 0 and rc_separate and not holds_merge:
        wr += 16
    return rd + wr


def reference_cpu_timing(workload):
    """The reference's own CPU sim path, timed in the BUILD container (the reference cannot travel to the GPU box): a committed
    constant written by tests/golden/make_golden.py --case time_x2_1080p for the headline workload (same net, same 1x3x1080x1920 frame,
    dump flags off); for the other workloads the survey's SESR-x4 1080p figure, labelled as a different net."""
    f = os.path.join(ROOT, "tests", "golden", "reference_x2_1080p.json")
    if workload == "sesr_x2_1080p" and os.path.isfile(f):
        r = json.load(open(f))
        return {"value": r["frames_per_s"], "unit": "frames/s", "cores": r["cores"], "seconds_per_frame": r["seconds_median"],
                "workload": r["workload"], "same_workload_as_timed": True,
                "where": r["host"] + " (tests/golden/make_golden.py --case time_x2_1080p; not re-run on the GPU box)"}
    return {"value": 0.106, "unit": "frames/s", "cores": 8, "workload": "SESR-x4 1x1x1080x1920 through the reference's own sim.py path, dump flags off",
            "same_workload_as_timed": False, "where": "survey container (SURVEY.md 6): the reference cannot travel to the GPU box, not re-run here"}


def layerwise_bytes_per_px(bundle, in_f32):
    """the layer-by-layer accounting the north star's HBM-roofline frames/s is quoted on."""
    return sum(launch_bytes_per_px(bundle, k, 1, in_f32) for k in range(bundle.L))


def dump_array(path, t, max_values, seed=0):
    """--dump-outputs: tensor t as a float32 .npy -- whole (its own shape) when it holds at most max_values values, else the values at a
    fixed seeded sample of max_values flat (C-order) indices, ascending, as a 1-D array.  Returns whether it was sampled."""
    import numpy as np
    import torch
    flat = t.reshape(-1)
    if flat.numel() <= max_values:
        np.save(path, t.float().cpu().numpy())
        return False
    idx = np.sort(np.random.default_rng(seed).choice(flat.numel(), size=max_values, replace=False))
    np.save(path, flat[torch.from_numpy(idx).to(flat.device)].float().cpu().numpy())
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=1,
                    help="timed blocks of exactly --steps steps each; value = the MEDIAN block.  Default 1: --steps is the number of timed "
                         "steps; more blocks are an opt-in of the A/B scripts (tools/)")
    ap.add_argument("--settle", type=int, default=-1,
                    help="untimed blocks of --steps steps before the warm-up, each fenced like the timed block: the rate of such blocks climbs "
                         "over the first tens of ms of a series.  -1 = auto: ceil(SETTLE_STEPS / steps) blocks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the output the timed path returned in its last step to DIR/out_q.npy (float32; "
                         "a fixed seeded sample where the whole would exceed DUMP_BYTES)")
    ap.add_argument("--batch", type=int, default=0, help="frames per step per GPU (0 = the workload's own)")
    ap.add_argument("--graph", action="store_true", help="replay each step as a captured HIP graph (Engine.capture): same kernels, one "
                                                         "host call per step instead of one per launch")
    ap.add_argument("--streams", type=int, default=0,
                    help="HIP streams the steps are enqueued on round-robin (frames are independent; each stream has "
                         "its own workspace and output buffer) -- fills the launch/prologue/tail gaps between kernels.  0 = the "
                         "workload's tuned plan (PLAN): 3 for the single-frame workloads, 2 for the 32-frame batch")
    ap.add_argument("--group", type=int, default=0,
                    help="--submit many, single-image frames: up to this many consecutive frames of a stream become the images of ONE launch sequence "
                         "(sesrq_forward_many with a workspace for that many frames; separate frame buffers, pointer table in the kernel arguments).  "
                         "0 = the workload's plan (GROUP): 1 at 1080p, 8 for the 540p single-frame workloads, whose launches' fixed cost is a third of their time")
    ap.add_argument("--workload", default="sesr_x2_1080p", choices=sorted(WORKLOADS))
    ap.add_argument("--engine", default="auto", choices=["auto", "dot4", "mfma"])
    ap.add_argument("--no-fuse", action="store_true", help="one launch per layer (no fused hidden trio)")
    ap.add_argument("--fuse", type=int, default=1, choices=[0, 1], help="0 per layer, 1 (default) fused hidden trios")
    ap.add_argument("--submit", default="auto", choices=["auto", "many", "step", "op"],
                    help="how the steps reach the library: 'step' = one sesrq_forward per step from Python; 'many' = sesrq_forward_many, all the steps "
                         "of a block handed over by ONE call (the C side loops over the frames and streams): the same kernels, launches and "
                         "buffers, only the host's per-step cost changes; 'op' = one torch.ops.sesrq.forward_into per step (the C++-registered operator, "
                         "csrc/torch_op/sesrq_torch_op.cpp: dispatcher -> current HIP stream -> sesrq_forward, no Python in between).  auto = many for a "
                         "single net without --graph, else step")
    ap.add_argument("--wg-budget", type=int, default=-1,
                    help="workgroup slots a launch may fill (sesrq_options.wg_budget; 0 = one full round of the chip).  -1 = the workload's "
                         "tuned plan (PLAN): two slots per compute unit (512 of an MI355X's 1024) for the single-frame workloads, so that kernels of three "
                         "frames stay co-resident on every CU instead of meeting only at their tails")
    ap.add_argument("--timing-iters", type=int, default=200, help="forwards of the per-launch HIP-event timing (roofline)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend of the timing fence (nccl = RCCL; gloo + --share-gpu rehearses N > 1 on a 1-GPU box)")
    ap.add_argument("--share-gpu", action="store_true", help="map every local rank onto the visible devices round-robin")
    ap.add_argument("--blocking-sync", action="store_true", help="fence with the blocking torch.cuda.synchronize() only")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-boundary-legs", action="store_true", help="skip the fp32-output / anchor-add throughput legs (boundary_return)")
    args = ap.parse_args()

    if args.steps < 1 or args.repeats < 1:
        raise SystemExit("bench.py: --steps and --repeats must be at least 1")
    plan_streams, plan_slots_per_cu = PLAN.get(args.workload, PLAN_DEFAULT)
    if args.group <= 0:
        args.group = GROUP.get(args.workload, 1)
    if args.streams <= 0:
        args.streams = plan_streams
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world == 1:
        # not launched by torchrun: start the ranks as children (before anything touches the GPU)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(29500 + os.getpid() % 2000), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd).returncode)

    # One rank = one GPU = one slice of the node's CPUs (round 5): pinned before torch and the library start their threads.  Where ranks
    # outnumber a quarter of the cores nothing may busy-wait: the library's submission threads sleep at once (SESRQ_SPIN_US=0, read when the
    # library is loaded) and the fence's event spin yields.
    from sesrq.dist import Group, env_world, oversubscribed, pin_rank_cpus, run_timed, shard
    rank, local, world = env_world()
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    cpus = pin_rank_cpus(local, local_world) if world > 1 else sorted(os.sched_getaffinity(0))
    yielding = oversubscribed(local_world if world > 1 else 1, cpus if world == 1 else None)
    if yielding:
        os.environ.setdefault("SESRQ_SPIN_US", "0")
    import numpy as np
    import torch
    # The timing fence: ALWAYS a gloo group first, created before this process touches the GPU; RCCL ("nccl") is tried on top of it once
    # the device is set and used only if every rank gets through (sesrq/dist.py) -- the data path has no collective to lose.
    grp = Group(backend=args.dist_backend)
    import sesrq
    from sesrq import _lib
    from sesrq.bundle import Bundle
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device")
    if args.share_gpu:
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")
    if args.wg_budget < 0:
        args.wg_budget = plan_slots_per_cu * torch.cuda.get_device_properties(dev).multi_processor_count
    grp.bind_device(dev)

    fixtures, cin, H, W, (mode, nframes), desc = WORKLOADS[args.workload]
    bundles = [Bundle.load(os.path.join(ROOT, "tests", "golden", f)) for f in fixtures]
    ekw = dict(engine={"auto": _lib.ENGINE_AUTO, "dot4": _lib.ENGINE_DOT4, "mfma": _lib.ENGINE_MFMA}[args.engine],
               fuse_hidden=0 if args.no_fuse else args.fuse, wg_budget=args.wg_budget)
    # chained nets: every net but the first takes the int8 output of the one before and re-quantises it into its own
    # input domain while staging (sesrq_options.i8_in_scale / i8_in_zero) -- no fp32 round trip through HBM
    engines = [sesrq.Engine(b, dev, upstream=(bundles[j - 1] if j else None), **ekw) for j, b in enumerate(bundles)]
    if mode == "total":                          # strong scaling: a fixed batch cut into contiguous per-rank blocks
        mine = shard(args.batch or nframes, world, rank)
        B = len(mine)
        total_frames_per_step = args.batch or nframes
    else:                                        # weak scaling: every rank runs the same per-GPU batch
        B = args.batch or nframes
        total_frames_per_step = B * world
    NS = max(1, args.streams)
    g = torch.Generator().manual_seed(1 + rank)
    if args.workload.endswith("_nat"):      # natural-ish frames; frame 0 of rank 0 = the frame the reference ran (its SHA is checked below)
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        from natural import natural_frame
        big = json.load(open(os.path.join(ROOT, "tests", "golden", fixtures[0].replace(".crop.npz", ".big.json"))))
        pool = [torch.from_numpy(np.concatenate([natural_frame(cin, H, W, big["nat_seed"] + 1000 * rank + 10 * j + b_) for b_ in range(max(B, 1))])).to(dev)
                for j in range(POOL)]
    else:
        pool = [torch.rand((max(B, 1), cin, H, W), generator=g, dtype=torch.float32).to(dev) for _ in range(POOL)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    # chain hand-off: every net but the last hands its int8 output (N, C, H', W') to the next one's int8 input
    shapes = []
    n, h, w = B, H, W
    for e in engines:
        shapes.append(e.out_shape(max(n, 1), h, w))
        h, w = shapes[-1][2], shapes[-1][3]
    outs = [[torch.empty(s, dtype=torch.int8, device=dev) for s in shapes] for _ in range(NS)]
    torch.cuda.synchronize()
    counter = [0]

    def forward_chain(x, slot, stream):
        # persistent pre-allocated buffers, streams fenced by run_timed: the engine's per-call stream bookkeeping is skipped
        cur = x
        for j, e in enumerate(engines):
            e.forward(cur, want_q=True, want_f=False, out_q=outs[slot][j], stream=stream, slot=slot, assume_ordered=True)
            cur = outs[slot][j]
        return cur

    # sesrq_forward_many: frame i of the rotation = pool[i % POOL] -> outs[i % NS] on stream i % NS; one period = lcm(POOL, NS) frames
    submit_many = (args.submit == "many" or (args.submit == "auto" and len(engines) == 1 and not args.graph)) and B > 0
    if args.submit == "many" and (len(engines) != 1 or args.graph):
        raise SystemExit("--submit many: single nets, without --graph (a chain interleaves two nets on each stream)")
    sub = None
    if submit_many:
        period = POOL * NS // math.gcd(POOL, NS)
        # output buffers: one per stream as in the per-step path; with --group G the G frames that may share a launch sequence (consecutive
        # frames of one stream) get one each: frame i -> buffer (i % NS, (i // NS) % G)
        G = max(1, args.group) if B == 1 else 1
        obuf = {(sl, 0): outs[sl][0] for sl in range(NS)}
        for sl in range(NS):
            for j in range(1, G):
                obuf[(sl, j)] = torch.empty(shapes[0], dtype=torch.int8, device=dev)
        while (period // NS) % G:                 # whole groups per period, so that a buffer is never written twice inside one launch sequence
            period += POOL * NS // math.gcd(POOL, NS)
        sub = engines[0].submission([pool[i % POOL] for i in range(period)], [obuf[(i % NS, (i // NS) % G)] for i in range(period)], streams, group=G)

    def step_many(n):
        sub.enqueue(n, first=counter[0])
        counter[0] += n

    op_ids, op_ws = [], []
    if args.submit == "op":
        from sesrq import torch_op
        op_ids = [getattr(e, "_op_id", None) or torch_op.register_engine(e) for e in engines]
        n_, h_, w_ = max(B, 1), H, W
        dims = []
        for e in engines:
            dims.append((n_, h_, w_))
            shp_ = e.out_shape(n_, h_, w_)
            h_, w_ = shp_[2], shp_[3]
        op_ws = [[e.workspace(*dims[j], sl) for j, e in enumerate(engines)] for sl in range(NS)]
        op_into, op_streams = torch.ops.sesrq.forward_into.default, [st.cuda_stream for st in streams]
    graphs = {}
    if args.graph and B > 0:       # one graph per (stream slot, pool frame): the input pointer is part of a graph
        for slot in range(NS):
            for j in range(POOL):
                graphs[(slot, j)] = engines[0].capture(pool[j], want_q=True, want_f=False, slot=slot, downstream=engines[1:])

    def step():
        i = counter[0]
        counter[0] += 1
        if B > 0 and graphs:
            with torch.cuda.stream(streams[i % NS]):
                graphs[(i % NS, i % POOL)].replay()
        elif B > 0 and args.submit == "op":
            sl = i % NS
            cur = pool[i % POOL]
            for j, eid in enumerate(op_ids):      # the stream travels as a raw handle: no Python stream context per step
                op_into(cur, eid, outs[sl][j], None, op_ws[sl][j], op_streams[sl])
                cur = outs[sl][j]
        elif B > 0:
            forward_chain(pool[i % POOL], i % NS, streams[i % NS])

    # ---- before the timed region (rank 0): parity of a whole frame against the C oracle (doubles as the CPU baseline), then
    # the per-launch HIP-event timing -- the device is busy and at its working clock when the timed blocks start
    parity = cpu = launch_ms = fwd_ms = None
    if rank == 0:
        # ---- parity: the WHOLE first frame of the pool against the C oracle (checker only), which doubles as the CPU baseline
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from oracle import sesrq_oracle as O, c_oracle as CO
        onets = [O.Net(layers=[O.Layer(wq=l.wq, add_const=l.add_const, M=l.M, n=l.n, relu=l.relu) for l in b.layers],
                       scale=b.scale, zero=b.zero, M_res=b.M_res, n_res=b.n_res, pixel_shuffle=b.pixel_shuffle, pe=b.pe_num,
                       acc_bits=b.pe_acc_bits, add_bits=b.pe_add_bits, name=b.name) for b in bundles]
        thr = min(os.cpu_count() or 1, 16)
        x0 = pool[0][0:1]
        if graphs:      # --graph: what is timed is the replay, so the replay's own output buffer is what is compared
            with torch.cuda.stream(streams[0]):
                gq, _ = graphs[(0, 0)].replay()
            torch.cuda.synchronize()
            got = gq[0:1].cpu().numpy()
        elif sub is not None:
            # what is timed is sesrq_forward_many (submission threads, and for the 540p workloads grouped pointer-table launches):
            # THAT path's output is what is compared.  One launch sequence per stream (NS x G frames: no buffer is written twice), frame 0's
            # buffer against the C oracle / the reference's SHA below, every other buffer against a one-stream sesrq_forward of its frame.
            nfirst = NS * sub.group
            for t in sub._keep[1]:
                t.zero_()
            torch.cuda.synchronize()
            sub.enqueue(nfirst)
            torch.cuda.synchronize()
            got = sub._keep[1][0][0:1].cpu().numpy()
            many_checked, many_bad = 0, 0
            for i in range(1, nfirst):
                q1, _ = engines[0].forward(pool[i % POOL], want_f=False)
                torch.cuda.synchronize()
                many_checked += 1
                many_bad += int(not torch.equal(q1, sub._keep[1][i]))
            counter[0] = nfirst      # the rotation goes on where this left it
        elif args.submit == "op":      # the C++ operator is what is timed: its output is what is compared
            step()
            torch.cuda.synchronize()
            got = outs[0][-1][0:1].cpu().numpy()
        else:
            got = forward_chain(pool[0], 0, torch.cuda.current_stream(dev))[0:1].cpu().numpy()
        torch.cuda.synchronize()
        xs = x0.cpu().numpy()
        CO.forward(onets[0], xs[:, :, :64, :64], threads=thr, want_f=False)       # warm the thread pool
        t1 = time.perf_counter()
        cur = xs
        for j, on in enumerate(onets):
            if j:       # float hand-off between chained nets: y = (q - zero_L) * f32(scale_L) of the upstream net
                up = onets[j - 1]
                cur = (cur.astype(np.float32) - np.float32(up.zero[up.L])) * np.float32(up.scale[up.L])
            cur = CO.forward(on, cur, threads=thr, want_f=False)["q_out"]
        dt = time.perf_counter() - t1
        want = cur
        diff = got.astype(np.int32) - want.astype(np.int32)
        maxdiff = int(np.abs(diff).max())
        path = ("HIP-graph replay" if graphs else (f"sesrq_forward_many ({NS} streams, {sub.group} frame(s) per launch sequence: the timed path)" if sub is not None
                                                    else ("torch.ops.sesrq.forward_into per step (the timed path)" if args.submit == "op" else "sesrq_forward per step (the timed path)")))
        parity = {"checked": f"full frame ({'x'.join(map(str, got.shape))}) of pool frame 0 through {path} vs C oracle", "max_abs_diff_int8": maxdiff,
                  "mismatches": int((diff != 0).sum()),
                  "psnr_db": "inf" if maxdiff == 0 else float(10 * np.log10(255.0 ** 2 / np.mean(diff.astype(np.float64) ** 2)))}
        if sub is not None and not graphs:
            parity["other_frames_of_the_timed_path"] = {"checked": many_checked, "differ_from_one_stream_forward": many_bad}
            parity["mismatches"] += many_bad
        # headline workload: pool frame 0 of rank 0 is the very frame the REFERENCE itself was run on in the build container
        # (tests/golden/reference_x2_1080p.json): the whole int8 4K frame against the reference's own output, by SHA-256
        rf = os.path.join(ROOT, "tests", "golden", "sesr_x2_rand_nat.big.json" if args.workload.endswith("_nat") else "reference_x2_1080p.json")
        if args.workload in ("sesr_x2_1080p", "sesr_x2_1080p_nat") and os.path.isfile(rf) and B == 1 and not ekw["engine"] == _lib.ENGINE_DOT4:
            import hashlib
            ref = json.load(open(rf))
            if hashlib.sha256(np.ascontiguousarray(xs).tobytes()).hexdigest() == ref["x_sha256"]:
                parity["reference_out_q_sha256_match"] = hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == ref["out_q_sha256"]
        cpu = None
        if world == 1 and not args.no_cpu_baseline:
            cpu = {"reference_sim_py": reference_cpu_timing(args.workload),
                   "value": round(1.0 / dt, 4), "unit": "frames/s", "cores": thr, "kind": "port",
                   "sample": f"1 frame {H}x{W} of the same workload through oracle/sesrq_oracle.c (OpenMP, {thr} threads), {dt:.2f} s wall "
                             f"= {dt * thr:.0f} core-seconds of CPU work (the same run is the parity reference)"}

        # 200 forwards with an event pair around every launch (~20 ms): enough samples for the per-launch averages whatever
        # --steps is, and the device is at its working clock when the timed blocks start right after
        launch_ms, fwd_ms = engines[0].forward_timed(pool[0], iters=args.timing_iters)
    fence_events = [torch.cuda.Event() for _ in streams]

    def drain():
        """Local drain of the fence: spin on one event per stream, then torch.cuda.synchronize().  The blocking wait alone
        adds its host wake-up latency (~0.1-0.3 ms here) to every timed block -- 10-15 % of a 20-step block; the spin sees
        the end of the device work within microseconds and the synchronize that follows returns at once."""
        if not args.blocking_sync:
            for e, st in zip(fence_events, streams):
                e.record(st)
            while not all(e.query() for e in fence_events):
                if yielding:
                    os.sched_yield()
        torch.cuda.synchronize()

    # untimed settle: the measurement loop itself, blocks of K steps fenced on both sides, results dropped -- the timed block that follows
    # runs in the state a long series of such blocks reaches (a fixed count: the frame of every later step is the same from run to run)
    settle = args.settle if args.settle >= 0 else -(-SETTLE_STEPS // args.steps)
    if settle:
        run_timed(grp, step, args.steps, 0, repeats=settle, sync=drain, units_per_step=B, step_many=step_many if sub else None)

    res = run_timed(grp, step, args.steps, args.warmup, repeats=args.repeats, sync=drain, units_per_step=B, step_many=step_many if sub else None)
    elapsed_med = statistics.median(res["elapsed"])

    dumped = None
    if args.dump_outputs and B > 0:
        # what the caller of the timed path received in the last timed step: the int8 output frame(s) of the last frame index enqueued
        i = counter[0] - 1
        if graphs:
            last_q = graphs[(i % NS, i % POOL)].q
        elif sub is not None:
            last_q = sub._keep[1][i % sub.n]
        else:
            last_q = outs[i % NS][-1]
        torch.cuda.synchronize()
        os.makedirs(args.dump_outputs, exist_ok=True)
        fname = "out_q.npy" if world == 1 else f"out_q.rank{rank}.npy"
        sampled = dump_array(os.path.join(args.dump_outputs, fname), last_q, DUMP_BYTES // 4 // world - 1024)
        dumped = {"dir": args.dump_outputs, "file": fname, "shape": list(last_q.shape), "pool_frame": i % POOL, "sampled": sampled}

    result = None
    if rank == 0:
        fps = args.steps * total_frames_per_step / elapsed_med
        fps_all = sorted(args.steps * total_frames_per_step / e for e in res["elapsed"])
        px = B * H * W
        # ---- roofline per launch: begin/end HIP events of every kernel on the launch stream, inside this process (first net of a chain)
        eng, bundle = engines[0], bundles[0]
        plan = eng.launch_plan()
        alg = [launch_bytes_per_px(bundle, f, c, True) * px for f, c in plan]
        names = eng.layer_engines()
        kdom = int(np.argmax(launch_ms))
        ach = alg[kdom] / (launch_ms[kdom] * 1e-3)
        per_frame_fused = sum(alg) / max(B, 1)
        per_frame_layerwise = layerwise_bytes_per_px(bundle, True) * H * W
        hh, ww = H * bundle.pixel_shuffle, W * bundle.pixel_shuffle
        for ej, bj in zip(engines[1:], bundles[1:]):        # chained nets: the downstream nets' bytes too (int8 hand-off in)
            per_frame_fused += sum(launch_bytes_per_px(bj, f, c, False) for f, c in ej.launch_plan()) * hh * ww
            per_frame_layerwise += layerwise_bytes_per_px(bj, False) * hh * ww
            hh, ww = hh * bj.pixel_shuffle, ww * bj.pixel_shuffle
        # HBM bytes per launch / VALU + MFMA utilisation of that kernel from the committed rocprofv3 PMC passes (profiles/):
        # FETCH_SIZE and WRITE_SIZE in separate runs, FETCH_SIZE doubled for 16-B/lane streaming reads (MI355X_MICROARCH.md, HBM)
        prof = {}
        pfile = os.path.join(ROOT, "profiles", "pmc_summary.json")
        if os.path.isfile(pfile):
            prof = json.load(open(pfile)).get(args.workload, {}).get(f"launch{kdom}:{names[plan[kdom][0]]}", {})
        # counters cannot be collected inside this run (rocprofv3 PMC passes are separate processes): what the committed profile of the
        # SAME kernel holds is reported under an explicit provenance key, never as if it had been measured here
        committed = None
        if prof:
            committed = {"source": "profiles/pmc_summary.json (builder's box, tools/profile_round.sh, 1 stream, one rocprofv3 --pmc pass per "
                                   "counter group)", "hbm_bytes_per_launch": prof.get("hbm_bytes_per_launch"),
                         "issue": {"valu_util": prof.get("valu_util"), "mfma_util": prof.get("mfma_util"),
                                   "wait_inst_frac": prof.get("wait_inst_frac"), "lds_util": prof.get("lds_util"),
                                   "inst_active_cycles_per_simd": prof.get("inst_active_cycles_per_simd"),
                                   "in_kernel_clock_ghz": "1.75-1.95 under load, 2.39 idle (profiles/r04_h5_stamps.txt, r04_clock_under_load.txt)"}}
        roofline = {"bound": "hbm", "achieved": round(ach / 1e9, 2), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                    "frac": round(ach / HBM_PEAK, 4), "traffic": None, "from_committed_profile": committed,
                    "kernel": f"launch{kdom}:layers{plan[kdom][0]}-{plan[kdom][0] + plan[kdom][1] - 1}:{names[plan[kdom][0]]}",
                    "kernel_ms": round(launch_ms[kdom], 5), "algorithmic_bytes_per_launch": alg[kdom],
                    # int8_ops: 2 x the layers' real multiply-accumulates (K x K x Cin x Cout per pixel, no padding); mfma_frac against the dense
                    # int8 MFMA peak (MI355X_MICROARCH.md: 2 x the bf16 rate, ~5 POP/s at 2.4 GHz) -- the kernels are nearer the HBM roofline
                    # than this one, hence bound = "hbm"
                    "launches": [{"layers": [f, f + c - 1], "kernel": names[f], "ms": round(launch_ms[j], 5), "alg_bytes": alg[j],
                                  "frac": round(alg[j] / (launch_ms[j] * 1e-3) / HBM_PEAK, 4),
                                  "int8_ops": int(2 * px * sum(int(np.prod(bundle.layers[k].wq.shape)) for k in range(f, f + c))),
                                  "mfma_frac": round(2 * px * sum(int(np.prod(bundle.layers[k].wq.shape)) for k in range(f, f + c))
                                                     / (launch_ms[j] * 1e-3) / MFMA_I8_PEAK, 4)} for j, (f, c) in enumerate(plan)],
                    "forward_device_ms": round(fwd_ms, 5),
                    "bytes_per_frame": {"as_launched": per_frame_fused, "layer_by_layer": per_frame_layerwise},
                    "throughput_frac": round(per_frame_fused * fps / world / HBM_PEAK, 4),
                    "layerwise_frac": round(per_frame_layerwise * fps / world / HBM_PEAK, 4),
                    "note": "launches[].ms: begin/end HIP events of each kernel on the launch stream (hipExtLaunchKernelGGL inside sesrq_forward_timed: the "
                            "duration a rocprofv3 kernel trace reports); forward_device_ms: begin of the first to end of the last kernel; alg_bytes: what the "
                            "launch must move (DESIGN 4.4; the fused trio of a 5-conv net moves 32 B/px, not its layers' 112); traffic: null -- PMC counters cannot be collected inside this run, "
                            "the committed profile of the same kernel is under from_committed_profile; layerwise_frac = SURVEY "
                            "8(d)'s layer-by-layer bytes per frame x frames/s/GPU / peak = the north star's HBM-roofline fraction"}

        # ---- the boundary's own return type (never `value`): the reference's model(inps) returns the fp32 frame (quan_func.py:594), its eval
        # loop adds the nearest-upsampled input to the x2 result (test.py:148-155).  Same plan, same pool, fp32 frame out (4 x the output bytes).
        boundary = None
        if world == 1 and len(engines) == 1 and B > 0 and not args.no_boundary_legs:
            boundary = boundary_legs(torch, np, sesrq, bundles[0], ekw, dev, pool, streams, args, drain, H, W, fps,
                                     launch_bytes_per_px, plan, want, onets[0])

        # ---- end to end through pinned host buffers (never `value`): H2D / compute / D2H on three streams
        e2e = None
        if world == 1 and not args.no_e2e and B > 0:
            e2e = e2e_leg(torch, engines, pool, outs, B)
            e2e["int8_frames"] = e2e_leg(torch, engines, pool, outs, B, int8_in=True)

        result = {"metric": "INT8 SESR frames/sec (whole job) + PSNR-vs-ref-sim (bit-exact)", "value": round(fps, 2),
                  "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                  "timed_steps": args.steps * args.repeats, "settle_blocks": settle, "dumped_outputs": dumped,
                  "ms_per_step": round(elapsed_med / args.steps * 1e3, 5), "higher_is_better": True,
                  "scaling": "strong" if mode == "total" else "weak",
                  "vs_baseline": None, "dtype": "i8", "data": "synthetic",
                  "fence": grp.fence, "host": {"cpus_of_rank0": len(cpus), "ranks_on_node": local_world, "busy_wait": "yield" if yielding else "spin"},
                  "host_enqueue_us_per_step": None if res["host_enqueue_s_per_step"] is None else round(res["host_enqueue_s_per_step"] * 1e6, 1),
                  "host_enqueue_sample_steps": res["host_enqueue_sample_steps"], "repeats": args.repeats, "blocks_fps": [round(args.steps * total_frames_per_step / e, 1) for e in res["elapsed"]], "spread": {"min": round(fps_all[0], 2), "median": round(fps, 2), "max": round(fps_all[-1], 2)},
                  "config": {"workload": desc, "name": args.workload, "frames_per_step_per_gpu": B, "frames_per_step": total_frames_per_step,
                             "streams": NS, "wg_budget": args.wg_budget, "hip_graph": bool(graphs),
                             "submit": (f"sesrq_forward_many: one call per timed block of K steps, up to {sub.group} frame(s) of a stream per launch sequence" if sub else
                                        ("torch.ops.sesrq.forward_into per step (C++ operator)" if args.submit == "op" else "sesrq_forward per step")), "input_pool": f"{POOL} distinct resident frames, rotated per step",
                             "in": [B, cin, H, W], "out": list(shapes[-1]), "input_dtype": "f32", "output_dtype": "i8",
                             "weights": [("reference random-init net, calibrated by the reference" if "rand" in f else
                                          "reference checkpoint, calibrated by this package (parity unpinned)" if "bundle" in f else
                                          "reference checkpoint, quantised and calibrated by the reference") + f" ({f})" for f in fixtures],
                             "sharding": f"frames over {world} rank(s), contiguous blocks, no collective",
                             "launch_plan": [[names[f], c] for f, c in plan], "engines": [e.layer_engines() for e in engines],
                             "requant_forms": [e.one_fma_layers() for e in engines]},      # per layer: 1 / 2 = a load-time proof let the kernels run a reduced form
                  "roofline": roofline, "cpu_baseline": cpu, "boundary_return": boundary, "e2e": e2e, "parity": parity}
    grp.close()
    if result is not None:
        print(json.dumps(result), flush=True)


def boundary_legs(torch, np, sesrq, bundle, ekw, dev, pool, streams, args, drain, H, W, fps_int8, launch_bytes_per_px, plan, want_q0, onet):
    """Frames/s with the boundary's REAL return type (never `value`): (1) fp32 frame out only -- what the reference's
    model(inps) returns, (q - zero_L) * f32(scale_L) (quan_func.py:594) -- and (2) fp32 out with the x2 anchor add of the reference's eval
    loop (test.py:148-155: gfake + inps_x2; nets with Cin * r^2 == Cout only).  Same launch plan, pool and streams as the headline, the steps
    handed over by sesrq_forward_many; median of up to 15 blocks of --steps steps.  Whole-frame parity of pool frame 0: the fp32 frame must
    be the one rounding of the int8 frame the parity leg has already checked (and, on the headline workload, hash to the reference's own
    out_f_sha256); the anchored frame must equal that plus the nearest-upsampled input, one fp32 add."""
    import hashlib
    import math
    import statistics
    r = bundle.pixel_shuffle
    NS = len(streams)
    period = len(pool) * NS // math.gcd(len(pool), NS)
    B = pool[0].shape[0]
    px = B * H * W
    cout_last = int(bundle.layers[-1].wq.shape[0])
    out = {}
    legs = [("fp32_out", False)]
    if bundle.in_channels * r * r == cout_last:
        legs.append(("fp32_out_anchor_add", True))
    rf = os.path.join(ROOT, "tests", "golden", "sesr_x2_rand_nat.big.json" if args.workload.endswith("_nat") else "reference_x2_1080p.json")
    ref = json.load(open(rf)) if (args.workload in ("sesr_x2_1080p", "sesr_x2_1080p_nat") and os.path.isfile(rf)) else None
    for name, anchor in legs:
        e = sesrq.Engine(bundle, dev, anchor_add=anchor, **ekw)
        shp = e.out_shape(B, H, W)
        of = [torch.empty(shp, dtype=torch.float32, device=dev) for _ in range(NS)]
        sub = e.submission([pool[i % len(pool)] for i in range(period)], None, streams, outs_f=[of[i % NS] for i in range(period)])
        sub.enqueue(1)
        torch.cuda.synchronize()
        y0 = of[0][0:1].cpu().numpy()
        rec = {"unit": "frames/s", "output_dtype": "f32", "anchor_add": anchor}
        if want_q0 is not None:
            yq = ((want_q0.astype(np.float32) - np.float32(onet.zero[onet.L])) * np.float32(onet.scale[onet.L])).astype(np.float32)
            if anchor:
                x0 = pool[0][0:1].cpu().numpy()
                yq = (yq + np.repeat(np.repeat(x0, r, axis=2), r, axis=3)).astype(np.float32)      # gfake + inps_x2 (test.py:148-155)
            rec["parity"] = {"checked": f"full fp32 frame ({'x'.join(map(str, y0.shape))}) of pool frame 0 vs the C oracle's int8 frame dequantised"
                                        + (" + nearest-upsampled input" if anchor else ""), "mismatches": int((y0 != yq).sum())}
            if ref is not None and not anchor:
                rec["parity"]["reference_out_f_sha256_match"] = hashlib.sha256(np.ascontiguousarray(y0).tobytes()).hexdigest() == ref["out_f_sha256"]
        done = 1
        sub.enqueue(max(args.warmup, 1), first=done)
        done += max(args.warmup, 1)
        drain()
        els = []
        for _ in range(min(args.repeats, 15)):
            t0 = time.perf_counter()
            sub.enqueue(args.steps, first=done)
            drain()
            els.append(time.perf_counter() - t0)
            done += args.steps
        el = statistics.median(els)
        v = args.steps * B / el
        # bytes as launched: the last launch writes 4 bytes per output value instead of 1 (and re-reads the fp32 input frame for the anchor)
        bpp = [launch_bytes_per_px(bundle, f, c, True) for f, c in plan]
        bpp[-1] += 3 * cout_last + (4 * bundle.in_channels if anchor else 0)
        rec.update(value=round(v, 2), ms_per_step=round(el / args.steps * 1e3, 5), vs_int8_out=round(v / fps_int8, 4),
                   bytes_per_frame_as_launched=int(sum(bpp) * px / B), throughput_frac=round(sum(bpp) * px / B * v / HBM_PEAK, 4))
        out[name] = rec
        e.close()
    out["note"] = ("the reference's model(inps) returns the fp32 frame (myQL/quan_func.py:594); its eval loop adds the nearest-upsampled input to the x2 "
                   "result (test.py:148-155).  Same plan / pool / streams as `value`, which writes the int8 frame (SURVEY 8d's end points); never `value`")
    return out


def e2e_leg(torch, engines, pool, outs, B, frames=96, depth=3, int8_in=False):
    """Host -> device -> host for `frames` steps through pinned host buffers, `depth` frames in flight; PCIe-bound by construction (SURVEY
    8e asks for it to be reported separately; never `value`).  Round 4: ONE STREAM PER FRAME SLOT -- H2D, the kernels and D2H of a frame
    are enqueued on the slot's stream in order, the overlap comes from the `depth` slots; no event crosses a stream.  Rounds 2-3 ran H2D /
    kernels / D2H on three streams tied together by events per frame: with the SDMA engines carrying the copies (ROCm's default) every such
    cross-queue dependency is resolved through the host's signal handler, and the loop ran at a third of the copies' own rate AND slowed
    down pass after pass (tools/e2e_probe.py, profiles/r04_e2e_probe.txt: 1317 / 880 / 657 steps/s, int8 frames slower than fp32; the copies
    alone: 2240 steps/s each way, 1920 both ways; HSA_ENABLE_SDMA=0: stable 885 / 1100; one stream per slot: 1120-1570 fp32, 1380-2090
    int8, no decay).  The first DMA out of / into a freshly pinned buffer is slow (6 vs 56 GB/s measured here), so every buffer is cycled
    twice before the clock starts.  int8_in: the frames cross PCIe already quantised (q0 = clamp8(rint(x / s0 + z0)) formed on the host --
    what a camera pipeline with uint8 frames hands over): a quarter of the input bytes, the engine's int8 entry (SESRQ_I8)."""
    dev = pool[0].device
    if int8_in:
        b0 = engines[0].bundle
        s0, z0 = float(__import__("numpy").float32(b0.scale[0])), float(b0.zero[0])
        hin = [torch.clamp(torch.round(pool[i % len(pool)].cpu() / s0 + z0), -128, 127).to(torch.int8).pin_memory() for i in range(depth)]
    else:
        hin = [pool[i % len(pool)].cpu().pin_memory() for i in range(depth)]
    shapes = [o.shape for o in outs[0]]
    douts = [[torch.empty(s, dtype=torch.int8, device=dev) for s in shapes] for _ in range(depth)]
    hout = [torch.empty(shapes[-1], dtype=torch.int8).pin_memory() for _ in range(depth)]
    din = [torch.empty(pool[0].shape, dtype=hin[0].dtype, device=dev) for _ in range(depth)]
    slot_streams = [torch.cuda.Stream(device=dev) for _ in range(depth)]
    torch.cuda.synchronize()

    def run(n):
        for i in range(n):
            b = i % depth
            st = slot_streams[b]
            with torch.cuda.stream(st):        # stream order: the slot's previous D2H is done before its buffers are written again
                din[b].copy_(hin[b], non_blocking=True)
                cur = din[b]
                for j, e in enumerate(engines):
                    e.forward(cur, want_q=True, want_f=False, out_q=douts[b][j], stream=st, slot=b, assume_ordered=True)
                    cur = douts[b][j]
                hout[b].copy_(cur, non_blocking=True)
        torch.cuda.synchronize()
    run(2 * depth)
    dts = []
    for _ in range(5):          # the copies share the DMA engines with whatever else the box does: median of five passes
        t0 = time.perf_counter()
        run(frames)
        dts.append(time.perf_counter() - t0)
    dt = sorted(dts)[2]
    mb_in = hin[0].numel() * hin[0].element_size() / 1e6
    mb_out = hout[0].numel() / 1e6
    return {"value": round(frames * B / dt, 2), "unit": "frames/s", "bound": "pcie", "input_dtype": "i8" if int8_in else "f32",
            "h2d_MB_per_step": round(mb_in, 2), "d2h_MB_per_step": round(mb_out, 2),
            "pcie_GBps": round((mb_in + mb_out) * frames / dt / 1e3, 2),
            "passes_fps": [round(frames * B / t, 1) for t in dts],
            "note": f"pinned host buffers, one stream per frame slot (H2D, kernels, D2H in stream order), {depth} frames in flight, median of 5 passes of {frames} steps; never `value`"}


if __name__ == "__main__":
    main()
