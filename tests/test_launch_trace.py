"""Which kernel every launch runs is pinned here (-m gpu).

The parity tests accept any kernel that computes the right tensors: a planner change that sent a layer to a slower but still correct
instantiation would pass them all.  For every golden crop of test_instances.py and every way of calling the forward that changes the
selection (plan variants x output kinds x fp32 / int8 frames, grouped launches, the debug forward's tap combinations) this file runs ONE
forward, takes the kernel instances whose launch counters (sesrq_instance_launches) moved and the per-layer engine names
(sesrq_layer_engine), and compares them with tests/golden/launch_trace.json -- a table recorded from the library
(tests/golden/make_launch_trace.py) before the planner was last restructured.  The results are checked against the reference's tensors too,
so the launches count as checked ones (Track).

What the table can and cannot see: the library counts launches per instance and keeps no order, so a case is the MULTISET of instances of
one forward (name -> launches) plus the per-layer engine names; two layers that swapped kernels of the same multiset would pass.  The plain
and the grouped forwards run under every plan variant; the debug forwards (taps switch the trio off and move layers to the dot4 kernels)
under four of them: default, dot4 engine, force_general, reduced_forms = 0.
"""
import json
import os

import pytest
import torch

from conftest import GOLDEN
from helpers import bundle_from_oracle, device, fixture_case, same
import sesrq
from sesrq import _lib
from instances import CROPS, OUT_KINDS, Track, plan_variants, shuffle

pytestmark = pytest.mark.gpu

TABLE = os.path.join(GOLDEN, "launch_trace.json")
# the debug forward's taps: PE sums, overflow counters, the input taps (input.0 among them), and everything at once
DEBUG_TAPS = {"pe": dict(pe=True, acts=False), "overflow": dict(pe=False, overflow=True, acts=False),
              "input0": dict(pe=False, acts=True), "all": dict(pe=True, overflow=True, acts=True, special=True)}


def label(kw):
    return ",".join(f"{k}={int(v)}" for k, v in sorted(kw.items())) or "default"


def trace_crop(path):
    """{case label: {"engines": [per layer], "launches": {instance name: launches of ONE forward}}} of one golden crop."""
    fx, meta, net, x = fixture_case(path)
    want_q, want_f = shuffle(fx["input5"], net.pixel_shuffle), fx["out"]
    inputs = {"f32": torch.from_numpy(x).to(device()), "i8": torch.from_numpy(fx["input0"]).to(device())}
    b = bundle_from_oracle(net)
    out = {}

    def record(case, e, run):
        with Track(pinned=True) as t:
            q, y = run()
            torch.cuda.synchronize()
            after = _lib.instances()
            if q is not None:
                same(f"{case} q_out", q, want_q)
            if y is not None:
                same(f"{case} y", y, want_f)
        assert case not in out
        out[case] = {"engines": e.layer_engines(), "launches": {k: v - t.before.get(k, 0) for k, v in after.items() if v > t.before.get(k, 0)}}

    stream = torch.cuda.Stream(device=device())
    for kw in plan_variants():
        e = sesrq.Engine(b, device(), **kw)
        for src, xt in inputs.items():
            for wq, wf in OUT_KINDS:
                record(f"{label(kw)}|{src}|q{int(wq)}f{int(wf)}", e, lambda: e.forward(xt, want_q=wq, want_f=wf))
                if kw not in (dict(), dict(fuse_hidden=0)):
                    continue
                # two frames of one stream as the images of ONE launch sequence (sesrq_forward_many, group = 2)
                frames = [xt.clone() for _ in range(2)]
                oq = [torch.zeros(want_q.shape, dtype=torch.int8, device=device()) for _ in range(2)] if wq else None
                of = [torch.zeros(want_f.shape, dtype=torch.float32, device=device()) for _ in range(2)] if wf else None
                torch.cuda.synchronize()

                def grouped():
                    e.submission(frames, oq, [stream], outs_f=of, group=2).enqueue(2)
                    torch.cuda.synchronize()
                    if oq:
                        same("grouped frame 0 q_out", oq[0], want_q)
                    if of:
                        same("grouped frame 0 y", of[0], want_f)
                    return (oq[1] if oq else None), (of[1] if of else None)
                record(f"{label(kw)}|{src}|q{int(wq)}f{int(wf)}|group2", e, grouped)
    for kw in (dict(), dict(engine=_lib.ENGINE_DOT4), dict(force_general=True), dict(reduced_forms=0)):
        e = sesrq.Engine(b, device(), **kw)
        for src, xt in inputs.items():
            for name, taps in DEBUG_TAPS.items():
                def debug():
                    res = e.forward_debug(xt, **taps)
                    return res["q_out"], res["y"]
                record(f"{label(kw)}|{src}|debug:{name}", e, debug)
    return out


def crop_id(path):
    return os.path.basename(path)[:-4]


def pack(traces):
    """{crop: {case: trace}} -> the table's form: instance names and distinct traces once, a trace index per case."""
    names = sorted({n for cases in traces.values() for t in cases.values() for n in t["launches"]})
    idx = {n: i for i, n in enumerate(names)}
    distinct, cases = [], {}
    for crop in sorted(traces):
        cases[crop] = {}
        for case, t in traces[crop].items():
            rec = {"engines": t["engines"], "launches": sorted([idx[n], c] for n, c in t["launches"].items())}
            if rec not in distinct:
                distinct.append(rec)
            cases[crop][case] = distinct.index(rec)
    return {"instances": names, "traces": distinct, "cases": cases}


def unpack(table, crop):
    names = table["instances"]
    return {case: {"engines": table["traces"][i]["engines"], "launches": {names[j]: c for j, c in table["traces"][i]["launches"]}}
            for case, i in table["cases"][crop].items()}


@pytest.mark.parametrize("path", CROPS, ids=[crop_id(p) for p in CROPS])
def test_every_launch_runs_the_recorded_kernel(path):
    with open(TABLE) as f:
        want = unpack(json.load(f), crop_id(path))
    got = trace_crop(path)
    assert sorted(got) == sorted(want), "the cases of this test and of tests/golden/launch_trace.json differ"
    bad = [c for c in got if got[c] != want[c]]
    assert not bad, f"{len(bad)} of {len(got)} cases launch other kernels than recorded; first: {bad[0]}\n  got  {got[bad[0]]}\n  want {want[bad[0]]}"
