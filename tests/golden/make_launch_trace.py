"""Writes the launch table tests/test_launch_trace.py compares with: per golden crop and case, the kernel instances one forward launches
and the per-layer engine names.  Needs the GPU and the built library; run it on the commit whose kernel selection is to be kept, BEFORE a
change to the launch planner.  Names and counts only.

    python tests/golden/make_launch_trace.py [out.json]      (default: tests/golden/launch_trace.json)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (import paths)
import test_launch_trace as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else T.TABLE
    table = T.pack({T.crop_id(p): T.trace_crop(p) for p in T.CROPS})
    with open(out, "w") as f:
        json.dump(table, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(table['cases'])} crops, {sum(len(c) for c in table['cases'].values())} cases, {len(table['traces'])} distinct traces, "
          f"{len(table['instances'])} instances")
