"""Writes tests/golden/work_plan_parent.json: what ShardPlan(n, m, world) and its hbm_bytes(rank) say over a grid that reaches
every branch of the GEMM path's work plan (csrc/work_plan.h).  The committed file was written by this script on the commit
BEFORE the plan moved into work_plan.h, i.e. by the Python re-derivation that commit still had; tests/test_dist_cpu.py holds
the library's pure query to it, integer by integer.

    python tools/work_plan_fixture.py [out.json]
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hdsdp_amd.dist import ShardPlan  # noqa: E402

ONE_DEVICE = [(200, 200), (640, 900), (1000, 1000), (2000, 2000), (2000, 8000)]
SHARDED = [(100, 101, 4), (17, 3, 2), (640, 900, 2), (2000, 2000, 8), (2000, 8000, 8), (2000, 8000, 2)]


def entry(n, m, world, rank):
    p = ShardPlan(n, m, world)
    parts = p.hbm_bytes(rank)
    label = [k for k in parts if "slabs for" in k]
    assert len(label) == 1, parts
    nslab, nsplit = map(int, re.search(r"\((\d+) slabs for (\d+) splits\)", label[0]).groups())
    nn = p.n16 * p.n16 * 8
    slab = nslab * p.R * p.R * 8
    # one device: T and the slabs are one part (the larger of the two); T's own size shows only where it is the larger
    tbytes = parts[label[0]] if world == 1 else parts["congruence intermediates T"]
    assert tbytes % nn == 0 and (world > 1 or tbytes > slab), (n, m, world, tbytes, slab)
    return {"n": n, "m": m, "world": world, "rank": rank,
            "layout": {k: int(getattr(p, k)) for k in ("n16", "nblk", "npb", "npb_loc", "Lr", "R", "chunk")},
            "Bc": tbytes // nn, "nsplit": nsplit, "nslab": nslab,
            "parts": {k: int(v) for k, v in parts.items()}}


def main(out):
    grid = [(n, m, 1, 0) for n, m in ONE_DEVICE]
    grid += [(n, m, w, r) for n, m, w in SHARDED for r in (0, w - 1)]
    with open(out, "w") as f:
        json.dump([entry(*g) for g in grid], f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "work_plan_parent.json"))
