"""The grouped Schur build against the per-cone loop, timed on one box in one process.

For each of truss1, blocks3, chain16 and arrow128 (tests/golden/*.dat-s, at the state of the instance's golden): one operator over
all its cones, HKKTBuildUp(KKT_TYPE_INFEASIBLE) and HKKTBuildUp(KKT_TYPE_HOMOGENEOUS) with the switch off (the loop) and on (the
grouped pass).  After a warm-up of both, the two alternate build by build; a time is the host clock around the call, which ends
in kkt_pull's stream synchronisation, so nothing of a build is still in flight when its clock stops.  Per instance and type: the
median of --reps builds of either form, the spread of each (interquartile range and min / max), and the ratio of the medians.

One JSON line per (instance, type).

    python tools/grouped_build_timing.py --out profiles/grouped_build_timing.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
INSTANCES = ("truss1", "blocks3", "chain16", "arrow128")


def stats(ms):
    a = np.sort(np.asarray(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": med, "iqr_ms": q3 - q1, "min_ms": float(a[0]), "max_ms": float(a[-1])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_build_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--instances", nargs="*", default=list(INSTANCES))
    args = ap.parse_args()
    from hdsdp_amd import api
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for inst in args.instances:
            g = dict(np.load(os.path.join(GOLDEN, inst + "_A.npz")))
            m = int(g["mb_dims"][1])
            prob = api.read_sdpa(os.path.join(GOLDEN, inst + ".dat-s"))
            cones = [api.SDPCone.from_csc(b["n"], m, b["beg"], b["idx"], b["val"], iCone=k) for k, b in enumerate(prob["blocks"])]
            kkt = None
            try:
                for c in cones:
                    c.set_start(float(g["Rd"][0]))
                    assert c.check_is_interior(float(g["tau"][0]), np.asarray(g["y"], dtype=np.float64))
                kkt = api.KKT(m, cones)
                for name, typ in (("INFEASIBLE", api.KKT_TYPE_INFEASIBLE), ("HOMOGENEOUS", api.KKT_TYPE_HOMOGENEOUS)):
                    t = {0: [], 1: []}
                    info = None
                    for rep in range(args.warmup + args.reps):
                        for on in (0, 1):
                            grouped = kkt.set_grouped_build(bool(on))
                            t0 = time.perf_counter()
                            kkt.build_up(typ)
                            dt = (time.perf_counter() - t0) * 1e3
                            if rep >= args.warmup:
                                t[on].append(dt)
                            if on:
                                info = kkt.grouped_build_info()
                                assert info["cones"] == grouped, (info, grouped)
                    loop, grp = stats(t[0]), stats(t[1])
                    rec = {"instance": inst, "type": name, "m": m, "cones": len(cones), "grouped_cones": info["cones"], "jobs": info["jobs"],
                           "launches": info["launches"], "reps": args.reps, "warmup": args.warmup, "loop": loop, "grouped": grp,
                           "loop_over_grouped": loop["median_ms"] / grp["median_ms"],
                           "difference_ms": loop["median_ms"] - grp["median_ms"], "spread_ms": max(loop["iqr_ms"], grp["iqr_ms"])}
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
            finally:
                if kkt is not None:
                    kkt.destroy()
                for c in cones:
                    c.destroy()


if __name__ == "__main__":
    main()
