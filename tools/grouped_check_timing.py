"""The grouped interior check against the per-cone loop, timed on one box in one process.

For each of truss1, chain16 and arrow128 (tests/golden/*.dat-s, near the state of the instance's golden): one operator over all its
cones and one question as the reference's line search puts it -- "interior at (tau, y)?" to every cone, then the log barrier at
that point from every cone -- at a point no cone stands at (every question moves y by a few parts in 10^7).  Four forms:

    loop            switch off, cone by cone through HMiConeCheckIsInterior / HMiConeGetLogBarrier   (the yardstick)
    grouped         switch on, the same cone-by-cone calls (what an unchanged driver does)
    loop_whole      switch off, one HMiKKTCheckIsInterior call
    grouped_whole   switch on, one HMiKKTCheckIsInterior call

After a warm-up of all four they alternate question by question; a time is the host clock around the whole question (every
answer is on the host when it stops).  Per instance: the median of --reps questions of each form, its interquartile range and
min / max, and the ratios of the medians.  One JSON line per instance.

    python tools/grouped_check_timing.py --out profiles/grouped_check_timing.jsonl
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
INSTANCES = ("truss1", "chain16", "arrow128")
FORMS = ("loop", "grouped", "loop_whole", "grouped_whole")


def stats(ms):
    a = np.sort(np.asarray(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": med, "iqr_ms": q3 - q1, "min_ms": float(a[0]), "max_ms": float(a[-1])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_check_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--instances", nargs="*", default=list(INSTANCES))
    args = ap.parse_args()
    if args.reps < 31:
        ap.error("--reps must be at least 31")
    from hdsdp_amd import api
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for inst in args.instances:
            g = dict(np.load(os.path.join(GOLDEN, inst + "_A.npz")))
            m = int(g["mb_dims"][1])
            tau, y0 = float(g["tau"][0]), np.asarray(g["y"], dtype=np.float64)
            prob = api.read_sdpa(os.path.join(GOLDEN, inst + ".dat-s"))
            cones = [api.SDPCone.from_csc(b["n"], m, b["beg"], b["idx"], b["val"], iCone=k) for k, b in enumerate(prob["blocks"])]
            kkt = None
            try:
                for c in cones:
                    c.set_start(float(g["Rd"][0]))
                kkt = api.KKT(m, cones)
                members = kkt.grouped_check_info()["members"]
                t = {form: [] for form in FORMS}
                asked = 0
                launches = {}
                for rep in range(args.warmup + args.reps):
                    for form in FORMS:
                        on = form.startswith("grouped")
                        assert kkt.set_grouped_check(on) == (members if on and members >= 2 else 0)
                        asked += 1
                        y = y0 * (1.0 - 2e-7 * asked)                 # a new point for every question
                        before = kkt.grouped_check_info()["launches"]
                        t0 = time.perf_counter()
                        if form.endswith("whole"):
                            flags, logdets, every = kkt.check_is_interior(tau, y)
                        else:
                            flags = [c.check_is_interior(tau, y) for c in cones]
                            logdets = [c.log_barrier(tau, y) for c in cones]
                            every = all(flags)
                        dt = time.perf_counter() - t0
                        assert every and np.all(np.isfinite(logdets)), (inst, form, rep)
                        launches[form] = kkt.grouped_check_info()["launches"] - before
                        if rep >= args.warmup:
                            t[form].append(dt * 1e3)
                rec = {"instance": inst, "cones": len(cones), "members": members, "m": m, "reps": args.reps, "warmup": args.warmup,
                       "question": "interior at (tau, y) for every cone, then the log barrier at that point for every cone",
                       "clock": "host perf_counter around the whole question", "grouped_launches_per_question": launches}
                for form in FORMS:
                    rec[form] = stats(t[form])
                rec["ratio_loop_over_grouped"] = rec["loop"]["median_ms"] / rec["grouped"]["median_ms"]
                rec["ratio_loop_whole_over_grouped_whole"] = rec["loop_whole"]["median_ms"] / rec["grouped_whole"]["median_ms"]
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
            finally:
                if kkt is not None:
                    kkt.destroy()
                for c in cones:
                    c.destroy()


if __name__ == "__main__":
    main()
