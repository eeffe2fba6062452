"""The grouped step-and-check against the per-cone loop, timed on one box in one process.

For each of truss1, chain16 and arrow128 (tests/golden/*.dat-s, at the state of the instance's golden): one operator over all its
cones, one ratio test on the dual buffer along a seeded direction, and then one question as the reference's line search puts it --
a step-and-check on the checker buffer to every cone -- at a step no slot holds (every question scales half the smallest ratio-test
step by a few parts in 10^7 more).  Four forms:

    loop            switch off, cone by cone through HMiConeAddStepToBufferAndCheck   (the yardstick)
    grouped         switch on, the same cone-by-cone calls (what an unchanged driver does)
    loop_whole      switch off, one HMiKKTAddStepToBufferAndCheck call
    grouped_whole   switch on, one HMiKKTAddStepToBufferAndCheck call

After a warm-up of all four they alternate question by question; a time is the host clock around the whole question (every
answer is on the host when it stops).  Per instance: the median of --reps questions of each form, its quartiles and min / max,
the ratios of the medians, and whether each grouped form's interquartile range lies below its loop's without overlap.  One JSON
line per instance.

    python tools/grouped_step_timing.py --out profiles/grouped_step_timing.jsonl
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
    return {"median_ms": med, "q1_ms": q1, "q3_ms": q3, "iqr_ms": q3 - q1, "min_ms": float(a[0]), "max_ms": float(a[-1])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_step_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=0.05, help="size of the direction relative to 1 + |y|")
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
                members = kkt.grouped_step_info()["members"]
                assert all(c.check_is_interior(tau, y0) for c in cones), inst
                dy = np.random.default_rng(11).uniform(-1.0, 1.0, m) * args.scale * (1.0 + np.abs(y0))
                smin = min(c.ratio_test(0.0, dy) for c in cones)
                assert 0.0 < smin < 1e6, (inst, smin)
                t = {form: [] for form in FORMS}
                asked = 0
                launches = {}
                for rep in range(args.warmup + args.reps):
                    for form in FORMS:
                        on = form.startswith("grouped")
                        assert kkt.set_grouped_step(on) == (members if on and members >= 2 else 0)
                        asked += 1
                        step = 0.5 * smin * (1.0 + 2e-7 * asked)      # a new step for every question
                        before = kkt.grouped_step_info()
                        t0 = time.perf_counter()
                        if form.endswith("whole"):
                            flags, every, rc = kkt.axpy_buffer_and_check(step)
                        else:
                            flags = [c.axpy_buffer_and_check(step) for c in cones]
                            every, rc = all(flags), 0
                        dt = time.perf_counter() - t0
                        assert rc == 0 and every, (inst, form, rep)
                        after = kkt.grouped_step_info()
                        launches[form] = after["launches"] - before["launches"]
                        if rep >= args.warmup:
                            t[form].append(dt * 1e3)
                rec = {"instance": inst, "cones": len(cones), "members": members, "m": m, "reps": args.reps, "warmup": args.warmup,
                       "question": "a step-and-check on the checker buffer for every cone, at a step no slot holds, after a ratio test",
                       "direction_scale": args.scale, "smallest_ratio_test_step": float(smin),
                       "clock": "host perf_counter around the whole question", "grouped_launches_per_question": launches}
                for form in FORMS:
                    rec[form] = stats(t[form])
                rec["ratio_loop_over_grouped"] = rec["loop"]["median_ms"] / rec["grouped"]["median_ms"]
                rec["ratio_loop_whole_over_grouped_whole"] = rec["loop_whole"]["median_ms"] / rec["grouped_whole"]["median_ms"]
                rec["grouped_iqr_below_loop_iqr"] = rec["grouped"]["q3_ms"] < rec["loop"]["q1_ms"]
                rec["grouped_whole_iqr_below_loop_whole_iqr"] = rec["grouped_whole"]["q3_ms"] < rec["loop_whole"]["q1_ms"]
                rec["grouped_ranges_below_loop_ranges"] = (rec["grouped"]["max_ms"] < rec["loop"]["min_ms"] and
                                                           rec["grouped_whole"]["max_ms"] < rec["loop_whole"]["min_ms"])
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
