"""A grouped question set against the per-cone loop, timed on one box in one process (DESIGN.md sections 19, 22, 24 and 25).

For each of truss1, chain16 and arrow128 (tests/golden/*.dat-s, at or near the state of the instance's golden): one operator over
all its cones and one question as the reference's line search puts it, never one a stored answer serves (every question moves by a
few parts in 10^7).  --kind says which:

    check   "interior at (tau, y)?" to every cone, then the log barrier at that point from every cone; y moves
    ratio   a ratio test on the dual buffer to every cone; a fixed seeded direction is scaled
    step    after one ratio test along a seeded direction, a step-and-check on the checker buffer to every cone; half the smallest
            ratio-test step is scaled

Four forms:

    loop            switch off, cone by cone through the cone's own call   (the yardstick)
    grouped         switch on, the same cone-by-cone calls (what an unchanged driver does)
    loop_whole      switch off, one call on the operator (HMiKKTCheckIsInterior / HMiKKTRatioTest / HMiKKTAddStepToBufferAndCheck)
    grouped_whole   switch on, one call on the operator

After a warm-up of all four they alternate question by question; a time is the host clock around the whole question (every
answer is on the host when it stops).  Per instance: the median of --reps questions of each form, its quartiles and min / max,
and the ratios of the medians; for step also whether each grouped form's interquartile range lies below its loop's without
overlap.  One JSON line per instance.

    python tools/grouped_question_timing.py --kind check     # -> profiles/grouped_check_timing.jsonl
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
QUESTION = {"check": "interior at (tau, y) for every cone, then the log barrier at that point for every cone",
            "ratio": "a ratio test on the dual buffer for every cone, along a direction no slot holds",
            "step": "a step-and-check on the checker buffer for every cone, at a step no slot holds, after a ratio test"}


def stats(ms):
    a = np.sort(np.asarray(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": med, "q1_ms": q1, "q3_ms": q3, "iqr_ms": q3 - q1, "min_ms": float(a[0]), "max_ms": float(a[-1])}


def pose(kind, asked, y0, dy, smin):
    """the `asked`-th question: a new point (check), a new direction (ratio), a new step (step)"""
    return y0 * (1.0 - 2e-7 * asked) if kind == "check" else dy * (1.0 + 2e-7 * asked) if kind == "ratio" else 0.5 * smin * (1.0 + 2e-7 * asked)


def forms(kind, kkt, cones, tau):
    """(cone by cone, whole operator): what is timed, x -> check (flags, logdets, all), ratio (steps, smallest), step (flags, all,
    rc).  Chosen once per instance, so that the timed region holds one call and the question itself"""
    if kind == "check":
        def loop(x):
            flags = [c.check_is_interior(tau, x) for c in cones]
            return flags, [c.log_barrier(tau, x) for c in cones], all(flags)
        return loop, lambda x: kkt.check_is_interior(tau, x)
    if kind == "ratio":
        def loop(x):
            steps = [c.ratio_test(0.0, x) for c in cones]
            return steps, min(steps)
        return loop, lambda x: kkt.ratio_test(0.0, x)

    def loop(x):
        flags = [c.axpy_buffer_and_check(x) for c in cones]
        return flags, all(flags), 0
    return loop, kkt.axpy_buffer_and_check


def good(kind, res):
    if kind == "check":
        return res[2] and np.all(np.isfinite(res[1]))
    if kind == "ratio":
        return res[1] > 0.0 and not np.any(np.isnan(res[0]))
    return res[2] == 0 and res[1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kind", required=True, choices=sorted(QUESTION))
    ap.add_argument("--out", default=None, help="default: profiles/grouped_<kind>_timing.jsonl")
    ap.add_argument("--reps", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=None, help="ratio, step: size of the direction relative to 1 + |y| (0.05)")
    ap.add_argument("--instances", nargs="*", default=list(INSTANCES))
    args = ap.parse_args()
    if args.reps < 31:
        ap.error("--reps must be at least 31")
    kind = args.kind
    if kind == "check" and args.scale is not None:
        ap.error("--scale has no meaning for --kind check: its question moves the point, not a direction")
    if args.scale is None:
        args.scale = 0.05
    out = args.out or os.path.join(ROOT, "profiles", f"grouped_{kind}_timing.jsonl")
    from hdsdp_amd import api
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
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
                info, switch = getattr(kkt, f"grouped_{kind}_info"), getattr(kkt, f"set_grouped_{kind}")
                members = info()["members"]
                dy = smin = None
                if kind != "check":
                    assert all(c.check_is_interior(tau, y0) for c in cones), inst
                    dy = np.random.default_rng(11).uniform(-1.0, 1.0, m) * args.scale * (1.0 + np.abs(y0))
                if kind == "step":
                    smin = min(c.ratio_test(0.0, dy) for c in cones)
                    assert 0.0 < smin < 1e6, (inst, smin)
                loop, whole = forms(kind, kkt, cones, tau)
                t = {form: [] for form in FORMS}
                asked = 0
                launches, fallbacks, smallest = {}, {form: 0 for form in FORMS}, {}
                for rep in range(args.warmup + args.reps):
                    for form in FORMS:
                        on = form.startswith("grouped")
                        assert switch(on) == (members if on and members >= 2 else 0)
                        asked += 1
                        x, ask = pose(kind, asked, y0, dy, smin), (whole if form.endswith("whole") else loop)
                        before = info()
                        t0 = time.perf_counter()
                        res = ask(x)
                        dt = time.perf_counter() - t0
                        assert good(kind, res), (inst, form, rep)
                        after = info()
                        launches[form] = after["launches"] - before["launches"]
                        smallest[form] = float(res[1]) if kind == "ratio" else None
                        if rep >= args.warmup:
                            t[form].append(dt * 1e3)
                            fallbacks[form] += after.get("fallbacks", 0) - before.get("fallbacks", 0)
                rec = {"instance": inst, "cones": len(cones), "members": members, "m": m, "reps": args.reps, "warmup": args.warmup,
                       "question": QUESTION[kind], "clock": "host perf_counter around the whole question",
                       "grouped_launches_per_question": launches}
                if kind == "ratio":
                    rec.update({"direction_scale": args.scale, "smallest_step_of_the_last_question": smallest,
                                "safeguard_fallbacks_in_all_timed_questions": fallbacks})
                if kind == "step":
                    rec.update({"direction_scale": args.scale, "smallest_ratio_test_step": float(smin)})
                for form in FORMS:
                    rec[form] = stats(t[form])
                rec["ratio_loop_over_grouped"] = rec["loop"]["median_ms"] / rec["grouped"]["median_ms"]
                rec["ratio_loop_whole_over_grouped_whole"] = rec["loop_whole"]["median_ms"] / rec["grouped_whole"]["median_ms"]
                if kind == "step":
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
