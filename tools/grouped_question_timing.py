"""A grouped question set against the per-cone loop, timed on one box in one process (DESIGN.md sections 19, 22, 24 and 25).

For each of truss1, chain16 and arrow128 (tests/golden/*.dat-s, at or near the state of the instance's golden): one operator over
all its cones and one question as the reference's line search puts it, never one a stored answer serves (every question moves by a
few parts in 10^7).  --kind says which:

    check   "interior at (tau, y)?" to every cone, then the log barrier at that point from every cone; y moves
    ratio   a ratio test on the dual buffer to every cone; a fixed seeded direction is scaled
            --buffer checker: on the checker buffer, after one ratio test along the direction and a step-and-check at half its
            smallest step have put every cone's checker at a trial point; the grouped forms have the ratio set's checker opt-in on
             -> profiles/grouped_ratio_checker_timing.jsonl
            --rest 1: the yardstick is not the loop but the grouped form with the safeguard's rest on the host; the other two
            forms have it in the launch (grouped_host_rest, grouped_device_rest and the two whole-operator forms); the record
            says how many members left the cone in the timed questions -> profiles/grouped_ratio_rest_timing.jsonl
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
REST_FORMS = ("grouped_host_rest", "grouped_device_rest", "grouped_host_rest_whole", "grouped_device_rest_whole")
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


def forms(kind, kkt, cones, tau, buffer=0):
    """(cone by cone, whole operator): what is timed, x -> check (flags, logdets, all), ratio (steps, smallest), step (flags, all,
    rc).  Chosen once per instance, so that the timed region holds one call and the question itself"""
    if kind == "check":
        def loop(x):
            flags = [c.check_is_interior(tau, x) for c in cones]
            return flags, [c.log_barrier(tau, x) for c in cones], all(flags)
        return loop, lambda x: kkt.check_is_interior(tau, x)
    if kind == "ratio":
        def loop(x):
            steps = [c.ratio_test(0.0, x, 0.0, buffer) for c in cones]
            return steps, min(steps)
        return loop, lambda x: kkt.ratio_test(0.0, x, 0.0, buffer)

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
    ap.add_argument("--buffer", choices=("dual", "checker"), default="dual", help="ratio: the buffer the ratio test is asked on")
    ap.add_argument("--rest", type=int, choices=(0, 1), default=0, help="ratio: 1 compares the safeguard's rest on the host and in the launch")
    args = ap.parse_args()
    if args.kind != "ratio" and (args.buffer != "dual" or args.rest):
        ap.error("--buffer and --rest belong to --kind ratio")
    if args.reps < 31:
        ap.error("--reps must be at least 31")
    kind = args.kind
    if kind == "check" and args.scale is not None:
        ap.error("--scale has no meaning for --kind check: its question moves the point, not a direction")
    if args.scale is None:
        args.scale = 0.05
    on_checker, names = args.buffer == "checker", (REST_FORMS if args.rest else FORMS)
    stem = "ratio_rest" if args.rest else "ratio_checker" if on_checker else kind
    out = args.out or os.path.join(ROOT, "profiles", f"grouped_{stem}_timing.jsonl")
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
                if kind == "step" or on_checker:
                    smin = min(c.ratio_test(0.0, dy) for c in cones)
                    assert 0.0 < smin < 1e6, (inst, smin)
                if on_checker:                                     # every cone's checker at a trial point, for good
                    assert all(c.axpy_buffer_and_check(0.5 * smin) for c in cones), inst
                loop, whole = forms(kind, kkt, cones, tau, api.BUFFER_DUALCHECK if on_checker else api.BUFFER_DUALVAR)
                t = {form: [] for form in names}
                asked = 0
                launches, fallbacks, smallest = {}, {form: 0 for form in names}, {}
                device_rests, device_cuts = {form: 0 for form in names}, {form: 0 for form in names}
                for rep in range(args.warmup + args.reps):
                    for form in names:
                        on = form.startswith("grouped")
                        assert switch(on) == (members if on and members >= 2 else 0)
                        if kind == "ratio":                         # (the opt-ins go off with the set's own switch)
                            assert kkt.set_grouped_ratio_checker(on and on_checker) == (members if on and on_checker else 0)
                            rest = on and "device_rest" in form
                            assert kkt.set_grouped_ratio_rest(rest) == (members if rest else 0)
                            dbefore = kkt.grouped_ratio_detail()
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
                            if kind == "ratio":
                                dafter = kkt.grouped_ratio_detail()
                                device_rests[form] += dafter["device_rests"] - dbefore["device_rests"]
                                device_cuts[form] += dafter["device_cuts"] - dbefore["device_cuts"]
                rec = {"instance": inst, "cones": len(cones), "members": members, "m": m, "reps": args.reps, "warmup": args.warmup,
                       "question": QUESTION[kind].replace("the dual buffer", "the checker buffer") if on_checker else QUESTION[kind], "clock": "host perf_counter around the whole question",
                       "grouped_launches_per_question": launches}
                if kind == "ratio":
                    rec.update({"direction_scale": args.scale, "smallest_step_of_the_last_question": smallest,
                                "safeguard_fallbacks_in_all_timed_questions": fallbacks, "buffer": args.buffer,
                                "device_rests_in_all_timed_questions": device_rests, "device_cuts_in_all_timed_questions": device_cuts})
                    if on_checker:
                        rec["checker_at_step"] = 0.5 * float(smin)
                if kind == "step":
                    rec.update({"direction_scale": args.scale, "smallest_ratio_test_step": float(smin)})
                for form in names:
                    rec[form] = stats(t[form])
                # (yardstick, form) pairs: the ratio of the medians, and whether the form's interquartile range lies below the yardstick's
                for a, b in ((names[0], names[1]), (names[2], names[3])):
                    rec[f"ratio_{a}_over_{b}"] = rec[a]["median_ms"] / rec[b]["median_ms"]
                    if kind == "ratio" and (on_checker or args.rest):
                        rec[f"{b}_iqr_below_{a}_iqr"] = rec[b]["q3_ms"] < rec[a]["q1_ms"]
                        rec[f"{b}_iqr_overlaps_{a}_iqr"] = not (rec[b]["q3_ms"] < rec[a]["q1_ms"] or rec[a]["q3_ms"] < rec[b]["q1_ms"])
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
