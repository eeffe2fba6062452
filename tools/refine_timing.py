"""What the refined Schur solve costs, timed on one box in one process.

For m = 500, 2000 and 8000: one dense operator over a synthetic block (host mirror off, so the residual reads the device matrix in
place and one factorisation serves every variant), and HKKTSolve of one right-hand side in five variants -- refinement off; on
under HKKTInit's own tolerance (here the first residual is below it: the cost is the residual pass alone); and on under a tolerance
nothing reaches with a cap of 1, 2 and 3 steps, so that the corrections are really made (their number per solve is recorded: the
loop still stops early when a step does not halve the residual).  After a warm-up the variants alternate solve by solve; a time is
the host clock around the call, which ends in a stream synchronisation.  Per size and variant: median, interquartile range and
min / max of --reps solves, and the difference to "off".

One JSON line per (m, variant).

    python tools/refine_timing.py --out profiles/refine_timing.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((500, 40), (2000, 80), (8000, 160))        # (m, n): n (n + 1) / 2 > m, so that M has full rank
# (name, step cap, tolerances): None = HKKTInit's own
VARIANTS = (("off", 0, None), ("residual only", 3, None), ("1 step", 1, 1e-30), ("2 steps", 2, 1e-30), ("3 steps", 3, 1e-30))


def stats(ms):
    a = np.sort(np.asarray(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": med, "iqr_ms": q3 - q1, "min_ms": float(a[0]), "max_ms": float(a[-1])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", nargs="*", type=int, default=[m for m, _ in SIZES])
    args = ap.parse_args()
    from hdsdp_amd import api
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for m, n in SIZES:
            if m not in args.sizes:
                continue
            cone = api.SDPCone.synthetic(n, m)
            kkt = None
            try:
                cone.set_start(-10.0 * n)
                assert cone.check_is_interior(1.0, np.zeros(m))
                kkt = api.KKT(m, [cone], host_mirror=False)
                kkt.set_refine(3)
                kkt.build_up(api.KKT_TYPE_INFEASIBLE)
                kkt.factorize()
                b = np.sin(np.arange(m) + 1.0)
                t = {name: [] for name, _, _ in VARIANTS}
                corr = {name: 0 for name, _, _ in VARIANTS}
                last = {}
                freed = True       # switching refinement off frees its work space: it comes back in a solve that is not timed
                for rep in range(args.warmup + args.reps):
                    for name, cap, tol in VARIANTS:
                        kkt.set_refine(cap)
                        if cap and freed:
                            kkt.solve(b)
                        freed = cap == 0
                        if tol is None:
                            kkt.set_param(relTol=5e-12 * (5.0 if m > 5000 else 1.0), absTol=1e-12 * (5.0 if m > 5000 else 1.0))
                        else:
                            kkt.set_param(relTol=tol, absTol=tol)
                        before = kkt.refine_stats()["total_steps"]
                        t0 = time.perf_counter()
                        kkt.solve(b)
                        dt = (time.perf_counter() - t0) * 1e3
                        st = kkt.refine_stats()
                        if rep >= args.warmup:
                            t[name].append(dt)
                            corr[name] += st["total_steps"] - before
                        last[name] = st
                off = stats(t["off"])
                for name, cap, tol in VARIANTS:
                    s = stats(t[name])
                    st = last[name]
                    rec = {"m": m, "n": n, "variant": name, "cap": cap, "tolerance": "HKKTInit" if tol is None else tol, "reps": args.reps,
                           "warmup": args.warmup, "status": st["status_name"], "corrections_per_solve": corr[name] / args.reps,
                           "resid0": st["resid0"], "resid": st["resid"], "work_bytes": last["3 steps"]["device_bytes"], **s,
                           "over_off_ms": s["median_ms"] - off["median_ms"], "spread_ms": max(s["iqr_ms"], off["iqr_ms"])}
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
            finally:
                if kkt is not None:
                    kkt.destroy()
                cone.destroy()


if __name__ == "__main__":
    main()
