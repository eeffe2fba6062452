"""What the refined solve of the TILE form costs, timed on one box in one process.

The banded cases of profiles/r03_d_tile_cholesky.txt (tools/probes/bsp_band.py's matrices): m = 20 000 and 200 000, a band of 40
below the diagonal, diagonally dominant.  An LP cone makes an operator dense and a banded operator of SDP cones at these sizes
takes tens of thousands of cones, so the measurement runs on the stand-alone tile object (HMiBspRefineTimingProbe): ONE
factorisation, then one right-hand side solved in five variants -- the unrefined tile solve (HdmBsp::solve_host, what HKKTSolve runs
with refinement off: the figure the others are to be compared with); refined under HKKTInit's own tolerance for the size (where the
first residual is below it the cost is the residual pass alone); and refined under a tolerance nothing reaches with a cap of 1, 2
and 3 steps, so that the corrections are really made (their number per solve is recorded: the loop still stops early when a step
does not halve the residual).  After a warm-up the variants alternate solve by solve; a time is the host clock around the solve,
which ends in a stream synchronisation.  Per size and variant: median, interquartile range and min / max of --reps solves, and
the difference to "off".  The refined variants read the accumulation store in place, as an operator with the host mirror off does;
with the mirror on the residual reads a copy instead, taken once per factorisation (a device copy of the store, not timed here).

One JSON line per (m, variant).

    python tools/refine_tiles_timing.py --out profiles/refine_tiles_timing.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (20000, 200000)
BAND = 40
# (name, step cap, tolerances): cap < 0 = the unrefined solve; None = HKKTInit's own
VARIANTS = (("off", -1, None), ("residual only", 3, None), ("1 step", 1, 1e-30), ("2 steps", 2, 1e-30), ("3 steps", 3, 1e-30))
STATUS = ("OFF", "CONVERGED", "STAGNATED", "MAXSTEPS", "NUMERICAL", "NO_MATRIX", "NOT_AVAILABLE")


def stats(ms):
    a = np.sort(np.asarray(ms))
    q1, med, q3 = (float(np.percentile(a, p)) for p in (25, 50, 75))
    return {"median_ms": med, "iqr_ms": q3 - q1, "min_ms": float(a[0]), "max_ms": float(a[-1])}


def banded(m):
    """bsp_band.py's matrix: uniform(-1, 1) on BAND sub-diagonals, diagonal = sum |row| + 1; lower-triangular CSC, diagonal first"""
    rng = np.random.RandomState(3)
    diags = [rng.uniform(-1, 1, m - k) for k in range(1, BAND + 1)]
    off = sp.diags(diags, [-k for k in range(1, BAND + 1)], shape=(m, m), format="csr")
    A = off + off.T
    A = (A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0)).tocsc()
    L = sp.tril(A, format="csc")
    L.sort_indices()
    beg, idx, val = L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(np.float64)
    assert np.all(idx[beg[:-1]] == np.arange(m))
    return beg, idx, val


def hkkt_tolerances(m):
    f = 100.0 if m > 20000 else 50.0 if m > 15000 else 5.0 if m > 5000 else 1.0     # hdsdp_schur.c:21-35
    return 5e-12 * f, 1e-12 * f


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_tiles_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", nargs="*", type=int, default=list(SIZES))
    args = ap.parse_args()
    from hdsdp_amd import api
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for m in args.sizes:
            beg, idx, val = banded(m)
            b = np.sin(np.arange(m) + 1.0)
            variants = [(cap,) + (hkkt_tolerances(m) if tol is None else (tol, tol)) for _, cap, tol in VARIANTS]
            ms, corr, status, r0, r1, st, work = api.bsp_refine_timing(m, beg, idx, val, b, variants, warmup=args.warmup, reps=args.reps)
            off = stats(ms[0])
            for k, (name, cap, tol) in enumerate(VARIANTS):
                s = stats(ms[k])
                rec = {"m": m, "band": BAND, "tiles": int(st[1]), "levels": int(st[2]), "store_bytes": 8 * 16384 * (int(st[1]) + 1),
                       "variant": name, "cap": max(cap, 0), "tolerance": "HKKTInit" if tol is None else tol, "reps": args.reps,
                       "warmup": args.warmup, "status": STATUS[int(status[k])], "corrections_per_solve": float(corr[k]) / args.reps,
                       "resid0": float(r0[k]), "resid": float(r1[k]), "work_bytes": int(work), **s,
                       "over_off_ms": s["median_ms"] - off["median_ms"], "spread_ms": max(s["iqr_ms"], off["iqr_ms"])}
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
