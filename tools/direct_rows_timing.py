"""The two cutoffs of the direct rows (csrc/direct_rows.h), measured on one box in one process.

Points: for n in {256, 1024, 2000} and k in {1, 2, 4, 8, 16, 32, 64}, a block of one dense row and R triplet rows of k entries
each; the congruence stage of HKKTBuildUp (KKT.stage_times_ms()[1]: congruence launches, the writer, the I row) with
HDSDP_MI355X_DIRECT_ROWS = k (the R rows are written directly) and = 0 (the same rows through the congruence), at two row counts.
The per-row time of either is the difference of the two stage times over the difference of the row counts: the dense row, the
I row and the launch overheads drop out.  Best of --reps builds.

Mixed: n = m in {128, 256, 512, 1024, 2000}, 5 % dense rows, the others half rank one (three factor entries) and half triplet rows
of 1 .. 4 entries: the whole HKKTBuildUp (host clock around the call, which ends in a device synchronise), form on and off.

Derived: kmax(n) = the largest measured k up to which the writer's per-row time is at most HALF the congruence's; the floor =
the smallest measured n from which on the mixed build is not slower with the form (also given: not slower by more than the
5 % by which boxes and runs differ, which is what csrc/direct_rows.h takes); the writer's bytes/s at n = 2000 (every
128-byte line of a row, 16 n16 (n16 / 16 + 1) / 2 * 128 bytes, over its per-row time) against the achievable HBM figure.

One JSON line per point, per mixed case and for the derived figures.

    python tools/direct_rows_timing.py --out profiles/direct_rows_timing.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCH = "HDSDP_MI355X_DIRECT_ROWS"
HBM_ACHIEVABLE = 6.3e12      # bytes/s a streaming kernel reaches on the MI355X (8.0e12 on paper)
POINT_N = (256, 1024, 2000)
POINT_K = (1, 2, 4, 8, 16, 32, 64)
POINT_ROWS = {256: (64, 320), 1024: (32, 160), 2000: (16, 80)}
MIXED_N = (128, 256, 512, 1024, 2000)


def packed(i, j, n):
    return j * n - j * (j - 1) // 2 + (i - j)


def dense_column(rng, n):
    P = n * (n + 1) // 2
    return np.arange(P, dtype=np.int32), rng.standard_normal(P) / np.sqrt(n)


def triplet_column(rng, n, k):
    """k entries strictly below the diagonal (a lone diagonal entry would be a rank-one row)"""
    pos = set()
    while len(pos) < k:
        i, j = rng.integers(0, n, size=2)
        if i != j:
            pos.add((int(max(i, j)), int(min(i, j))))
    idx = np.array(sorted(packed(i, j, n) for i, j in pos), dtype=np.int32)
    return idx, rng.standard_normal(k)


def rank_one_column(rng, n, fill=3):
    sup = np.sort(rng.choice(n, size=fill, replace=False))
    a = 0.5 + rng.random(fill)
    sign = 1.0 if rng.random() < 0.5 else -1.0
    ent = sorted((packed(int(sup[p]), int(sup[q]), n), sign * a[p] * a[q]) for q in range(fill) for p in range(q, fill))
    return np.array([e[0] for e in ent], dtype=np.int32), np.array([e[1] for e in ent])


def objective_column(n):
    return np.array([packed(i, i, n) for i in range(n)], dtype=np.int32), 1.0 + 0.01 * (np.arange(n) % 5)


def point_columns(n, k, rows, seed=1):
    rng = np.random.default_rng(seed + 7 * n + k)
    yield (0,) + objective_column(n)
    yield (1,) + dense_column(rng, n)
    for r in range(rows):
        yield (2 + r,) + triplet_column(rng, n, k)


def mixed_columns(n, m, seed=2):
    """every 20th row dense; of the others, alternately rank one and a triplet row of 1 .. 4 entries"""
    rng = np.random.default_rng(seed + n)
    yield (0,) + objective_column(n)
    for r in range(m):
        if r % 20 == 10:
            yield (1 + r,) + dense_column(rng, n)
        elif r % 2 == 0:
            yield (1 + r,) + rank_one_column(rng, n)
        else:
            yield (1 + r,) + triplet_column(rng, n, 1 + (r // 2) % 4)


def timed_builds(api, n, m, columns, switch, reps):
    """(best congruence-stage ms, best whole-build ms, direct_rows()) of `reps` INFEASIBLE builds after one untimed build"""
    os.environ[SWITCH] = str(switch)
    cone = api.SDPCone.from_columns(n, m, columns)
    kkt = None
    try:
        cone.set_start(-10.0 * n)
        assert cone.check_is_interior(1.0, np.zeros(m))
        kkt = api.KKT(m, [cone])
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        stage, whole = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
            whole.append((time.perf_counter() - t0) * 1e3)
            stage.append(float(kkt.stage_times_ms()[1]))
        return min(stage), min(whole), cone.direct_rows()
    finally:
        if kkt is not None:
            kkt.destroy()
        cone.destroy()


def line_bytes(n):
    n16 = (n + 15) // 16 * 16
    nblk = n16 // 16
    return 16 * (nblk * (nblk + 1) // 2) * 128


def derive(points, mixed):
    kmax = {}
    for n in sorted({p["n"] for p in points}):
        best = 0
        for p in sorted((p for p in points if p["n"] == n), key=lambda p: p["k"]):
            if not (p["writer_us_per_row"] <= 0.5 * p["congruence_us_per_row"]):
                break
            best = p["k"]
        kmax[str(n)] = best
    floor = clear = None       # not slower at all; not slower by more than the boxes' 5 % spread
    for q in sorted(mixed, key=lambda q: -q["n"]):
        if not (q["build_ms_on"] <= q["build_ms_off"]):
            break
        floor = q["n"]
    for q in sorted(mixed, key=lambda q: -q["n"]):
        if not (q["build_ms_on"] <= 0.95 * q["build_ms_off"]):
            break
        clear = q["n"]
    big = [p for p in points if p["n"] == max(POINT_N) and p["k"] == 1]
    out = {"kind": "derived", "kmax_by_n": kmax, "floor_n": floor, "floor_n_outside_spread": clear, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}
    if big:
        bps = line_bytes(big[0]["n"]) / (big[0]["writer_us_per_row"] * 1e-6)
        out.update(writer_bytes_per_row=line_bytes(big[0]["n"]), writer_bytes_per_s=bps, writer_share_of_achievable=bps / HBM_ACHIEVABLE)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "direct_rows_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(POINT_N))
    ap.add_argument("--mixed-sizes", type=int, nargs="*", default=list(MIXED_N))
    args = ap.parse_args()
    from hdsdp_amd import api
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    points, mixed = [], []
    with open(args.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        for n in args.sizes:
            r1, r2 = POINT_ROWS.get(n, (32, 160))
            for k in POINT_K:
                t = {}
                for sw in (k, 0):
                    for rows in (r1, r2):
                        stage, _, dr = timed_builds(api, n, rows + 1, point_columns(n, k, rows), sw, args.reps)
                        assert dr[0] == (rows if sw else 0), (n, k, sw, rows, dr)
                        t[(sw != 0, rows)] = stage
                rec = {"kind": "point", "n": n, "k": k, "rows": [r1, r2],
                       "stage_ms_direct": [t[(True, r1)], t[(True, r2)]], "stage_ms_congruence": [t[(False, r1)], t[(False, r2)]],
                       "writer_us_per_row": (t[(True, r2)] - t[(True, r1)]) / (r2 - r1) * 1e3,
                       "congruence_us_per_row": (t[(False, r2)] - t[(False, r1)]) / (r2 - r1) * 1e3}
                points.append(rec)
                emit(rec)
        for n in args.mixed_sizes:
            on = timed_builds(api, n, n, mixed_columns(n, n), 8, 3)
            off = timed_builds(api, n, n, mixed_columns(n, n), 0, 3)
            rec = {"kind": "mixed", "n": n, "m": n, "direct_rows": list(on[2]), "build_ms_on": on[1], "build_ms_off": off[1],
                   "stage_ms_on": on[0], "stage_ms_off": off[0]}
            mixed.append(rec)
            emit(rec)
        emit(derive(points, mixed))


if __name__ == "__main__":
    main()
