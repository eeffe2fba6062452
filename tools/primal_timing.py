"""One KKT_TYPE_PRIMAL HKKTBuildUp of a synthetic block at n = m = 2000 on each route (csrc/engine_build.h: build_primal):
route 0 with the goldens' positive definite X, route 1 with an indefinite X (a shift to five negative eigenvalues, and a strongly
indefinite X with a third of its eigenvalues negative), route 2 (HDSDP_MI355X_PRIMAL_SIGNED=0) on the near-definite X.  Routes 0
and 1 are built once untimed, then timed; route 2 is one timed build of every row, or -- with --route2-rows R -- of a block with R
constraints, extrapolated linearly in the row count (a row costs three n^3 GEMMs and one pass over all m constraint matrices,
so the extrapolation to m rows scales that pass with m too: t(m) ~ t(R) * m / R * m / R for the pass share; stated in the record).
Route 1's record carries the split of its signed part (HMiConeGetPrimalProfile) and the correction's TFLOP/s.  One JSON line per case.

    python tools/primal_timing.py --out profiles/r07_primal_timing.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def primal_X(n):
    """tests/util.py: primal_X -- the KKT_TYPE_PRIMAL goldens' positive definite X"""
    i = np.arange(n, dtype=np.float64)
    I, J = np.meshgrid(i, i, indexing="ij")
    X = 0.5 / n * np.cos(0.37 * (I + J) + 0.11 * I * J)
    X[np.arange(n), np.arange(n)] = 2.0 + 0.01 * (np.arange(n) % 7)
    return np.ascontiguousarray(X)


def shifted_X(n, q):
    P = primal_X(n)
    w = np.linalg.eigvalsh(P)
    return P - 0.5 * (w[q - 1] + w[q]) * np.eye(n)


def strong_X(n, seed=7):
    rng = np.random.default_rng(seed + n)
    W = np.tril(rng.uniform(-1.0, 1.0, (n, n))) * 0.5 / np.sqrt(n)
    W[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n)
    sig = np.ones(n)
    sig[rng.choice(n, n // 3, replace=False)] = -1.0
    return np.ascontiguousarray(W.T @ (sig[:, None] * W))


def build(api, n, m, X, warm, signed=True):
    if signed:
        os.environ.pop("HDSDP_MI355X_PRIMAL_SIGNED", None)
    else:
        os.environ["HDSDP_MI355X_PRIMAL_SIGNED"] = "0"
    cone = api.SDPCone.synthetic(n, m)
    kkt = api.KKT(m, [cone], host_mirror=False)
    try:
        cone.set_start(-10.0 * n)
        assert cone.check_is_interior(1.0, np.zeros(m))
        kkt.register_psdp([X])
        if warm:
            kkt.build_up(api.KKT_TYPE_PRIMAL)
        t0 = time.perf_counter()
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        ms = (time.perf_counter() - t0) * 1e3
        return ms, cone.primal_route(), cone.primal_profile()
    finally:
        kkt.destroy()
        cone.destroy()
        os.environ.pop("HDSDP_MI355X_PRIMAL_SIGNED", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--m", type=int, default=2000)
    ap.add_argument("--route2-rows", type=int, default=0, help="time route 2 on this many rows and extrapolate (0: all rows)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hdsdp_amd import api
    n, m = a.n, a.m
    lines = []

    def emit(d):
        d.update({"n": n, "m": m})
        print(json.dumps(d), flush=True)
        lines.append(d)

    ms, r, _ = build(api, n, m, primal_X(n), True)
    emit({"case": "route0_pd", "build_ms": ms, "route": r[0]})
    for label, X in (("route1_shift_q5", shifted_X(n, 5)), ("route1_strong_q_n3", strong_X(n))):
        ms, r, prof = build(api, n, m, X, True)
        d = {"case": label, "build_ms": ms, "route": r[0], "q": r[1], "growth": r[2], "growth_over_sqrt_n": r[2] / np.sqrt(n)}
        if prof:
            d.update(prof)
            R = m + 3                                    # Gram rows (constraints + augmented): flops of the correction
            flops = R * (R + 1) / 2.0 * prof["columns"] * 2.0
            d["correction_tflops"] = flops / (prof["correction_ms"] * 1e-3) / 1e12 if prof["correction_ms"] > 0 else None
            d["signed_share_of_build"] = (prof["gather_ms"] + prof["correction_ms"] + prof["combine_ms"]) / ms
            d["gather_share_of_build"] = prof["gather_ms"] / ms
            d["correction_share_of_build"] = (prof["correction_ms"] + prof["combine_ms"]) / ms
        emit(d)
    rows = a.route2_rows if 0 < a.route2_rows < m else m
    ms, r, _ = build(api, n, rows, shifted_X(n, 5), False, signed=False)
    d = {"case": "route2_fallback", "route": r[0], "rows_timed": rows, "build_ms_timed": ms}
    if rows < m:
        d["build_ms"] = ms * (m / rows) ** 2
        d["extrapolated"] = "build_ms = build_ms_timed * (m / rows)^2: every row's pass over the constraint data grows with m too"
    else:
        d["build_ms"] = ms
        d["extrapolated"] = False
    emit(d)
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
