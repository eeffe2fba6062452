"""HKKTBuildUp of an LP cone alone at the sizes of the LP-cone issue, on both Schur paths where they fit, and the dense path's
GEMM rate (Gram-role kernel timing).  One JSON line per case.

    python tools/lp_timing.py                         # all cases
    rocprofv3 --kernel-trace --stats -d OUT -o lp -- python tools/lp_timing.py     # kernel statistics, no counters
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (m, LP columns, entries per column or None = dense)
CASES = [(1000, 1000, None), (2000, 2000, None), (2000, 20000, 20)]
HOST_S = {(1000, 1000): 0.19, (2000, 2000): 1.54, (2000, 20000): 26.2}   # the reference's LPConeGetKKT, one host core


def make(m, n, per_col, seed=3):
    rng = np.random.default_rng(seed)
    if per_col is None:
        A = rng.uniform(-1.0, 1.0, (m, n))
        c = 0.5 * np.abs(A).sum(axis=0) + 1.0 + rng.uniform(0, 1, n)
        beg = (np.arange(m + 2, dtype=np.int64) * n).astype(np.int32)
        return beg, np.tile(np.arange(n, dtype=np.int32), m + 1), np.concatenate([c, A.ravel()])
    rows = np.sort(np.argsort(rng.random((n, m)), axis=1)[:, :per_col], axis=1)     # per_col distinct constraints a column
    vals = rng.uniform(-1.0, 1.0, (n, per_col))
    c = 0.5 * np.abs(vals).sum(axis=1) + 1.0 + rng.uniform(0, 1, n)
    cols = np.repeat(np.arange(n), per_col)
    order = np.lexsort((cols, rows.ravel()))                                          # by constraint, then LP column
    r, j, v = rows.ravel()[order], cols[order], vals.ravel()[order]
    beg = np.zeros(m + 2, dtype=np.int64)
    beg[1] = n
    beg[2:] = n + np.cumsum(np.bincount(r, minlength=m))
    return beg.astype(np.int32), np.concatenate([np.arange(n), j]).astype(np.int32), np.concatenate([c, v])


def main():
    from hdsdp_amd import api
    lib = api.load_library()
    for m, n, per in CASES:
        beg, idx, val = make(m, n, per)
        y = 0.3 * np.sin(1.7 * np.arange(1, m + 1))
        for path in (1, 2):
            cone = api.LPCone.from_csc(m, n, beg, idx, val)
            try:
                cone.set_schur_path(path)
            except api.HDSDPError:
                cone.destroy()
                continue
            cone.set_start(-20.0)
            assert cone.check_is_interior(0.9, y)
            kkt = api.KKT(m, [cone], host_mirror=False)
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)     # warm-up
            lib.HMiSetKernelTiming(1)
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
            ms, fl, la = np.zeros(5), np.zeros(5), np.zeros(5, dtype=np.int64)
            lib.HMiGetKernelTiming(api._dptr(ms), api._dptr(fl), la.ctypes.data_as(C.POINTER(C.c_int64)))
            lib.HMiSetKernelTiming(0)
            t = []
            for _ in range(10):
                t0 = time.perf_counter()
                kkt.build_up(api.KKT_TYPE_INFEASIBLE)
                t.append(time.perf_counter() - t0)
            _, td, tsp, nb = cone.schur_path()
            print(json.dumps({"m": m, "lp_cols": n, "per_col": per or m, "path": "dense" if path == 1 else "sparse",
                              "auto_path": "sparse" if tsp < td else "dense", "build_ms_min": round(1e3 * min(t), 4),
                              "build_ms_median": round(1e3 * float(np.median(t)), 4), "host_reference_s": HOST_S[(m, n)],
                              "gemm_ms": round(float(ms[3]), 4), "gemm_tflops": round(fl[3] / (ms[3] * 1e-3) / 1e12, 2) if ms[3] > 0 else None,
                              "pair_list_bytes": int(nb)}), flush=True)
            kkt.destroy()
            cone.destroy()


if __name__ == "__main__":
    main()
