"""Writes tests/golden/gemm_calls_parent.json: what every call site of the fp64 GEMM family computes and reports, case by case, on
the commit BEFORE the call forms of csrc/gemm_calls.h -- run from a work tree of that commit -- and again on the tree, which must
reproduce every string and integer (tests/test_gpu_gemm_calls.py): the arguments of every launch are the same, so the bits are.

Per case, through hdsdp_amd.api only: the per-role [flops, issued, launches] of HMiGetKernelTimingEx (float.hex and int) over the
case's calls, and its results -- M's lower triangle and the exported vectors of a build, the returned matrix or vector of a
utility -- every double as float.hex().  An array of more than 1024 doubles is recorded as the SHA-256 of its bytes, its length
and some 256 evenly spaced entries instead (a committed file stays under 1 MiB; equality of the digest is equality of every bit).

A case runs in a child process of its own when its switches are read once per process or it creates a sharded block.  Every case
is recorded twice; one whose two records differ is not deterministic, is left out and is named on stdout.

    python tools/gemm_calls_fixture.py [--root DIR] [out.json]      # DIR: the tree whose package is imported (default: this one)
    python tools/gemm_calls_fixture.py --case NAME                  # one record as a JSON line (what the child processes run)
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")          # inputs are always this tree's
N, M_ROWS = 144, 24                                      # the dense synthetic block: a short diagonal tile and a bottom edge


# ---- recording -----------------------------------------------------------------------------------------
def hexes(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64)).ravel()
    if a.size <= 1024:
        return [float(v).hex() for v in a]
    # (the samples, every (count / 256)-th entry, say where a difference begins; the digest says that there is none)
    step = a.size // 256
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "count": int(a.size), "samples": [float(v).hex() for v in a[::step]]}


class Timing:
    """kernel timing on over the body: the per-role [flops, issued, launches] of what it launched"""

    def __enter__(self):
        from hdsdp_amd import api
        self.lib = api.load_library()
        self._collect()                                  # (resets)
        self.lib.HMiSetKernelTiming(1)
        return self

    def _collect(self):
        ms, fl, iss, ln = np.zeros(5), np.zeros(5), np.zeros(5), np.zeros(5, dtype=np.int64)
        dp = C.POINTER(C.c_double)
        self.lib.HMiGetKernelTimingEx(ms.ctypes.data_as(dp), fl.ctypes.data_as(dp), iss.ctypes.data_as(dp), ln.ctypes.data_as(C.POINTER(C.c_int64)))
        return [[float(fl[r]).hex(), float(iss[r]).hex(), int(ln[r])] for r in range(5)]

    def __exit__(self, *exc):
        self.lib.HMiSetKernelTiming(0)
        self.roles = self._collect()
        return False


def build_record(kkt, m, kind, rec):
    from hdsdp_amd import api
    with Timing() as t:
        kkt.build_up(kind)
    ex = kkt.export()
    rec["roles"] = t.roles
    if kind != api.KKT_TYPE_CORRECTOR:                   # (the corrector builds no matrix)
        M = np.array(kkt.M, dtype=np.float64)            # C order: M[j, i] is element (row i, column j), valid where i >= j
        rec["M"] = hexes([M[j, i] for j in range(m) for i in range(j, m)])
    for k in ("ASinv", "ASinvRdSinv", "ASinvCSinv"):
        rec[k] = hexes(ex[k])
    rec["scalars"] = hexes([ex[k] for k in ("CSinvCSinv", "CSinv", "CSinvRdSinv", "TraceSinv")])
    return rec


def y_of(m):
    return 0.05 * np.sin(1.7 * np.arange(1, m + 1))


def primal_X(n):
    """the positive definite matrix of the KKT_TYPE_PRIMAL goldens (tests/util.py: primal_X)"""
    i = np.arange(n, dtype=np.float64)
    I, J = np.meshgrid(i, i, indexing="ij")
    X = 0.5 / n * np.cos(0.37 * (I + J) + 0.11 * I * J)
    X[np.arange(n), np.arange(n)] = 2.0 + 0.01 * (np.arange(n) % 7)
    return np.ascontiguousarray(X)


def strong_X(n, seed=7):
    """X = W^T diag(sigma) W with a third of sigma negative and a factor of modest growth (tests/test_gpu_primal_signed.py)"""
    rng = np.random.default_rng(seed + n)
    W = np.tril(rng.uniform(-1.0, 1.0, (n, n))) * 0.5 / np.sqrt(n)
    W[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n)
    sig = np.ones(n)
    sig[rng.choice(n, n // 3, replace=False)] = -1.0
    return np.ascontiguousarray(W.T @ (sig[:, None] * W))


def feasible_y(n, m):
    """the synthetic family's strictly feasible point (draws 2 m P .. of its stream, U(-1, 1)): primal recovery
    works on S = C - sum y_i A_i without the residual term"""
    g = np.uint64(0x9E3779B97F4A7C15)
    t = np.uint64(2 * m * (n * (n + 1) // 2)) + np.arange(m, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = g + (t + np.uint64(1)) * g
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return 2.0 * ((z >> np.uint64(11)).astype(np.float64) / 9007199254740992.0) - 1.0


def indef96_X():
    M = np.load(os.path.join(GOLDEN, "indef96.npz"))["indef_M"]
    return np.ascontiguousarray(np.triu(M) + np.triu(M, 1).T)


# ---- the cases -----------------------------------------------------------------------------------------
def dense_build(kind, n=N, m=M_ROWS, X=None, route=None):
    """one build of the synthetic dense block on the congruence + Gram path"""
    from hdsdp_amd import api
    cone = api.SDPCone.synthetic(n, m)
    try:
        cone.set_start(-200.0)
        assert cone.check_is_interior(0.9, y_of(m)) and cone.path == 0
        kkt = api.KKT(m, [cone])
        if X is not None:
            kkt.register_psdp([X])
        rec = build_record(kkt, m, kind, {"n": n, "m": m})
        if X is not None:
            r = cone.primal_route()
            rec["route"] = [int(r[0]), int(r[1]), float(r[2]).hex()]
            assert route is None or r[0] == route, (r, route)
        rec["exchange"] = [int(v) for v in cone.exchange_stats()]
        rec["shards"] = int(cone.shard_count())
        kkt.destroy()
        return rec
    finally:
        cone.destroy()


def golden_build(name, path, kinds):
    """the builds `kinds` of a golden problem's block, which takes `path` (1: rank one, 2: sparse gather)"""
    from hdsdp_amd import api
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n, m = int(g["dims"][0]), int(g["dims"][1])
    cone = api.SDPCone.from_csc(n, m, g["csc_beg"], g["csc_idx"], g["csc_val"])
    try:
        assert cone.path == path, (cone.path, path)
        cone.set_start(float(g["Rd"][0]))
        assert float(g["Rd"][0]) != 0.0 and cone.check_is_interior(float(g["tau"][0]), np.asarray(g["y"], dtype=np.float64))
        kkt = api.KKT(m, [cone])
        rec = {"n": n, "m": m, "builds": [build_record(kkt, m, k, {"kind": k}) for k in kinds]}
        kkt.destroy()
        return rec
    finally:
        cone.destroy()


def lp_build():
    from hdsdp_amd import api
    sys.path.insert(0, ROOT)
    from tools.lp_golden import make_case
    cs = make_case("small")                              # the inputs tests/golden/lp_small.npz was computed from (it holds results only)
    cone = api.LPCone.from_csc(cs["m"], cs["n"], cs["beg"], cs["idx"], cs["val"])
    cone.set_schur_path(api.LPCone.DENSE)
    assert cone.schur_path()[0] == api.LPCone.DENSE
    cone.set_start(cs["Rd"])
    assert cone.check_is_interior(cs["tau"], cs["y"])
    kkt = api.KKT(cs["m"], [cone])
    try:
        return build_record(kkt, cs["m"], api.KKT_TYPE_INFEASIBLE, {"m": cs["m"]})
    finally:
        kkt.destroy()
        cone.destroy()


def primal_utils():
    """build_primal_xsx and get_primal on the dense block"""
    from hdsdp_amd import api
    cone = api.SDPCone.synthetic(N, M_ROWS)
    try:
        cone.set_start(-200.0)
        y = y_of(M_ROWS)
        assert cone.check_is_interior(0.9, y)
        with Timing() as t:
            xsx = cone.build_primal_xsx(primal_X(N), np.zeros((N, N)))
            X = cone.get_primal(0.5, feasible_y(N, M_ROWS) + 1e-3 * np.sin(np.arange(M_ROWS)), 0.003 * np.cos(0.7 * np.arange(M_ROWS) + 0.2))
        assert X is not None
        return {"roles": t.roles, "xsx": hexes(xsx), "primal": hexes(X)}
    finally:
        cone.destroy()


def spd(n):
    i = np.arange(n, dtype=np.float64)
    A = np.cos(0.21 * np.add.outer(i, i)) + 0.3 * np.sin(0.05 * np.multiply.outer(i, i))
    return np.ascontiguousarray(0.5 * (A + A.T) / n + np.diag(1.5 + 0.01 * (np.arange(n) % 11)))


def invert(n):
    from hdsdp_amd import api
    ls = api.LinSys(n)
    try:
        with Timing() as t:
            ls.numeric(spd(n))
            inv = ls.invert()
        return {"roles": t.roles, "inverse": hexes(inv)}
    finally:
        ls.destroy()


def lu_solve():
    """the Schur system's object on a matrix that is not positive definite: the pivoted LU factor, 33 rows = one panel of 32 and a
    trailing update"""
    from hdsdp_amd import api
    m = 33
    A = spd(m)
    A[0, 0] = -1.0
    ls = api.LinSys(m, api.HDSDP_LINSYS_DENSE_ITERATIVE)
    try:
        with Timing() as t:
            ls.numeric(np.triu(A))
            x = ls.solve(np.cos(0.3 * np.arange(m)))
        assert ls.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
        return {"roles": t.roles, "x": hexes(x)}
    finally:
        ls.destroy()


def two_shards():
    from hdsdp_amd import api
    api.set_devices([0, 0], shard_min_dim=32, transport=api.TRANSPORT_COPY)
    rec = dense_build(api.KKT_TYPE_INFEASIBLE)
    assert rec["shards"] == 2 and rec["exchange"][0] == 2, rec["exchange"]      # two pieces: step 2 by tile-column mask when staged
    return rec


def _api():
    from hdsdp_amd import api
    return api


# name -> (environment of the case, whether it needs a process of its own, the record)
CASES = {
    "homogeneous": ({}, False, lambda: dense_build(_api().KKT_TYPE_HOMOGENEOUS)),
    "corrector": ({}, False, lambda: dense_build(_api().KKT_TYPE_CORRECTOR)),
    "primal_definite": ({}, False, lambda: dense_build(_api().KKT_TYPE_PRIMAL, X=primal_X(N), route=0)),
    "primal_indef96": ({}, False, lambda: dense_build(_api().KKT_TYPE_PRIMAL, n=96, X=indef96_X())),
    "primal_indef96_unsigned": ({"HDSDP_MI355X_PRIMAL_SIGNED": "0"}, False, lambda: dense_build(_api().KKT_TYPE_PRIMAL, n=96, X=indef96_X(), route=2)),
    "primal_signed": ({}, False, lambda: dense_build(_api().KKT_TYPE_PRIMAL, X=strong_X(N), route=1)),
    "primal_signed_off": ({"HDSDP_MI355X_PRIMAL_SIGNED": "0"}, False, lambda: dense_build(_api().KKT_TYPE_PRIMAL, X=strong_X(N), route=2)),
    "bc8": ({"HDM_BC": "8"}, False, lambda: dense_build(_api().KKT_TYPE_INFEASIBLE)),
    "nsplit8": ({"HDM_NSPLIT": "8", "HDM_GRAM_KSTAGES": "16"}, False, lambda: dense_build(_api().KKT_TYPE_INFEASIBLE, n=384)),
    "rank_one": ({}, False, lambda: golden_build("mcp100_A", 1, (0, 2, 1))),
    "sparse": ({}, False, lambda: golden_build("theta1_A", 2, (2,))),
    "lp": ({}, False, lp_build),
    "primal_utils": ({}, False, primal_utils),
    "invert256": ({}, False, lambda: invert(256)),
    "invert384": ({}, False, lambda: invert(384)),
    "invert384_generic": ({"HDM_CHOL_K128": "0"}, True, lambda: invert(384)),
    "lu33": ({}, False, lu_solve),
    "two_shards": ({"HDSDP_MI355X_A2A_PIECES": "2", "HDM_NSPLIT": "2"}, True, two_shards),   # (pieces are whole groups of splits)
}
MAY_DIFFER = ("two_shards",)


def record(name, root=ROOT, timeout=240):
    """the record of one case: here, under its environment, or in a child process (always when `root` is another tree)"""
    env, child, fn = CASES[name]
    if not child and root == ROOT:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return fn()
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    e = dict(os.environ, **env)
    e["PYTHONPATH"] = root + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--case", name], capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main(argv):
    root = ROOT
    if "--root" in argv:
        root = os.path.abspath(argv.pop(argv.index("--root") + 1))
        argv.remove("--root")
    sys.path.insert(0, root)
    if "--case" in argv:
        print(json.dumps(CASES[argv[argv.index("--case") + 1]][2](), sort_keys=True), flush=True)
        return 0
    out = next((a for a in argv if not a.startswith("--")), os.path.join(GOLDEN, "gemm_calls_parent.json"))
    res, left_out = {}, []
    for name in CASES:
        a, b = record(name, root, 600), record(name, root, 600)
        if a != b:
            assert name in MAY_DIFFER, f"case {name}: two records on one commit differ"
            left_out.append(name)
            continue
        res[name] = a
        print(f"{name}: recorded", flush=True)
    with open(out, "w") as f:
        json.dump(res, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(res)} cases" + (f"; not deterministic, left out: {left_out}" if left_out else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
