"""KKT_TYPE_PRIMAL with a registered X that is not positive definite, route 1 (csrc/engine_build.h: build_primal): the signed
factor J X J = F S F^T without pivoting (HdmChol::factor_signed), W = J F^T J and sigma = J S J so that X = W^T diag(sigma) W, the
congruence path with W in Linv's place and the signed Gram correction.  Checked against the plain-C oracle's typeKKT = 3 branch
(tr(A_i X A_j X) with X in S^-1's place), against route 2 (the row-by-row fallback), on sharded blocks in child processes, at
n = m = 2000 against numpy fp64, and with HDSDP_MI355X_PRIMAL_SIGNED=0."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import check_close, load_golden, lower_mask, primal_X, rel_err, y_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def near_pd_X(n, q):
    """the KKT_TYPE_PRIMAL goldens' positive definite X shifted between its q-th and (q+1)-th eigenvalue: q negative"""
    P = primal_X(n)
    w = np.linalg.eigvalsh(P)
    return P - 0.5 * (w[q - 1] + w[q]) * np.eye(n), q


def strong_X(n, seed=7):
    """X = W^T diag(sigma) W with a third of sigma negative: strongly indefinite (inertia n/3 negative), and a factor of
    modest growth by construction (the no-pivot LDL' of J X J reproduces W and sigma)"""
    rng = np.random.default_rng(seed + n)
    W = np.tril(rng.uniform(-1.0, 1.0, (n, n))) * 0.5 / np.sqrt(n)
    W[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n)
    sig = np.ones(n)
    sig[rng.choice(n, n // 3, replace=False)] = -1.0
    return np.ascontiguousarray(W.T @ (sig[:, None] * W)), n // 3


def _check_all(kkt, ref, m, what):
    ex = kkt.export()
    check_close(kkt.M[lower_mask(m)], ref["M"][lower_mask(m)], what + " M")
    check_close(ex["ASinv"], ref["ASinv"], what + " ASinv")
    check_close(ex["ASinvRdSinv"], ref["ASinvRdSinv"], what + " ASinvRdSinv")
    check_close([ex["TraceSinv"]], [ref["TraceSinv"]], what + " TraceSinv")


def _golden_cone(name):
    import oracle_py
    from hdsdp_amd import api
    g = load_golden(name)
    n, m = int(g["dims"][0]), int(g["dims"][1])
    if "csc_beg" in g:
        beg, idx, val = g["csc_beg"], g["csc_idx"], g["csc_val"]
        cone = api.SDPCone.from_csc(n, m, beg, idx, val)
    else:
        beg, idx, val, _ = oracle_py.synth_csc(n, m)
        cone = api.SDPCone.synthetic(n, m)
    return g, n, m, cone, oracle_py.Block(n, m, beg, idx, val)


@pytest.mark.parametrize("kind", ["near_pd", "strong"])
@pytest.mark.parametrize("name", ["syn64", "syn100", "syn96x40_B", "mix40_A", "theta1_B"])
def test_signed_route_against_the_oracle(name, kind, monkeypatch):
    from hdsdp_amd import api
    monkeypatch.setenv("HDSDP_MI355X_FORCE_GEMM", "1")      # theta1 would take the gather path (a primal build runs the GEMM path anyway)
    g, n, m, cone, blk = _golden_cone(name)
    kkt = api.KKT(m, [cone])
    try:
        Rd = float(g["Rd"][0])
        cone.set_start(Rd)
        assert cone.check_is_interior(float(g["tau"][0]), y_of(g))
        X, q = near_pd_X(n, 4) if kind == "near_pd" else strong_X(n)
        assert int(np.sum(np.linalg.eigvalsh(X) < 0)) == q
        kkt.register_psdp([X])
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        route, nq, growth = cone.primal_route()
        assert (route, nq) == (1, q), (route, nq, growth)
        assert 0.0 < growth <= 8.0 * np.sqrt(n)
        _check_all(kkt, blk.kkt_build(X, Rd, 3), m, f"{name} {kind}")
        # a positive definite X afterwards is route 0 again, with the unchanged "S row"
        P = primal_X(n)
        kkt.register_psdp([P])
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        assert cone.primal_route()[0] == 0
        _check_all(kkt, blk.kkt_build(P, Rd, 3), m, f"{name} definite after signed")
    finally:
        kkt.destroy()
        cone.destroy()
        blk.close()


def test_route_one_agrees_with_route_two_and_a_zero_pivot_falls_back(monkeypatch):
    """n = 200: the signed route and the row-by-row fallback (HDSDP_MI355X_PRIMAL_SIGNED=0, read per build) to 1e-12; then an X
    whose first pivot in reversed order (X[n-1, n-1]) is exactly zero: route 2, still the oracle's numbers"""
    import oracle_py
    from hdsdp_amd import api
    n, m = 200, 60
    beg, idx, val, _ = oracle_py.synth_csc(n, m)
    blk = oracle_py.Block(n, m, beg, idx, val)
    cone = api.SDPCone.synthetic(n, m)
    kkt = api.KKT(m, [cone])
    try:
        Rd = -2.5 * n
        cone.set_start(Rd)
        assert cone.check_is_interior(1.0, 0.02 * np.sin(1.3 * np.arange(m) + 0.4))
        X, q = strong_X(n)
        kkt.register_psdp([X])
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        assert cone.primal_route()[:2] == (1, q)
        prof = cone.primal_profile()
        assert prof is not None and prof["columns"] > 0 and prof["correction_ms"] > 0.0
        M1, e1 = kkt.M.copy(), kkt.export()
        monkeypatch.setenv("HDSDP_MI355X_PRIMAL_SIGNED", "0")
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        assert cone.primal_route() == (2, 0, 0.0)
        M2, e2 = kkt.M.copy(), kkt.export()
        msk = lower_mask(m)
        assert rel_err(M1[msk], M2[msk]) < 1e-12
        for k in ("ASinv", "ASinvRdSinv"):
            assert rel_err(e1[k], e2[k]) < 1e-12, k
        assert abs(e1["TraceSinv"] - e2["TraceSinv"]) <= 1e-12 * abs(e2["TraceSinv"])
        monkeypatch.delenv("HDSDP_MI355X_PRIMAL_SIGNED")
        Z = X.copy()
        Z[n - 1, n - 1] = 0.0
        kkt.register_psdp([Z])
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        route, _, growth = cone.primal_route()
        assert route == 2 and growth == 0.0
        _check_all(kkt, blk.kkt_build(Z, Rd, 3), m, "zero first pivot")
        # a random symmetric X: its no-pivot factor grows far past the acceptance bound -- route 2, growth reported
        G = np.random.default_rng(5).uniform(-1.0, 1.0, (n, n))
        Y = 0.5 * (G + G.T)
        kkt.register_psdp([Y])
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        route, _, growth = cone.primal_route()
        assert route == 2 and growth > 8.0 * np.sqrt(n), (route, growth)
        _check_all(kkt, blk.kkt_build(Y, Rd, 3), m, "large growth")
    finally:
        kkt.destroy()
        cone.destroy()
        blk.close()


def _worker(tmp_path, tag, n, m, world, X, env=None, timeout=240):
    xp, op = str(tmp_path / f"x_{tag}.npy"), str(tmp_path / f"o_{tag}.npz")
    np.save(xp, X)
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(HERE, "primal_signed_worker.py"), str(n), str(m), str(world), xp, op],
                       capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return dict(np.load(op)), r.stderr


@pytest.mark.parametrize("n,m,world,pieces", [(200, 131, 3, None), (96, 50, 2, None), (200, 131, 2, "1")])
def test_sharded_block_takes_the_signed_route(tmp_path, n, m, world, pieces):
    """a sharded block (in-process loopback group, fresh child process) with an indefinite X: route 1, the single-device build's
    numbers and the oracle's.  Before route 1 the sharded build refused any indefinite X."""
    import oracle_py
    X, q = strong_X(n, seed=3)
    env = {"HDSDP_MI355X_A2A_PIECES": pieces} if pieces else {}
    one, _ = _worker(tmp_path, "one", n, m, 1, X, env)
    sh, _ = _worker(tmp_path, "sh", n, m, world, X, env)
    assert int(sh["shards"][0]) == world and int(one["shards"][0]) == 1
    assert int(sh["ok"][0]) == 1 and int(one["ok"][0]) == 1
    assert (int(sh["route"][0]), int(sh["route"][1])) == (1, q)
    assert (int(one["route"][0]), int(one["route"][1])) == (1, q)
    msk = lower_mask(m)
    beg, idx, val, _ = oracle_py.synth_csc(n, m)
    blk = oracle_py.Block(n, m, beg, idx, val)
    try:
        ref = blk.kkt_build(X, -2.5 * n, 3)
    finally:
        blk.close()
    for got in (one, sh):
        check_close(got["M"][msk], ref["M"][msk], "sharded M")
        for k in ("ASinv", "ASinvRdSinv"):
            check_close(got[k], ref[k], k)
        check_close(got["TraceSinv"], [ref["TraceSinv"]], "TraceSinv")
    assert rel_err(sh["M"][msk], one["M"][msk]) < 1e-12


def test_switch_off_restores_the_old_routing(tmp_path):
    """HDSDP_MI355X_PRIMAL_SIGNED=0 in a child: one device takes route 2 (and still builds), a sharded block refuses, as before"""
    n, m = 96, 50
    X, _ = strong_X(n, seed=3)
    env = {"HDSDP_MI355X_PRIMAL_SIGNED": "0"}
    one, _ = _worker(tmp_path, "one0", n, m, 1, X, env)
    assert int(one["ok"][0]) == 1 and int(one["route"][0]) == 2
    sh, err = _worker(tmp_path, "sh0", n, m, 2, X, env)
    assert int(sh["ok"][0]) == 0 and int(sh["route"][0]) == 2
    assert "not supported on a sharded block" in err


def _sampled_check(kkt, cone, X, n, rows, cols):
    """M_ij = tr(A_i X A_j X) and ASinv_i = tr(A_i X) from the generator's matrices in numpy fp64, for a sample"""
    import oracle_py
    ex = kkt.export()
    A = {c: oracle_py.synth_matrix(n, c) for c in sorted(set(rows) | set(cols))}
    M = kkt.M
    got, want = [], []
    for i in rows:
        B = X @ A[i] @ X
        for j in cols:
            r, c = max(i, j), min(i, j)
            got.append(M[c, r])
            want.append(float(np.sum(B * A[j])))
    check_close(got, want, "sampled M")
    check_close(ex["ASinv"][rows], [float(np.sum(A[i] * X)) for i in rows], "sampled ASinv")


def test_at_size_resident_n2000():
    """n = m = 2000, resident synthetic data, X = the goldens' positive definite primal matrix shifted to five negative
    eigenvalues: route 1 with q = 5, a seeded sample of M and ASinv against numpy fp64"""
    from hdsdp_amd import api
    n = m = 2000
    X, q = near_pd_X(n, 5)
    cone = api.SDPCone.synthetic(n, m)
    kkt = api.KKT(m, [cone])
    try:
        cone.set_start(-10.0 * n)
        assert cone.check_is_interior(1.0, np.zeros(m))
        kkt.register_psdp([X])
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        route, nq, growth = cone.primal_route()
        assert (route, nq) == (1, q), (route, nq, growth)
        rng = np.random.default_rng(2000)
        rows = sorted(rng.choice(m, 3, replace=False).tolist())
        cols = sorted(set(rng.choice(m, 5, replace=False).tolist()) | set(rows))
        _sampled_check(kkt, cone, X, n, rows, cols)
    finally:
        kkt.destroy()
        cone.destroy()


def test_streamed_one_device(monkeypatch):
    """n = 1000, m = 4000 with the constraint data regenerated batch by batch (HDSDP_MI355X_STREAM_A=1), a strongly indefinite X:
    route 1, sampled rows against numpy fp64"""
    from hdsdp_amd import api
    monkeypatch.setenv("HDSDP_MI355X_STREAM_A", "1")
    n, m = 1000, 4000
    X, q = strong_X(n)
    cone = api.SDPCone.synthetic(n, m)
    kkt = api.KKT(m, [cone])
    try:
        assert cone.streaming()[0]
        cone.set_start(-10.0 * n)
        assert cone.check_is_interior(1.0, np.zeros(m))
        kkt.register_psdp([X])
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        assert cone.primal_route()[:2] == (1, q)
        rng = np.random.default_rng(4000)
        rows = sorted(rng.choice(m, 3, replace=False).tolist())
        cols = sorted(set(rng.choice(m, 5, replace=False).tolist()) | set(rows))
        _sampled_check(kkt, cone, X, n, rows, cols)
    finally:
        kkt.destroy()
        cone.destroy()
