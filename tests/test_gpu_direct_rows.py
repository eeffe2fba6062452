"""Direct rows (csrc/direct_rows.h): rank-one rows and short triplet rows of a block on the congruence + Gram
path written into the transformed-row buffer in closed form, the block's other rows through the congruence as ever.

Two independent answers: the compiled reference's goldens (mix40_A / mix40_B) and, for the fixture family built here, numpy fp64
from the definition -- M_ij = tr(A_i S^-1 A_j S^-1), the three vectors, the scalars, and tr(A_i X A_j X) for KKT_TYPE_PRIMAL --
on the engine's own cone.dual_matrix() (the S assembly is not under test).  Computed through S^-1 and through the Cholesky
congruence the definition agrees with itself to 1.1e-14 norm-wise and 6e-13 on the reference's bar at these shapes (cond(S) up to
7e2), four orders inside check_close's 1e-10 / 1e-8.

The switch HDSDP_MI355X_DIRECT_ROWS is read at cone creation: every test sets it before it makes its cone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import KKT_TOL, check_close, load_golden, lower_mask, primal_X, y_of

pytestmark = pytest.mark.gpu

ZERO, SPARSE, DENSE, SPR1, DSR1 = range(5)      # MiCoeffType
SWITCH = "HDSDP_MI355X_DIRECT_ROWS"
FLOOR_N = 256                                   # csrc/direct_rows.h: HDM_DR_MIN_N
M_ROWS = 24


# ---- fixtures -------------------------------------------------------------------------------------------------------
def packed(i, j, n):
    return j * n - j * (j - 1) // 2 + (i - j)


def csc_of(n, C, rows):
    """CSC of shape n(n+1)/2 x (m+1) from symmetric matrices: column 0 = C, column i = A_i; stored = the non-zero lower entries"""
    jj, ii = np.triu_indices(n)               # (j, i) with i >= j in column-major order of the lower triangle
    beg, idx, val = [0], [], []
    for A in [C] + list(rows):
        v = A[ii, jj]
        nz = np.nonzero(v)[0]
        idx.append(nz)
        val.append(v[nz])
        beg.append(beg[-1] + nz.size)
    return np.array(beg, dtype=np.int32), np.concatenate(idx).astype(np.int32), np.concatenate(val)


def sym_from(n, entries):
    A = np.zeros((n, n))
    for i, j, v in entries:
        A[i, j] = A[j, i] = v
    return A


def make_fixture(n, dense_rows=True, seed=20240):
    """The mixed block: m = 24 rows in a fixed shuffle -- 6 dense, 3 SPR1 and 3 DSR1 with both signs, sparse rows of 1 .. 8 entries
    (among them a diagonal-only row, a row in the last rows / columns of the matrix, where the 16 x 16 sub-blocks are ragged, and a
    row touching row / column 0) plus two more of 2 and 5 entries, one sparse row of 9 entries, one zero row; dense C.
    Returns (C, rows, classes); dense_rows = False leaves the six dense rows out (zero rows in their place)."""
    rng = np.random.default_rng(seed + n)

    def dense():
        G = rng.standard_normal((n, n)) / np.sqrt(n)
        return G + G.T

    def r1(fill, sign):
        a = np.zeros(n)
        a[rng.choice(n, size=fill, replace=False)] = 0.5 + rng.random(fill)
        a *= 2.0 / np.linalg.norm(a)
        return sign * np.outer(a, a)

    def scattered(k):
        pos = set()
        while len(pos) < k:
            i, j = sorted(rng.integers(0, n, size=2), reverse=True)
            pos.add((int(i), int(j)))
        return sym_from(n, [(i, j, float(rng.standard_normal())) for i, j in sorted(pos)])

    kinds = []
    for _ in range(6):
        kinds.append((DENSE, dense() if dense_rows else np.zeros((n, n))))
    for sign in (1.3, -0.8, 2.1):
        kinds.append((SPR1, r1(3, sign)))
    for sign in (-1.1, 0.7, -2.4):
        kinds.append((DSR1, r1(n, sign)))
    kinds.append((SPARSE, sym_from(n, [(5, 2, 0.9)])))                                                  # 1 entry, off the diagonal
    kinds.append((SPARSE, sym_from(n, [(0, 0, -1.2), (n - 1, 0, 0.6)])))                                # 2: row / column 0
    kinds.append((SPARSE, sym_from(n, [(n - 1, n - 1, 0.8), (n - 1, n - 2, -0.5), (n - 1, n - 3, 1.1)])))   # 3: the last rows
    kinds.append((SPARSE, sym_from(n, [(1, 1, 0.7), (7, 7, -1.4), (9, 9, 0.5), (n - 1, n - 1, 1.0)])))  # 4: diagonal only
    for k in (5, 6, 7, 8, 2, 5):
        kinds.append((SPARSE, scattered(k)))
    kinds.append((SPARSE, scattered(9)))                                                                # kmax + 1 at the switch's 8
    kinds.append((ZERO, np.zeros((n, n))))
    assert len(kinds) == M_ROWS
    order = np.random.default_rng(7).permutation(M_ROWS)
    rows = [kinds[k][1] for k in order]
    classes = [kinds[k][0] if (dense_rows or kinds[k][0] != DENSE) else ZERO for k in order]
    C = dense() + np.diag(rng.random(n))
    return C, rows, classes


def stored_of(A):
    return int(np.count_nonzero(np.tril(A)))


def expected_counts(rows, classes, kmax):
    """(direct, rank one, congruence, kmax) as the class counts imply"""
    r1 = sum(c in (SPR1, DSR1) for c in classes)
    sp = sum(c == SPARSE and stored_of(A) <= kmax for A, c in zip(rows, classes))
    nz = sum(c != ZERO for c in classes)
    return (r1 + sp, r1, nz - r1 - sp, kmax)


def make_cone(n, C, rows, classes=None, iCone=0):
    from hdsdp_amd import api
    beg, idx, val = csc_of(n, C, rows)
    if classes is not None:
        got = api.presolve_csc(n, len(rows), beg, idx, val)["coef_type"].tolist()
        assert got == list(classes), (got, classes)
    return api.SDPCone.from_csc(n, len(rows), beg, idx, val, iCone=iCone)


def full_S(cone):
    D = cone.dual_matrix()                    # element (row i, col j) at [j, i], valid where i >= j
    return np.triu(D) + np.triu(D, 1).T


def numpy_answer(rows, C, W, Rd):
    """the definition, with W = S^-1 (or the registered primal matrix X)"""
    B = [W @ A for A in rows]
    m = len(rows)
    M = np.array([[np.sum(B[i] * B[j].T) for j in range(m)] for i in range(m)])
    WW, WC = W @ W, W @ C
    WCW = WC @ W
    return {"M": M, "ASinv": np.array([np.trace(b) for b in B]), "ASinvRdSinv": Rd * np.array([np.sum(A * WW) for A in rows]),
            "ASinvCSinv": np.array([np.sum(A * WCW) for A in rows]),
            "CSinv": np.trace(WC), "CSinvCSinv": np.sum(WC * WC.T), "CSinvRdSinv": Rd * np.sum(C * WW),
            "TraceSinv": np.trace(W) if Rd != 0.0 else 0.0}


def states(n, C, rows):
    """(tau, y, Rd): y = 0 with Rd = -10 n; y != 0 with Rd such that the smallest eigenvalue of S is 0.05"""
    m = len(rows)
    y = 0.3 * np.sin(1.7 * np.arange(1, m + 1))
    S0 = 0.9 * C - sum(yi * A for yi, A in zip(y, rows))
    return [(1.0, np.zeros(m), -10.0 * n), (0.9, y, float(np.linalg.eigvalsh(S0)[0]) - 0.05)]


def check_builds(cone, kkt, rows, C, Rd, what):
    """INFEASIBLE, HOMOGENEOUS, CORRECTOR and PRIMAL builds of the operator against the numpy answer"""
    from hdsdp_amd import api
    m, n = len(rows), C.shape[0]
    msk = lower_mask(m)
    ref = numpy_answer(rows, C, np.linalg.inv(full_S(cone)), Rd)
    kkt.build_up(api.KKT_TYPE_INFEASIBLE)
    ex = kkt.export()
    check_close(kkt.M[msk], ref["M"][msk], what + " M_inf")
    check_close(ex["ASinv"], ref["ASinv"], what + " ASinv")
    check_close(ex["ASinvRdSinv"], ref["ASinvRdSinv"], what + " ASinvRdSinv")
    check_close([ex["TraceSinv"]], [ref["TraceSinv"]], what + " TraceSinv")
    kkt.build_up(api.KKT_TYPE_HOMOGENEOUS)
    ex = kkt.export()
    check_close(kkt.M[msk], ref["M"][msk], what + " M_hsd")
    for key in ("ASinv", "ASinvRdSinv", "ASinvCSinv"):
        check_close(ex[key], ref[key], what + " hsd " + key)
    for key in ("CSinv", "CSinvCSinv", "CSinvRdSinv", "TraceSinv"):
        check_close([ex[key]], [ref[key]], what + " hsd " + key)
    Mbefore = kkt.M.copy()
    kkt.build_up(api.KKT_TYPE_CORRECTOR)
    ex = kkt.export()
    check_close(ex["ASinv"], ref["ASinv"], what + " cor ASinv")
    check_close(ex["ASinvRdSinv"], ref["ASinvRdSinv"], what + " cor ASinvRdSinv")
    assert np.array_equal(Mbefore, kkt.M)
    X = primal_X(n)
    refp = numpy_answer(rows, C, X, Rd)
    kkt.register_psdp([X])
    kkt.build_up(api.KKT_TYPE_PRIMAL)
    ex = kkt.export()
    check_close(kkt.M[msk], refp["M"][msk], what + " M_pri")
    check_close(ex["ASinv"], refp["ASinv"], what + " pri ASinv")
    check_close(ex["ASinvRdSinv"], refp["ASinvRdSinv"], what + " pri ASinvRdSinv")
    check_close([ex["TraceSinv"]], [refp["TraceSinv"]], what + " pri TraceSinv")


# ---- 1. goldens of the compiled reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mix40_A", "mix40_B"])
def test_golden_of_the_compiled_reference(name, monkeypatch):
    """mix40 (six each of dense, SPR1, DSR1 and zero rows, twelve sparse ones) with the switch at 8: every typeKKT, the fixed
    strategy build and the three Phase-A solves against the reference's numbers"""
    from hdsdp_amd import api
    monkeypatch.setenv(SWITCH, "8")
    g = load_golden(name)
    n, m = int(g["dims"][0]), int(g["dims"][1])
    cone = api.SDPCone.from_csc(n, m, g["csc_beg"], g["csc_idx"], g["csc_val"])
    try:
        assert cone.path == 0
        types, stored = g["coef_type"], np.diff(g["csc_beg"])[1:]
        r1 = int(np.sum((types == SPR1) | (types == DSR1)))
        sp = int(np.sum((types == SPARSE) & (stored <= 8)))
        assert r1 == 12 and sp == 6
        assert cone.direct_rows() == (r1 + sp, r1, int(np.sum(types != ZERO)) - r1 - sp, 8)
        Rd, tau, y = float(g["Rd"][0]), float(g["tau"][0]), y_of(g)
        cone.set_start(Rd)
        assert cone.check_is_interior(tau, y)
        kkt = api.KKT(m, [cone])
        msk = lower_mask(m)
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        ex = kkt.export()
        check_close(kkt.M[msk], g["M_inf"][msk], name)
        check_close(ex["ASinv"], g["ASinv_inf"], name)
        check_close(ex["ASinvRdSinv"], g["ASinvRdSinv_inf"], name)
        check_close([ex["TraceSinv"]], g["TraceSinv_inf"], name)
        kkt.add_to_diag(float(g["diag_add"][0]))
        kkt.factorize()
        for rhs, key in ((g["b"], "sol_b"), (g["ASinv_inf"], "sol_ASinv"), (g["ASinvRdSinv_inf"], "sol_ASinvRdSinv")):
            x = kkt.solve(np.array(rhs, dtype=np.float64))
            assert np.linalg.norm(x - g[key]) <= KKT_TOL * np.linalg.norm(g[key]), key
        kkt.build_up(api.KKT_TYPE_HOMOGENEOUS)
        ex = kkt.export()
        check_close(kkt.M[msk], g["M_hsd"][msk], name)
        check_close(ex["ASinv"], g["ASinv_hsd"], name)
        check_close(ex["ASinvRdSinv"], g["ASinvRdSinv_hsd"], name)
        check_close(ex["ASinvCSinv"], g["ASinvCSinv_hsd"], name)
        for got, ref in zip((ex["CSinv"], ex["CSinvCSinv"], ex["CSinvRdSinv"], ex["TraceSinv"]), g["hsd_scalars"]):
            check_close([got], [ref], name)
        Mbefore = kkt.M.copy()
        kkt.build_up(api.KKT_TYPE_CORRECTOR)
        ex = kkt.export()
        check_close(ex["ASinv"], g["ASinv_cor"], name)
        check_close(ex["ASinvRdSinv"], g["ASinvRdSinv_cor"], name)
        assert np.array_equal(Mbefore, kkt.M)
        kkt.build_up_fixed(api.KKT_TYPE_INFEASIBLE, api.KKT_M4)
        check_close(kkt.M[msk], g["M_inf"][msk], name + " fixed M4")
        kkt.register_psdp([primal_X(n)])
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        ex = kkt.export()
        check_close(kkt.M[msk], g["M_pri"][msk], name + " primal")
        check_close(ex["ASinv"], g["ASinv_pri"], name + " primal")
        check_close(ex["ASinvRdSinv"], g["ASinvRdSinv_pri"], name + " primal")
        check_close([ex["TraceSinv"]], g["TraceSinv_pri"], name + " primal")
        kkt.destroy()
    finally:
        cone.destroy()


# ---- 2. the fixture family ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 128, 150])
def test_fixture_family_against_the_definition(n, monkeypatch):
    """n = 17: two sub-blocks, the second with one valid row; 128: exactly one tile; 150: two tiles and a ragged last sub-block"""
    from hdsdp_amd import api
    monkeypatch.setenv(SWITCH, "8")
    C, rows, classes = make_fixture(n)
    cone = make_cone(n, C, rows, classes)
    try:
        assert cone.path == 0
        assert cone.direct_rows() == expected_counts(rows, classes, 8)
        assert cone.direct_rows()[:3] == (16, 6, 7)
        kkt = api.KKT(M_ROWS, [cone])
        for k, (tau, y, Rd) in enumerate(states(n, C, rows)):
            cone.set_start(Rd)
            assert cone.check_is_interior(tau, y)
            check_builds(cone, kkt, rows, C, Rd, "n %d state %d" % (n, k))
        kkt.destroy()
    finally:
        cone.destroy()


# ---- 3. no congruence row at all ------------------------------------------------------------------------------------------
def test_block_without_a_congruence_row(monkeypatch):
    """the n = 150 fixture without its dense rows, the switch at 9 so that the nine-entry row is direct too (a row's terms then
    cross the writer's chunk of eight): every row is written directly, the block stays on path 0"""
    from hdsdp_amd import api
    n = 150
    monkeypatch.setenv(SWITCH, "9")
    C, rows, classes = make_fixture(n, dense_rows=False)
    cone = make_cone(n, C, rows, classes)
    try:
        assert cone.path == 0
        nd, nr1, nc, kmax = cone.direct_rows()
        assert (nd, nr1, nc, kmax) == (17, 6, 0, 9)
        kkt = api.KKT(M_ROWS, [cone])
        for k, (tau, y, Rd) in enumerate(states(n, C, rows)):
            cone.set_start(Rd)
            assert cone.check_is_interior(tau, y)
            check_builds(cone, kkt, rows, C, Rd, "no congruence row, state %d" % k)
        kkt.destroy()
    finally:
        cone.destroy()


# ---- 4. bit-identical -------------------------------------------------------------------------------------------------------
def test_two_builds_are_bit_identical(monkeypatch):
    from hdsdp_amd import api
    n = 150
    monkeypatch.setenv(SWITCH, "8")
    C, rows, classes = make_fixture(n)
    tau, y, Rd = states(n, C, rows)[1]
    out = []
    for _ in range(2):
        cone = make_cone(n, C, rows)
        try:
            cone.set_start(Rd)
            assert cone.check_is_interior(tau, y)
            kkt = api.KKT(M_ROWS, [cone])
            for _ in range(2):
                kkt.build_up(api.KKT_TYPE_HOMOGENEOUS)
                ex = kkt.export()
                out.append((kkt.M.copy(), ex["ASinv"], ex["ASinvRdSinv"], ex["ASinvCSinv"]))
            kkt.destroy()
        finally:
            cone.destroy()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# ---- 5. the rule and the switch ---------------------------------------------------------------------------------------------
def test_the_rule_and_the_switch(monkeypatch):
    from hdsdp_amd import api
    monkeypatch.delenv(SWITCH, raising=False)
    n = 150
    C, rows, classes = make_fixture(n)
    cone = make_cone(n, C, rows)
    try:
        assert cone.path == 0 and cone.direct_rows() == (0, 0, 0, 0)          # below the floor
    finally:
        cone.destroy()
    # a six-row mixed block at the floor size: two dense rows, two rank-one rows, two one-entry rows
    n = FLOOR_N
    rng = np.random.default_rng(5)
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    H = rng.standard_normal((n, n)) / np.sqrt(n)
    a, b = np.zeros(n), rng.random(n) + 0.5
    a[[3, 77, n - 1]] = (1.0, -2.0, 0.5)
    small = [G + G.T, np.outer(a, a), sym_from(n, [(200, 3, 1.5)]), H + H.T, -np.outer(b, b), sym_from(n, [(n - 1, 17, -0.4)])]
    Cs = G @ G.T
    cone = make_cone(n, Cs, small, [DENSE, SPR1, SPARSE, DENSE, DSR1, SPARSE])
    try:
        nd, nr1, nc, kmax = cone.direct_rows()
        assert cone.path == 0 and kmax >= 1 and (nd, nr1, nc) == (4, 2, 2)
        cone.set_start(-10.0 * n)
        assert cone.check_is_interior(1.0, np.zeros(6))
        kkt = api.KKT(6, [cone])
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        ref = numpy_answer(small, Cs, np.linalg.inv(full_S(cone)), -10.0 * n)
        check_close(kkt.M[lower_mask(6)], ref["M"][lower_mask(6)], "floor-size block")
        kkt.destroy()
    finally:
        cone.destroy()
    monkeypatch.setenv(SWITCH, "0")
    cone = make_cone(n, Cs, small)
    try:
        assert cone.path == 0 and cone.direct_rows() == (0, 0, 0, 0)
    finally:
        cone.destroy()
    monkeypatch.setenv(SWITCH, "8")
    cone = api.SDPCone.synthetic(96, 12)
    try:
        assert cone.direct_rows() == (0, 0, 0, 0)
    finally:
        cone.destroy()


def test_a_shard_of_a_sharded_block_has_no_direct_rows(tmp_path):
    """world = 2: made in a process of its own (a sharded cone reserves compute units for the exchange, process-wide)"""
    n = 17
    C, rows, _ = make_fixture(n)
    beg, idx, val = csc_of(n, C, rows)
    np.savez(tmp_path / "blk.npz", beg=beg, idx=idx, val=val)
    code = ("import sys, numpy as np\n"
            "from hdsdp_amd import api\n"
            "g = np.load(sys.argv[1])\n"
            "c = api.SDPCone.from_csc(%d, %d, g['beg'], g['idx'], g['val'], rank=0, world=2)\n"
            "print('DIRECT', c.direct_rows(), c.path)\n"
            "c.destroy()\n" % (n, M_ROWS))
    env = dict(os.environ, **{SWITCH: "8"})
    env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path / "blk.npz")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "DIRECT (0, 0, 0, 0) 0" in out.stdout, out.stdout


# ---- 6. the pattern protocol under the new row order -----------------------------------------------------------------------
def write_sdpa(path, m, blocks, b):
    """blocks: list of (n, F0, {constraint (1-based): F_i}); SDPA sparse format, upper triangle, 1-based"""
    with open(path, "w") as f:
        f.write("%d\n%d\n%s\n%s\n" % (m, len(blocks), " ".join(str(n) for n, _, _ in blocks), " ".join(repr(float(x)) for x in b)))
        for k, (n, F0, mats) in enumerate(blocks):
            for i, F in [(0, F0)] + sorted(mats.items()):
                for r in range(n):
                    for c in range(r, n):
                        if F[r, c] != 0.0:
                            f.write("%d %d %d %d %r\n" % (i, k + 1, r + 1, c + 1, float(F[r, c])))


def test_pattern_protocol_under_the_new_row_order(tmp_path, monkeypatch):
    """Most constraints are zero on every block, so the operator takes the sparse form (aggregated pattern, hdsdp_schur.c:46-139).
    The first block's rows are, in ascending order, sparse / dense / rank one / dense / sparse / dense: with direct rows its local
    order is not ascending, and the two pattern slots must still walk the rows in ascending order.  (blocks3.dat-s does not serve:
    its congruence-path block has no row of eight entries or fewer, and its operator is dense.)"""
    from hdsdp_amd import api
    m, n = 60, 20
    rng = np.random.default_rng(11)

    def dense(k):
        G = rng.standard_normal((k, k)) / np.sqrt(k)
        return G + G.T

    a = np.zeros(n)
    a[[2, 11, 19]] = (1.0, -0.7, 0.4)
    first = {5: sym_from(n, [(4, 1, 0.8), (19, 19, -0.6)]), 10: dense(n), 16: 1.7 * np.outer(a, a), 23: dense(n),
             31: sym_from(n, [(0, 0, 1.1), (7, 3, -0.9), (19, 0, 0.3)]), 42: dense(n)}
    blocks = [(n, -dense(n), first)]
    # every constraint has data on some block (a sparse operator has no empty column): the other 54 in six blocks of nine, the
    # first of which shares constraints 10 and 31 with the block above
    others = [i for i in range(1, m + 1) if i not in first]
    for q in range(6):
        mine = others[9 * q:9 * q + 9] + ([10, 31] if q == 0 else [])
        blocks.append((6, -dense(6), {i: dense(6) for i in mine}))
    fname = str(tmp_path / "sparse_pattern.dat-s")
    write_sdpa(fname, m, blocks, np.ones(m))
    prob = api.read_sdpa(fname)
    assert prob["m"] == m and len(prob["blocks"]) == 7
    y = 0.05 * np.sin(1.3 * np.arange(1, m + 1))
    res = {}
    for sw in ("8", "0"):
        monkeypatch.setenv(SWITCH, sw)
        cones = [api.SDPCone.from_csc(blk["n"], m, blk["beg"], blk["idx"], blk["val"], iCone=k) for k, blk in enumerate(prob["blocks"])]
        try:
            assert cones[0].path == 0
            assert cones[0].direct_rows() == ((3, 1, 3, 8) if sw == "8" else (0, 0, 0, 0))
            for c in cones:
                c.set_start(-30.0)
                assert c.check_is_interior(1.0, y)
            kkt = api.KKT(m, cones)
            assert kkt.is_sparse
            kkt.build_up(api.KKT_TYPE_HOMOGENEOUS)
            beg, idx, val = kkt.csc()
            ex = kkt.export()
            res[sw] = (beg.copy(), idx.copy(), val.copy(), ex)
            kkt.destroy()
        finally:
            for c in cones:
                c.destroy()
    assert np.array_equal(res["8"][0], res["0"][0]) and np.array_equal(res["8"][1], res["0"][1])
    check_close(res["8"][2], res["0"][2], "CSC values")
    for key in ("ASinv", "ASinvRdSinv", "ASinvCSinv"):
        check_close(res["8"][3][key], res["0"][3][key], key)
    for key in ("CSinv", "CSinvCSinv", "CSinvRdSinv", "TraceSinv"):
        check_close([res["8"][3][key]], [res["0"][3][key]], key)


# ---- 7. two blocks in one operator -------------------------------------------------------------------------------------------
def test_two_blocks_in_one_operator(monkeypatch):
    """a direct-row block next to a plain dense block: M is the sum of the two numpy answers"""
    from hdsdp_amd import api
    monkeypatch.setenv(SWITCH, "8")
    n1, n2 = 17, 24
    C1, rows1, classes1 = make_fixture(n1)
    rng = np.random.default_rng(3)
    rows2 = []
    for _ in range(M_ROWS):
        G = rng.standard_normal((n2, n2)) / np.sqrt(n2)
        rows2.append(G + G.T)
    C2 = rows2[0] @ rows2[0].T
    c1, c2 = make_cone(n1, C1, rows1, classes1, iCone=0), make_cone(n2, C2, rows2, [DENSE] * M_ROWS, iCone=1)
    try:
        assert c1.direct_rows()[:3] == (16, 6, 7) and c2.direct_rows() == (0, 0, 0, 0)
        y = 0.1 * np.cos(0.9 * np.arange(M_ROWS))
        Rd = -40.0
        for c in (c1, c2):
            c.set_start(Rd)
            assert c.check_is_interior(1.0, y)
        kkt = api.KKT(M_ROWS, [c1, c2])
        kkt.build_up(api.KKT_TYPE_HOMOGENEOUS)
        ex = kkt.export()
        r1 = numpy_answer(rows1, C1, np.linalg.inv(full_S(c1)), Rd)
        r2 = numpy_answer(rows2, C2, np.linalg.inv(full_S(c2)), Rd)
        msk = lower_mask(M_ROWS)
        check_close(kkt.M[msk], (r1["M"] + r2["M"])[msk], "two blocks M")
        for key in ("ASinv", "ASinvRdSinv", "ASinvCSinv"):
            check_close(ex[key], r1[key] + r2[key], "two blocks " + key)
        for key in ("CSinv", "CSinvCSinv", "CSinvRdSinv", "TraceSinv"):
            check_close([ex[key]], [r1[key] + r2[key]], "two blocks " + key)
        kkt.destroy()
    finally:
        c1.destroy()
        c2.destroy()
