"""The two sparse factorisations of the Schur matrix where structure and size matter: the tile LDL' (csrc/bsparse.hip) through
HMiBspSolve and the block-envelope Cholesky (HdmChol::set_envelope, hdm_trsv_flow_kernel) through HMiCholEnvelopeSolve, on the
patterns, values and envelope vectors of tests/sparse_schur_cases.py (whose properties tests/test_sparse_schur_cases_cpu.py
proves without a GPU): fill tiles, a last tile with one valid row, sizes that are multiples of 128, graded matrices up to
cond 1e10, quasi-definite matrices whose pivots change sign a few hundred times, zero pivots and where they are reported,
envelopes of every shape at 2 to 10 blocks.

Every solution is held to the rule of test_gpu_conditioning.py on the normwise backward error (residual in longdouble),

    e(gpu) <= 8 e(ref) + 16 u            (u = 2^-53)

ref = scipy's dense Cholesky solve for a positive definite matrix, a plain fp64 LDL' without pivoting in the same order for a
quasi-definite one; both stay below 64 u on everything used here (CPU test).  Lines starting SPARSE_REPORT give the worst ratio
e(gpu) / max(e(ref), 16 u) of each group; `pytest -s` shows them, tests/golden/sparse_schur_report.txt keeps those of one run
on an MI355X (the 42 tests of this file took 32 s there, none more than 3 s)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sl

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import sparse_schur_cases as sc  # noqa: E402
import xprec_ref as xp  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xp.HAVE_LD, reason=xp.NO_LD_REASON)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Rule:
    """collects the cases of one group: e(gpu) against e(ref); the worst ratio goes into the report"""

    def __init__(self, group):
        self.group, self.bad, self.n, self.worst = group, [], 0, (0.0, 0.0, 0.0)

    def hold(self, what, e_gpu, e_ref):
        self.n += 1
        ratio = e_gpu / max(e_ref, 16.0 * sc.U)
        print(f"    {what}: e(gpu) = {e_gpu / sc.U:.3f} u, e(ref) = {e_ref / sc.U:.3f} u")
        if ratio >= self.worst[0]:
            self.worst = (ratio, e_gpu, e_ref)
        if not (np.isfinite(e_gpu) and sc.within(e_gpu, e_ref)):
            self.bad.append(f"{what}: {e_gpu / sc.U:.3f} u vs the reference's {e_ref / sc.U:.3f} u")

    def solution(self, what, A, x, b, e_ref):
        if not np.all(np.isfinite(x)):
            self.bad.append(f"{what}: solution not finite")
            return
        self.hold(what, sc.backward_error(A, x, b), e_ref)

    def finish(self, note=""):
        sc.report(self.group, *self.worst, self.n, note)
        assert not self.bad, "\n".join(self.bad)


# ---------------------------------------------------------------- tile form

def bsp_solve(c, val=None, b=None, timed=False, solve=True):
    """HMiBspSolve on a TileCase (other values / right-hand side on request): (rc, info, stats[4], x)"""
    from hdsdp_amd import api
    lib = api.load_library()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    val = np.ascontiguousarray(c.val if val is None else val, dtype=np.float64)
    b = np.ascontiguousarray(c.b if b is None else b, dtype=np.float64)
    x = np.full(c.m, np.nan)
    info, stats, ms = C.c_int(-1), (C.c_int * 4)(-1, -1, -1, -1), C.c_double(0.0)
    rc = lib.HMiBspSolve(c.m, c.beg.ctypes.data_as(ip), c.idx.ctypes.data_as(ip), val.ctypes.data_as(dp),
                         b.ctypes.data_as(dp) if solve else None, x.ctypes.data_as(dp) if solve else None, C.byref(info), stats,
                         C.byref(ms) if timed else None)
    return rc, info.value, list(stats), x


def model_stats(c):
    return [c.sym.nb, c.sym.ntiles, c.sym.nlevels]


def run_tile_case(rule, family, m, renumbered, kind, cond, grade):
    c = sc.tile_case(family, m, renumbered, kind, cond, grade)
    e_ref, nneg_ref = sc.tile_reference(family, m, renumbered, kind, cond, grade)
    assert e_ref <= sc.CAP
    rc, info, stats, x = bsp_solve(c)
    what = f"{family} m={m} {'renumbered' if renumbered else 'natural'} {kind} cond={cond:g} {grade}"
    assert rc == 0 and info == 0, (what, rc, info)
    assert stats[:3] == model_stats(c), (what, stats, model_stats(c))
    nneg = 0 if c.s is None else int(np.sum(c.s < 0))
    assert stats[3] == nneg == nneg_ref, (what, stats[3], nneg, nneg_ref)
    rule.solution(what, c.A, x, c.b, e_ref)
    return c, x


def test_one_block_row_is_refused_and_the_next_solve_works():
    """m = 128 is one tile: HdmBsp::init declines (the dense path takes such a matrix) and HMiBspSolve returns nonzero; the
    next call, at m = 129, is served"""
    c = sc.TileCase()
    c.m, c.pairs = 128, sc.pattern("band", 128, False)
    c.beg, c.idx = sc.lower_csc(128, c.pairs)
    c.A = sc.dominant(128, c.pairs, "one tile")
    c.val, c.b = sc.csc_values(c.A, c.beg, c.idx), np.ones(128)
    rc, _, _, _ = bsp_solve(c)
    assert rc != 0
    rule = Rule("tile after a refusal")
    run_tile_case(rule, "band", 129, False, "spd", 1e6, "down")
    rule.finish()


@pytest.mark.parametrize("family", sc.SWEEP_FAMILIES)
def test_tile_form_size_sweep(family):
    """m = 129 (a last tile with ONE valid row), 255, 256 and 384 (no padding), 257, 385, 640: positive definite at cond 1e6,
    graded along and against the elimination order, natural and renumbered; block rows, tiles and levels as the model says"""
    rule = Rule(f"tile sweep {family}")
    for f, m, r, g in sc.sweep_cases():
        if f == family:
            run_tile_case(rule, f, m, r, "spd", 1e6, g)
    rule.finish()


@pytest.mark.parametrize("renumbered", [False, True], ids=["natural", "renumbered"])
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_tile_form_conditioning(family, renumbered):
    """every family at m = 1153 (filltail: 1040): positive definite at cond 1e2, 1e6, 1e10 and quasi-definite at 1e2, 1e6; the
    negative pivots counted are the negative signs put in, exactly, and (cond 1e2, where no eigenvalue is near zero) the negative
    eigenvalues"""
    rule = Rule(f"tile conditioning {family} {'renumbered' if renumbered else 'natural'}")
    for m, r, kind, cond, grade in sc.big_cases(family):
        if r != renumbered:
            continue
        c, _ = run_tile_case(rule, family, m, r, kind, cond, grade)
        if kind == "qd" and cond == 1e2 and grade == "down":
            w = np.linalg.eigvalsh(c.A)
            assert np.min(np.abs(w)) > 1e-6 * np.max(np.abs(w))
            assert int(np.sum(w < 0)) == int(np.sum(c.s < 0))
    rule.finish()


@pytest.mark.parametrize("kind", ["spd", "qd"])
def test_fill_tiles_are_cleared_when_the_store_is_loaded_again(kind):
    """filltail (8 of its 30 tiles exist only through updates).  The timed form runs three load-and-factor rounds on one store:
    its solution is the untimed form's, bit for bit -- a fill tile that kept the previous round's factor would be updated
    twice.  And solving other values on the same pattern in between does not change the first solution's bits."""
    m = sc.FILLTAIL_M
    c = sc.tile_case("filltail", m, False, kind, 1e6, "down")
    assert c.sym.ntiles - int(c.sym.P0.sum()) == 8
    rc, info, stats, x = bsp_solve(c)
    assert rc == 0 and info == 0 and stats[:3] == model_stats(c)
    rc, info, stats_t, xt = bsp_solve(c, timed=True)
    assert rc == 0 and info == 0 and stats_t == stats
    assert same_bits(xt, x)
    other = sc.tile_case("filltail", m, False, kind, 1e6, "down", 1)
    assert np.array_equal(other.idx, c.idx) and not np.array_equal(other.val, c.val)
    rc, info, _, xo = bsp_solve(other, timed=True)
    assert rc == 0 and info == 0 and not same_bits(xo, x)
    rule = Rule(f"tile filltail reuse {kind}")
    rule.solution("other values", other.A, xo, other.b, sc.tile_reference("filltail", m, False, kind, 1e6, "down", 1)[0])
    for timed in (False, True):
        rc, info, _, x2 = bsp_solve(c, timed=timed)
        assert rc == 0 and info == 0 and same_bits(x2, x), timed
    rule.solution("first values again", c.A, x, c.b, sc.tile_reference("filltail", m, False, kind, 1e6, "down")[0])
    rule.finish()


@pytest.mark.parametrize("family,m,renumbered,rows,what", sc.ZERO_PIVOT, ids=lambda v: str(v).replace(" ", "_"))
def test_zero_pivot_is_reported_at_its_permuted_index(family, m, renumbered, rows, what):
    """a row with nothing but its diagonal, and that 0.0 (or NaN): info = its index in the factorisation's order + 1; with two
    such rows the smaller index -- both in one tile, in tiles of different levels, in different tiles of the same level.  A
    good solve follows."""
    c = sc.zero_pivot_case(family, m, renumbered, rows)
    perm = c.sym.perm
    diag_at = {r: int(c.beg[r]) for r in rows}
    assert all(c.idx[q] == r and c.beg[r + 1] - c.beg[r] == 1 for r, q in diag_at.items())     # only its diagonal
    for bad in (0.0, np.nan):
        for zero in ((rows[0],), (rows[1],), rows):
            val = c.val.copy()
            for r in zero:
                val[diag_at[r]] = bad
            rc, info, stats, _ = bsp_solve(c, val=val, solve=False)
            assert rc == 0 and stats[:3] == model_stats(c)
            assert info == min(int(perm[r]) for r in zero) + 1, (what, bad, zero, info, [int(perm[r]) for r in zero])
    rc, info, stats, x = bsp_solve(c)
    assert rc == 0 and info == 0 and stats[3] == 0
    rule = Rule(f"tile after a zero pivot {family}")
    rule.solution(f"{family} m={m} rows {rows} cut off", c.A, x, c.b, sc.backward_error(c.A, sc.cholesky_solve(c.A, c.b), c.b))
    rule.finish()


@pytest.mark.parametrize("family,m,kind", [("band", 257, "spd"), ("filltail", sc.FILLTAIL_M, "qd")])
def test_scaling_by_a_power_of_two_scales_the_solution_exactly(family, m, kind):
    """the matrix times 2^-400 or 2^+400: the solution times 2^+400 or 2^-400, bit for bit -- no absolute threshold anywhere
    in the factorisation or the substitutions"""
    c = sc.tile_case(family, m, False, kind, 1e6, "down")
    rc, info, stats, x = bsp_solve(c)
    assert rc == 0 and info == 0
    for p in (-400, 400):
        rc, info, stats_p, xs = bsp_solve(c, val=np.ldexp(c.val, p))
        assert rc == 0 and info == 0 and stats_p == stats, (p, info, stats_p)
        assert same_bits(xs, np.ldexp(x, -p)), p


# ---------------------------------------------------------------- envelope form

def _chunks(cases, size):
    return [tuple(cases[i:i + size]) for i in range(0, len(cases), size)]


ENV_CHUNKS = [ch for n in sc.ENV_N for ch in _chunks([c for c in sc.env_cases() if c[1] == n], 6)]


def outside_blocks_are_zero(c, L):
    low = np.tril(np.ones((c.n, c.n), dtype=bool))
    blockwise_outside = low & ~c.inside
    return not np.any(bits(L[blockwise_outside]))            # every bit zero: +0.0


@pytest.mark.parametrize("chunk", ENV_CHUNKS, ids=lambda ch: f"n{ch[0][1]}-{ch[0][0]}-to-{ch[-1][0]}")
def test_envelope_cholesky(chunk):
    """n = 129, 256, 257, 600, 1153 (2 to 10 blocks, last blocks of 1 and 88 rows), every `first` family that differs from the
    others at that block count: info 0; x under the rule against scipy; L L' against the matrix (normwise, product in
    longdouble) under the same rule against scipy's factor; every block of L outside the row envelope exactly zero.
    Against the dense run (first = NULL) on the same matrix: the lower triangle of L and x are the same bits -- blocks outside
    the envelope contribute exact zeros, and panel and update sum a block column in the same order whatever its height."""
    from hdsdp_amd import api
    n = chunk[0][1]
    rule, frule = Rule(f"envelope solve n={n} {chunk[0][0]}..{chunk[-1][0]}"), Rule(f"envelope factor n={n} {chunk[0][0]}..{chunk[-1][0]}")
    for family, n, cond, grade in chunk:
        c = sc.env_case(family, n, cond, grade)
        e_ref, f_ref = sc.env_reference(family, n, cond, grade)
        assert e_ref <= sc.CAP
        what = f"{family} n={n} cond={cond:g} {grade}"
        x, L, info = api.chol_envelope_solve(c.A, c.first, c.b)
        assert info == 0, what
        rule.solution(what, c.A, x, c.b, e_ref)
        frule.hold(what + " L L'", sc.factor_error(c.A, L), f_ref)
        assert outside_blocks_are_zero(c, L), what
        xd, Ld, info = api.chol_envelope_solve(c.A, None, c.b)
        assert info == 0, what
        assert same_bits(L, Ld), (what, "factor differs from the dense run's")
        assert same_bits(x, xd), (what, "solution differs from the dense run's")
    rule.finish()
    frule.finish()


@pytest.mark.parametrize("n", sc.ENV_N)
def test_envelope_solve_through_the_per_block_substitution(n, tmp_path):
    """the same cases with HDM_TRSV_FLOW=0 (read once per process, hence a child): the per-block launches skip nothing by the
    envelope.  x under the rule, and the same bits on the envelope and dense."""
    out = str(tmp_path / "x.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "sparse_schur_worker.py"), str(n), out], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, HDM_TRSV_FLOW="0"))
    assert r.returncode == 0 and "SPARSE_WORKER_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    res = np.load(out)
    cases = [c for c in sc.env_cases() if c[1] == n]
    assert len(res.files) == 2 * len(cases)
    rule = Rule(f"envelope per-block substitution n={n}")
    for k, (family, _, cond, grade) in enumerate(cases):
        c = sc.env_case(family, n, cond, grade)
        xe, xd = res[f"x_env_{k}"], res[f"x_dense_{k}"]
        rule.solution(f"{family} n={n} cond={cond:g} {grade}", c.A, xe, c.b, sc.env_reference(family, n, cond, grade)[0])
        assert same_bits(xe, xd), (family, n, cond, grade)
    rule.finish()


@pytest.mark.parametrize("n,row", [(600, 300), (600, 599), (600, 128), (257, 256), (1153, 1152)])
def test_envelope_cholesky_stops_at_the_first_negative_pivot(n, row):
    """S = L D L' inside a band1 envelope, D = I except one -1: in a block inside the envelope, at the last row of a partial
    last block (599 of 600; 256 of 257 and 1152 of 1153: a block of one row), at row 128.  info is dpotrf's; the same object
    type then factors a good matrix"""
    from hdsdp_amd import api
    nblk = (n + 127) // 128
    first = sc.env_first("band1" if nblk >= 3 else "dense", nblk)
    S = sc.not_pd(n, row, first)
    _, lapack_info = sl.lapack.dpotrf(S, lower=1)
    assert lapack_info == row + 1
    for f in (first, None):
        x, L, info = api.chol_envelope_solve(S, f, np.ones(n))
        assert info == lapack_info and x is None, (info, lapack_info)
    fam = "band1" if nblk >= 3 else "dense"
    c = sc.env_case(fam, n, 1e6, "down")
    x, L, info = api.chol_envelope_solve(c.A, c.first, c.b)
    assert info == 0
    rule = Rule(f"envelope after a negative pivot n={n} row={row}")
    rule.solution(f"{fam} n={n}", c.A, x, c.b, sc.env_reference(fam, n, 1e6, "down")[0])
    rule.finish()


@pytest.mark.parametrize("n", [600, 1153])
def test_envelope_vector_is_clamped(n):
    """first[] with an entry above its row and a negative one gives the bits of the clamped vector"""
    from hdsdp_amd import api
    c = sc.env_case("unclamped", n, 1e6, "down")
    assert not np.array_equal(c.first, c.clamped)
    x, L, info = api.chol_envelope_solve(c.A, c.first, c.b)
    xc, Lc, info_c = api.chol_envelope_solve(c.A, c.clamped, c.b)
    assert info == 0 and info_c == 0
    assert same_bits(x, xc) and same_bits(L, Lc)


# ---------------------------------------------------------------- operator level

def _full(Mh):
    return np.triu(Mh) + np.triu(Mh, 1).T


def _hold_operator(rule, what, kkt, m):
    from hdsdp_amd import api
    kkt.build_up(api.KKT_TYPE_INFEASIBLE)
    A = np.ascontiguousarray(_full(kkt.M))
    kkt.factorize()
    B = np.random.default_rng(11).standard_normal((3, m))
    for k in range(3):
        x = kkt.solve(B[k])
        e_ref = sc.backward_error(A, sc.cholesky_solve(A, B[k]), B[k])
        assert e_ref <= sc.CAP, (what, e_ref / sc.U)
        rule.solution(f"{what} rhs {k}", A, x, B[k], e_ref)


def test_operators_that_run_the_two_forms():
    """what the solver runs on top of the direct entries: arrow128's operator (tile form) and the scrambled chain (envelope of
    P M P', reverse Cuthill-McKee) at their interior states, HKKTSolve on three right-hand sides under the rule against scipy's
    Cholesky solve of the operator's own matrix"""
    from chain_operator import CHAIN_M, banded_chain
    from util import load_golden, y_of
    from hdsdp_amd import api
    rule = Rule("operators")
    g = load_golden("arrow128_A")
    m = int(g["mb_dims"][1])
    Rd, tau, y = float(g["Rd"][0]), float(g["tau"][0]), y_of(g)
    prob = api.read_sdpa(os.path.join(HERE, "golden", "arrow128.dat-s"))
    cones = [api.SDPCone.from_csc(blk["n"], m, blk["beg"], blk["idx"], blk["val"], iCone=k) for k, blk in enumerate(prob["blocks"])]
    try:
        for c in cones:
            c.set_start(Rd)
            assert c.check_is_interior(tau, y)
        kkt = api.KKT(m, cones)
        assert kkt.is_sparse and kkt.tile_info() is not None
        _hold_operator(rule, "arrow128 (tiles)", kkt, m)
        assert kkt.negative_pivots() == 0
        kkt.destroy()
    finally:
        for c in cones:
            c.destroy()
    cones = []
    try:
        banded_chain(True, cones)
        kkt = api.KKT(CHAIN_M, cones)
        assert kkt.is_sparse
        permuted, fraction = kkt.envelope_info()
        if os.environ.get("HDSDP_MI355X_KKT_ENVELOPE", "1") != "0" and os.environ.get("HDSDP_MI355X_KKT_RCM", "1") != "0":
            assert kkt.tile_info() is None and permuted and fraction <= 0.8, (permuted, fraction)
        _hold_operator(rule, "scrambled chain (envelope)", kkt, CHAIN_M)
        kkt.destroy()
    finally:
        for c in cones:
            c.destroy()
    rule.finish()
