"""The factor, the Schur build and the Schur solve at ill-conditioned dual matrices: cond(S) = 1e2, 1e6, 1e10, the regime of an
interior-point solve's last iterations, where the engine's arithmetic (explicitly inverted 128-blocks, Linv by doubling or
by a sweep, the congruence + Gram form of M, Linv^T (Linv a) on the rank-one path) differs most from the reference's LAPACK.

Every comparison is made on the S the engine actually holds (cone.dual_matrix(), valid triangle): the truth is the
extended-precision reference of tests/xprec_ref.py at that S, the plain-C oracle (the reference's algorithm in fp64) gets the
same S, and with err(x) = max|x - x*| / max|x*| every quantity must satisfy

    err(gpu) <= 8 err(oracle) + 16 u            (u = 2^-53)

The dense factor object is held the same way to LAPACK on the same matrix.  Lines starting COND_REPORT give the measured
ratios err(gpu) / err(oracle) (or / LAPACK's) per group, path, spectrum and condition number (`pytest -s` shows them)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import line_search_model as lm  # noqa: E402
import xprec_ref as xp  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xp.HAVE_LD, reason=xp.NO_LD_REASON)]

U = 2.0 ** -53
LD = xp.LD
CONDS = (1e2, 1e6, 1e10)
SPECTRA = ("spread", "late", "graded")
RD = -0.25                  # a power of two: Rd I enters C and S exactly


def report(group, path, spectrum, cond, ratio, what=""):
    print(f"COND_REPORT {json.dumps(dict(group=group, path=path, spectrum=spectrum, cond=cond, ratio=float(ratio), what=what))}")


def err(x, ref):
    x, ref = np.asarray(x, dtype=LD), np.asarray(ref, dtype=LD)
    den = np.max(np.abs(ref))
    return float(np.max(np.abs(x - ref)) / den) if den > 0 else float(np.max(np.abs(x)))


def diag_err(M, ref):
    """max_i |M_ii - M*_ii| / M*_ii"""
    d, r = np.diag(np.asarray(M, dtype=LD)), np.diag(np.asarray(ref, dtype=LD))
    return float(np.max(np.abs(d - r) / np.abs(r)))


def within(e_gpu, e_ref):
    return e_gpu <= 8.0 * e_ref + 16.0 * U


def target(rng, n, spectrum, cond):
    """S* with the given spectrum kind and condition number (symmetric fp64)"""
    Q = lm.householder_q(rng, n, 8)
    if spectrum == "spread":
        lam = np.geomspace(1.0, 1.0 / cond, n)
    elif spectrum == "late":            # n - r eigenvalues near 1, r = n/8 near 1/cond: against a rank-r primal
        r = max(1, n // 8)
        lam = np.concatenate([0.5 + 0.5 * rng.random(n - r), (1.0 + rng.random(r)) / cond]) if n > 1 else np.ones(1)
    else:                               # graded: D B D, B well conditioned, D geometric over sqrt(cond)
        B = (Q * np.linspace(1.0, 2.0, n)) @ Q.T
        d = np.geomspace(1.0, 1.0 / np.sqrt(cond), n)
        return xp.sym(d[:, None] * xp.sym(B) * d[None, :])
    return xp.sym((Q * lam) @ Q.T)


# ---------------------------------------------------------------- group A: the dense factor object against LAPACK

A_GRID = (129, 256, 383, 640, 2000)
A_SIZES = (1, 2, 3, 5, 33, 127, 128, 129, 255, 256, 257, 383, 512, 513, 640, 1024, 2000, 2049)


def check_dense_factor(n, spectrum, cond, seed=0, label="A"):
    """every observable of HFpLinsys* (DENSE_DIRECT, and the Schur system's DENSE_ITERATIVE) at one matrix, each against LAPACK on
    the same matrix; returns the worst ratio gpu / LAPACK"""
    import ctypes as C
    from hdsdp_amd import api
    rng = np.random.default_rng(seed * 7919 + n)
    S = target(rng, n, spectrum, cond)
    Lc = sl.cho_factor(S, lower=True)
    worst = 0.0
    bad = []

    def hold(what, e_gpu, e_lap):
        nonlocal worst
        worst = max(worst, e_gpu / max(e_lap, 16.0 * U))
        if not within(e_gpu, e_lap):
            bad.append(f"{what}: {e_gpu:.3e} vs LAPACK {e_lap:.3e}")

    ls = api.LinSys(n)
    try:
        ls.numeric(np.triu(S))                      # column-major lower == C-order upper
        for nrhs in (1, 4, 5, 9):
            B = rng.standard_normal((nrhs, n))
            X = ls.solve(B if nrhs > 1 else B[0]).reshape(nrhs, n)
            hold(f"solve nrhs={nrhs}", np.max(xp.backward_error(S, X.T, B.T)),
                 np.max(xp.backward_error(S, sl.cho_solve(Lc, B.T), B.T)))
        b = rng.standard_normal(n)
        e_lap = float(xp.backward_error(S, sl.cho_solve(Lc, b), b)[0])
        x = b.copy()                                 # in place, as the reference's driver solves
        assert api.load_library().HFpLinsysSolve(ls._h, 1, x.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
        hold("in-place solve", float(xp.backward_error(S, x, b)[0]), e_lap)
        hold("bsolve(fsolve)", float(xp.backward_error(S, ls.bsolve(ls.fsolve(b)), b)[0]), e_lap)
        Xi = ls.invert()
        assert np.max(np.abs(Xi - Xi.T)) <= 16.0 * U * np.max(np.abs(Xi)), "invert: not symmetric"
        Li, info = sl.lapack.dpotri(Lc[0], lower=1)
        assert info == 0
        Li = np.tril(Li) + np.tril(Li, -1).T
        hold("invert", xp.inverse_residual_normwise(S, Xi), xp.inverse_residual_normwise(S, Li))
        ld_gpu = LD(2.0) * np.sum(np.log(ls.get_diag().astype(LD)))
        ld_lap = LD(2.0) * np.sum(np.log(np.diag(Lc[0]).astype(LD)))
        scale = max(1.0, float(np.sum(np.abs(2.0 * np.log(np.diag(Lc[0]))))))
        if n <= 640:
            # one scalar: LAPACK's own miss is one draw of its rounding and can be far below a typical one (two correct fp64
            # factorisations differ by 10x and more here), so the reference error is at least the first-order bound of one unit
            # of rounding in the factorisation (xprec_ref.rounding_bound)
            tru = xp.logdet(S)
            floor = xp.rounding_bound(xp.scalar_sensitivities(xp.inverse(S), np.eye(n), 0.0)["logdet"], S)
            hold("logdet", abs(float(ld_gpu - tru)) / scale, max(abs(float(ld_lap - tru)), floor) / scale)
        else:   # a pivot's relative error is bounded by about n u cond: so is the log-determinant's absolute one
            assert abs(float(ld_gpu - ld_lap)) <= 2.0 * n * U * cond + 16.0 * U * scale, ("logdet", float(ld_gpu), float(ld_lap))
    finally:
        ls.destroy()
    li = api.LinSys(n, api.HDSDP_LINSYS_DENSE_ITERATIVE)     # the Schur system's object: Cholesky while it succeeds
    try:
        li.numeric(np.triu(S))
        assert li.lin_type == api.HDSDP_LINSYS_DENSE_ITERATIVE
        B = rng.standard_normal((5, n))
        hold("DENSE_ITERATIVE solve", np.max(xp.backward_error(S, li.solve(B).T, B.T)),
             np.max(xp.backward_error(S, sl.cho_solve(Lc, B.T), B.T)))
    finally:
        li.destroy()
    report(label, "dense factor", spectrum, cond, worst, f"n={n}")
    assert not bad, f"n={n} {spectrum} cond={cond:g}: " + "; ".join(bad)
    return worst


@pytest.mark.parametrize("n", A_GRID)
def test_dense_factor_against_lapack_over_the_grid(n):
    """spread / late iterate / graded at cond 1e2, 1e6, 1e10: solves (1, 4, 5, 9 right-hand sides; solve_host works in chunks of
    4), the in-place form, the two half solves, the inverse and the log-determinant, against LAPACK on the same matrix"""
    for spectrum in SPECTRA:
        for cond in CONDS:
            check_dense_factor(n, spectrum, cond)


@pytest.mark.parametrize("n", [k for k in A_SIZES])
def test_dense_factor_against_lapack_at_every_size(n):
    """spread at cond 1e8 at every size: partial last blocks, the four-pivot steps and the identity padding, one and two blocks,
    Linv by doubling (power-of-two block counts) and by the sweep"""
    check_dense_factor(n, "spread", 1e8, seed=1)


@pytest.mark.parametrize("n,row", [(129, 128), (383, 382), (256, 127), (256, 128)],
                         ids=["last-row-of-partial-block-129", "last-row-of-partial-block-383", "row-127", "row-128"])
def test_psd_decision_where_the_padding_code_matters(n, row):
    """S = L D L^T with unit lower L and D = I except one pivot: negative there, the object says not PSD and numeric raises;
    positive, it says PSD; LAPACK says the same both times"""
    from hdsdp_amd import api
    rng = np.random.default_rng(n + row)
    L = np.eye(n) + np.tril(rng.standard_normal((n, n)), -1) * (0.3 / np.sqrt(n))
    for sign in (-1.0, 1.0):
        d = np.ones(n)
        d[row] = sign
        S = xp.sym((L * d) @ L.T)
        try:
            np.linalg.cholesky(S)
            lapack = True
        except np.linalg.LinAlgError:
            lapack = False
        assert lapack == (sign > 0)
        ls = api.LinSys(n)
        try:
            assert ls.psd_check(np.triu(S)) is lapack, (n, row, sign)
            if lapack:
                ls.numeric(np.triu(S))
            else:
                with pytest.raises(api.HDSDPError):
                    ls.numeric(np.triu(S))
        finally:
            ls.destroy()


# ---------------------------------------------------------------- group B / C / D: the Schur build and solve

def family(rng, kind, n, m):
    """(constraint matrices m x n x n, xprec family)"""
    if kind == "dense":
        A = np.stack([lm.random_sym(rng, n) / np.sqrt(n) for _ in range(m)])
        return A, ("dense", A)
    if kind in ("r1", "r1sparse"):
        # entries +-2^-j: a a^T is exact in fp64, and so is the factor the rank-one probe reads back from its first column
        a = rng.choice([-1.0, 1.0], (m, n)) * np.exp2(-rng.integers(0, 4, (m, n)))
        if kind == "r1sparse":      # four nonzeros per factor (the fused Phase-A kernel takes at most four dense ones)
            keep = np.zeros((m, n), dtype=bool)
            for i in range(m):
                keep[i, rng.choice(n, 4, replace=False)] = True
            a = a * keep
        s = rng.choice([-1.0, 1.0], m)
        A = np.stack([s[i] * np.outer(a[i], a[i]) for i in range(m)])
        return A, ("r1", a, s)
    ents = []
    for i in range(m):                 # a few entries each, never a lone one (that would be rank one)
        e = {}
        while len(e) < 3:
            r, c = sorted(rng.integers(0, n, 2))[::-1]
            e[(int(r), int(c))] = float(rng.uniform(0.5, 1.5)) * rng.choice([-1.0, 1.0])
        ents.append([(r, c, v) for (r, c), v in sorted(e.items())])
    A = np.zeros((m, n, n))
    for i, e in enumerate(ents):
        for r, c, v in e:
            A[i, r, c] = A[i, c, r] = v
    return A, xp.family_from_sparse(n, m, ents)


PATH = {"dense": 0, "r1": 1, "r1sparse": 1, "sparse": 2}


class State:
    """one interior state on the device beside its oracle block: S* chosen, C = S* + sum y* A_i + Rd* I"""

    def __init__(self, monkeypatch, kind, n, m, spectrum, cond, seed, force_path=True):
        from hdsdp_amd import api
        import oracle_py
        rng = np.random.default_rng(seed)
        self.kind, self.n, self.m = kind, n, m
        Sst = target(rng, n, spectrum, cond)
        self.A, self.fam = family(rng, kind, n, m)
        self.y = 0.1 * rng.standard_normal(m) / float(np.max(np.abs(self.A)))
        self.C = Sst + np.tensordot(self.y, self.A, axes=1) + RD * np.eye(n)
        self.C = xp.sym(self.C)
        csc = lm.to_csc([self.C] + list(self.A))
        if force_path:
            monkeypatch.setenv("HDSDP_MI355X_FORCE_PATH", str(PATH[kind]))
        self.cone = api.SDPCone.from_csc(n, m, *csc)
        monkeypatch.delenv("HDSDP_MI355X_FORCE_PATH", raising=False)
        self.blk = oracle_py.Block(n, m, *csc)
        self.cone.set_start(RD)
        assert self.cone.check_is_interior(1.0, self.y), "state not interior"
        self.rebase()

    def rebase(self):
        """oracle and truth from the S the engine holds NOW: an entry point that assembles S again (the fused Phase-A kernel
        sums its terms in another order) must be followed by this"""
        self.S = lm.dev_lower(self.cone.dual_matrix())
        Lf, info = self.blk.factor(self.S)
        assert info == 0
        self.Sinv = self.blk.inverse(Lf)
        self.K = xp.inverse(self.S)

    def oracle_build(self, K, t):
        """the oracle's build with K in S^-1's place; the generic strategy (M3) where the planned one cannot take this data
        (the sparse strategy's pair traces have no dense objective)"""
        try:
            return self.blk.kkt_build(K, RD, t)
        except RuntimeError:
            return self.blk.kkt_build(K, RD, t, fixed=2)

    def reference(self):
        """(oracle, truth, floors) of a HOMOGENEOUS build at this S (a superset of what INFEASIBLE and CORRECTOR builds give);
        floors: for each single scalar, the relative first-order effect of one unit of rounding in the factorisation of S"""
        tru = xp.schur(self.K, self.C, RD, self.fam, 2)
        P = xp.scalar_sensitivities(self.K, self.C, RD)
        floors = {k: xp.rounding_bound(P[k], self.S) / abs(float(tru[k])) for k in SCALARS}
        return self.oracle_build(self.Sinv, 2), tru, floors

    def close(self):
        self.cone.destroy()
        self.blk.close()


KEYS = {0: ("M", "ASinv", "ASinvRdSinv", "TraceSinv"),
        1: ("ASinv", "ASinvRdSinv"),
        2: ("M", "ASinv", "ASinvRdSinv", "ASinvCSinv", "CSinv", "CSinvCSinv", "CSinvRdSinv", "TraceSinv"),
        3: ("M", "ASinv", "ASinvRdSinv", "TraceSinv")}
# Single scalars of a build at S: one number each, and the oracle's miss on it is one draw of its rounding.  Two correct fp64
# evaluations at the same S (the oracle's potrf / potri, LAPACK's dpotri) were measured 10x to 200x apart on them at cond 1e6 -
# 1e10, so err(oracle) alone is no yardstick there: the reference error of a scalar is at least its rounding floor.
SCALARS = ("TraceSinv", "CSinv", "CSinvCSinv", "CSinvRdSinv")


def compare_build(got, ref, tru, t, m, bad, label, floors=None, keys=None):
    """got / ref: dicts with kkt_build's keys (M as the engine leaves it, C-order upper valid); floors: lower bounds of the
    reference error of single scalars (State.reference); keys: the quantities to hold (default: all the build type gives);
    returns the worst ratio"""
    iu = np.triu_indices(m)
    worst = 0.0
    for key in (KEYS[t] if keys is None else keys):
        g, r, x = got[key], ref[key], tru[key]
        if key == "M":
            g, r, x = np.asarray(g)[iu], np.asarray(r)[iu], np.asarray(x)[iu]
            full = lambda v: np.triu(v) + np.triu(v, 1).T   # noqa: E731
            eg, er = diag_err(full(got["M"]), tru["M"]), diag_err(full(ref["M"]), tru["M"])
            worst = max(worst, eg / max(er, 16 * U))
            if not within(eg, er):
                bad.append(f"{label} type {t} diag(M): {eg:.3e} vs oracle {er:.3e}")
        eg, er = err(np.atleast_1d(g), np.atleast_1d(x)), err(np.atleast_1d(r), np.atleast_1d(x))
        if floors and key in floors:
            er = max(er, floors[key])
        worst = max(worst, eg / max(er, 16 * U))
        if not within(eg, er):
            bad.append(f"{label} type {t} {key}: {eg:.3e} vs oracle {er:.3e}")
    return worst


def engine_out(kkt, ex):
    out = dict(ex)
    out["M"] = kkt.M.copy()
    return out


def check_schur_solve(kkt, spectrum, cond, path, bad, label):
    """group C: factorize + solve on the engine's own M, against LAPACK on the same matrix"""
    from hdsdp_amd import api
    Mh = kkt.M.copy()
    A = np.triu(Mh) + np.triu(Mh, 1).T
    b = np.cos(np.arange(A.shape[0]) + 0.5)
    kkt.factorize()
    x = kkt.solve(b)
    try:
        Lc = sl.cho_factor(A, lower=True)
        lapack_pd = True
        e_lap = float(xp.backward_error(A, sl.cho_solve(Lc, b), b)[0])
    except np.linalg.LinAlgError:
        lapack_pd = False
        e_lap = float(xp.backward_error(A, sl.solve(A, b, assume_a="sym"), b)[0])
    switched = kkt.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
    if switched == lapack_pd:
        bad.append(f"{label} Schur solve: pivoted solver {switched}, LAPACK potrf {'succeeds' if lapack_pd else 'fails'}")
    e = float(xp.backward_error(A, x, b)[0])
    report("C", path, spectrum, cond, e / max(e_lap, 16 * U), label)
    if not within(e, e_lap):
        bad.append(f"{label} Schur solve backward error {e:.3e} vs LAPACK {e_lap:.3e}")


B_CASES = [("dense", 100, 16), ("dense", 129, 16), ("dense", 256, 24),
           ("r1", 128, 48), ("r1", 300, 48), ("r1", 640, 32),
           ("sparse", 129, 40), ("sparse", 383, 40)]


@pytest.mark.parametrize("kind,n,m,spectrum", [pytest.param(k, n, m, sp, id=f"{k}-{n}x{m}-{sp}") for k, n, m in B_CASES for sp in SPECTRA])
def test_schur_build_at_ill_conditioned_states(kind, n, m, spectrum, monkeypatch):
    """groups B and C: INFEASIBLE, HOMOGENEOUS and CORRECTOR builds on the family's own device path against the longdouble
    truth at the engine's S, under the oracle-relative bar; then the Schur solve on the engine's M against LAPACK"""
    from hdsdp_amd import api
    bad = []
    for ci, cond in enumerate(CONDS):
        st = State(monkeypatch, kind, n, m, spectrum, cond, seed=1000 * n + 10 * m + ci)
        try:
            assert st.cone.path == PATH[kind]
            kkt = api.KKT(m, [st.cone])
            try:
                worst = 0.0
                label = f"{kind} {n}x{m} {spectrum} cond={cond:g}"
                ref, tru, floors = st.reference()
                for t in (api.KKT_TYPE_INFEASIBLE, api.KKT_TYPE_HOMOGENEOUS, api.KKT_TYPE_CORRECTOR):
                    kkt.build_up(t)
                    got = engine_out(kkt, kkt.export())
                    worst = max(worst, compare_build(got, ref, tru, t, m, bad, label, floors))
                report("B", PATH[kind], spectrum, cond, worst, f"{kind} {n}x{m}")
                kkt.build_up(api.KKT_TYPE_INFEASIBLE)
                check_schur_solve(kkt, spectrum, cond, PATH[kind], bad, label)
            finally:
                kkt.destroy()
        finally:
            st.close()
    assert not bad, "\n".join(bad)


def phase_a_case(monkeypatch, spectrum, ci, part):
    """one fused Phase-A pass of a small rank-one block (its M factored in registers, cond(M) about cond(S)^2).  part "build":
    M, ASinv, ASinvRdSinv, tr S^-1 against the truth; part "solutions": the three solutions against the truth M* and
    right-hand sides, where cond(M*) < 1e14 (beyond that the longdouble refinement of the truth itself stalls); the oracle's
    solutions are LAPACK's on the oracle's M.  The kernel assembles S again, in its own order: oracle and truth are taken at
    the S it leaves, read after the pass"""
    from hdsdp_amd import api
    n, m = 128, 48
    cond = CONDS[ci]
    bad = []
    st = State(monkeypatch, "r1sparse", n, m, spectrum, cond, seed=77 + ci)
    try:
        assert st.cone.path == 1
        kkt = api.KKT(m, [st.cone])
        try:
            assert kkt.phase_a_eligible()
            rhs = np.sin(np.arange(m) + 1.0)
            ok, _, d1, d2, d3 = kkt.phase_a(1.0, st.y, rhs)
            assert ok
            label = f"phase A {spectrum} cond={cond:g}"
            got = engine_out(kkt, kkt.export())
            st.rebase()
            ref, tru, floors = st.reference()
            if part == "build":
                report("B", "1 phase A", spectrum, cond, compare_build(got, ref, tru, 0, m, bad, label, floors), f"r1sparse {n}x{m}")
            else:
                worst = 0.0
                Ms = tru["M"]
                if np.linalg.cond(Ms.astype(np.float64)) < 1e14:
                    Mo = np.triu(ref["M"]) + np.triu(ref["M"], 1).T
                    for d, r_orc, r_tru in ((d1, rhs, rhs), (d2, ref["ASinv"], tru["ASinv"]), (d3, ref["ASinvRdSinv"], tru["ASinvRdSinv"])):
                        xt = xp.solve(Ms, np.asarray(r_tru, dtype=LD))
                        xo = sl.cho_solve(sl.cho_factor(Mo, lower=False), r_orc)
                        eg, eo = err(d, xt), err(xo, xt)
                        worst = max(worst, eg / max(eo, 16 * U))
                        if not within(eg, eo):
                            bad.append(f"{label} solution: {eg:.3e} vs oracle {eo:.3e}")
                report("B", "1 phase A solutions", spectrum, cond, worst, f"r1sparse {n}x{m}")
        finally:
            kkt.destroy()
    finally:
        st.close()
    assert not bad, "\n".join(bad)


# Not fixed: the fused kernel misses the bar by about 11x at cond 1e6 in two places (measured twice, 11x-17x).  Not strict: the
# kernel sums the sparse terms of S with LDS atomics, so its S -- and the size of the miss -- is not the same bits every run.
PHASE_A_M = pytest.mark.xfail(strict=False, reason="fused Phase-A M and ASinvRdSinv at late 1e6: 3.0e-10 vs oracle 2.7e-11")
PHASE_A_SOLUTION = pytest.mark.xfail(strict=False, reason="fused Phase-A third solution at graded 1e6: 5.9e-14 vs oracle 5.3e-15")
PA_IDS = [(sp, ci) for sp in SPECTRA for ci in range(len(CONDS))]


@pytest.mark.parametrize("spectrum,ci", [pytest.param(sp, ci, id=f"{sp}-{CONDS[ci]:g}",
                                                      marks=[PHASE_A_M] if (sp, ci) == ("late", 1) else []) for sp, ci in PA_IDS])
def test_fused_phase_a_build_at_ill_conditioned_states(spectrum, ci, monkeypatch):
    phase_a_case(monkeypatch, spectrum, ci, "build")


@pytest.mark.parametrize("spectrum,ci", [pytest.param(sp, ci, id=f"{sp}-{CONDS[ci]:g}",
                                                      marks=[PHASE_A_SOLUTION] if (sp, ci) == ("graded", 1) else []) for sp, ci in PA_IDS])
def test_fused_phase_a_solutions_at_ill_conditioned_states(spectrum, ci, monkeypatch):
    phase_a_case(monkeypatch, spectrum, ci, "solutions")


@pytest.fixture
def group():
    """a loopback device group of the requested size; back to the plain engine afterwards (tests/test_gpu_group.py)"""
    from hdsdp_amd import api

    def make(world, min_dim=0):
        api.set_devices([0] * world, shard_min_dim=min_dim)
        ids, transport = api.device_group()
        assert ids == [0] * world and transport == 0
    yield make
    api.set_devices([0])


@pytest.mark.parametrize("spectrum", SPECTRA)
def test_sharded_schur_build_at_ill_conditioned_states(spectrum, group, monkeypatch):
    """one dense case through two loopback shards: the sharded build sums M in another order"""
    from hdsdp_amd import api
    n, m = 129, 16
    group(2)
    bad = []
    for ci, cond in enumerate(CONDS):
        st = State(monkeypatch, "dense", n, m, spectrum, cond, seed=31 + ci, force_path=False)
        try:
            assert st.cone.shard_count() == 2
            kkt = api.KKT(m, [st.cone])
            try:
                worst = 0.0
                ref, tru, floors = st.reference()
                for t in (api.KKT_TYPE_INFEASIBLE, api.KKT_TYPE_HOMOGENEOUS, api.KKT_TYPE_CORRECTOR):
                    kkt.build_up(t)
                    got = engine_out(kkt, kkt.export())
                    worst = max(worst, compare_build(got, ref, tru, t, m, bad, f"sharded {spectrum} cond={cond:g}", floors))
                report("B", "0 sharded x2", spectrum, cond, worst, f"dense {n}x{m}")
            finally:
                kkt.destroy()
        finally:
            st.close()
    assert not bad, "\n".join(bad)


def primal_matrices(n, m):
    """X = V V^T + eps I, rank(V) = n/8, eps 1e-6 and 1e-12, and V V^T itself (integers / 16: exact, exactly rank n/8, PSD)"""
    rng = np.random.default_rng(n + m)
    V = rng.integers(-4, 5, (n, max(1, n // 8))).astype(np.float64)
    Xs = {"rank-deficient": (V @ V.T) / 16.0}
    for eps in (1e-6, 1e-12):
        Xs[f"eps={eps:g}"] = (V @ V.T) / 16.0 + eps * np.eye(n)
    return Xs


def primal_build(monkeypatch, kind, n, m, names, keys, group_report=True):
    from hdsdp_amd import api
    st = State(monkeypatch, kind, n, m, "spread", 1e2, seed=5 + n)
    bad = []
    try:
        Xs = primal_matrices(n, m)
        kkt = api.KKT(m, [st.cone])
        try:
            for name in names:
                X = Xs[name]
                kkt.register_psdp([X])
                kkt.build_up(api.KKT_TYPE_PRIMAL)
                got = engine_out(kkt, kkt.export())
                ref = st.oracle_build(X, 3)
                tru = xp.schur(X.astype(LD), st.C, RD, st.fam, 3)
                route = st.cone.primal_route()
                worst = compare_build(got, ref, tru, 3, m, bad, f"primal {kind} {name} route {route}", keys=keys)
                if group_report:
                    report("D", PATH[kind], name, 0, worst, f"{kind} {n}x{m} route {route}")
        finally:
            kkt.destroy()
    finally:
        st.close()
    assert not bad, "\n".join(bad)


D_CASES = [("dense", 129, 16), ("r1", 128, 48), ("sparse", 129, 40)]


@pytest.mark.parametrize("kind,n,m", D_CASES, ids=[f"{k}-{n}x{m}" for k, n, m in D_CASES])
def test_primal_build_at_a_nearly_singular_x(kind, n, m, monkeypatch):
    """group D: KKT_TYPE_PRIMAL with X = V V^T + eps I (rank(V) = n/8, eps 1e-6 and 1e-12) and an exactly rank-deficient PSD X,
    whatever route the engine takes, against the longdouble tr(A_i X A_j X); the oracle gets S^-1 := X.  M and tr X at every X,
    everything at the two X = V V^T + eps I; ASinv and ASinvRdSinv at the rank-deficient X are the next test's"""
    primal_build(monkeypatch, kind, n, m, ["eps=1e-06", "eps=1e-12"], None)
    primal_build(monkeypatch, kind, n, m, ["rank-deficient"], ("M", "TraceSinv"))


SIGNED_ROUTE_TRACES = pytest.mark.xfail(strict=True, reason=(
    "not fixed: an exactly rank-deficient PSD X takes the signed factor (route 1: unpivoted LDL^T, 55-58 negative pivots of "
    "rounding size, growth 3.8), and tr(A_i X), Rd tr(A_i X X) are formed from the factor, not from X: 2.4e-14 / 1.2e-13 "
    "against the oracle's direct 4.3e-16 / 8.2e-16, the size of the factor's backward error n u |F||S||F^T|"))


@pytest.mark.parametrize("kind,n,m", [pytest.param("dense", 129, 16, marks=SIGNED_ROUTE_TRACES), ("r1", 128, 48),
                                      pytest.param("sparse", 129, 40, marks=SIGNED_ROUTE_TRACES)],
                         ids=[f"{k}-{n}x{m}" for k, n, m in D_CASES])
def test_primal_trace_vectors_at_a_rank_deficient_x(kind, n, m, monkeypatch):
    """ASinv and ASinvRdSinv of KKT_TYPE_PRIMAL at an exactly rank-deficient PSD X, under the oracle-relative bar"""
    primal_build(monkeypatch, kind, n, m, ["rank-deficient"], ("ASinv", "ASinvRdSinv"), group_report=False)


# ---------------------------------------------------------------- group E: the factor's other code paths

WORKER = r'''
import sys
sys.path.insert(0, %r)
import test_gpu_conditioning as tc
for n in (129, 383, 512, 2000):
    tc.check_dense_factor(n, "spread", 1e8, seed=2, label="E")
    tc.check_dense_factor(n, "late", 1e10, seed=3, label="E")
print("CONDITIONING_WORKER_OK")
'''


@pytest.mark.parametrize("env", [{"HDM_DIAG_SWEEP": "0"}, {"HDM_CHOL_K128": "0"}, {"HDM_TRSV_FLOW": "0"}],
                         ids=["lds-panel-diagonal-block", "general-gemm-panel-and-update", "per-block-substitution"])
def test_dense_factor_code_paths_at_ill_conditioned_matrices(env):
    """a reduced group A (spread at 1e8, late iterate at 1e10; n = 129, 383, 512, 2000) behind each switch; child process:
    the switches are read once per process"""
    # (HDSDP_MI355X_LIB is kept: it names the library build under test)
    e = {k: v for k, v in os.environ.items()
         if not (k.startswith("HDM_") or k.startswith("HDSDP_MI355X_")) or k == "HDSDP_MI355X_LIB"}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", WORKER % HERE], capture_output=True, text=True, timeout=300, env=e)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("COND_REPORT")))
    assert r.returncode == 0 and "CONDITIONING_WORKER_OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
