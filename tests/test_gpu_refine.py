"""The refined Schur solve on the device: the twice-precision residual kernel against exact arithmetic, the
accuracy of refined solves against a host model of the same iteration, "off is off", the stop reasons, every storage form of the
Schur operator, and the environment switch.

Host model (`host_model`): LAPACK's Cholesky (dgetrf once an object is switched to the pivoted solver), the same number of
refinement steps the engine reports, the residual accumulated in long double.  Truth: xprec_ref.solve(S, b, steps=6).  Forward error
e = max|x - x*| / max|x*| (test_gpu_conditioning.err).  The yardstick is that file's: e(gpu) <= 8 e(model) + 16 u.

A linear system made by HFpLinsysCreate has no tolerance set, so its refined solve stops at the reference's default 1e-6
(hdsdp_linsolver.c:1314-1315) -- above the unrefined residual of every matrix here.  The accuracy cases therefore hand the object the
Schur operator's own tolerances (HKKTInit: 5e-12 relative, 1e-12 absolute) through HFpLinsysSetParam, as HKKTInit does.

Measured on an MI355X (profiles/refine_accuracy.jsonl has every line): see the REFINE_REPORT lines this file prints."""
import fractions
import functools
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
import xprec_ref as xp  # noqa: E402
from chain_operator import CHAIN_M, banded_chain  # noqa: E402
from test_gpu_conditioning import err, target, within  # noqa: E402
from util import load_golden, y_of  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xp.HAVE_LD, reason=xp.NO_LD_REASON)]

U = 2.0 ** -53
LD = xp.LD
F = fractions.Fraction
SCHUR_REL, SCHUR_ABS = 5e-12, 1e-12          # HKKTInit's tolerances for m <= 5000 (hdsdp_schur.c:21-35)


def report(**kw):
    print("REFINE_REPORT " + json.dumps({k: (float(v) if isinstance(v, (np.floating, float)) else v) for k, v in kw.items()}))


def full(Mc):
    """C-order view of a column-major lower triangle -> the full symmetric matrix"""
    return np.triu(Mc) + np.triu(Mc, 1).T


# ---------------------------------------------------------------- 1. the kernel against exact arithmetic

@functools.lru_cache(maxsize=None)
def kernel_case(n):
    """(M, x, b, r* rounded once, (|M| |x| + |b|), sum r*_i^2 exactly) -- computed once per n, shared, not to be written to"""
    rng = np.random.default_rng(n)
    M = target(rng, n, "spread", 1e6)
    b = rng.standard_normal(n)
    x = np.linalg.solve(M, b)
    Mf = [[F(float(M[max(i, j), min(i, j)])) for j in range(n)] for i in range(n)]     # the lower triangle, mirrored
    xf = [F(float(v)) for v in x]
    rex = [F(float(b[i])) - sum(Mf[i][j] * xf[j] for j in range(n)) for i in range(n)]
    L = np.tril(M)
    Ms = L + np.tril(L, -1).T
    env = np.abs(Ms) @ np.abs(x) + np.abs(b)
    out = (Ms, x, b, np.array([float(v) for v in rex]), env, rex)
    for a in out[:5]:
        a.setflags(write=False)
    return out


def poisoned_layout(Ms, n, ld):
    """the column-major ld x n array of the lower triangle, NaN above the diagonal and in the rows >= n (C order: A[j, i] = M(i, j))"""
    A = np.full((n, ld), np.nan)
    for j in range(n):
        A[j, j:n] = Ms[j:, j]
    return A


@pytest.mark.parametrize("padded", [False, True], ids=["ld=n", "ld=roundup(n,128)"])
@pytest.mark.parametrize("n", [1, 2, 17, 64, 127, 128, 129, 257])
def test_residual_kernel_against_exact_arithmetic(n, padded):
    """x is the fp64 solution of M x = b, so b - M x is pure cancellation: about n u |M| |x| in working precision, and exact to
    one rounding plus the second-order term in twice the working precision.  Required (the Dot2 bound of Ogita, Rump and Oishi):
    |r - r*|_i <= 2 u |r*_i| + 2 (n + 2)^2 u^2 (|M| |x| + |b|)_i, the squared norm within 4 u of the sum of squares of what the
    kernel returned and of the exact residual's once that bound is carried through, and two runs identical bit for bit.
    Nothing above the diagonal or below row n may be read: it is all NaN."""
    from hdsdp_amd import api
    Ms, x, b, rstar, env, rex = kernel_case(n)
    ld = ((n + 127) // 128) * 128 if padded else n
    A = poisoned_layout(Ms, n, ld)
    r, nrm = api.sym_residual(A, x, b, n=n, ld=ld)
    r2, nrm2 = api.sym_residual(A, x, b, n=n, ld=ld)
    assert np.array_equal(r, r2) and nrm == nrm2, "two runs differ"
    assert np.all(np.isfinite(r)) and np.isfinite(nrm), "the kernel read the NaN filling"
    bound = 2.0 * U * np.abs(rstar) + 2.0 * (n + 2) ** 2 * U * U * env
    miss = np.array([abs(F(float(r[i])) - rex[i]) for i in range(n)], dtype=object)
    worst = max(float(miss[i]) / bound[i] for i in range(n))
    plain = np.abs((b - Ms @ x) - rstar)             # what a working-precision residual leaves
    ss_kernel = sum(F(float(v)) ** 2 for v in r)
    ss_exact = float(sum(v * v for v in rex))
    carried = float(np.sum(2.0 * np.abs(rstar) * bound + bound * bound))
    e_own = abs(float(F(nrm) - ss_kernel))
    report(case="kernel", n=n, ld=ld, worst_over_bound=worst, plain_over_bound=float(np.max(plain / bound)), norm2=nrm,
           norm2_err_own_u=e_own / (U * float(ss_kernel)) if ss_kernel else 0.0)
    assert worst <= 1.0, (n, ld, worst)
    assert e_own <= 4.0 * U * float(ss_kernel), (n, ld)
    assert abs(nrm - ss_exact) <= 4.0 * U * ss_exact + carried, (n, ld)


# ---------------------------------------------------------------- the host model

def host_model(A, b, steps, pivoted=False):
    """LAPACK factorisation, `steps` refinement steps with the residual in long double"""
    if pivoted:
        f = sl.lu_factor(A, check_finite=False)
        solve = lambda v: sl.lu_solve(f, v, check_finite=False)   # noqa: E731
    else:
        f = sl.cho_factor(A, lower=True, check_finite=False)
        solve = lambda v: sl.cho_solve(f, v, check_finite=False)   # noqa: E731
    x = solve(b)
    for _ in range(steps):
        r = (b.astype(LD) - xp.mm(A, x.reshape(-1, 1)).ravel()).astype(np.float64)
        x = x + solve(r)
    return x


@functools.lru_cache(maxsize=None)
def system(n, spectrum, cond):
    """(S, b, truth) of the issue's model: default_rng(n), b = rng.standard_normal(n); shared, not to be written to"""
    rng = np.random.default_rng(n)
    S = target(rng, n, spectrum, cond)
    b = rng.standard_normal(n)
    t = xp.solve(S, b, steps=6)
    for a in (S, b, t):
        a.setflags(write=False)
    return S, b, t


# ---------------------------------------------------------------- 2. accuracy of the refined solve

@pytest.mark.parametrize("cond", [1e6, 1e10])
@pytest.mark.parametrize("spectrum", ["spread", "graded"])
@pytest.mark.parametrize("n", [33, 129, 257])
@pytest.mark.parametrize("ltype", ["DENSE_DIRECT", "DENSE_ITERATIVE"])
def test_refined_solve_accuracy(ltype, n, spectrum, cond):
    from hdsdp_amd import api
    S, b, truth = system(n, spectrum, cond)
    lt = getattr(api, "HDSDP_LINSYS_" + ltype)
    plain, refined = api.LinSys(n, lt), api.LinSys(n, lt)
    try:
        plain.numeric(S)
        x0 = plain.solve(b)
        refined.set_param(relTol=SCHUR_REL, absTol=SCHUR_ABS)
        refined.set_refine(3)
        refined.numeric(S)
        x = refined.solve(b)
        st = refined.refine_stats()
        pivoted = refined.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
    finally:
        plain.destroy()
        refined.destroy()
    e0, e = err(x0, truth), err(x, truth)
    e_model = err(host_model(S, b, st["steps"], pivoted), truth)
    be0, be = float(xp.backward_error(S, x0, b)[0]), float(xp.backward_error(S, x, b)[0])
    report(case="accuracy", ltype=ltype, n=n, spectrum=spectrum, cond=cond, status=st["status_name"], steps=st["steps"],
           resid0=st["resid0"], resid=st["resid"], tol=st["tol"], e_unrefined=e0, e_refined=e, e_model=e_model, gain=e0 / max(e, U),
           backward_unrefined=be0, backward_refined=be)
    assert st["cap"] == 3 and st["status"] not in (api.REFINE_OFF, api.REFINE_NO_MATRIX, api.REFINE_NOT_AVAILABLE), st
    assert st["steps"] <= 3 and st["resid"] <= st["resid0"]
    assert within(e, e_model), (e, e_model)
    assert be <= be0, (be, be0)
    if spectrum == "spread" and cond == 1e10:
        assert e <= e0 / 30.0, (e, e0)


# ---------------------------------------------------------------- 3. off is off

@pytest.mark.parametrize("nrhs", [1, 5])
@pytest.mark.parametrize("ltype", ["DENSE_DIRECT", "DENSE_ITERATIVE"])
def test_off_is_off(ltype, nrhs):
    """an object that never heard of refinement and one switched on and off again: the same bits, out of place and in place, status
    OFF, no device memory held"""
    from hdsdp_amd import api
    n = 129
    S, _, _ = system(n, "spread", 1e6)
    B = np.random.default_rng(5).standard_normal((nrhs, n))
    B = B[0] if nrhs == 1 else B
    lt = getattr(api, "HDSDP_LINSYS_" + ltype)
    a, c = api.LinSys(n, lt), api.LinSys(n, lt)
    try:
        a.numeric(S)
        xa = a.solve(B)
        xa_in = a.solve(B.copy(), inplace=True)
        assert np.array_equal(xa, xa_in)
        sa = a.refine_stats()
        assert (sa["cap"], sa["status"], sa["device_bytes"], sa["solves"]) == (0, api.REFINE_OFF, 0, 0)
        c.set_param(relTol=SCHUR_REL, absTol=SCHUR_ABS)
        c.set_refine(3)
        c.numeric(S)
        xr = c.solve(B)
        sr = c.refine_stats()
        assert sr["status"] != api.REFINE_OFF and sr["device_bytes"] > 0 and sr["solves"] == nrhs
        assert np.array_equal(xr, c.solve(B.copy(), inplace=True)), "refined: in place differs from out of place"
        c.set_refine(0)
        for again in (False, True):                  # with the factor it has, and after a new factorisation
            if again:
                c.numeric(S)
            xc = c.solve(B)
            xc_in = c.solve(B.copy(), inplace=True)
            sc = c.refine_stats()
            assert np.array_equal(xc, xa) and np.array_equal(xc_in, xa), again
            assert (sc["cap"], sc["status"], sc["steps"], sc["device_bytes"]) == (0, api.REFINE_OFF, 0, 0), sc
    finally:
        a.destroy()
        c.destroy()


# ---------------------------------------------------------------- 4. stops

def test_stop_converged_at_once_is_the_unrefined_solve():
    from hdsdp_amd import api
    n = 33
    S, b, _ = system(n, "spread", 1e2)
    plain, refined = api.LinSys(n), api.LinSys(n)
    try:
        plain.numeric(S)
        refined.set_refine(3)
        refined.numeric(S)
        x0, x = plain.solve(b), refined.solve(b)
        st = refined.refine_stats()
    finally:
        plain.destroy()
        refined.destroy()
    report(case="stop", which="cond 1e2", **{k: st[k] for k in ("status_name", "steps", "resid0", "resid", "tol")})
    assert (st["status"], st["steps"]) == (api.REFINE_CONVERGED, 0) and st["resid"] == st["resid0"] < st["tol"]
    assert st["tol"] == 1e-6                          # nothing set: the reference's defaults, |b| > 1
    assert np.array_equal(x, x0)


def test_stops_short_of_an_unreachable_tolerance():
    from hdsdp_amd import api
    n = 129
    S, b, _ = system(n, "spread", 1e10)
    ls = api.LinSys(n, api.HDSDP_LINSYS_DENSE_ITERATIVE)
    try:
        ls.set_param(relTol=SCHUR_REL, absTol=SCHUR_ABS)
        ls.set_refine(3)
        ls.numeric(S)
        ls.solve(b)
        st = ls.refine_stats()
        report(case="stop", which="cond 1e10", **{k: st[k] for k in ("status_name", "steps", "resid0", "resid", "tol")})
        assert st["status"] in (api.REFINE_STAGNATED, api.REFINE_MAXSTEPS) and st["steps"] <= 3 and st["resid"] <= st["resid0"]
        assert st["tol"] == SCHUR_ABS
        # a tolerance nothing reaches: never CONVERGED, whatever the conditioning
        for cond in (1e2, 1e10):
            S2, b2, _ = system(n, "spread", cond)
            ls.set_param(relTol=1e-30, absTol=1e-30)
            ls.numeric(S2)
            ls.solve(b2)
            st = ls.refine_stats()
            report(case="stop", which=f"tol 1e-30, cond {cond:g}", **{k: st[k] for k in ("status_name", "steps", "resid0", "resid", "tol")})
            assert st["status"] in (api.REFINE_STAGNATED, api.REFINE_MAXSTEPS), st
            assert st["resid"] <= st["resid0"] and st["steps"] <= 3
        # a cap of one
        ls.set_refine(1)
        before = ls.refine_stats()["total_steps"]
        ls.solve(b2)
        st = ls.refine_stats()
        assert st["cap"] == 1 and st["steps"] <= 1 and st["total_steps"] - before <= 1
        ls.set_refine(100)
        assert ls.refine_stats()["cap"] == 8
    finally:
        ls.destroy()


def test_a_nan_right_hand_side_still_escalates():
    """NUMERICAL hands back the unrefined solution, NaN and all, and HFpLinsysSolve's own check does what it always did: the Schur
    system switches to the pivoted solver and fails on the NaN; the dual-matrix object just fails"""
    from hdsdp_amd import api
    n = 33
    S, b, _ = system(n, "spread", 1e2)
    bad = b.copy()
    bad[0] = np.nan
    ls = api.LinSys(n, api.HDSDP_LINSYS_DENSE_ITERATIVE)
    try:
        ls.set_refine(2)
        ls.numeric(S)
        with pytest.raises(api.HDSDPError):
            ls.solve(bad)
        assert ls.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
        assert ls.refine_stats()["status"] == api.REFINE_NUMERICAL
        x = ls.solve(b)                               # the switched object goes on refining, through the pivoted solver
        st = ls.refine_stats()
        assert st["status"] == api.REFINE_CONVERGED and np.allclose(S @ x, b, atol=1e-9)
    finally:
        ls.destroy()


# ---------------------------------------------------------------- 5. every storage form of the Schur operator

def operator_checks(kkt, label, b, device_source, pivoted=False, shift=True):
    """build, shift the diagonal, regularise, factorise, solve with set_refine(2); then a corrector build (still refined), a new
    build without a factorisation (device source: NO_MATRIX and the unrefined solve of the old factor; host source: the copy still
    serves), and refinement off (the unrefined solve).  Returns nothing; asserts."""
    from hdsdp_amd import api
    m = kkt.m
    kkt.set_refine(2)
    kkt.build_up(api.KKT_TYPE_INFEASIBLE)
    if kkt.diag_target() == 0:
        # HKKTRegularize caps its own term at 1e-5 (hdsdp_schur.c:348-373), so the shift of 1e-3 max diag(M) goes in the way the
        # driver's bound cone adds to the diagonal: through kktDiag, on the host matrix, where only the factorised matrix has it
        d = np.diag(full(kkt.M))
        if shift:
            kkt.add_to_diag(1e-3 * float(np.max(d)))
    kkt.regularize(1e-3)
    kkt.factorize()
    x = kkt.solve(b)
    st = kkt.refine_stats()
    A = full(kkt.M) if kkt.diag_target() == 0 else kkt.rows(np.arange(m))
    A = np.ascontiguousarray(xp.sym(A))
    truth = xp.solve(A, b)
    assert st["cap"] == 2 and st["status"] in (api.REFINE_CONVERGED, api.REFINE_STAGNATED, api.REFINE_MAXSTEPS), (label, st)
    assert st["tol"] == SCHUR_ABS                     # HKKTInit's own tolerances, whatever the storage form (|b| > 1)
    # these operators are well conditioned: the first residual is below HKKTInit's tolerance already.  Held to a tolerance nothing
    # reaches, the loop has to correct -- through the permutation and the pivoted solver where the form has them
    forced = forced_steps(kkt, A, b, truth, label, pivoted)
    kkt.set_param(relTol=SCHUR_REL, absTol=SCHUR_ABS)
    # a corrector build touches neither M nor the factor: still refined, the same bits
    kkt.build_up(api.KKT_TYPE_CORRECTOR)
    xc = kkt.solve(b)
    sc = kkt.refine_stats()
    assert sc["status"] == st["status"] and np.array_equal(xc, x), (label, sc)
    # a new build without a factorisation
    kkt.build_up(api.KKT_TYPE_INFEASIBLE)
    xn = kkt.solve(b)
    sn = kkt.refine_stats()
    kkt.set_refine(0)
    x0 = kkt.solve(b)
    s0 = kkt.refine_stats()
    assert (s0["cap"], s0["status"], s0["device_bytes"]) == (0, api.REFINE_OFF, 0), (label, s0)
    if device_source:
        assert sn["status"] == api.REFINE_NO_MATRIX and sn["steps"] == 0 and np.array_equal(xn, x0), (label, sn)
    else:
        assert sn["status"] == st["status"] and np.array_equal(xn, x), (label, sn)
    e, e0 = err(x, truth), err(x0, truth)
    e_model = err(host_model(A, b, st["steps"], pivoted), truth)
    report(case="operator", form=label, m=m, status=st["status_name"], steps=st["steps"], resid0=st["resid0"], resid=st["resid"],
           tol=st["tol"], e_unrefined=e0, e_refined=e, e_model=e_model, cond=float(np.linalg.cond(A)))
    assert within(e, e_model), (label, e, e_model)
    assert e <= 2.0 * e0 + 16.0 * U, (label, e, e0)
    assert forced <= 2.0 * e0 + 16.0 * U, (label, forced, e0)


def forced_steps(obj, A, b, truth, label, pivoted):
    """the same solve under a tolerance of 1e-30: at least one correction is made, the loop stops at STAGNATED or MAXSTEPS, and what
    comes back is held to the model after as many steps; returns its forward error"""
    from hdsdp_amd import api
    before = obj.refine_stats()["total_steps"]
    obj.set_param(relTol=1e-30, absTol=1e-30)
    x = obj.solve(b)
    st = obj.refine_stats()
    e, e_model = err(x, truth), err(host_model(A, b, st["steps"], pivoted), truth)
    report(case="operator, tolerance 1e-30", form=label, status=st["status_name"], steps=st["steps"], corrections=st["total_steps"] - before,
           resid0=st["resid0"], resid=st["resid"], e_refined=e, e_model=e_model)
    assert st["status"] in (api.REFINE_STAGNATED, api.REFINE_MAXSTEPS) and st["total_steps"] - before >= 1, (label, st)
    assert st["steps"] <= st["cap"] and st["resid"] <= st["resid0"], (label, st)
    assert within(e, e_model), (label, e, e_model)
    return e


@pytest.mark.parametrize("mirror", [True, False], ids=["mirror-on", "mirror-off"])
def test_dense_operator_refines_from_the_right_matrix(mirror):
    from hdsdp_amd import api
    n = m = 64
    cone = api.SDPCone.synthetic(n, m)
    try:
        cone.set_start(-10.0 * n)
        assert cone.check_is_interior(1.0, np.zeros(m))
        kkt = api.KKT(m, [cone])
        try:
            if not mirror:
                kkt.set_host_mirror(False)
            assert not kkt.is_sparse and kkt.diag_target() == (0 if mirror else 1)
            operator_checks(kkt, "dense, mirror " + ("on" if mirror else "off"), np.sin(np.arange(m) + 1.0), device_source=not mirror)
        finally:
            kkt.destroy()
    finally:
        cone.destroy()


@pytest.mark.parametrize("scrambled", [False, True], ids=["csc", "csc-permuted"])
def test_csc_operator_refines_from_the_right_matrix(scrambled):
    from hdsdp_amd import api
    cones = []
    try:
        banded_chain(scrambled, cones)
        kkt = api.KKT(CHAIN_M, cones)
        try:
            assert kkt.is_sparse and kkt.tile_info() is None
            if os.environ.get("HDSDP_MI355X_KKT_ENVELOPE", "1") != "0" and os.environ.get("HDSDP_MI355X_KKT_RCM", "1") != "0":
                assert kkt.envelope_info()[0] == scrambled
            operator_checks(kkt, "csc, permuted" if scrambled else "csc", np.sin(np.arange(CHAIN_M) + 1.0), device_source=True)
        finally:
            kkt.destroy()
    finally:
        for c in cones:
            c.destroy()


def test_pivoted_solver_refines_through_its_own_corrections():
    """indef96: the Schur system object switches to the pivoted solver at its first numeric; the residual reads the device copy of
    the loaded image and the corrections are the pivoted solver's"""
    from hdsdp_amd import api
    g = load_golden("indef96")
    M, b = np.ascontiguousarray(g["indef_M"]), np.ascontiguousarray(g["indef_b"])
    m = M.shape[0]
    A = np.ascontiguousarray(full(M))
    truth = xp.solve(A, b)
    plain, ls = api.LinSys(m, api.HDSDP_LINSYS_DENSE_ITERATIVE), api.LinSys(m, api.HDSDP_LINSYS_DENSE_ITERATIVE)
    try:
        plain.numeric(M)
        x0 = plain.solve(b)
        ls.set_param(relTol=SCHUR_REL, absTol=SCHUR_ABS)
        ls.set_refine(2)
        ls.numeric(M)
        assert ls.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
        x = ls.solve(b)
        st = ls.refine_stats()
        xin = ls.solve(b.copy(), inplace=True)
        forced = forced_steps(ls, A, b, truth, "switched to the pivoted solver (indef96)", True)
    finally:
        plain.destroy()
        ls.destroy()
    e, e0 = err(x, truth), err(x0, truth)
    assert forced <= 2.0 * e0 + 16.0 * U, (forced, e0)
    e_model = err(host_model(A, b, st["steps"], pivoted=True), truth)
    report(case="operator", form="switched to the pivoted solver (indef96)", m=m, status=st["status_name"], steps=st["steps"],
           resid0=st["resid0"], resid=st["resid"], tol=st["tol"], e_unrefined=e0, e_refined=e, e_model=e_model, cond=float(np.linalg.cond(A)))
    assert st["cap"] == 2 and st["status"] in (api.REFINE_CONVERGED, api.REFINE_STAGNATED, api.REFINE_MAXSTEPS), st
    assert np.array_equal(x, xin)
    assert within(e, e_model), (e, e_model)
    assert e <= 2.0 * e0 + 16.0 * U, (e, e0)


def test_switched_operator_refines_from_the_recorded_source():
    """the dense operator with its diagonal lowered until M is indefinite: HKKTFactorize switches, the refined solve reads the
    recorded source (the copy of the host matrix; the device matrix with the mirror off) and corrects through the pivoted solver"""
    from hdsdp_amd import api
    n = m = 64
    cone = api.SDPCone.synthetic(n, m)
    try:
        cone.set_start(-10.0 * n)
        assert cone.check_is_interior(1.0, np.zeros(m))
        b = np.sin(np.arange(m) + 1.0)
        kkt = api.KKT(m, [cone])
        try:
            kkt.set_refine(2)
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
            w = np.linalg.eigvalsh(full(kkt.M))
            kkt.add_to_diag(-0.5 * (w[0] + w[-1]))
            A = np.ascontiguousarray(full(kkt.M))
            kkt.factorize()
            assert kkt.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
            x = kkt.solve(b)
            st = kkt.refine_stats()
            truth = xp.solve(A, b)
            forced = forced_steps(kkt, A, b, truth, "dense, switched at HKKTFactorize", True)
            kkt.set_refine(0)
            x0 = kkt.solve(b)
        finally:
            kkt.destroy()
    finally:
        cone.destroy()
    e, e0 = err(x, truth), err(x0, truth)
    assert forced <= 2.0 * e0 + 16.0 * U, (forced, e0)
    e_model = err(host_model(A, b, st["steps"], pivoted=True), truth)
    report(case="operator", form="dense, switched at HKKTFactorize", m=m, status=st["status_name"], steps=st["steps"], resid0=st["resid0"],
           resid=st["resid"], tol=st["tol"], e_unrefined=e0, e_refined=e, e_model=e_model, cond=float(np.linalg.cond(A)))
    assert st["status"] in (api.REFINE_CONVERGED, api.REFINE_STAGNATED, api.REFINE_MAXSTEPS), st
    assert within(e, e_model) and e <= 2.0 * e0 + 16.0 * U, (e, e_model, e0)


def test_tile_form_reports_not_available_and_solves_as_before():
    from hdsdp_amd import api
    g = load_golden("arrow128_A")
    m = int(g["mb_dims"][1])
    Rd, tau, y = float(g["Rd"][0]), float(g["tau"][0]), y_of(g)
    prob = api.read_sdpa(os.path.join(ROOT, "tests", "golden", "arrow128.dat-s"))
    cones = [api.SDPCone.from_csc(blk["n"], m, blk["beg"], blk["idx"], blk["val"], iCone=k) for k, blk in enumerate(prob["blocks"])]
    try:
        for cn in cones:
            cn.set_start(Rd)
            assert cn.check_is_interior(tau, y)
        b = np.sin(np.arange(m) + 1.0)
        got = []
        for refine in (0, 2):
            kkt = api.KKT(m, cones)
            try:
                assert kkt.is_sparse and kkt.tile_info() is not None
                kkt.set_refine(refine)
                kkt.build_up(api.KKT_TYPE_INFEASIBLE)
                kkt.add_to_diag(1e-3 * float(np.max(np.diag(full(kkt.M)))))
                kkt.regularize(1e-3)
                kkt.factorize()
                got.append(kkt.solve(b))
                st = kkt.refine_stats()
                assert st["cap"] == refine and st["device_bytes"] == 0
                assert st["status"] == (api.REFINE_NOT_AVAILABLE if refine else api.REFINE_OFF), st
                A = np.ascontiguousarray(full(kkt.M))
            finally:
                kkt.destroy()
        assert np.array_equal(got[0], got[1])
        assert np.linalg.norm(A @ got[1] - b) <= 1e-10 * np.linalg.cond(A) * np.linalg.norm(b)
    finally:
        for cn in cones:
            cn.destroy()


# ---------------------------------------------------------------- 6. the switch

def test_the_environment_switch_turns_refinement_on():
    env = dict(os.environ, HDSDP_MI355X_REFINE="2")
    r = subprocess.run([sys.executable, os.path.join(HERE, "refine_worker.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("REFINE_WORKER_JSON ")]
    assert line, r.stdout[-2000:]
    out = json.loads(line[0][len("REFINE_WORKER_JSON "):])
    assert out["before"]["cap"] == 2 and out["after"]["cap"] == 2
    assert out["after"]["status"] != 0 and out["after"]["solves"] == 1
    assert "HDSDP_MI355X_REFINE=2" in r.stderr
    assert out["residual"] <= 1e-12 * out["cond"], out
