"""The refined solve of the TILE form of a sparse Schur operator (csrc/tile_residual_plan.h, refine.hip's
hdm_tile_residual_kernel, HdmBspRefine): the residual kernel against exact arithmetic, accuracy through HMiBspRefinedSolve against
the host model of tests/test_gpu_refine.py, a quasi-definite matrix, the operator with the host mirror on and off, what keeps the
residual's matrix valid, and the environment switches.

The yardsticks are test_gpu_refine.py's: forward error e = max|x - x*| / max|x*| against xprec_ref.solve(.., steps=6), the host
model = LAPACK Cholesky + as many corrections as the engine reports with the residual in long double, e(gpu) <= 8 e(model) + 16 u.

Measured on an MI355X (profiles/refine_tiles_accuracy.jsonl has every REFINE_REPORT line of one run)."""
import fractions
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import sparse_schur_cases as sc  # noqa: E402
import xprec_ref as xp  # noqa: E402
from test_gpu_conditioning import err, within  # noqa: E402
from test_gpu_refine import forced_steps, full, host_model, report  # noqa: E402
from util import load_golden, y_of  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xp.HAVE_LD, reason=xp.NO_LD_REASON)]

U = 2.0 ** -53
F = fractions.Fraction
SCHUR_REL, SCHUR_ABS = 5e-12, 1e-12          # HKKTInit's tolerances for m <= 5000


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def bsp_solve(c):
    """HMiBspSolve (the unrefined tile solve) on an object with m, beg, idx, val, b: (x, negative pivots)"""
    import ctypes as C
    from hdsdp_amd import api
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    val, b = np.ascontiguousarray(c.val, dtype=np.float64), np.ascontiguousarray(c.b, dtype=np.float64)
    x, info, stats = np.full(c.m, np.nan), C.c_int(-1), (C.c_int * 4)(-1, -1, -1, -1)
    rc = api.load_library().HMiBspSolve(c.m, c.beg.ctypes.data_as(ip), c.idx.ctypes.data_as(ip), val.ctypes.data_as(dp), b.ctypes.data_as(dp),
                                        x.ctypes.data_as(dp), C.byref(info), stats, None)
    assert rc == 0 and info.value == 0, (rc, info.value)
    return x, stats[3]


# ---------------------------------------------------------------- 1. the kernel against exact arithmetic

KERNEL_CASES = [("band", 129, False), ("band", 193, False), ("band", 257, False), ("band", 257, True), ("arrow", 385, False),
                ("filltail", sc.FILLTAIL_M, False)]


@functools.lru_cache(maxsize=None)
def kernel_case(family, m, renumbered):
    """(case, x, r* rounded once, (|M| |x| + |b|), r* exactly): x is the fp64 solution; the exact residual runs over the pattern's
    non-zeros only.  Computed once, shared, not to be written to"""
    c = sc.tile_case(family, m, renumbered, "spd", 1e6, "down")
    x = np.linalg.solve(c.A, c.b)
    xf = [F(float(v)) for v in x]
    rex = [F(float(v)) for v in c.b]
    for i in range(m):
        rex[i] -= F(float(c.A[i, i])) * xf[i]
    for i, j in c.pairs:
        a = F(float(c.A[i, j]))
        rex[i] -= a * xf[j]
        rex[j] -= a * xf[i]
    env = np.abs(c.A) @ np.abs(x) + np.abs(c.b)
    out = (c, x, np.array([float(v) for v in rex]), env, rex)
    for a in out[1:4]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("family,m,renumbered", KERNEL_CASES)
def test_tile_residual_kernel_against_exact_arithmetic(family, m, renumbered):
    """the dense kernel's bars (test_gpu_refine.py::test_residual_kernel_against_exact_arithmetic) on the tile store: m = 129 leaves
    a last tile with one valid row, 193 a last quadrant with one, band 257 has no tile (2, 0) -- slot lists of different length --
    and filltail 1040 has tiles that exist only as fill.  The probe fills the store's padding and its spare tile with NaN."""
    from hdsdp_amd import api
    c, x, rstar, env, rex = kernel_case(family, m, renumbered)
    r, nrm = api.tile_residual(m, c.beg, c.idx, c.val, x, c.b)
    r2, nrm2 = api.tile_residual(m, c.beg, c.idx, c.val, x, c.b)
    assert same_bits(r, r2) and nrm == nrm2, "two runs differ"
    assert np.all(np.isfinite(r)) and np.isfinite(nrm), "the kernel read the NaN filling"
    bound = 2.0 * U * np.abs(rstar) + 2.0 * (m + 2) ** 2 * U * U * env
    worst = max(float(abs(F(float(r[i])) - rex[i])) / bound[i] for i in range(m))
    plain = np.abs((c.b - c.A @ x) - rstar)
    ss_kernel = sum(F(float(v)) ** 2 for v in r)
    ss_exact = float(sum(v * v for v in rex))
    carried = float(np.sum(2.0 * np.abs(rstar) * bound + bound * bound))
    e_own = abs(float(F(nrm) - ss_kernel))
    report(case="tile kernel", family=family, m=m, renumbered=renumbered, tiles=c.sym.ntiles, worst_over_bound=worst,
           plain_over_bound=float(np.max(plain / bound)), norm2=nrm, norm2_err_own_u=e_own / (U * float(ss_kernel)) if ss_kernel else 0.0)
    assert worst <= 1.0, (family, m, worst)
    assert e_own <= 4.0 * U * float(ss_kernel), (family, m)
    assert abs(nrm - ss_exact) <= 4.0 * U * ss_exact + carried, (family, m)


# ---------------------------------------------------------------- 2. accuracy through HMiBspRefinedSolve

ACCURACY_M = (257, 385, 640)


@functools.lru_cache(maxsize=None)
def second_difference_squared(m, permuted):
    """A = K^2, K = tridiag(-1, 2, -1) (pentadiagonal, exactly representable, not graded), b_i = sin(i + 1); `permuted`: under a
    fixed random symmetric permutation.  An object with m, beg, idx, val, b, A, truth; shared, not to be written to"""
    K = 2.0 * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1)
    A = K @ K
    b = np.sin(np.arange(m) + 1.0)
    if permuted:
        p = np.random.default_rng(m).permutation(m)
        A, b = np.ascontiguousarray(A[np.ix_(p, p)]), np.ascontiguousarray(b[p])
    c = types.SimpleNamespace(m=m, A=A, b=b)
    ii, jj = np.nonzero(np.tril(A, -1))
    c.beg, c.idx = sc.lower_csc(m, list(zip(ii.tolist(), jj.tolist())))
    c.val = sc.csc_values(A, c.beg, c.idx)
    c.truth = xp.solve(A, b, steps=6)
    for a in (c.A, c.b, c.val, c.truth):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def accuracy_run(m, permuted):
    """(unrefined x, refined x, the refined solve's report) -- one run per case, shared"""
    from hdsdp_amd import api
    c = second_difference_squared(m, permuted)
    x0, _ = bsp_solve(c)
    x, info, st = api.bsp_refined_solve(m, c.beg, c.idx, c.val, c.b, 3, SCHUR_REL, SCHUR_ABS)
    assert info == 0
    return x0, x, st


@pytest.mark.parametrize("permuted", [False, True], ids=["natural", "permuted"])
@pytest.mark.parametrize("m", ACCURACY_M)
def test_refined_tile_solve_accuracy(m, permuted):
    from hdsdp_amd import api
    c = second_difference_squared(m, permuted)
    x0, x, st = accuracy_run(m, permuted)
    e0, e = err(x0, c.truth), err(x, c.truth)
    e_model = err(host_model(c.A, c.b, st["steps"]), c.truth)
    report(case="tile accuracy", m=m, permuted=permuted, status=st["status_name"], steps=st["steps"], resid0=st["resid0"], resid=st["resid"],
           tol=st["tol"], e_unrefined=e0, e_refined=e, e_model=e_model, gain=e0 / max(e, U), tiles=st["tiles"], levels=st["levels"])
    assert st["status"] in (api.REFINE_CONVERGED, api.REFINE_STAGNATED, api.REFINE_MAXSTEPS), st
    assert st["steps"] <= 3 and st["resid"] <= st["resid0"], st
    assert within(e, e_model), (e, e_model)
    assert e <= 2.0 * e0 + 16.0 * U, (e, e0)
    if st["resid"] < st["resid0"]:                    # a corrected iterate went back: the dense file's bar for cond 1e10
        assert st["steps"] >= 1 and e <= e0 / 30.0, (e, e0)
    else:
        assert st["steps"] == 0 and same_bits(x, x0)


def test_at_least_one_accuracy_case_is_corrected():
    runs = [accuracy_run(m, p) for m in ACCURACY_M for p in (False, True)]
    assert any(st["resid"] < st["resid0"] for _, _, st in runs), [st for _, _, st in runs]


def test_a_reachable_tolerance_returns_the_unrefined_tile_solve():
    from hdsdp_amd import api
    c = second_difference_squared(257, False)
    x0, _ = bsp_solve(c)
    x, info, st = api.bsp_refined_solve(c.m, c.beg, c.idx, c.val, c.b, 3, 1e-6, 1e-6)
    report(case="tile stop", which="tolerance 1e-6", **{k: st[k] for k in ("status_name", "steps", "resid0", "resid", "tol")})
    assert info == 0 and (st["status"], st["steps"]) == (api.REFINE_CONVERGED, 0) and st["resid"] == st["resid0"] < st["tol"] == 1e-6
    assert same_bits(x, x0)


def test_timing_probe_runs_the_same_solves():
    """HMiBspRefineTimingProbe (tools/refine_tiles_timing.py) alternates HdmBsp::solve_host and the production refined solve on
    one factorisation: what it reports of the refined variant is what HMiBspRefinedSolve reports"""
    from hdsdp_amd import api
    c = second_difference_squared(257, False)
    _, _, st = accuracy_run(257, False)
    ms, corr, status, r0, r1, stats, work = api.bsp_refine_timing(c.m, c.beg, c.idx, c.val, c.b, [(-1, 0.0, 0.0), (3, SCHUR_REL, SCHUR_ABS)],
                                                                  warmup=1, reps=2)
    assert ms.shape == (2, 2) and np.all(ms > 0.0) and work > 0
    assert (status[0], corr[0]) == (api.REFINE_OFF, 0)
    assert (status[1], r0[1], r1[1]) == (st["status"], st["resid0"], st["resid"]) and corr[1] >= 2 * st["steps"]
    assert list(stats[:3]) == [st["block_rows"], st["tiles"], st["levels"]]


# ---------------------------------------------------------------- 3. quasi-definite

def test_quasi_definite_tile_matrix_is_refined_through_the_signed_factor():
    from hdsdp_amd import api
    c = sc.tile_case("band", 257, False, "qd", 1e6, "down")
    x0, nneg0 = bsp_solve(c)
    x, info, st = api.bsp_refined_solve(c.m, c.beg, c.idx, c.val, c.b, 3, SCHUR_REL, SCHUR_ABS)
    be0, be = sc.backward_error(c.A, x0, c.b), sc.backward_error(c.A, x, c.b)
    report(case="tile quasi-definite", m=c.m, negative=st["negative"], status=st["status_name"], steps=st["steps"], resid0=st["resid0"],
           resid=st["resid"], backward_unrefined=be0, backward_refined=be)
    assert info == 0 and st["negative"] == nneg0 == int(np.sum(c.s < 0)) > 0
    assert st["status"] in (api.REFINE_CONVERGED, api.REFINE_STAGNATED, api.REFINE_MAXSTEPS), st
    assert st["resid"] <= st["resid0"] and be <= be0, (be, be0)


# ---------------------------------------------------------------- 4. and 5. the operator

class Arrow:
    """the arrow128 golden cones: a sparse operator that takes the tile form"""

    def __enter__(self):
        from hdsdp_amd import api
        g = load_golden("arrow128_A")
        self.m = int(g["mb_dims"][1])
        Rd, tau, y = float(g["Rd"][0]), float(g["tau"][0]), y_of(g)
        prob = api.read_sdpa(os.path.join(ROOT, "tests", "golden", "arrow128.dat-s"))
        self.cones = [api.SDPCone.from_csc(blk["n"], self.m, blk["beg"], blk["idx"], blk["val"], iCone=k) for k, blk in enumerate(prob["blocks"])]
        for cn in self.cones:
            cn.set_start(Rd)
            assert cn.check_is_interior(tau, y)
        self.b = np.sin(np.arange(self.m) + 1.0)
        return self

    def __exit__(self, *exc):
        for cn in self.cones:
            cn.destroy()

    def factorised(self, mirror, cap, switch):
        """a fresh operator: built, shifted (mirror on: through kktDiag, as the driver's bound cone does), regularised, factorised.
        Returns (kkt, A): A = the matrix that was factorised"""
        from hdsdp_amd import api
        kkt = api.KKT(self.m, self.cones)
        try:
            assert kkt.is_sparse and kkt.tile_info() is not None
            if not mirror:
                kkt.set_host_mirror(False)
            assert kkt.diag_target() == (0 if mirror else 1)
            kkt.set_refine(cap)
            kkt.set_refine_tiles(switch)
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
            if mirror:
                kkt.add_to_diag(1e-3 * float(np.max(np.diag(full(kkt.M)))))
            kkt.regularize(1e-3)
            kkt.factorize()
            A = full(kkt.M) if mirror else kkt.rows(np.arange(self.m))
            return kkt, np.ascontiguousarray(xp.sym(A))
        except BaseException:
            kkt.destroy()
            raise


@pytest.mark.parametrize("mirror", [True, False], ids=["mirror-on", "mirror-off"])
def test_tile_operator_refines_from_the_right_matrix(mirror):
    from hdsdp_amd import api
    label = "tiles, mirror " + ("on" if mirror else "off")
    with Arrow() as ar:
        plain, _ = ar.factorised(mirror, 0, False)
        try:
            x0 = plain.solve(ar.b)
            assert plain.refine_stats()["device_bytes"] == 0
        finally:
            plain.destroy()
        kkt, A = ar.factorised(mirror, 2, True)
        try:
            assert kkt.tile_info() is not None and kkt.refine_tiles()
            x = kkt.solve(ar.b)
            st = kkt.refine_stats()
            xin = kkt.solve(ar.b.copy(), inplace=True)
            truth = xp.solve(A, ar.b)
            assert st["cap"] == 2 and st["status"] in (api.REFINE_CONVERGED, api.REFINE_STAGNATED, api.REFINE_MAXSTEPS), (label, st)
            assert st["device_bytes"] > 0 and st["tol"] == SCHUR_ABS, (label, st)
            # a residual from any matrix but the factorised one (without the shift, the channel or the regularisation) would be
            # off by that term times x
            assert st["resid0"] < 1e-12, (label, st)
            assert same_bits(x, xin), "in place differs from out of place"
            forced = forced_steps(kkt, A, ar.b, truth, label, False)
            kkt.set_param(relTol=SCHUR_REL, absTol=SCHUR_ABS)
            bytes_on = kkt.refine_stats()["device_bytes"]
            # the copy of the factor store exists only with the mirror on: ntiles tiles of 128 x 128 doubles
            assert (bytes_on >= kkt.tile_info()[0] * 131072) == mirror, (label, bytes_on)
        finally:
            kkt.destroy()
    e, e0 = err(x, truth), err(x0, truth)
    e_model = err(host_model(A, ar.b, st["steps"]), truth)
    report(case="tile operator", form=label, m=ar.m, status=st["status_name"], steps=st["steps"], resid0=st["resid0"], resid=st["resid"],
           tol=st["tol"], e_unrefined=e0, e_refined=e, e_model=e_model, cond=float(np.linalg.cond(A)), device_bytes=bytes_on)
    assert within(e, e_model), (label, e, e_model)
    assert e <= 2.0 * e0 + 16.0 * U and forced <= 2.0 * e0 + 16.0 * U, (label, e, forced, e0)


def test_tile_source_validity_and_the_switches():
    from hdsdp_amd import api
    with Arrow() as ar:
        # mirror off: a new build zeroes the accumulation store -- NO_MATRIX and the old factor's unrefined solve
        kkt, _ = ar.factorised(False, 2, True)
        try:
            kkt.solve(ar.b)
            assert kkt.refine_stats()["status"] in (api.REFINE_CONVERGED, api.REFINE_STAGNATED, api.REFINE_MAXSTEPS)
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
            xn = kkt.solve(ar.b)
            sn = kkt.refine_stats()
            kkt.set_refine(0)
            x0 = kkt.solve(ar.b)
            s0 = kkt.refine_stats()
            assert sn["status"] == api.REFINE_NO_MATRIX and sn["steps"] == 0 and same_bits(xn, x0), sn
            assert (s0["cap"], s0["status"], s0["device_bytes"]) == (0, api.REFINE_OFF, 0), s0
        finally:
            kkt.destroy()
        for mirror in (True, False):
            # the switch without the cap: OFF, nothing held, the unrefined bits
            kkt, _ = ar.factorised(mirror, 0, True)
            try:
                xs = kkt.solve(ar.b)
                ss = kkt.refine_stats()
                assert kkt.refine_tiles() and (ss["cap"], ss["status"], ss["device_bytes"]) == (0, api.REFINE_OFF, 0), (mirror, ss)
            finally:
                kkt.destroy()
            # both on, used, then the switch off: everything is freed and the solve is the unrefined one again
            kkt, _ = ar.factorised(mirror, 2, True)
            try:
                kkt.solve(ar.b)
                assert kkt.refine_stats()["device_bytes"] > 0
                kkt.set_refine_tiles(False)
                xo = kkt.solve(ar.b)
                so = kkt.refine_stats()
                assert not kkt.refine_tiles() and (so["cap"], so["status"], so["device_bytes"]) == (2, api.REFINE_NOT_AVAILABLE, 0), (mirror, so)
                assert same_bits(xo, xs), mirror
            finally:
                kkt.destroy()


# ---------------------------------------------------------------- 6. the environment

def worker(**env):
    r = subprocess.run([sys.executable, os.path.join(HERE, "refine_tiles_worker.py")], capture_output=True, text=True,
                       env=dict({k: v for k, v in os.environ.items() if k not in ("HDSDP_MI355X_REFINE", "HDSDP_MI355X_REFINE_TILES")}, **env),
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("REFINE_TILES_WORKER_JSON ")]
    assert line, r.stdout[-2000:]
    return json.loads(line[0][len("REFINE_TILES_WORKER_JSON "):]), r.stderr


def test_the_environment_switches_refine_a_tile_operator():
    from hdsdp_amd import api
    out, stderr = worker(HDSDP_MI355X_REFINE="2", HDSDP_MI355X_REFINE_TILES="1")
    assert out["tile_form"] and out["switch"] and out["before"]["cap"] == 2
    assert out["after"]["status"] in (api.REFINE_CONVERGED, api.REFINE_STAGNATED, api.REFINE_MAXSTEPS) and out["after"]["solves"] == 1, out
    assert out["after"]["device_bytes"] > 0 and out["after"]["resid0"] < 1e-12
    assert "HDSDP_MI355X_REFINE=2" in stderr and "HDSDP_MI355X_REFINE_TILES=1" in stderr
    assert out["residual"] <= 1e-12 * out["cond"], out


def test_the_step_cap_alone_leaves_a_tile_operator_not_available():
    from hdsdp_amd import api
    out, stderr = worker(HDSDP_MI355X_REFINE="2")
    assert out["tile_form"] and not out["switch"] and out["before"]["cap"] == 2
    assert (out["after"]["status"], out["after"]["device_bytes"], out["after"]["solves"]) == (api.REFINE_NOT_AVAILABLE, 0, 0), out
    assert "HDSDP_MI355X_REFINE_TILES" not in stderr
