"""The Schur system's pivoted way out (csrc/lu.hip behind lin_factor_indef / lin_switch_indefinite) where the pivot choice, the
row exchanges and the switch itself matter: matrices on which the right pivot is far away, tied or the only usable one
(tests/pivoted_cases.py), a size on each side of every boundary of the kernels (32, 64, 128, 256 trailing columns, 512, 1024,
and the solve's 48 KiB of LDS), 1 / 2 / 3 / 5 right-hand sides and the in-place form, singular matrices and what the object does
after one, the switch at solve time (HFpLinsysSolve on a NaN), and a CSC-form operator switched with and without its RCM order.

Every solution is held to the rule of test_gpu_conditioning.py on the normwise backward error (residual in longdouble),

    e(gpu) <= 8 e(dgetrs) + 16 u            (u = 2^-53)

with dgetrf / dgetrs on the same matrix and right-hand sides: the same algorithm and pivot rule.  e(dgetrs) itself is at most
64 u on everything used here (tests/test_pivoted_cases_cpu.py; asserted again where the matrix is the engine's own).  Lines
starting PIVOT_REPORT give e(gpu) and its ratios to dgetrs' and to dsytrs' (the pair the reference calls; nothing is asserted
against it); `pytest -s` shows them, tests/golden/pivoted_report.txt keeps those of one run on an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pivoted_cases as pc  # noqa: E402
import xprec_ref as xp  # noqa: E402
from chain_operator import CHAIN_M, banded_chain  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xp.HAVE_LD, reason=xp.NO_LD_REASON)]


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def full(Mh):
    """KKT.M (C-order view of the column-major matrix, upper triangle valid) as the full symmetric matrix"""
    return np.triu(Mh) + np.triu(Mh, 1).T


class Rule:
    """collects every solve of one test: e(gpu) against e(dgetrs) on the same data; the worst of each for the report"""

    def __init__(self):
        self.bad, self.e_gpu, self.e_getrs, self.e_sytrs = [], 0.0, 0.0, 0.0

    def hold(self, what, A, X, B, e_getrs=None, e_sytrs=None):
        X, B = np.atleast_2d(X), np.atleast_2d(B)
        if e_getrs is None:
            e_getrs, e_sytrs = pc.lapack_errors(A, B)
            if not np.all(e_getrs <= pc.CAP):
                self.bad.append(f"{what}: dgetrs itself at {np.max(e_getrs) / pc.U:.1f} u, above the cap of 64 u")
        if not np.all(np.isfinite(X)):
            self.bad.append(f"{what}: solution not finite")
            return
        e = float(np.max(pc.backward_errors(A, X, B)))
        ref = float(np.max(e_getrs[:X.shape[0]]))
        print(f"    {what}: e(gpu) = {e / pc.U:.2f} u, e(dgetrs) = {ref / pc.U:.2f} u")
        self.e_gpu, self.e_getrs = max(self.e_gpu, e), max(self.e_getrs, ref)
        self.e_sytrs = max(self.e_sytrs, float(np.max(e_sytrs[:X.shape[0]])))
        if not pc.within(e, ref):
            self.bad.append(f"{what}: {e / pc.U:.2f} u vs dgetrs {ref / pc.U:.2f} u")

    def report(self, what, n, note=""):
        pc.report(what, n, self.e_gpu, self.e_getrs, self.e_sytrs, note)
        self.e_gpu = self.e_getrs = self.e_sytrs = 0.0

    def check(self):
        assert not self.bad, "\n".join(self.bad)


def stderr_so_far(capfd):
    """what the library wrote to stderr since the last call; the test's own stdout lines go back where they were"""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    return cap.err


def solve_in_place(ls, b):
    """solVec == NULL, as the reference's driver calls it"""
    from hdsdp_amd import api
    x = np.array(b, dtype=np.float64)
    assert api.load_library().HFpLinsysSolve(ls._h, 1, dptr(x), None) == 0
    return x


# ---------------------------------------------------------------- every family at every size

@pytest.mark.parametrize("n", pc.SIZES)
def test_every_family_on_each_side_of_every_boundary(n):
    """saddle / antidiag / ties / tinydiag / graded (the 1 x 1 negative matrix at n = 1): the object switches on numeric; 1, 2, 3
    and 5 right-hand sides (solve_host works in chunks of two) and the in-place form under the rule; then, bit for bit: a row
    of a stacked solve is the single solve of that row, in place is out of place, a second numeric gives the same solution, and
    (n <= 129) so does the system scaled by 2^-500 or 2^+500 -- the engine holds no absolute threshold"""
    from hdsdp_amd import api
    rule = Rule()
    for f in pc.families_at(n):
        A, B, e_getrs, e_sytrs = pc.case(f, n)
        ls = api.LinSys(n, api.HDSDP_LINSYS_DENSE_ITERATIVE)
        try:
            ls.numeric(np.triu(A))                                   # column-major lower == C-order upper
            assert ls.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE, f
            X = {k: ls.solve(B[:k] if k > 1 else B[0]).reshape(k, n) for k in (1, 2, 3, 5)}
            for k, Xk in X.items():
                rule.hold(f"{f} n={n} nrhs={k}", A, Xk, B[:k], e_getrs, e_sytrs)
            x = solve_in_place(ls, B[0])
            rule.hold(f"{f} n={n} in place", A, x, B[0], e_getrs, e_sytrs)
            for k in (1, 2, 3):
                assert np.array_equal(X[k], X[5][:k]), (f, "stack of", k)
            for r in range(1, 5):
                assert np.array_equal(ls.solve(B[r]), X[5][r]), (f, "row", r)
            assert np.array_equal(x, X[5][0]), (f, "in place")
            ls.numeric(np.triu(A))
            assert np.array_equal(ls.solve(B), X[5]), (f, "second numeric")
            if n <= 129:
                for s in (2.0 ** -500, 2.0 ** 500):
                    ls.numeric(np.triu(A) * s)
                    assert np.array_equal(ls.solve(B * s), X[5]), (f, "scaled by", s)
        finally:
            ls.destroy()
        rule.report(f, n)
    rule.check()


# ---------------------------------------------------------------- one large case

def test_a_solve_above_48_kib_of_lds_and_a_small_one_after_it():
    """n = 6176: the solve keeps 49 408 bytes of the vector in LDS, so HdmLu::init raises the kernel's dynamic limit (and npad =
    6272 differs from roundup(n, 32)); uniform with A[0,0] = -1, two right-hand sides.  Then, in the same process, a fresh
    object of order 33: the raised limit must not break the small launch."""
    from hdsdp_amd import api
    rule = Rule()
    for f, n in (("uniform", pc.LARGE_N), ("saddle", 33)):
        A, B, e_getrs, e_sytrs = pc.case(f, n)
        ls = api.LinSys(n, api.HDSDP_LINSYS_DENSE_ITERATIVE)
        try:
            ls.numeric(np.triu(A))
            assert ls.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
            rule.hold(f"{f} n={n}", A, ls.solve(B), B, e_getrs, e_sytrs)
        finally:
            ls.destroy()
        rule.report(f, n, "after the large case" if n == 33 else "lds limit raised")
    rule.check()


# ---------------------------------------------------------------- singular matrices and state

SINGULAR = [(1, 0)] + [(n, z) for n in (33, 64, 129) for z in (0, 31, 32, n - 1, None)]


@pytest.mark.parametrize("n,z", SINGULAR, ids=[f"{n}-{'all-zero' if z is None else 'zeroed-%d' % z}" for n, z in SINGULAR])
def test_a_singular_matrix_fails_and_leaves_no_stale_factor(n, z):
    """uniform with row and column z zeroed (or the zero matrix): numeric raises; the solve after it raises too, although the
    object held a good factor before; the next good matrix factors and solves within the rule, with the bits of before.  The
    same on a fresh object, where the failed Cholesky switches first."""
    from hdsdp_amd import api
    A, B, e_getrs, e_sytrs = pc.case("uniform" if n > 1 else "one", n)
    Z = pc.singular(n, z)
    rule = Rule()
    for fresh in (False, True):
        ls = api.LinSys(n, api.HDSDP_LINSYS_DENSE_ITERATIVE)
        try:
            if not fresh:
                ls.numeric(np.triu(A))
                X0 = ls.solve(B)
                rule.hold(f"n={n} before", A, X0, B, e_getrs, e_sytrs)
            with pytest.raises(api.HDSDPError):
                ls.numeric(np.triu(Z))
            assert ls.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
            with pytest.raises(api.HDSDPError):
                ls.solve(B[0])
            x = B[0].copy()
            assert api.load_library().HFpLinsysSolve(ls._h, 1, dptr(x), None) != 0
            ls.numeric(np.triu(A))
            X = ls.solve(B)
            rule.hold(f"n={n} after ({'fresh object' if fresh else 'same object'})", A, X, B, e_getrs, e_sytrs)
            assert np.array_equal(X, X0)
        finally:
            ls.destroy()
    rule.report("uniform after a singular matrix", n, "all-zero" if z is None else f"zeroed {z}")
    rule.check()


# ---------------------------------------------------------------- the switch at solve time

@pytest.mark.parametrize("n", [33, 200])
def test_a_nan_at_solve_time_switches_a_factored_system(n, capfd):
    """HFpLinsysSolve (hdsdp_linsolver.c:2085-2110): a right-hand side that starts with NaN fails, and the Schur system's object
    is switched -- the pivoted factorisation re-reads the matrix the Cholesky had succeeded on, from the caller's array (the
    object records the pointer, as the reference does with cg->fullMatElem: the array is kept alive here)"""
    from hdsdp_amd import api
    lib = api.load_library()
    S = pc.spd(n)
    kept = np.ascontiguousarray(np.triu(S))
    B = pc.rhs("spd", n)
    rule = Rule()
    ls = api.LinSys(n, api.HDSDP_LINSYS_DENSE_ITERATIVE)
    try:
        assert lib.HFpLinsysNumeric(ls._h, None, None, dptr(kept)) == 0
        assert ls.lin_type == api.HDSDP_LINSYS_DENSE_ITERATIVE
        rule.hold(f"n={n} Cholesky", S, ls.solve(B), B)
        assert np.all(ls.get_diag() > 0)
        stderr_so_far(capfd)
        poisoned = B[1].copy()
        poisoned[0] = np.nan
        with pytest.raises(api.HDSDPError):
            ls.solve(poisoned)
        assert ls.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
        assert "KKT system is unstable" in stderr_so_far(capfd)
        rule.hold(f"n={n} switched", S, ls.solve(B), B)
        rule.hold(f"n={n} switched, in place", S, solve_in_place(ls, B[2]), B[2])
        with pytest.raises(api.HDSDPError):
            ls.get_diag()
        assert np.array_equal(kept, np.triu(S))
    finally:
        ls.destroy()
    rule.report("spd switched at solve time", n)
    rule.check()


def test_a_nan_at_solve_time_switches_a_factored_operator(capfd):
    """the same through HKKTSolve, with the host mirror on (the pivoted factorisation reads the host matrix) and off (device M
    plus channel; no byte of M comes to the host): the switched operator gives the Cholesky's solution to 1e-12 cond(M), solves
    M x = b within the rule, and the next build + factorisation stays switched and solves its own M"""
    from hdsdp_amd import api
    n = m = 64
    cone = api.SDPCone.synthetic(n, m)
    rule = Rule()
    try:
        cone.set_start(-10.0 * n)
        assert cone.check_is_interior(1.0, np.zeros(m))
        b = cone.traces()
        A = None
        for mirror in (True, False):
            kkt = api.KKT(m, [cone], host_mirror=mirror)
            try:
                kkt.build_up(api.KKT_TYPE_INFEASIBLE)
                if mirror:
                    A = full(kkt.M.copy())                       # (mirror off: the same build, tests/test_gpu_device_m.py)
                    cond = np.linalg.cond(A)
                kkt.factorize()
                assert kkt.lin_type == api.HDSDP_LINSYS_DENSE_ITERATIVE
                x0 = kkt.solve(b)
                stderr_so_far(capfd)
                poisoned = b.copy()
                poisoned[0] = np.nan
                with pytest.raises(api.HDSDPError):
                    kkt.solve(poisoned)
                assert kkt.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
                assert "KKT system is unstable" in stderr_so_far(capfd)
                x = kkt.solve(b)
                assert np.linalg.norm(x - x0) <= 1e-12 * cond * np.linalg.norm(x0), mirror
                rule.hold(f"operator, mirror {mirror}, switched", A, x, b)
                kkt.build_up(api.KKT_TYPE_INFEASIBLE)
                kkt.factorize()
                assert kkt.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
                rule.hold(f"operator, mirror {mirror}, next build", full(kkt.M.copy()) if mirror else A, kkt.solve(b), b)
                if not mirror:
                    assert kkt.matrix_traffic()[0] == 0
            finally:
                kkt.destroy()
            rule.report("operator switched at solve time", m, f"mirror {'on' if mirror else 'off'}")
    finally:
        cone.destroy()
    rule.check()


# ---------------------------------------------------------------- CSC-form operators

@pytest.mark.parametrize("scrambled", [False, True], ids=["band-in-the-drivers-order", "band-after-reordering"])
def test_a_csc_form_operator_switches_and_stops_permuting(scrambled):
    """the chain of fifty blocks (a sparse pattern over a dense device matrix; scrambled: the factor object holds P M P' and
    lin_solve permutes right-hand sides): Cholesky first; then the diagonal lowered until M is indefinite -- the factorisation
    switches, the pivoted solver reads the unpermuted device matrix and the solve permutes nothing; then a positive definite
    build again, which stays switched"""
    from hdsdp_amd import api
    m = CHAIN_M
    cones = []
    rule = Rule()
    try:
        Mref = banded_chain(scrambled, cones)
        kkt = api.KKT(m, cones)
        try:
            assert kkt.is_sparse and kkt.tile_info() is None
            if os.environ.get("HDSDP_MI355X_KKT_ENVELOPE", "1") != "0" and os.environ.get("HDSDP_MI355X_KKT_RCM", "1") != "0":
                assert kkt.envelope_info()[0] == scrambled
            Aref = full(Mref)
            rhs = np.sin(np.arange(m) + 1.0)
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
            kkt.factorize()
            assert kkt.lin_type != api.HDSDP_LINSYS_DENSE_INDEFINITE
            x = kkt.solve(rhs)
            assert np.linalg.norm(x - np.linalg.solve(Aref, rhs)) <= 1e-10 * np.linalg.cond(Aref) * np.linalg.norm(rhs)
            rule.hold("chain, Cholesky", full(kkt.M), x, rhs)
            w = np.linalg.eigvalsh(Aref)
            kkt.add_to_diag(-0.5 * (w[0] + w[-1]))                  # eigenvalues now straddle zero
            A = full(kkt.M)
            w = np.linalg.eigvalsh(A)
            assert w[0] < 0 < w[-1]
            kkt.factorize()
            assert kkt.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
            rule.hold("chain, shifted and switched", A, kkt.solve(rhs), rhs)
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
            kkt.factorize()
            assert kkt.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
            A = full(kkt.M)
            assert np.linalg.eigvalsh(A)[0] > 0
            rule.hold("chain, next build", A, kkt.solve(rhs), rhs)
            rule.hold("chain, next build, in place", A, kkt.solve(rhs.copy(), inplace=True), rhs)
        finally:
            kkt.destroy()
    finally:
        for c in cones:
            c.destroy()
    rule.report("chain operator switched", m, "scrambled" if scrambled else "banded")
    rule.check()
