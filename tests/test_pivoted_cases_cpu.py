"""The matrices of tests/pivoted_cases.py are what tests/test_gpu_pivoted.py needs them to be, and its reference deserves to be
one: every family at every size is symmetric bit for bit, not positive definite, conditioned as stated, makes the pivot search
do what the family is for (on the first-maximum model of the elimination), and dgetrf / dgetrs solves it to a backward error of
at most 64 u -- the condition under which `e(gpu) <= 8 e(dgetrs) + 16 u` cannot hide a wrong factorisation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pivoted_cases as pc  # noqa: E402
import xprec_ref as xp  # noqa: E402

needs_ld = pytest.mark.skipif(not xp.HAVE_LD, reason=xp.NO_LD_REASON)
CASES = [(f, n) for n in pc.SIZES for f in pc.families_at(n)]


def test_every_size_has_its_families():
    assert pc.families_at(1) == ("one",) and pc.matrix("one", 1)[0, 0] < 0          # the 1 x 1 negative matrix
    assert pc.families_at(2) == ("antidiag", "ties", "tinydiag", "graded")
    for n in pc.SIZES[2:]:
        assert pc.families_at(n) == pc.FAMILIES


@pytest.mark.parametrize("n", pc.SIZES)
def test_families_are_symmetric_and_not_positive_definite(n):
    for f in pc.families_at(n):
        A = pc.matrix(f, n)
        assert A.shape == (n, n) and A.dtype == np.float64 and np.all(np.isfinite(A)), f
        assert np.array_equal(A, A.T), f                                             # bit for bit
        assert np.array_equal(A, pc.matrix(f, n)), f                                 # the same bits every time
        if f == "graded":       # D G D: G has the other families' spectrum, and v' G v < 0 gives (D^-1 v)' A (D^-1 v) < 0
            G, d = pc.graded_parts(n)
            assert np.array_equal(A, pc.from_lower((d[:, None] * np.tril(G)) * d[None, :]))
            assert d.max() == 1.0 and abs(d.min() - 1e-6) <= 1e-20 and pc.spectrum_ok(G)
            x = (np.linalg.eigh(G)[1][:, 0] / d).astype(pc.LD)
            assert float(x @ (A.astype(pc.LD) @ x)) < 0
            continue
        w = np.linalg.eigvalsh(A)
        assert w[0] < 0 and np.min(np.abs(w)) > 0, (f, w[0])
        assert np.max(np.abs(w)) / np.min(np.abs(w)) <= pc.COND_MAX * (1 + 1e-9), f
        if f == "saddle":
            q = n // 3
            assert not A[n - q:, n - q:].any() and np.linalg.eigvalsh(A[:n - q, :n - q])[0] > 0
        if f == "antidiag":
            assert not np.diag(A)[np.arange(n) != n - 1 - np.arange(n)].any()
        if f == "ties":
            assert set(np.unique(A)) <= {-1.0, 0.0, 1.0}
        if f == "tinydiag":
            assert 0 < np.max(np.abs(np.diag(A))) <= 1e-18


@pytest.mark.parametrize("n", [n for n in pc.SIZES if n >= 2])
def test_antidiag_pivots_come_from_the_far_end(n):
    """on the first-maximum model the pivot of column j < n/2 is row n-1-j; from n = 65 on some panel takes all its 32 pivots
    from distinct rows outside itself; dgetrf picks the same rows"""
    A = pc.matrix("antidiag", n)
    piv = pc.first_max_pivots(A)
    j = np.arange(n // 2)
    assert np.array_equal(piv[: n // 2], n - 1 - j)
    if n >= 65:
        assert max(pc.far_rows_per_panel(piv)) == 32
    assert np.array_equal(piv, pc.dgetrs(A, np.ones(n))[1])


@pytest.mark.parametrize("n", [n for n in pc.SIZES if 31 <= n <= 129])
def test_families_make_the_pivot_search_matter(n):
    """elimination without row exchanges would be wrong or impossible: on the model some pivot is not the diagonal, in the
    first panel already; in `ties` the chosen maximum is attained by several rows at some column of the first panel"""
    for f in pc.families_at(n):
        A = pc.matrix(f, n)
        piv = pc.first_max_pivots(A)
        assert np.any(piv[:32] != np.arange(n)[:32]), f
    col = np.abs(pc.matrix("ties", n)[:, 0])
    assert np.sum(col == col.max()) >= 2


@needs_ld
@pytest.mark.parametrize("family,n", CASES, ids=[f"{f}-{n}" for f, n in CASES])
def test_dgetrs_is_a_reference_worth_the_name(family, n):
    _, _, e_getrs, e_sytrs = pc.case(family, n)
    assert np.all(e_getrs <= pc.CAP), (family, n, e_getrs / pc.U)
    assert np.all(np.isfinite(e_sytrs))


@needs_ld
@pytest.mark.parametrize("n", [33, 64, 129, pc.LARGE_N])
def test_dgetrs_on_the_uniform_matrices(n):
    """the good matrix of the singular-matrix tests, and the one large case"""
    A, B, e_getrs, _ = pc.case("uniform", n)
    assert np.array_equal(A, A.T) and A[0, 0] == -1.0
    assert B.shape == ((2 if n == pc.LARGE_N else pc.NRHS), n)
    assert np.all(e_getrs <= pc.CAP), (n, e_getrs / pc.U)


@needs_ld
@pytest.mark.parametrize("n", [33, 200])
def test_dgetrs_on_the_positive_definite_matrices(n):
    S = pc.spd(n)
    assert np.array_equal(S, S.T) and np.linalg.eigvalsh(S)[0] > 0.5
    B = pc.rhs("spd", n)
    assert np.all(pc.backward_errors(S, pc.dgetrs(S, B)[0], B) <= pc.CAP)


@pytest.mark.parametrize("n", [1, 33, 64, 129])
def test_singular_matrices_are_singular_without_a_nan(n):
    for z in ([None, 0] if n == 1 else [None, 0, 31, 32, n - 1]):
        Z = pc.singular(n, z)
        assert np.array_equal(Z, Z.T) and np.all(np.isfinite(Z))
        assert not Z[z if z is not None else 0].any()
        if z is not None and n > 1:
            assert np.linalg.matrix_rank(Z) == n - 1


def test_the_rule_and_the_model():
    assert pc.within(16 * pc.U, 0.0) and not pc.within(17 * pc.U, 0.0)
    assert pc.within(8e-15 + 16 * pc.U, 1e-15) and not pc.within(8.1e-15 + 16 * pc.U, 1e-15)
    A = np.array([[1.0, 2.0, 0.0], [-2.0, 1.0, 1.0], [2.0, 0.0, 1.0]])               # a tie in column 0: the first row wins
    assert list(pc.first_max_pivots(A)) == [1, 1, 2]
    assert pc.far_rows_per_panel(np.array([3, 2, 2, 3]), nb=2) == [2, 0]


def test_the_recorded_report_covers_every_case_and_keeps_the_rule():
    """tests/golden/pivoted_report.txt: the PIVOT_REPORT lines of one run of tests/test_gpu_pivoted.py on an MI355X -- a line for
    every (family, size), the large case and the switched operators, each within the rule it was recorded under"""
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pivoted_report.txt")
    rows = [json.loads(line.split(" ", 1)[1]) for line in open(path) if line.startswith("PIVOT_REPORT ")]
    seen = {(r["what"], r["n"]) for r in rows}
    assert set(CASES) | {("uniform", pc.LARGE_N), ("chain operator switched", 408), ("operator switched at solve time", 64),
                         ("spd switched at solve time", 33), ("spd switched at solve time", 200)} <= seen
    for r in rows:
        assert r["e_dgetrs_u"] <= 64.0 and r["e_gpu_u"] <= 8.0 * r["e_dgetrs_u"] + 16.0, r
        assert 0.0 <= r["ratio_dgetrs"] <= 8.0 + 1.0 and r["ratio_dsytrs"] >= 0.0, r       # (e / max(e_ref, 16 u) <= 8 + 1 under the rule)
