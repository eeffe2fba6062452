"""Matrices, right-hand sides and the comparison rule for the pivoted Schur fallback (csrc/lu.hip behind lin_factor_indef /
lin_switch_indefinite) -- plain numpy / scipy, importable without a GPU.

The rule is test_gpu_conditioning.py's, on the normwise backward error of xprec_ref.backward_error (residual in longdouble):
with e(x) the maximum over the right-hand sides and u = 2^-53,

    e(gpu) <= 8 e(LAPACK) + 16 u

where LAPACK is dgetrf / dgetrs on the same matrix and right-hand sides: the same algorithm with the same pivot rule (first
maximum of the column), so the two share their growth factor.  tests/test_pivoted_cases_cpu.py holds e(LAPACK) itself under
CAP = 64 u on everything generated here, so that the rule cannot hide a failure behind a bad reference.  dsytrf / dsytrs, the
pair the reference solver really calls, is evaluated beside it and reported, never asserted against.

Every family is symmetric bit for bit (mirrored from a lower triangle), nonsingular, and has a negative eigenvalue, so that a
DENSE_ITERATIVE object switches to the pivoted solver on its first numeric:

    saddle    [[H, B'], [B, 0]], H positive definite of order n - n//3, B Gaussian: no pivot on the zero block's diagonal
    antidiag  noise of size 0.05 with a zero diagonal, 4.0 added on the anti-diagonal: the pivot of column j is row n-1-j, so
              from n = 65 on a panel's 32 exchanges reach 32 distinct rows outside it (the swap map's full 64 entries)
    ties      entries from {-1, 0, 1}: every pivot search has many equal maxima
    tinydiag  uniform(-1, 1) with the diagonal scaled to 1e-18: catastrophic without pivoting
    graded    D G D, G uniform(-1, 1), D a randomly permuted geometric scale over 1e-6 (condition number up to about 1e12)
    one       the 1 x 1 matrix [-0.75]

Generators are seeded from (family, n): the CPU check and the GPU test see the same bits."""
import functools
import json
import zlib

import numpy as np
import scipy.linalg as sl

import xprec_ref as xp

U = 2.0 ** -53
CAP = 64.0 * U
LD = xp.LD

SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 287, 288, 289, 511, 512, 513, 545, 1023, 1024, 1025, 1057)
FAMILIES = ("saddle", "antidiag", "ties", "tinydiag", "graded")
MIN_N = {"saddle": 3, "antidiag": 2, "ties": 2, "tinydiag": 2, "graded": 2}
COND_MAX = 1e4          # of every family but graded (of G there)
LARGE_N = 6176          # roundup(n, 32) * 8 = 49 408 bytes of LDS for the solve: above the 48 KiB default limit
NRHS = 5


def within(e_gpu, e_ref):
    return e_gpu <= 8.0 * e_ref + 16.0 * U


def families_at(n):
    return ("one",) if n == 1 else tuple(f for f in FAMILIES if n >= MIN_N[f])


def _rng(tag, n, attempt=0):
    return np.random.default_rng([zlib.crc32(tag.encode()), n, attempt])


def from_lower(L):
    """the symmetric matrix with L's lower triangle: A == A.T bit for bit"""
    L = np.tril(L)
    return np.ascontiguousarray(L + np.tril(L, -1).T)


def spectrum_ok(A):
    """nonsingular to cond <= COND_MAX, and an eigenvalue of either sign (n >= 2)"""
    w = np.linalg.eigvalsh(A)
    a = np.abs(w)
    return a.min() > 0 and a.max() / a.min() <= COND_MAX and w[0] < 0 and (w[-1] > 0 or A.shape[0] == 1)


def _uniform_sym(rng, n):
    return from_lower(rng.uniform(-1.0, 1.0, (n, n)))


def _draw(family, n, rng):
    if family == "one":
        return np.array([[-0.75]])
    if family == "saddle":
        q = n // 3
        p = n - q
        W = rng.standard_normal((p, p))
        A = np.zeros((n, n))
        A[:p, :p] = np.eye(p) + (W @ W.T) / p
        A[p:, :p] = rng.standard_normal((q, p))         # (not scaled down: its entries compete with H's diagonal for the pivot)
        return from_lower(A)
    if family == "antidiag":
        A = np.tril(0.05 * rng.uniform(-1.0, 1.0, (n, n)), -1)
        i = np.arange(n)
        lo = i >= n - 1 - i
        A[i[lo], n - 1 - i[lo]] += 4.0
        return from_lower(A)
    if family == "ties":
        return from_lower(rng.integers(-1, 2, (n, n)).astype(np.float64))
    if family == "tinydiag":
        A = np.tril(rng.uniform(-1.0, 1.0, (n, n)), -1)
        A[np.arange(n), np.arange(n)] = 1e-18 * rng.uniform(-1.0, 1.0, n)
        return from_lower(A)
    if family == "uniform":
        A = _uniform_sym(rng, n)
        A[0, 0] = -1.0
        return A
    raise ValueError(family)


@functools.lru_cache(maxsize=None)
def graded_parts(n):
    """(G, d) of the graded matrix D G D: G uniform symmetric with the spectrum of the other families, d the scale"""
    for attempt in range(64):
        rng = _rng("graded", n, attempt)
        G = _uniform_sym(rng, n)
        if spectrum_ok(G):
            return G, rng.permutation(np.geomspace(1.0, 1e-6, n))
    raise RuntimeError(f"no graded matrix of order {n} in 64 draws")


@functools.lru_cache(maxsize=None)
def _matrix(family, n):
    if family == "graded":                      # same inertia as G
        G, d = graded_parts(n)
        return from_lower((d[:, None] * np.tril(G)) * d[None, :])
    if family == "uniform" and n >= 2048:       # the large case: no eigenvalues taken (A[0,0] < 0 makes it not positive definite)
        return _draw(family, n, _rng(family, n))
    for attempt in range(64):                   # (deterministic: the first draw of the seeded sequence that has the properties)
        rng = _rng(family, n, attempt)
        A = _draw(family, n, rng)
        if spectrum_ok(A):
            return A
    raise RuntimeError(f"no {family} matrix of order {n} with the required spectrum in 64 draws")


def matrix(family, n):
    """the family's matrix of order n (a fresh copy: callers may scale or zero it)"""
    return _matrix(family, n).copy()


def rhs(family, n, k=NRHS):
    """k right-hand sides as the rows of a C-order (k, n) array (== column-major n x k, what HFpLinsysSolve takes)"""
    return _rng("rhs " + family, n).standard_normal((k, n))


def spd(n):
    """a positive definite matrix (cond about 1e2) for the solve-time switch: its Cholesky succeeds"""
    W = _rng("spd", n).standard_normal((n, n))
    return from_lower(np.eye(n) + (W @ W.T) * (10.0 / n))


def singular(n, z):
    """uniform with row and column z zeroed (z = None: the all-zero matrix).  No NaN or Inf anywhere."""
    if z is None:
        return np.zeros((n, n))
    A = matrix("uniform", n) if n > 1 else np.zeros((1, 1))
    A[z, :] = 0.0
    A[:, z] = 0.0
    return A


# ---------------------------------------------------------------- the references

def backward_errors(A, X, B):
    """per right-hand side; X, B: (k, n) or (n,)"""
    X, B = np.atleast_2d(X), np.atleast_2d(B)
    return np.asarray(xp.backward_error(A, X.T, B.T), dtype=np.float64)


def dgetrs(A, B):
    """scipy.linalg.lu_factor / lu_solve: (solutions as rows, dgetrf's zero-based piv)"""
    lu, piv = sl.lu_factor(A, check_finite=False)
    return sl.lu_solve((lu, piv), np.atleast_2d(B).T, check_finite=False).T, piv


def dsytrs(A, B):
    """dsytrf / dsytrs, the reference solver's own pair (hdsdp_linsolver.c:1706-1780)"""
    lwork, info = sl.lapack.dsytrf_lwork(A.shape[0], lower=1)      # (the default is the unblocked factorisation)
    assert info == 0, info
    ldu, ipiv, info = sl.lapack.dsytrf(A, lower=1, lwork=int(lwork))
    assert info == 0, info
    x, info = sl.lapack.dsytrs(ldu, ipiv, np.asfortranarray(np.atleast_2d(B).T), lower=1)
    assert info == 0, info
    return x.T


def lapack_errors(A, B):
    """(e(dgetrs), e(dsytrs)) per right-hand side"""
    return backward_errors(A, dgetrs(A, B)[0], B), backward_errors(A, dsytrs(A, B), B)


@functools.lru_cache(maxsize=None)
def case(family, n):
    """(A, B, e(dgetrs) per right-hand side, e(dsytrs) per right-hand side); computed once, shared, not to be written to"""
    A, B = _matrix(family, n), rhs(family, n, 2 if n >= 2048 else NRHS)
    eg, es = lapack_errors(A, B)
    for a in (A, B, eg, es):
        a.setflags(write=False)
    return A, B, eg, es


def first_max_pivots(A):
    """zero-based pivot rows of unblocked partial-pivot elimination taking the FIRST maximum of each column (idamax): the rule
    of dgetrf and of hdm_lu_panel_kernel"""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    piv = np.arange(n)
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        piv[j] = p
        if p != j:
            A[[j, p], :] = A[[p, j], :]
        if A[j, j] != 0.0 and j + 1 < n:
            A[j + 1:, j] *= 1.0 / A[j, j]
            A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j, j + 1:])
    return piv


def far_rows_per_panel(piv, nb=32):
    """for each nb-wide panel, the number of distinct pivot rows behind the panel's own rows"""
    n = len(piv)
    return [len({int(p) for p in piv[j0:j0 + nb] if p >= j0 + nb}) for j0 in range(0, n, nb)]


def report(what, n, e_gpu, e_getrs, e_sytrs, note=""):
    """PIVOT_REPORT {json}: the three backward errors in units of u, and e(gpu)'s ratios to dgetrs' and dsytrs' (each floored
    at 16 u, as COND_REPORT's are)"""
    e_gpu, e_getrs, e_sytrs = float(e_gpu), float(e_getrs), float(e_sytrs)
    print("PIVOT_REPORT " + json.dumps(dict(
        what=what, n=int(n), note=note, e_gpu_u=round(e_gpu / U, 3), e_dgetrs_u=round(e_getrs / U, 3), e_dsytrs_u=round(e_sytrs / U, 3),
        ratio_dgetrs=round(e_gpu / max(e_getrs, 16.0 * U), 4), ratio_dsytrs=round(e_gpu / max(e_sytrs, 16.0 * U), 4))))
