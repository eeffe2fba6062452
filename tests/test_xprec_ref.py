"""The extended-precision reference of tests/xprec_ref.py, checked on the host (no GPU): its products against plain longdouble
arithmetic, its Schur quantities against the plain-C oracle where fp64 is accurate, and its inverse's own residual where
it is not (cond(S) = 1e10)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)
import line_search_model as lm  # noqa: E402
import xprec_ref as xp  # noqa: E402

pytestmark = pytest.mark.skipif(not xp.HAVE_LD, reason=xp.NO_LD_REASON)

LD = xp.LD


def _err(x, ref):
    x, ref = np.asarray(x, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("p,k,q", [(5, 1, 3), (17, 33, 9), (40, 300, 7), (3, 2049, 4)])
def test_products_are_longdouble_accurate(p, k, q):
    """mm of fp64 and longdouble operands against longdouble matmul, entries spread over 30 binades: within 1e-18 of the row
    maximum of A times the column maximum of B, per term of the inner dimension"""
    rng = np.random.default_rng(p * k + q)
    A = rng.standard_normal((p, k)) * np.exp2(rng.integers(-15, 15, (p, k)))
    B = rng.standard_normal((k, q)) * np.exp2(rng.integers(-15, 15, (k, q)))
    scale = LD(k) * np.max(np.abs(A), axis=1)[:, None].astype(LD) * np.max(np.abs(B), axis=0)[None, :].astype(LD)
    ref = A.astype(LD) @ B.astype(LD)
    assert np.max(np.abs(xp.mm(A, B) - ref) / scale) <= 1e-18
    Bl = B.astype(LD) * (1 + LD(rng.standard_normal()) * LD(2.0) ** -60)   # a longdouble operand with a live tail
    assert np.max(np.abs(xp.mm(A, Bl) - A.astype(LD) @ Bl) / scale) <= 1e-18


def _state(n, m, kind, seed, cond=10.0):
    """S* = Q diag(geometric 1 .. 1/cond) Q^T, C = S* + sum y A_i + Rd I; returns (csc, C, family, y, Rd, S*)"""
    rng = np.random.default_rng(seed)
    Q = lm.householder_q(rng, n, 8)
    Sst = xp.sym((Q * np.geomspace(1.0, 1.0 / cond, n)) @ Q.T)
    if kind == "dense":
        A = np.stack([lm.random_sym(rng, n) / np.sqrt(n) for _ in range(m)])
        fam = ("dense", A)
    elif kind == "r1":
        a = rng.choice([-1.0, 1.0], (m, n)) * np.exp2(-rng.integers(0, 4, (m, n)))
        s = rng.choice([-1.0, 1.0], m)
        A = np.stack([s[i] * np.outer(a[i], a[i]) for i in range(m)])
        fam = ("r1", a, s)
    else:
        ents = []
        for i in range(m):
            r = rng.integers(0, n, 3)
            c = rng.integers(0, n, 3)
            ents.append(sorted({(max(x, z), min(x, z)): rng.uniform(0.5, 1.5) for x, z in zip(r, c)}.items()))
        A = np.zeros((m, n, n))
        for i, e in enumerate(ents):
            for (r, c), v in e:
                A[i, r, c] = A[i, c, r] = v
        fam = xp.family_from_sparse(n, m, [[(r, c, v) for (r, c), v in e] for e in ents])
    y = 0.1 * rng.standard_normal(m) / max(1.0, float(np.max(np.abs(A))))
    Rd = -0.25
    C = Sst + np.tensordot(y, A, axes=1) + Rd * np.eye(n)
    return lm.to_csc([C] + list(A)), C, fam, y, Rd


def _tri(d, key):
    """the valid triangle of the Schur matrix (column-major lower == C-order upper), any other quantity as it is"""
    v = np.asarray(d[key])
    return v[np.triu_indices(v.shape[0])] if key == "M" else v


def _bar(key):
    """2e-15 relative for the vectors and M; the scalars are single sums with cancellation (tr(C S^-1) of an indefinite C):
    fp64 keeps about 1e-15 of their terms' size, up to 1e-14 of the sum here"""
    return 2e-15 if key in ("M", "ASinv", "ASinvRdSinv", "ASinvCSinv") else 1e-14


def _ld_cholesky_logdet(S):
    """log det S from a plain longdouble Cholesky (right-looking, O(n^3) in numpy longdouble: small n only)"""
    A = np.array(S, dtype=LD)
    n = A.shape[0]
    out = LD(0.0)
    for j in range(n):
        d = np.sqrt(A[j, j])
        out += LD(2.0) * np.log(d)
        c = A[j + 1:, j] / d
        A[j + 1:, j + 1:] -= np.outer(c, c)
    return out


@pytest.mark.parametrize("kind,n,m", [("dense", 24, 6), ("r1", 30, 12), ("sparse", 40, 15)])
def test_schur_quantities_match_the_oracle_at_well_conditioned_states(kind, n, m):
    """at cond(S) = 10 the oracle's fp64 is within a few units of rounding of the truth: the two agree to about 1e-15"""
    import oracle_py
    (beg, idx, val), C, fam, y, Rd = _state(n, m, kind, seed=n + m)
    blk = oracle_py.Block(n, m, beg, idx, val)
    try:
        S = lm.dev_lower(blk.assemble_S(1.0, y, Rd))
        K = xp.inverse(S)
        Lf, info = blk.factor(S)
        assert info == 0
        Sinv = blk.inverse(Lf)
        for t in (0, 1, 2):
            ref = blk.kkt_build(Sinv, Rd, t)
            tru = xp.schur(K, C, Rd, fam, t)
            for key, v in tru.items():
                assert _err(_tri(ref, key), _tri(tru, key)) <= _bar(key), (kind, t, key, _err(_tri(ref, key), _tri(tru, key)))
        ref = blk.kkt_build(S, Rd, 3)                      # KKT_TYPE_PRIMAL with X := S
        tru = xp.schur(S.astype(LD), C, Rd, fam, 3)
        for key, v in tru.items():
            assert _err(_tri(ref, key), _tri(tru, key)) <= _bar(key), (kind, 3, key, _err(_tri(ref, key), _tri(tru, key)))
    finally:
        blk.close()


@pytest.mark.parametrize("n", [7, 129, 256])
def test_inverse_residual_at_cond_1e10(n):
    """the longdouble inverse at cond(S) = 1e10 has residual |S X - I| <= 1e-17 cond (fp64's own is about 1e-16 cond);
    the refined solve is held to the same bar, the log-determinant to eps_ld cond absolute against a plain longdouble
    Cholesky"""
    rng = np.random.default_rng(n)
    Q = lm.householder_q(rng, n, 8)
    cond = 1e10
    lam = np.geomspace(1.0, 1.0 / cond, n)
    S = xp.sym((Q * lam) @ Q.T)
    X = xp.inverse(S)
    assert xp.inverse_residual_max(S, X) <= 1e-17 * cond
    b = rng.standard_normal(n)
    x = xp.solve(S, b)
    assert _err(x, X @ b.astype(LD)) <= 1e-17 * cond
    # (the GPU tests hold log-determinants to differences of 1e-9 absolute and more at cond 1e10: the truth is checked well below)
    assert abs(float(xp.logdet(S) - _ld_cholesky_logdet(S))) <= xp.EPS_LD * cond
