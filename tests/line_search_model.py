"""Plain fp64 model of the dual-matrix quantities the line search asks the engine for, from the dense data itself:

    T(tau, y, eye) = tau C - sum_i y_i A_i + eye I          (the device's S = T(tau, y, -Rd + perturb))
    log det T                                               (Cholesky)
    alpha*(S, dS) = 1 / lambda_max(L^-1 (-dS) L^-T)         (S = L L^T; inf when that eigenvalue is <= 0)

No engine and no oracle code is involved: tests/test_line_search_model.py pins these helpers to oracle/oracle_py.py on the
CPU, and tests/test_gpu_line_search.py then holds the device to them."""
import numpy as np


def pack_lower(A):
    """n x n symmetric -> packed lower triangle, column by column (the CSC row numbering of interface/def_hdsdp_user_data.h)"""
    n = A.shape[0]
    return np.concatenate([A[j:, j] for j in range(n)])


def unpack_lower(pk, n):
    A = np.zeros((n, n))
    k = 0
    for j in range(n):
        A[j:, j] = pk[k:k + n - j]
        k += n - j
    return A + np.tril(A, -1).T


def to_csc(mats):
    """[C, A_1, ..., A_m] (dense symmetric) -> (beg, idx, val) of the n(n+1)/2 x (m+1) CSC; exact zeros are left out"""
    beg, idx, val = [0], [], []
    for A in mats:
        pk = pack_lower(A)
        nz = np.nonzero(pk)[0]
        idx.append(nz.astype(np.int32))
        val.append(pk[nz])
        beg.append(beg[-1] + nz.size)
    return (np.asarray(beg, dtype=np.int32), np.concatenate(idx).astype(np.int32), np.concatenate(val))


def from_csc(n, m, beg, idx, val):
    """the CSC back to dense (C, A stack m x n x n)"""
    P = n * (n + 1) // 2
    mats = []
    for col in range(m + 1):
        pk = np.zeros(P)
        pk[idx[beg[col]:beg[col + 1]]] = val[beg[col]:beg[col + 1]]
        mats.append(unpack_lower(pk, n))
    return mats[0], np.stack(mats[1:]) if m else np.zeros((0, n, n))


def random_sym(rng, n, density=1.0, scale=1.0):
    B = rng.standard_normal((n, n)) * scale
    if density < 1.0:
        B *= rng.random((n, n)) < density
    return np.tril(B) + np.tril(B, -1).T


def householder_q(rng, n, k=4):
    """orthogonal Q as a product of k seeded Householder reflectors (exactly orthogonal up to rounding, cheap)"""
    Q = np.eye(n)
    for _ in range(k):
        v = rng.standard_normal(n)
        v /= np.linalg.norm(v)
        Q -= 2.0 * np.outer(Q @ v, v)
    return Q


def T(C, A, tau, y, eye):
    S = tau * C - np.tensordot(np.asarray(y, dtype=np.float64), A, axes=1) if A.shape[0] else tau * C.copy()
    S = np.array(S, dtype=np.float64)
    S[np.diag_indices_from(S)] += eye
    return S


def logdet(S):
    L = np.linalg.cholesky(S)
    return 2.0 * float(np.sum(np.log(np.diag(L))))


def is_pd(S):
    try:
        np.linalg.cholesky(S)
        return True
    except np.linalg.LinAlgError:
        return False


def alpha_star(S, dS):
    """the exact largest step with S + alpha dS positive semidefinite (S positive definite)"""
    L = np.linalg.cholesky(S)
    W = np.linalg.solve(L, -dS)
    W = np.linalg.solve(L, W.T)
    ev = np.linalg.eigvalsh(0.5 * (W + W.T))
    # (an eigenvalue that is zero in exact arithmetic comes out at rounding level: <= 1e-13 of the spectrum counts as zero)
    lam = float(ev[-1])
    return np.inf if lam <= 1e-13 * max(float(np.max(np.abs(ev))), 1e-300) else 1.0 / lam


def primal_X(S, dS, mu):
    """mu L^-T (sym(L^-1 dS L^-T) + I) L^-1 with S = L L^T (the reference's primal recovery, by definition)"""
    L = np.linalg.cholesky(S)
    Li = np.linalg.inv(L)
    Z = Li @ dS @ Li.T
    Z = 0.5 * (Z + Z.T) + np.eye(S.shape[0])
    X = mu * (Li.T @ Z @ Li)
    return 0.5 * (X + X.T)


def dev_lower(D):
    """the engine's raw dual matrix (dual_matrix(): column-major seen in C order) -> the valid triangle as a full symmetric
    matrix; the other triangle of the device buffer is not maintained"""
    U = np.triu(D)
    return U + np.triu(U, 1).T


def ratio_block(n, seed):
    """data of the ratio-test checks: C = Q diag(lambda) Q^T (lambda in [1, 10]) and four constraint matrices built on the
    factor L of C, so that with S = C the direction dy = e_k has L^-1 (-dS) L^-T = W_k exactly (up to rounding):
    A_1 generic (W_1 symmetric random, top eigenvalue of order 1), A_2 = L (2 v v') L' (rank one: dy = e_2 moves one
    eigenvalue, alpha* = 1/2; dy = -e_2 gives a positive semidefinite dS), A_3 with a top eigenvalue pair 1, 1 - 1e-9
    (alpha* = 1), A_4 = C (dy = e_4: dS = -S, alpha* = 1)"""
    rng = np.random.default_rng(seed)
    Q = householder_q(rng, n)
    lam = np.linspace(1.0, 10.0, n)
    C = (Q * lam) @ Q.T
    C = 0.5 * (C + C.T)
    L = np.linalg.cholesky(C)
    W1 = random_sym(rng, n, scale=1.0 / np.sqrt(max(n, 1)))
    v = rng.standard_normal(n)
    v /= np.linalg.norm(v)
    W2 = 2.0 * np.outer(v, v)
    Q3 = householder_q(rng, n, 3)
    w3 = np.concatenate([[1.0, 1.0 - 1e-9][:n], np.linspace(-1.0, 0.8, max(n - 2, 0))])
    W3 = (Q3 * w3) @ Q3.T
    A = np.stack([L @ W @ L.T for W in (W1, W2, W3)] + [C])
    A = 0.5 * (A + np.transpose(A, (0, 2, 1)))
    return C, A


# (dtau, dy, ada, name) of the ratio-test sequence on ratio_block data, in the order the device and the oracle both run it
# (the Lanczos start vector of a call depends on the calls before it); ada only acts where Rd != 0.  dS = -S comes last: its
# recurrence breaks down after one step (L^-1 (-dS) L^-T = I), and the vector it leaves for the next call's warm start is
# rounding noise, different in any two implementations.
def ratio_directions(m=4):
    e = np.eye(m)
    return [(0.0, e[0], 0.0, "generic"), (0.0, e[1], 0.0, "rank-one"), (0.0, -e[1], 0.0, "psd"),
            (0.0, e[2], 0.0, "near-degenerate pair"), (-0.3, 0.5 * e[0] + 0.2 * e[2], 0.4, "dtau and ada"),
            (0.0, e[3], 0.0, "dS = -S")]


# A property of the reference's Lanczos estimate, not of any kernel: its step is 1 / (theta + gamma) with theta the largest
# Ritz value and gamma a residual bound, and falls short of alpha* by about the bound when it has converged to the top
# eigenvalue (a warm-started test can stop at a lower one: cone_ratio_test's safeguard).  Smallest oracle step / alpha*
# measured once on the ratio_block spectra at every size the GPU test uses (fresh cone, the ratio_directions sequence);
# tests/test_line_search_model.py re-checks the floor at n = 2, 16, 17, 129 and 257.
ORACLE_STEP_FLOOR = 0.95      # measured minimum 0.9775 (n = 257, generic direction)
