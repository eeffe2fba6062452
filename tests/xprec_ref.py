"""Extended-precision host reference of the Schur quantities of one SDP block -- plain numpy, no engine, no oracle code.

The GPU conditioning tests (tests/test_gpu_conditioning.py) measure the engine and the plain-C oracle against the SAME truth:
the quantities below evaluated at the dual matrix S the engine holds, to about 1e-18 relative to the products involved
(np.longdouble: 64-bit mantissa on x86-64).  At cond(S) = 1e10 that leaves the truth about 1e-8 off in relative terms, two
orders of magnitude below what any fp64 evaluation reaches there.

Products go through `mm`: every fp64 operand is cut into three slices of at most 20 significant bits against its row
(column) maximum, so that each slice product -- an ordinary fp64 matrix product -- is exact for inner dimensions up to 2^12;
the six leading slice products are summed in longdouble.  That is longdouble accuracy at the speed of the fp64 BLAS.
A longdouble operand enters as its fp64 head (exact product) plus its fp64 tail (plain product; the tail's own rounding is
1e-16 of something already 1e-16 small).

Formulas and signs are those of the oracle's orc_kkt_build (oracle/hdsdp_oracle.c), with K = S^-1 (or the registered
primal X for KKT_TYPE_PRIMAL):

    M_ij        = tr(A_i K A_j K)             ASinv_i     = tr(A_i K)
    ASinvRdSinv = Rd tr(A_i K K)              ASinvCSinv  = tr(A_i K C K)          (HOMOGENEOUS only)
    CSinv       = tr(C K)   CSinvCSinv = tr(C K C K)   CSinvRdSinv = Rd tr(K C K)   (HOMOGENEOUS only)
    TraceSinv   = tr(K) when Rd != 0, else 0

A constraint family is one of
    ("dense", A)                 A: m x n x n symmetric
    ("r1", a, s)                 A_i = s_i a_i a_i^T, a: m x n, s: m signs (+-1)
    ("sparse", rows, cols, vals, owner)  entries of the FULL symmetric matrices (both triangles), owner = constraint index
"""
import numpy as np

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
HAVE_LD = EPS_LD <= 1e-18
NO_LD_REASON = f"np.longdouble has eps {EPS_LD:.3g} here (needs the 64-bit x87 mantissa, eps 1.08e-19)"

_NSLICE = 3


def _bits(k):
    """slice width for an inner dimension k: k products of two b-bit integers sum exactly in fp64"""
    return max(1, (53 - int(np.ceil(np.log2(max(k, 2))))) // 2)


def _slice(A, axis, b):
    """A (fp64) = sum_s P_s * 2^e (row-wise along axis=1 scales, column-wise along axis=0) + rem, each P_s an integer multiple
    of 2^-(b(s+1)) below 2^-(b s) + 1 in magnitude; returns (slices, exponents)"""
    mx = np.max(np.abs(A), axis=axis, keepdims=True)
    _, e = np.frexp(np.where(mx > 0, mx, 1.0))
    As = np.ldexp(A, -e)                       # |As| < 1, exact
    out = []
    for s in range(_NSLICE):
        sc = float(2.0 ** (b * (s + 1)))
        p = np.rint(As * sc) / sc              # exact: power-of-two scalings and an integer rounding
        As = As - p                            # exact: p is As cut at a bit position inside its own mantissa
        out.append(p)
    return out, e


def _mm64(A, B):
    """longdouble-accurate A @ B of two fp64 matrices (2-D)"""
    b = _bits(A.shape[1])
    Pa, ea = _slice(A, 1, b)
    Pb, eb = _slice(B, 0, b)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for s in range(_NSLICE):
        for t in range(_NSLICE - s):           # the pairs below 2^-3b of the product are dropped: < 2^-60 relative
            acc += (Pa[s] @ Pb[t]).astype(LD)
    return acc * np.power(LD(2.0), ea.astype(LD)) * np.power(LD(2.0), eb.astype(LD))


def split(X):
    """longdouble -> (fp64 head, fp64 tail)"""
    X = np.asarray(X)
    if X.dtype != LD:
        return np.asarray(X, dtype=np.float64), None
    hi = X.astype(np.float64)
    return hi, (X - hi.astype(LD)).astype(np.float64)


def mm(A, B):
    """A @ B to longdouble accuracy (2-D operands, fp64 or longdouble), as longdouble"""
    Ah, Al = split(A)
    Bh, Bl = split(B)
    out = _mm64(Ah, Bh)
    if Bl is not None:
        out += (Ah @ Bl).astype(LD)
    if Al is not None:
        out += (Al @ Bh).astype(LD)
    return out


def sym(X):
    return (X + X.T) / 2


def inverse(S, steps=2):
    """S^-1 of a symmetric positive definite fp64 matrix in longdouble: the fp64 inverse, then Newton-Schulz steps
    X <- X + X (I - S X) with the residual in longdouble (its correction X R may be formed in fp64: R is small).
    The result is left as the steps make it: its forward error and its asymmetry are both about eps_ld cond relative, but
    symmetrising it would put that asymmetry into the residual S X - I at full size (S (X - X^T) is not small)."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    X = sym(np.linalg.inv(S)).astype(LD)
    I = np.eye(n, dtype=LD)
    for _ in range(steps):
        R = I - mm(S, X)
        Xh = X.astype(np.float64)
        X = X + (Xh @ R.astype(np.float64)).astype(LD)
    return X


def solve(S, b, steps=3):
    """S^-1 b (vector or n x k; S fp64 or longdouble) by an fp64 solve refined with longdouble residuals"""
    Sh = split(S)[0]
    b2 = np.asarray(b).reshape(Sh.shape[0], -1)
    x = np.linalg.solve(Sh, b2.astype(np.float64)).astype(LD)
    for _ in range(steps):
        r = b2.astype(LD) - mm(S, x)
        x = x + np.linalg.solve(Sh, r.astype(np.float64)).astype(LD)
    return x.reshape(np.shape(b))


def inverse_residual_max(S, X):
    """max_ij |(S X - I)_ij|, evaluated in longdouble (no normalisation)"""
    return float(np.max(np.abs(mm(S, X) - np.eye(S.shape[0], dtype=LD))))


def backward_error(S, x, b):
    """normwise backward error of x as a solution of S x = b, per column (residual in longdouble):
    |b - S x|_inf / (|S|_inf |x|_inf + |b|_inf)"""
    S = np.asarray(S, dtype=np.float64)
    x2 = np.asarray(x, dtype=np.float64).reshape(S.shape[0], -1)
    b2 = np.asarray(b, dtype=np.float64).reshape(S.shape[0], -1)
    r = (b2.astype(LD) - mm(S, x2)).astype(np.float64)
    nS = float(np.max(np.sum(np.abs(S), axis=1)))
    return np.max(np.abs(r), axis=0) / (nS * np.max(np.abs(x2), axis=0) + np.max(np.abs(b2), axis=0))


def inverse_residual_normwise(S, X):
    """|S X - I|_inf / (|S|_inf |X|_inf), the product in longdouble"""
    S = np.asarray(S, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    R = (mm(S, X) - np.eye(S.shape[0], dtype=LD)).astype(np.float64)
    ninf = lambda A: float(np.max(np.sum(np.abs(A), axis=1)))   # noqa: E731
    return ninf(R) / (ninf(S) * ninf(X))


def logdet(S):
    """log det S of a symmetric positive definite fp64 matrix: 2 sum log diag(L) of the fp64 Cholesky factor L plus
    log det(I + E), E = L^-1 (S - L L^T) L^-T with the residual in longdouble"""
    S = np.asarray(S, dtype=np.float64)
    L = np.linalg.cholesky(S)
    R = (S.astype(LD) - mm(L, L.T)).astype(np.float64)
    import scipy.linalg as sl
    E = sl.solve_triangular(L, sl.solve_triangular(L, R, lower=True).T, lower=True)
    ev = np.linalg.eigvalsh(sym(E))
    return LD(2.0) * np.sum(np.log(np.diag(L).astype(LD))) + LD(float(np.sum(np.log1p(ev))))


def _contract(Z, fam):
    """<Z, A_i> for every constraint i (Z symmetric, longdouble)"""
    kind = fam[0]
    if kind == "dense":
        A = fam[1]
        m = A.shape[0]
        return (A.reshape(m, -1).astype(LD) @ Z.reshape(-1).astype(LD))
    if kind == "r1":
        a, s = fam[1], fam[2]
        W = mm(Z, a.T)                                        # n x m
        return s.astype(LD) * np.sum(a.T.astype(LD) * W, axis=0)
    rows, cols, vals, owner, m = fam[1:6]
    out = np.zeros(m, dtype=LD)
    np.add.at(out, owner, vals.astype(LD) * Z[rows, cols])
    return out


def _gram(K, fam):
    """M_ij = tr(A_i K A_j K) (longdouble, full symmetric)"""
    kind = fam[0]
    if kind == "dense":
        A = fam[1]
        m = A.shape[0]
        B = np.stack([mm(mm(K, A[i]), K) for i in range(m)])
        return sym(B.reshape(m, -1) @ A.reshape(m, -1).T.astype(LD))
    if kind == "r1":
        a, s = fam[1], fam[2]
        G = mm(a, mm(K, a.T))                                  # a_i^T K a_j
        sl = s.astype(LD)
        return sym(sl[:, None] * sl[None, :] * G * G)
    rows, cols, vals, owner, m = fam[1:6]
    # sum over entries (p, q) of A_i and (r, t) of A_j of a_pq a_rt K_qr K_tp
    P = vals.astype(LD)[:, None] * vals.astype(LD)[None, :] * K[cols][:, rows] * K[cols][:, rows].T
    onehot = np.zeros((m, rows.size), dtype=LD)
    onehot[owner, np.arange(rows.size)] = 1
    return sym(onehot @ P @ onehot.T)


def schur(K, C, Rd, fam, typeKKT):
    """the oracle's kkt_build outputs at the (longdouble) matrix K in S^-1's place: dict with the same keys, longdouble.
    typeKKT: 0 INFEASIBLE, 1 CORRECTOR, 2 HOMOGENEOUS, 3 PRIMAL (K = the registered X)"""
    K = np.asarray(K, dtype=LD)
    C = np.asarray(C, dtype=np.float64)
    out = {"ASinv": _contract(K, fam)}
    K2 = sym(mm(K, K))
    out["ASinvRdSinv"] = LD(Rd) * _contract(K2, fam) if Rd != 0.0 else np.zeros_like(out["ASinv"])
    if typeKKT == 1:
        return out
    out["M"] = _gram(K, fam)
    out["TraceSinv"] = np.trace(K) if Rd != 0.0 else LD(0.0)
    if typeKKT == 2:
        KCK = sym(mm(mm(K, C), K))
        out["ASinvCSinv"] = _contract(KCK, fam)
        out["CSinv"] = np.sum(K * C.astype(LD))
        out["CSinvCSinv"] = np.sum(KCK * C.astype(LD))
        out["CSinvRdSinv"] = LD(Rd) * np.trace(KCK) if Rd != 0.0 else LD(0.0)
    return out


def scalar_sensitivities(K, C, Rd):
    """for each single scalar f(S) of the build, the matrix P with f(S + dS) - f(S) = -tr(P dS) + O(dS^2) (K = S^-1):
    log det S (P = -K), tr K (P = K K), tr C K (P = K C K), tr C K C K (P = 2 K C K C K), Rd tr K C K (P = Rd (KCK K + K KCK))"""
    Kd = np.asarray(K, dtype=np.float64)
    KCK = Kd @ np.asarray(C, dtype=np.float64) @ Kd
    return {"logdet": -Kd, "TraceSinv": Kd @ Kd, "CSinv": KCK, "CSinvCSinv": 2.0 * KCK @ np.asarray(C, dtype=np.float64) @ Kd,
            "CSinvRdSinv": Rd * (KCK @ Kd + Kd @ KCK)}


def rounding_bound(P, S):
    """first-order size of the change of a scalar with sensitivity P when S is factored by a backward-stable Cholesky:
    u sum_ij |P_ij| (|L| |L^T|)_ij -- one unit of rounding of the componentwise backward error |dS| <= gamma_n |L| |L^T| of the
    factorisation (the worst case carries n u instead of u)"""
    S = np.asarray(S, dtype=np.float64)
    L = np.abs(np.linalg.cholesky(S))
    return float(2.0 ** -53 * np.sum(np.abs(P) * (L @ L.T)))


def family_from_sparse(n, m, mats_entries):
    """("sparse", ...) from a list of per-constraint lower-triangle entry lists [(row, col, val), ...] (row >= col)"""
    rows, cols, vals, owner = [], [], [], []
    for i, ent in enumerate(mats_entries):
        for r, c, v in ent:
            rows.append(r); cols.append(c); vals.append(v); owner.append(i)
            if r != c:
                rows.append(c); cols.append(r); vals.append(v); owner.append(i)
    return ("sparse", np.asarray(rows), np.asarray(cols), np.asarray(vals, dtype=np.float64), np.asarray(owner), m)
