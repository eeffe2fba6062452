"""Patterns, matrices, a model of the symbolic phase and the comparison rule for the two sparse factorisations of the Schur
matrix: the tile LDL' (csrc/bsparse.hip, through HMiBspSolve) and the block-envelope Cholesky (HdmChol::set_envelope, through
HMiCholEnvelopeSolve) -- plain numpy / scipy, importable without a GPU.  The only library call in here is HMiRcmOrder (host code).

The rule is test_gpu_conditioning.py's and pivoted_cases.py's, on the normwise backward error of xprec_ref.backward_error
(residual in longdouble), with u = 2^-53:

    e(gpu) <= 8 e(ref) + 16 u

ref = scipy's dense Cholesky solve of the same matrix for a positive definite case, and a plain fp64 LDL' without pivoting
(`ldl_nopivot`, in the model's permuted order) for a quasi-definite one: the algorithm the tile form runs, so the two share
their pivot growth.  tests/test_sparse_schur_cases_cpu.py holds both references under CAP = 64 u on everything generated here.

THE MODEL of HdmBsp::symbolic (written from csrc/bsparse.h's description, not from the code):
    * rows with more than max(128, 10 x median degree) neighbours form the dense tail: they keep their order and go last;
      the others are ordered by reverse Cuthill-McKee (HMiRcmOrder on the pattern restricted to them);
    * the block pattern of the permuted matrix (128-row blocks, lower triangle, diagonal blocks always present) is closed by
      boolean block elimination, column by column: every pair of blocks below the diagonal of column k makes a block;
    * the parent of block column k is its first block below the diagonal; a column's level is one more than the highest level
      among its children; the update source pairs are the pairs (a >= b) of blocks below the diagonal of a column.

PATTERN FAMILIES (pairs i > j of linked rows; each in the natural numbering and under a random renumbering):
    band      j in [i - 37, i)
    blocks    independent 50-row blocks (they straddle the tile edges: the block columns form a chain)
    arrow     16-row blocks (the one short block first), and the last 5 rows linked to every row.  (16, not 12: blocks whose
              edges fall on tile edges leave block columns independent of each other, so that a level holds several of them;
              12-row blocks straddle every tile edge at m = 640 and the levels degenerate to a chain.)
    tree      i linked to (i - 1) // 2
    filltail  a band of width 2 over the first m - 140 rows (degree 4: the median), then 140 rows each linked to 130 rows
              drawn from the first 300 and not to each other: degree 130 > 128 sends them to the dense tail, which spans two
              tiles, and the tile between those two exists only as fill

VALUES
    spd       G = D B D, B the pattern's diagonally dominant matrix (off-diagonal uniform(-1, 1), diagonal = sum |row| + 1 + u_i,
              u_i uniform(0, 1)), D geometric from 1 to cond^-1/2 along the model's elimination order ("down") or against it ("up")
    qd        quasi-definite: signs s_i = +-1 (about a third negative), diagonal s_i (sum |row| + 1 + u_i), an off-diagonal entry
              between rows of equal sign multiplied by that sign, one between rows of opposite sign as drawn.  The two sign
              classes give [[H, C'], [C, -K]] with H and K strictly diagonally dominant, hence positive definite: every symmetric
              permutation has an LDL', with exactly #{s_i < 0} negative pivots.  Graded by the same D.

ENVELOPES: `first[i]` families over nblk 128-blocks (ENV_FAMILIES below); the matrix is dense in the lower part of every block
inside the row envelope, exactly 0.0 outside, (sum |row| + 1)-dominant and graded as above.

Everything is seeded from (family, size): the CPU checks and the GPU tests see the same bits."""
import ctypes as C
import functools
import json
import zlib

import numpy as np
import scipy.linalg as sl

import xprec_ref as xp

U = 2.0 ** -53
CAP = 64.0 * U
BT = 128

FAMILIES = ("band", "blocks", "arrow", "tree", "filltail")
SWEEP_FAMILIES = ("band", "arrow")
SWEEP_M = (129, 255, 256, 257, 384, 385, 640)
FILLTAIL_M = 1040
BIG_M = {"band": 1153, "blocks": 1153, "arrow": 1153, "tree": 1153, "filltail": FILLTAIL_M}
CONDS = (1e2, 1e6, 1e10)
QD_CONDS = (1e2, 1e6)
GRADES = ("down", "up")


def within(e_gpu, e_ref):
    return e_gpu <= 8.0 * e_ref + 16.0 * U


def _rng(tag, n, extra=0):
    return np.random.default_rng([zlib.crc32(tag.encode()), int(n), int(extra)])


# ---------------------------------------------------------------- patterns

def _natural_pairs(family, m):
    if family == "band":
        return [(i, j) for i in range(m) for j in range(max(0, i - 37), i)]
    if family == "blocks":
        return [(i, j) for i in range(m) for j in range(i - i % 50, i)]
    if family == "arrow":
        short = (m - 5) % 16                       # rows 0 .. short-1 are the one short block

        def start(i):
            return 0 if i < short else i - (i - short) % 16
        return [(i, j) for i in range(m - 5) for j in range(start(i), i)] + [(i, j) for i in range(m - 5, m) for j in range(i)]
    if family == "tree":
        return [(i, (i - 1) // 2) for i in range(1, m)]
    if family == "filltail":
        body = m - 140
        assert body >= 600
        rng = _rng("filltail links", m)
        pairs = [(i, j) for i in range(body) for j in range(max(0, i - 2), i)]
        for t in range(body, m):
            pairs += [(t, int(j)) for j in rng.choice(300, 130, replace=False)]
        return pairs
    raise ValueError(family)


@functools.lru_cache(maxsize=None)
def pattern(family, m, renumbered, isolate=()):
    """sorted tuple of (i, j), i > j, in the driver's numbering; rows in `isolate` (driver's numbers) lose every link"""
    pairs = _natural_pairs(family, m)
    if renumbered:
        p = _rng("renumber " + family, m).permutation(m)
        pairs = [(int(p[i]), int(p[j])) for i, j in pairs]
    out = {(max(i, j), min(i, j)) for i, j in pairs if i not in isolate and j not in isolate}
    return tuple(sorted(out))


def lower_csc(m, pairs):
    """(beg, idx) int32 of the lower triangle: the diagonal entry first in every column, then the rows in increasing order"""
    cols = [[] for _ in range(m)]
    for i, j in pairs:
        cols[j].append(i)
    beg, idx = [0], []
    for c in range(m):
        idx.append(c)
        idx += sorted(cols[c])
        beg.append(len(idx))
    return np.array(beg, dtype=np.int32), np.array(idx, dtype=np.int32)


def csc_values(A, beg, idx):
    """the entries of the dense symmetric A at the CSC positions"""
    cols = np.repeat(np.arange(len(beg) - 1), np.diff(beg))
    return np.ascontiguousarray(A[idx, cols])


# ---------------------------------------------------------------- the model of the symbolic phase

def rcm_order(m, beg, idx):
    from hdsdp_amd import api
    lib = api.load_library()
    ip = C.POINTER(C.c_int)
    perm = np.zeros(m, dtype=np.int32)
    assert lib.HMiRcmOrder(m, beg.ctypes.data_as(ip), idx.ctypes.data_as(ip), perm.ctypes.data_as(ip)) == 0
    return perm


class Symbolic:
    """perm (old -> new), nb, tail (rows in the dense tail), P0 / P (boolean nb x nb lower block pattern of the permuted
    matrix / of its factor), ntiles, level (per block column), nlevels, pairs (update source pairs)"""


@functools.lru_cache(maxsize=None)
def model(m, pairs):
    s = Symbolic()
    deg = np.zeros(m, dtype=np.int64)
    for i, j in pairs:
        deg[i] += 1
        deg[j] += 1
    median = int(np.sort(deg)[m // 2])
    dense = deg > max(BT, 10 * max(1, median))
    keep = np.flatnonzero(~dense)
    sub = -np.ones(m, dtype=np.int64)
    sub[keep] = np.arange(keep.size)
    perm = np.zeros(m, dtype=np.int64)
    if keep.size:
        sbeg, sidx = lower_csc(keep.size, [(int(sub[i]), int(sub[j])) for i, j in pairs if not dense[i] and not dense[j]])
        perm[keep] = rcm_order(keep.size, sbeg, sidx)
    perm[np.flatnonzero(dense)] = keep.size + np.arange(m - keep.size)
    assert sorted(perm.tolist()) == list(range(m))
    nb = (m + BT - 1) // BT
    P0 = np.eye(nb, dtype=bool)
    for i, j in pairs:
        a, b = int(perm[i]) // BT, int(perm[j]) // BT
        P0[max(a, b), min(a, b)] = True
    P = P0.copy()
    for k in range(nb):                                   # boolean block elimination, the naive way
        below = [int(r) for r in np.flatnonzero(P[:, k]) if r > k]
        for a in below:
            for b in below:
                if b <= a:
                    P[a, b] = True
    level = np.zeros(nb, dtype=np.int64)
    npairs = 0
    for k in range(nb):
        below = [int(r) for r in np.flatnonzero(P[:, k]) if r > k]
        npairs += len(below) * (len(below) + 1) // 2
        if below:
            level[below[0]] = max(level[below[0]], level[k] + 1)
    s.perm, s.nb, s.tail, s.P0, s.P = perm, nb, int(m - keep.size), P0, P
    s.ntiles, s.level, s.nlevels, s.pairs = int(P.sum()), level, int(level.max()) + 1, npairs
    return s


def block_csc(P):
    """(blockPtr, blockRow) of a boolean lower block pattern, by block column"""
    ptr, row = [0], []
    for k in range(P.shape[0]):
        row += [int(r) for r in np.flatnonzero(P[:, k])]
        ptr.append(len(row))
    return ptr, row


# ---------------------------------------------------------------- values

def dominant(m, pairs, tag):
    """B: symmetric, off-diagonal uniform(-1, 1) on the pattern, diagonal = sum |row| + 1 + uniform(0, 1)"""
    rng = _rng("values " + tag, m)
    A = np.zeros((m, m))
    ij = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    v = rng.uniform(-1.0, 1.0, ij.shape[0])
    A[ij[:, 0], ij[:, 1]] = v
    A[ij[:, 1], ij[:, 0]] = v
    A[np.arange(m), np.arange(m)] = np.sum(np.abs(A), axis=1) + 1.0 + rng.uniform(0.0, 1.0, m)
    return A


def signs(m, tag):
    """s_i = +-1, about a third negative"""
    return np.where(_rng("signs " + tag, m).uniform(0.0, 1.0, m) < 1.0 / 3.0, -1.0, 1.0)


def quasi_definite(B, s):
    same = s[:, None] == s[None, :]
    A = np.where(same, B * s[:, None], B)
    A[np.arange(len(s)), np.arange(len(s))] = s * np.diag(B)
    assert np.array_equal(A, A.T)
    return A


def grading(perm, cond, grade):
    """d_i geometric from 1 to cond^-1/2 along the elimination order `perm` (grade "down") or against it ("up")"""
    m = len(perm)
    g = np.geomspace(1.0, 1.0 / np.sqrt(cond), m)
    return g[perm] if grade == "down" else g[m - 1 - perm]


def graded(A, d):
    """D A D, symmetric bit for bit (mirrored from the lower triangle)"""
    L = (d[:, None] * np.tril(A)) * d[None, :]
    return np.ascontiguousarray(L + np.tril(L, -1).T)


class TileCase:
    """one matrix for HMiBspSolve: m, pairs, beg, idx, val, A (dense symmetric), b, sym (the model), s (signs or None)"""


@functools.lru_cache(maxsize=None)
def tile_case(family, m, renumbered, kind, cond, grade, variant=0):
    """kind "spd" or "qd"; variant != 0: other values on the same pattern"""
    c = TileCase()
    c.m, c.pairs = m, pattern(family, m, renumbered)
    c.sym = model(m, c.pairs)
    tag = f"{family} {int(renumbered)} {variant}"
    B = dominant(m, c.pairs, tag)
    c.s = signs(m, tag) if kind == "qd" else None
    if kind == "qd":
        B = quasi_definite(B, c.s)
    c.A = graded(B, grading(c.sym.perm, cond, grade))
    c.beg, c.idx = lower_csc(m, c.pairs)
    c.val = csc_values(c.A, c.beg, c.idx)
    c.b = _rng("rhs " + tag, m).standard_normal(m)
    for a in (c.A, c.val, c.b):
        a.setflags(write=False)
    return c


def backward_error(A, x, b):
    return float(np.max(xp.backward_error(A, x, b)))


def cholesky_solve(A, b):
    """scipy's dense Cholesky solve (dpotrf / dpotrs)"""
    return sl.cho_solve(sl.cho_factor(A, lower=True, check_finite=False), b, check_finite=False)


def ldl_nopivot(A, perm, b):
    """plain fp64 LDL' without pivoting of P A P' (perm: old -> new), right-looking, one column at a time, and the solve.
    Returns (x in the original numbering, number of negative pivots).  Only the rows with an entry in the pivot column are
    updated -- the others would receive exact zeros."""
    m = A.shape[0]
    inv = np.argsort(perm)
    W = np.array(A[np.ix_(inv, inv)], dtype=np.float64)
    d = np.zeros(m)
    for j in range(m):
        d[j] = W[j, j]
        assert d[j] != 0.0 and np.isfinite(d[j])
        r = j + 1 + np.flatnonzero(W[j + 1:, j])
        if r.size:
            l = W[r, j] / d[j]
            W[np.ix_(r, r)] -= np.outer(l, W[r, j])
            W[r, j] = l
    L = np.tril(W, -1) + np.eye(m)
    y = sl.solve_triangular(L, np.asarray(b)[inv], lower=True, unit_diagonal=True, check_finite=False)
    z = sl.solve_triangular(L.T, y / d, lower=False, unit_diagonal=True, check_finite=False)
    return z[perm], int(np.sum(d < 0))


@functools.lru_cache(maxsize=None)
def tile_reference(family, m, renumbered, kind, cond, grade, variant=0):
    """(e(ref), negative pivots of the reference) -- computed once, shared"""
    c = tile_case(family, m, renumbered, kind, cond, grade, variant)
    if kind == "spd":
        return backward_error(c.A, cholesky_solve(c.A, c.b), c.b), 0
    x, nneg = ldl_nopivot(c.A, c.sym.perm, c.b)
    return backward_error(c.A, x, c.b), nneg


def sweep_cases():
    """(family, m, renumbered, grade): SPD at cond 1e6"""
    return [(f, m, r, g) for f in SWEEP_FAMILIES for m in SWEEP_M for r in (False, True) for g in GRADES]


def big_cases(family):
    """(m, renumbered, kind, cond, grade) of the conditioning group"""
    m = BIG_M[family]
    return [(m, r, "spd", c, g) for r in (False, True) for c in CONDS for g in GRADES] + \
           [(m, r, "qd", c, g) for r in (False, True) for c in QD_CONDS for g in GRADES]


def all_patterns():
    """every (family, m, renumbered) the GPU tests use"""
    out = [(f, m, r) for f in SWEEP_FAMILIES for m in SWEEP_M for r in (False, True)]
    out += [(f, BIG_M[f], r) for f in FAMILIES for r in (False, True)]
    return out


# ---------------------------------------------------------------- zero pivots

# (family, m, renumbered, the two rows that are cut off and get a zero diagonal, what the pair covers)
ZERO_PIVOT = (
    ("blocks", 640, False, (310, 330), "same tile"),
    ("band", 640, False, (0, 320), "different levels"),
    ("arrow", 1153, False, (200, 700), "same level, different tiles"),
)


@functools.lru_cache(maxsize=None)
def zero_pivot_case(family, m, renumbered, rows):
    """an SPD matrix (cond 1e2) on the pattern with `rows` cut off; the caller zeroes their diagonals.  Returns a TileCase
    whose model is that of the cut pattern"""
    c = TileCase()
    c.m, c.pairs = m, pattern(family, m, renumbered, tuple(rows))
    c.sym = model(m, c.pairs)
    tag = f"zero {family} {rows}"
    c.A = graded(dominant(m, c.pairs, tag), grading(c.sym.perm, 1e2, "down"))
    c.beg, c.idx = lower_csc(m, c.pairs)
    c.val = csc_values(c.A, c.beg, c.idx)
    c.b = _rng("rhs " + tag, m).standard_normal(m)
    c.s = None
    return c


# ---------------------------------------------------------------- envelopes

ENV_N = (129, 256, 257, 600, 1153)
ENV_FAMILIES = ("dense", "diagonal", "band1", "band2", "arrow", "steps", "reachback", "unclamped")
ENV_MIN_NBLK = {"dense": 2, "diagonal": 2, "band1": 3, "band2": 4, "arrow": 3, "steps": 3, "reachback": 5, "unclamped": 5}
ENV_COND_N = 600


def env_first(family, nblk):
    """first[i] as handed to set_envelope (for `unclamped`: with one entry above i and one negative)"""
    i = np.arange(nblk)
    if family == "dense":
        f = np.zeros(nblk, dtype=np.int64)
    elif family == "diagonal":
        f = i.copy()
    elif family in ("band1", "reachback", "unclamped"):
        f = np.maximum(0, i - 1)
        if family == "reachback":                 # one middle row reaches two blocks further back than the row after it
            r = nblk // 2
            f[r] = f[r + 1] - 2
            assert f[r] >= 0
        if family == "unclamped":
            f[1] = nblk                           # above its row: clamped to the diagonal block
            f[nblk - 2] = -3                      # negative: clamped to 0
    elif family == "band2":
        f = np.maximum(0, i - 2)
    elif family == "arrow":
        f = i.copy()
        f[-1] = 0
    elif family == "steps":
        f = i - i % 2
    else:
        raise ValueError(family)
    return f.astype(np.int32)


def env_clamp(first):
    """set_envelope's clamp: 0 <= first[i] <= i"""
    first = np.asarray(first, dtype=np.int64)
    return np.minimum(np.maximum(first, 0), np.arange(len(first))).astype(np.int32)


def env_colh(first):
    """last block row whose (clamped) envelope reaches block column k, as a running maximum: it never rises"""
    f = env_clamp(first)
    nblk = len(f)
    colh = np.array([max(i for i in range(nblk) if f[i] <= k and i >= k) for k in range(nblk)])
    return np.maximum.accumulate(colh)


def env_families_at(nblk):
    return tuple(f for f in ENV_FAMILIES if nblk >= ENV_MIN_NBLK[f])


def env_cases():
    """(family, n, cond, grade)"""
    out = []
    for n in ENV_N:
        nblk = (n + BT - 1) // BT
        for f in env_families_at(nblk):
            out.append((f, n, 1e6, "down"))
            if n == ENV_COND_N:
                out += [(f, n, 1e2, "up"), (f, n, 1e10, "down")]
    return out


def env_mask(first, n):
    """boolean n x n: the lower triangle inside the (clamped) row envelope"""
    f = env_clamp(first)
    r = np.arange(n)
    return (r[None, :] <= r[:, None]) & (r[None, :] >= BT * f[r // BT][:, None])


class EnvCase:
    """n, nblk, first (as handed over), clamped, A (dense symmetric), b, inside (mask of the lower triangle in the envelope)"""


@functools.lru_cache(maxsize=None)
def env_case(family, n, cond, grade):
    c = EnvCase()
    c.n, c.nblk = n, (n + BT - 1) // BT
    c.first = env_first(family, c.nblk)
    c.clamped = env_clamp(c.first)
    c.inside = env_mask(c.first, n)
    rng = _rng("envelope " + family, n)
    Lo = np.where(c.inside, rng.uniform(-1.0, 1.0, (n, n)), 0.0)
    A = np.tril(Lo, -1)
    A = A + A.T
    A[np.arange(n), np.arange(n)] = np.sum(np.abs(A), axis=1) + 1.0
    c.A = graded(A, grading(np.arange(n), cond, grade))
    c.b = _rng("envelope rhs " + family, n).standard_normal(n)
    for a in (c.A, c.b):
        a.setflags(write=False)
    return c


def factor_error(A, L):
    """|A - L L'|_inf / |A|_inf with the product in longdouble"""
    R = (np.asarray(A, dtype=xp.LD) - xp.mm(L, np.ascontiguousarray(L.T))).astype(np.float64)
    return float(np.max(np.sum(np.abs(R), axis=1)) / np.max(np.sum(np.abs(A), axis=1)))


@functools.lru_cache(maxsize=None)
def env_reference(family, n, cond, grade):
    """(e(scipy's solve), factor error of scipy's factor)"""
    c = env_case(family, n, cond, grade)
    Lf = np.tril(sl.cholesky(c.A, lower=True, check_finite=False))
    x = sl.cho_solve((Lf, True), c.b, check_finite=False)
    return backward_error(c.A, x, c.b), factor_error(c.A, Lf)


def not_pd(n, row, first):
    """S = L D L' inside the envelope `first`, L unit lower, D = I except D[row] = -1: the first non-positive pivot of the
    Cholesky factorisation is `row`"""
    rng = _rng("not pd", n, row)
    L = np.eye(n) + np.where(env_mask(first, n), np.tril(rng.standard_normal((n, n)), -1), 0.0) * (0.3 / np.sqrt(n))
    d = np.ones(n)
    d[row] = -1.0
    return xp.sym((L * d) @ L.T)


# ---------------------------------------------------------------- the report

def report(group, worst_ratio, e_gpu, e_ref, n_cases, note=""):
    """SPARSE_REPORT {json}: the worst e(gpu) / max(e(ref), 16 u) of a group, and the errors of that case in units of u"""
    print("SPARSE_REPORT " + json.dumps(dict(group=group, cases=int(n_cases), worst_ratio=round(float(worst_ratio), 4),
                                             e_gpu_u=round(float(e_gpu) / U, 3), e_ref_u=round(float(e_ref) / U, 3), note=note)))
