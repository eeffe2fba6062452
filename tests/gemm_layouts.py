"""A numpy model of the three storage formats the fp64 GEMM roles of a Schur build read and write -- written from their
descriptions, with no engine code: tests/test_gemm_layouts_cpu.py holds every index below to csrc/gemm_geom.h, csrc/work_plan.h
and the Gram operand's address arithmetic, and tests/test_gpu_gemm_roles.py packs operands and unpacks results with it.

* skyline storage of a matrix in A_L form (strict lower triangle + half the diagonal, A = A_L + A_L^T): the 128-column panels
  from their diagonal block downwards, panel t a plain column-major (n - 128 t) x 128 matrix (the last one has n - 128 t
  columns only), one after the other;
* the 16 x 16 blocked congruence output: the lower triangle in 16 x 16 sub-blocks numbered column by column, element (r, c) of
  sub-block `sub` of constraint row `row` at ((sub * 16 + c) * Lr + row) * 16 + r; diagonal sub-blocks hold all 256 entries at
  weight 1, the others are scaled by sqrt(2);
* the Gram operand W (R rows, K = 16 npb_loc columns) as [k block][row][16], the rows of a sharded block in segment order:
  ((i // Lr) * npb_loc + k // 16) * Lr * 16 + (i % Lr) * 16 + k % 16.
"""
import numpy as np

TILE = 128
RT2 = float(np.sqrt(2.0))


def roundup(x, q):
    return (x + q - 1) // q * q


# ---- layout numbers ----------------------------------------------------------------------------------
def layout(n, world=1, maxloc=0):
    n16 = roundup(n, 16)
    nblk = n16 // 16
    npb = nblk * (nblk + 1) // 2 * 16
    Lr = roundup(maxloc + 3, 8 if world == 1 else TILE)
    return dict(n16=n16, nblk=nblk, npb=npb, npb_loc=(npb + world - 1) // world, Lr=Lr, R=world * Lr, astride=sky_size(n16))


# ---- skyline -------------------------------------------------------------------------------------------
def sky_panel(t, n):
    """first element of panel t: the panels before it are (n - 128 s) x 128, s < t"""
    return sum((n - TILE * s) * TILE for s in range(t))


def sky_off(i, j, n):
    t = j // TILE
    return sky_panel(t, n) + (j - TILE * t) * (n - TILE * t) + (i - TILE * t)


def sky_size(n):
    t = (n + TILE - 1) // TILE - 1
    w = n - TILE * t
    return sky_panel(t, n) + w * w


def sky_pack(AL):
    """n x n lower triangular (numpy, [i, j]) -> its skyline storage"""
    n = AL.shape[0]
    assert AL.shape == (n, n) and not np.any(np.triu(AL, 1))
    out = np.zeros(sky_size(n))
    for t in range((n + TILE - 1) // TILE):
        blk = AL[TILE * t:, TILE * t:TILE * (t + 1)]
        out[sky_panel(t, n):sky_panel(t, n) + blk.size] = blk.T.reshape(-1)      # column after column
    return out


def sky_unpack(buf, n):
    AL = np.zeros((n, n))
    for t in range((n + TILE - 1) // TILE):
        h, w = n - TILE * t, min(TILE, n - TILE * t)
        AL[TILE * t:, TILE * t:TILE * t + w] = buf[sky_panel(t, n):sky_panel(t, n) + h * w].reshape(w, h).T
    return AL


# ---- blocked congruence output ---------------------------------------------------------------------------
def blk_sub(bi, bj, nblk):
    """number of sub-block (bi, bj), bi >= bj: the columns before bj hold nblk, nblk - 1, ... sub-blocks"""
    return sum(nblk - c for c in range(bj)) + (bi - bj)


def pblock_decode(q, nblk):
    """p-block q -> (sub, bi, bj, matrix column)"""
    sub, c = divmod(q, 16)
    bj = 0
    while sub >= blk_sub(bj + 1, bj + 1, nblk) and bj + 1 < nblk:
        bj += 1
    return sub, bj + sub - blk_sub(bj, bj, nblk), bj, 16 * bj + c


def blocked_index(n16, Lr):
    """(idx, w): element (i, j) of constraint row `row` lives at idx[i, j] + 16 * row with weight w[i, j]; idx = -1 where the
    layout holds nothing (sub-blocks above the diagonal)"""
    nblk = n16 // 16
    i, j = np.meshgrid(np.arange(n16), np.arange(n16), indexing="ij")
    bi, bj = i // 16, j // 16
    sub = bj * nblk - bj * (bj - 1) // 2 + (bi - bj)
    assert all(sub[16 * a, 16 * b] == blk_sub(a, b, nblk) for a in range(nblk) for b in range(a + 1))
    idx = ((sub * 16 + j % 16) * Lr) * 16 + i % 16
    return np.where(bi >= bj, idx, -1), np.where(bi == bj, 1.0, RT2)


def blocked_doubles(n16, Lr):
    nblk = n16 // 16
    return nblk * (nblk + 1) // 2 * 16 * Lr * 16


def blocked_pack(dst, At, Lr, row):
    """write the symmetric n16 x n16 matrix At as constraint row `row` into dst (in place)"""
    idx, w = blocked_index(At.shape[0], Lr)
    keep = idx >= 0
    dst[idx[keep] + 16 * row] = (w * At)[keep]


def blocked_unpack(dst, n16, Lr, row):
    """(stored values as an n16 x n16 matrix -- NaN where the layout holds nothing --, their weights)"""
    idx, w = blocked_index(n16, Lr)
    keep = idx >= 0
    out = np.full((n16, n16), np.nan)
    out[keep] = dst[idx[keep] + 16 * row]
    return out, w


# ---- Gram operand ------------------------------------------------------------------------------------------
def gram_index(R, K, Lr, npb_loc):
    i, k = np.meshgrid(np.arange(R), np.arange(K), indexing="ij")
    return ((i // Lr) * npb_loc + k // 16) * Lr * 16 + (i % Lr) * 16 + k % 16


def gram_pack(W, Lr, npb_loc):
    """W: R x K with R = world * Lr, K = 16 npb_loc -> world * npb_loc * Lr * 16 doubles"""
    R, K = W.shape
    assert R % Lr == 0 and K == 16 * npb_loc
    out = np.zeros(R * K)
    out[gram_index(R, K, Lr, npb_loc)] = W
    return out


def gram_unpack(buf, R, Lr, npb_loc):
    return buf[gram_index(R, 16 * npb_loc, Lr, npb_loc)]
