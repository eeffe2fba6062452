"""Every role kernel of the fp64 MFMA GEMM family against an extended-precision product, one launch form at a time.

Each case packs random operands with the numpy model of the storage formats (tests/gemm_layouts.py, held to the headers by
tests/test_gemm_layouts_cpu.py), runs ONE call form of csrc/gemm_calls.h through its test entry (csrc/probes.hip: HMiCongStep1,
HMiCongStep2, HMiCongIRow, HMiGramSplits, HMiGramGathered, HMiGramLp), unpacks the result and compares EVERY element with
xprec_ref.mm of the same fp64 operands.

Tolerance (derived, not measured): |got - ref|_ij <= (K + 4) 2^-53 (|A| |B|^T)_ij, K the number of k values the launch sums for
that element -- the classical bound gamma_K of a length-K inner product in any summation order, with four units to spare for
alpha, beta and the reference's own rounding to fp64.  Step 2 sums both of its products (K counts both) and takes one more
rounding for the sqrt(2) scale: (K + 5).  An accumulating launch (beta = 1) adds |C| to the absolute-value product.  The
absolute-value product is a plain fp64 product.  Where the bound is zero (padding rows) the result must be exactly zero.

Sentinels: every destination is pre-filled with a NaN that carries a payload, and every element the form does not own must
hold those bits afterwards.  Operand memory past the matrix but inside the span the form vouches for -- what the unmasked tile
loads read and throw away -- is NaN, as are the tiles of Linv and T above the diagonal and the source matrices a launch does not
name: the output must be finite and right all the same.

Can hdm_work_plan produce an empty K split (k_base + z k_chunk beyond K)?  Yes.  Enumerating HMiWorkPlanQuery on the CPU over
n = 16 .. 4096, world 1, 2, 3, 8: on one device never without a knob, and never under HDM_GRAM_KSTAGES; a sharded block does by
default (n = 928, world = 2: 144 splits of 96 p-blocks over 13688 leave split 143 empty), and so does HDM_NSPLIT on one device
(n = 112, HDM_NSPLIT=26: 26 splits of 18 p-blocks over 448).  GRAM_SPLITS therefore holds a range of splits whose last four are
empty: their slabs must come out as zeros (or unchanged when accumulating)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gemm_layouts as gl  # noqa: E402
import xprec_ref as xr  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xr.HAVE_LD, reason=xr.NO_LD_REASON)]

U = 2.0 ** -53
LD = np.longdouble
TILE = 128
SENT_BITS = np.uint64(0x7FF85EED0BADC0DE)     # a quiet NaN with a payload: no kernel produces it

# ---- the cases (tests/test_gemm_layouts_cpu.py reads these lists for its coverage table) ------------------------------------
# (n16, n): 16 with n = 5 (padding inside a sub-block), 64 .. 112 (one short diagonal tile, RV 4 .. 7), 128 (one full diagonal
# tile: step 2's P + P^T tile alone), 144 .. 240 (edge and short diagonal tiles at rv 1 .. 7 beside a full diagonal tile), 464
# (step 1's main tile (2, 0) with a middle K block; rv 5)
CONG_SIZES = [(16, 5)] + [(s, s) for s in (64, 80, 96, 112, 128)] + [(s, s) for s in range(144, 241, 16)] + [(464, 464)]
# 1, 7: one tile per workgroup, z = wg % nb; 8: persistent; 9: persistent, the grid padded to 16
CONG_BATCHES = (1, 7, 8, 9)
MASK_N16 = 272
MASKS = (0b001, 0b010, 0b100, 0b101)
GRAM_N16 = 48                                 # npb = 96, K = 1536
# rows R = Lr on one device: half-valid sub-tile rows (R = 8 mod 16), short diagonal tiles of RV 4 .. 7 (8, 24, 72, 88, 104), a
# full diagonal tile with a half-valid last row (120), edge tiles of RV 4 .. 7 (136, 200, 216, 232, 264), main tiles (264)
GRAM_ROWS = (8, 24, 72, 88, 104, 120, 128, 136, 200, 216, 232, 264)
# (nsplit, z0, nz) over npb_loc = 96 p-blocks: 3 x 32 stages (one tile per workgroup); 3 stages each -- an odd count, closed by
# the zero stage -- from split 5 on (k_base > 0); 7 x 14 with a last split of 12; 8 x 12 (persistent); 11 x 9 (odd) with a last
# split of 6, the grid padded to 16; 16 x 6 (persistent); 36 x 3: splits 30, 31 and the four EMPTY splits 32 .. 35
GRAM_SPLITS = ((3, 0, 3), (32, 5, 3), (7, 0, 7), (8, 0, 8), (11, 0, 11), (16, 0, 16), (36, 30, 6))
# (world, maxloc, splits): Lr = 128; world 2: R = 256, 48 p-blocks per rank; world 3: R = 384, 32 p-blocks per rank
GRAM_SHARDED = ((2, 100, ((3, 0, 3), (5, 0, 5), (8, 0, 8))), (3, 125, ((3, 0, 3), (8, 0, 8), (16, 4, 9))))

RATIOS = {}          # role -> worst error / bound seen in this process (printed case by case)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def _lib():
    from hdsdp_amd import api
    return api.load_library()


def _span(which, n16=16, world=1, maxloc=0, a0=0, a1=0):
    from hdsdp_amd import api
    return api.gemm_role_span(which, n16, world, maxloc, a0, a1)


def _up(a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    return torch.from_numpy(a).cuda()


def _down(t):
    return t.cpu().numpy()


def _ptr(t, off=0):
    return t.data_ptr() + 8 * off


def sentinels(k):
    return np.full(k, SENT_BITS, dtype=np.uint64).view(np.float64)


def is_sent(a):
    return np.ascontiguousarray(a).view(np.uint64) == SENT_BITS


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def hold(role, what, got, ref, bound, mask, blocked=False):
    """every element of got[mask] within bound of ref (longdouble), finite; records and returns the worst error / bound"""
    assert np.all(np.isfinite(got[mask])), f"{what}: {np.count_nonzero(~np.isfinite(got[mask]))} owned elements are not finite"
    err = np.abs(got.astype(LD) - ref)
    bad = mask & ~(err <= bound)
    if np.any(bad):
        i, j = np.nonzero(bad)
        worst = np.argmax((err[bad] / np.maximum(bound[bad], np.finfo(float).tiny)).astype(np.float64))
        where = f"tiles {sorted(set(zip((i // TILE).tolist(), (j // TILE).tolist())))[:6]}"
        if blocked:
            off = np.count_nonzero(i // 16 != j // 16)
            where += (f"; {off} in off-diagonal sub-blocks, {i.size - off} in diagonal sub-blocks; sub-blocks "
                      f"{sorted(set(zip((i // 16).tolist(), (j // 16).tolist())))[:6]}")
        raise AssertionError(f"{what}: {i.size} of {np.count_nonzero(mask)} elements beyond the bound, worst at ({i[worst]}, {j[worst]}): got "
                             f"{got[i[worst], j[worst]]!r}, reference {float(ref[i[worst], j[worst]])!r}, bound {bound[i[worst], j[worst]]:.3e}; {where}")
    pos = mask & (bound > 0)
    ratio = float(np.max(err[pos] / bound[pos])) if np.any(pos) else 0.0
    RATIOS[role] = max(RATIOS.get(role, 0.0), ratio)
    return ratio


def _ij(n):
    return np.meshgrid(np.arange(n), np.arange(n), indexing="ij")


# ---- congruence ---------------------------------------------------------------------------------------------------------------
class CongOperands:
    """Linv (npad x npad, lower triangular, NaN in the tiles above the diagonal and past n16), nb skyline matrices from b0 on in a
    source buffer of src_rows (the others NaN), host-made intermediates T, and the sizes of everything"""

    def __init__(self, n16, n, nb, seed=0):
        rng = np.random.default_rng(100000 * seed + 1000 * n16 + nb)
        self.n16, self.n, self.nb = n16, n, nb
        self.maxloc = nb + 6
        self.L = gl.layout(n16, 1, self.maxloc)
        self.Lr, self.row0 = self.L["Lr"], 3
        assert self.Lr > nb and self.row0 + nb <= self.Lr
        self.npad = gl.roundup(n16, TILE)
        self.b0, self.src_rows, self.Bc = 1, nb + 2, nb + 1
        i, j = _ij(n16)
        self.same_tile_upper = (i < j) & (i // TILE == j // TILE)
        self.above = i // TILE < j // TILE
        pad = lambda X: np.pad(X, ((0, n16 - n), (0, n16 - n)))                          # noqa: E731
        self.Linv = pad(np.tril(rng.standard_normal((n, n))))
        lin = np.full((self.npad, self.npad), np.nan)                                  # [k][i]: column-major
        lin[:n16, :n16] = np.where(self.above, np.nan, self.Linv).T
        self.linv_buf = lin.reshape(-1)
        self.AL = [pad(np.tril(rng.standard_normal((n, n)))) for _ in range(nb)]
        ast = self.L["astride"]
        self.asrc_buf = np.full(_span(2, n16, 1, self.maxloc, self.src_rows), np.nan)
        for z in range(nb):
            self.asrc_buf[(self.b0 + z) * ast:(self.b0 + z + 1) * ast] = gl.sky_pack(self.AL[z])
        self.t_len = _span(0, n16, 1, self.maxloc, self.Bc)
        self.That = [np.tril(rng.standard_normal((n16, n16))) for _ in range(nb)]
        self.t_host = np.full(self.t_len, np.nan)
        for z in range(nb):
            self.t_host[z * n16 * n16:(z + 1) * n16 * n16] = np.where(self.above, np.nan, self.That[z]).T.reshape(-1)
        # step 1's destination: zeros where step 2 reads what step 1 does not write (the strict upper triangle of the diagonal
        # tiles: the engine's contract), the sentinel everywhere else
        self.t_pre = sentinels(self.t_len)
        for z in range(nb):
            self.t_pre[z * n16 * n16:(z + 1) * n16 * n16][self.same_tile_upper.T.reshape(-1)] = 0.0
        self.dst_len = gl.blocked_doubles(n16, self.Lr)
        self.k1 = np.minimum(n16, (i // TILE + 1) * TILE) - (j // TILE) * TILE           # step 1: k in [128 tn, 128 (tm + 1))
        self.k2 = np.minimum(n16, (j // TILE + 1) * TILE)                                # step 2, I row: k < 128 (tn + 1), per product

    def tmat(self, buf, z):
        n16 = self.n16
        return buf[z * n16 * n16:(z + 1) * n16 * n16].reshape(n16, n16).T


def run_step1(op, dLinv, dA):
    dT = _up(op.t_pre)
    rc = _lib().HMiCongStep1(op.n, 1, op.maxloc, _ptr(dLinv), dLinv.numel(), op.npad, _ptr(dA), dA.numel(), op.src_rows, op.b0, op.nb, _ptr(dT),
                             dT.numel())
    assert rc == 0
    return dT


def run_step2(op, dLinv, dT, colmask=0):
    dD = _up(sentinels(op.dst_len))
    rc = _lib().HMiCongStep2(op.n, 1, op.maxloc, op.Bc, _ptr(dLinv), dLinv.numel(), op.npad, _ptr(dT), dT.numel(), op.nb, _ptr(dD), dD.numel(),
                             op.row0, colmask)
    assert rc == 0
    return _down(dD)


def run_irow(op, dLinv):
    dD = _up(sentinels(op.dst_len))
    assert _lib().HMiCongIRow(op.n, 1, op.maxloc, _ptr(dLinv), dLinv.numel(), op.npad, _ptr(dD), dD.numel(), op.row0) == 0
    return _down(dD)


def check_step1(op, T, tag):
    n16, lower = op.n16, ~(op.same_tile_upper | op.above)
    worst = 0.0
    for z in range(op.nb):
        Tz = op.tmat(T, z)
        ref, ab = xr.mm(op.Linv, op.AL[z]), np.abs(op.Linv) @ np.abs(op.AL[z])
        worst = max(worst, hold("step 1", f"{tag} step 1 matrix {z}", Tz, ref, (op.k1 + 4) * U * ab, lower))
        assert np.all(Tz[op.same_tile_upper] == 0.0), f"{tag} step 1 matrix {z}: wrote above the diagonal of a diagonal tile"
        assert np.all(is_sent(Tz)[op.above]), f"{tag} step 1 matrix {z}: wrote a tile above the diagonal"
    assert np.all(is_sent(T[op.nb * n16 * n16:])), f"{tag} step 1: wrote past its {op.nb} matrices"
    return worst


def check_blocked(op, dst, refs, kmat, role, tag, colmask=0):
    """refs: constraint row -> (symmetric reference in longdouble, its absolute-value product): every owned element within the
    bound, everything else still the sentinel"""
    n16 = op.n16
    idx, w = gl.blocked_index(n16, op.Lr)
    _, j = _ij(n16)
    keep = idx >= 0
    if colmask:
        keep = keep & (((colmask >> (j // TILE)) & 1) == 1)
    owned = np.zeros(dst.size, dtype=bool)
    worst = 0.0
    for row, (ref, ab) in refs.items():
        got, _ = gl.blocked_unpack(dst, n16, op.Lr, row)
        worst = max(worst, hold(role, f"{tag} {role} constraint row {row}", got, w.astype(LD) * ref, (kmat + 5) * U * w * ab, keep, blocked=True))
        owned[idx[keep] + 16 * row] = True
    stray = ~owned & ~is_sent(dst)
    assert not np.any(stray), f"{tag} {role}: {np.count_nonzero(stray)} elements outside the launch's rows / columns were written"
    return worst


def step2_refs(op, Ts):
    refs = {}
    for z, Tz in enumerate(Ts):
        P, ab = xr.mm(Tz, op.Linv.T), np.abs(Tz) @ np.abs(op.Linv).T
        refs[op.row0 + z] = (P + P.T, ab + ab.T)
    return refs


def cong_case(n16, n, nb, check=True):
    """step 1, step 2 on a host-made T, step 2 chained on step 1's own output, the I row; returns the outputs"""
    op = CongOperands(n16, n, nb)
    tag = f"n16={n16} nb={nb}"
    dLinv, dA = _up(op.linv_buf), _up(op.asrc_buf)
    dT = run_step1(op, dLinv, dA)
    T = _down(dT)
    s2h = run_step2(op, dLinv, _up(op.t_host))
    s2c = run_step2(op, dLinv, dT)
    ir = run_irow(op, dLinv)
    if check:
        r1 = check_step1(op, T, tag)
        r2h = check_blocked(op, s2h, step2_refs(op, op.That), 2 * op.k2, "step 2", tag + " host-made T")
        r2c = check_blocked(op, s2c, step2_refs(op, [np.tril(op.tmat(T, z)) for z in range(nb)]), 2 * op.k2, "step 2", tag + " chained")
        ri = check_blocked(op, ir, {op.row0: (xr.mm(op.Linv, op.Linv.T), np.abs(op.Linv) @ np.abs(op.Linv).T)}, op.k2, "I row", tag)
        print(f"\ngemm roles {tag}: error / bound  step 1 {r1:.3f}  step 2 (host-made T) {r2h:.3f}  step 2 (chained) {r2c:.3f}  I row {ri:.3f}")
    return {"T": T, "step2_host": s2h, "step2_chained": s2c, "irow": ir}


@pytest.mark.parametrize("nb", CONG_BATCHES)
@pytest.mark.parametrize("n16,n", CONG_SIZES)
def test_congruence_forms_against_the_extended_precision_product(n16, n, nb):
    cong_case(n16, n, nb)


def test_congruence_step2_column_masks():
    """n16 = 272, three tile columns: a masked launch writes the sub-blocks of its columns only, to the bound, and the three
    single-column launches together are the unmasked launch bit for bit"""
    op = CongOperands(MASK_N16, MASK_N16, 2, seed=1)
    dLinv, dT = _up(op.linv_buf), _up(op.t_host)
    refs = step2_refs(op, op.That)
    full = run_step2(op, dLinv, dT)
    check_blocked(op, full, refs, 2 * op.k2, "step 2", "n16=272 unmasked")
    single = {}
    for mask in MASKS:
        out = run_step2(op, dLinv, dT, mask)
        r = check_blocked(op, out, refs, 2 * op.k2, "step 2", f"n16=272 mask {mask:03b}", colmask=mask)
        print(f"\ngemm roles n16=272 mask {mask:03b}: error / bound {r:.3f}")
        single[mask] = out
    merged = sentinels(op.dst_len)
    for mask in (0b001, 0b010, 0b100):
        wrote = ~is_sent(single[mask])
        assert not np.any(wrote & ~is_sent(merged)), "two single-column launches wrote the same element"
        merged[wrote] = single[mask][wrote]
    assert digest(merged) == digest(full), "the three single-column launches differ from the unmasked launch"
    both = np.where(is_sent(single[0b001]), single[0b100], single[0b001])
    assert digest(both) == digest(single[0b101]), "mask 101 differs from the launches of its two columns"


# ---- Gram ---------------------------------------------------------------------------------------------------------------------
def run_gram(L, world, maxloc, dW, slabs, nsplit, z0, nz, accumulate=0, queue_global=1, slab_off=0):
    dS = slabs if hasattr(slabs, "data_ptr") else _up(slabs)
    rc = _lib().HMiGramSplits(GRAM_N16, world, maxloc, maxloc, nsplit, z0, nz, _ptr(dW), dW.numel(), _ptr(dS, slab_off), dS.numel() - slab_off,
                              accumulate, queue_global)
    assert rc == 0
    return dS


def split_range(K, chunk, z):
    """the k range of K split z: [z chunk, (z + 1) chunk) cut at K (empty beyond it)"""
    k0 = min(K, z * chunk)
    return k0, min(K, k0 + chunk)


def gram_case(world, maxloc, splits, check=True):
    """the K splits of `splits` on one operand of R = world * Lr rows in segment order: overwrite, accumulate, per-XCD queues,
    two sub-ranges; returns the overwrite launches' slabs"""
    L = gl.layout(GRAM_N16, world, maxloc)
    R, Lr, kb = L["R"], L["Lr"], L["npb_loc"]
    K = 16 * kb
    rng = np.random.default_rng(7000 + 10 * R + world)
    buf = np.full(_span(3, GRAM_N16, world, maxloc), np.nan)
    buf[:R * K] = gl.gram_pack(rng.standard_normal((R, K)), Lr, kb)
    W = gl.gram_unpack(buf, R, Lr, kb)                   # the reference reads the rows back out of the packed operand
    dW = _up(buf)
    i, j = _ij(R)
    lower = i >= j
    outs = {}
    for nsplit, z0, nz in splits:
        tag = f"R={R} world={world} splits [{z0}, {z0 + nz}) of {nsplit}"
        chunk = -(-kb // nsplit) * 16
        pre = sentinels((nz + 1) * R * R)
        out = _down(run_gram(L, world, maxloc, dW, pre, nsplit, z0, nz))
        outs[(nsplit, z0, nz)] = out
        # accumulate onto preset slabs (lower triangles; the rest stays the sentinel)
        preset = rng.standard_normal((nz, R, R))
        acc0 = pre.copy()
        for z in range(nz):
            acc0[z * R * R:(z + 1) * R * R] = np.where(lower, preset[z], acc0[z * R * R:(z + 1) * R * R].reshape(R, R).T).T.reshape(-1)
        acc = _down(run_gram(L, world, maxloc, dW, acc0, nsplit, z0, nz, accumulate=1))
        # one queue per XCD; two sub-ranges (z0 > 0, k_base > 0, the second into its own first slab)
        assert digest(_down(run_gram(L, world, maxloc, dW, pre, nsplit, z0, nz, queue_global=0))) == digest(out), f"{tag}: per-XCD queues give other bits"
        za = max(1, nz // 2)
        d2 = run_gram(L, world, maxloc, dW, pre, nsplit, z0, za)
        if nz > za:
            run_gram(L, world, maxloc, dW, d2, nsplit, z0 + za, nz - za, slab_off=za * R * R)
        assert digest(_down(d2)) == digest(out), f"{tag}: two sub-range launches give other bits"
        if not check:
            continue
        worst = worst_acc = 0.0
        for z in range(nz):
            k0, k1 = split_range(K, chunk, z0 + z)
            Wz = W[:, k0:k1]
            ref = xr.mm(Wz, Wz.T) if k1 > k0 else np.zeros((R, R), dtype=LD)
            ab = np.abs(Wz) @ np.abs(Wz).T
            Sz = out[z * R * R:(z + 1) * R * R].reshape(R, R).T
            worst = max(worst, hold("Gram", f"{tag} slab {z}", Sz, ref, (k1 - k0 + 4) * U * ab, lower))
            assert np.all(is_sent(Sz)[~lower]), f"{tag} slab {z}: wrote above the diagonal"
            Az = acc[z * R * R:(z + 1) * R * R].reshape(R, R).T
            worst_acc = max(worst_acc, hold("Gram accumulate", f"{tag} slab {z} accumulating", Az, ref + preset[z].astype(LD),
                                            (k1 - k0 + 4) * U * (ab + np.abs(preset[z])), lower))
            assert np.all(is_sent(Az)[~lower]), f"{tag} slab {z} accumulating: wrote above the diagonal"
        assert np.all(is_sent(out[nz * R * R:])) and np.all(is_sent(acc[nz * R * R:])), f"{tag}: wrote a slab past the launch's splits"
        print(f"\ngemm roles Gram {tag}: error / bound {worst:.3f}, accumulating {worst_acc:.3f}")
    return outs


@pytest.mark.parametrize("split", GRAM_SPLITS, ids=lambda s: "%dof%dfrom%d" % (s[2], s[0], s[1]))
@pytest.mark.parametrize("R", GRAM_ROWS)
def test_gram_splits_against_the_extended_precision_product(R, split):
    gram_case(1, R - 3, (split,))


@pytest.mark.parametrize("world,maxloc,split", [(w, ml, s) for w, ml, sp in GRAM_SHARDED for s in sp])
def test_gram_splits_of_a_sharded_operand_on_one_device(world, maxloc, split):
    """the row-segmented operand (seg_rows, seg_extra): rows in segment order, one segment per source rank"""
    gram_case(world, maxloc, (split,))


@pytest.mark.parametrize("accumulate", (0, 1))
def test_gram_gathered_form(accumulate):
    """the signed route's gathered product: nc = 70 columns (nc16 = 80, no multiple of the 32-deep splits), R = 136, alpha = -1"""
    R, nc, nz, alpha = 136, 70, 3, -1.0
    nc16 = gl.roundup(nc, 16)
    rng = np.random.default_rng(81 + accumulate)
    Wp = np.zeros((R, nc16))
    Wp[:, :nc] = rng.standard_normal((R, nc))
    buf = np.full(nc16 * R + 8192, np.nan)
    buf[:nc16 * R] = gl.gram_pack(Wp, R, nc16 // 16)
    i, j = _ij(R)
    lower = i >= j
    pre = sentinels((nz + 1) * R * R)
    preset = rng.standard_normal((nz, R, R))
    if accumulate:
        for z in range(nz):
            pre[z * R * R:(z + 1) * R * R] = np.where(lower, preset[z], pre[z * R * R:(z + 1) * R * R].reshape(R, R).T).T.reshape(-1)
    dG, dS = _up(buf), _up(pre)
    assert _lib().HMiGramGathered(R, nc, nz, alpha, accumulate, _ptr(dG), dG.numel(), _ptr(dS), dS.numel(), 1) == 0
    out = _down(dS)
    chunk = -(-(nc16 // 16) // nz) * 16
    worst = 0.0
    for z in range(nz):
        Wz = Wp[:, z * chunk:min(nc16, (z + 1) * chunk)]
        ref, ab = alpha * xr.mm(Wz, Wz.T), np.abs(Wz) @ np.abs(Wz).T
        if accumulate:
            ref, ab = ref + preset[z].astype(LD), ab + np.abs(preset[z])
        Sz = out[z * R * R:(z + 1) * R * R].reshape(R, R).T
        worst = max(worst, hold("Gram gathered", f"gathered slab {z}", Sz, ref, (Wz.shape[1] + 4) * U * ab, lower))
        assert np.all(is_sent(Sz)[~lower])
    assert np.all(is_sent(out[nz * R * R:]))
    print(f"\ngemm roles Gram gathered accumulate={accumulate}: error / bound {worst:.3f}")


def test_gram_lp_form():
    """the LP cone's product: STORE epilogue, beta = 1 into the lower triangle of an ldm > m16 matrix, kv < kp < kc; everything
    outside the lower triangle of the leading m16 x m16 keeps its bits"""
    m, mpad, kc, kv, ldm = 70, 128, 64, 37, 100
    m16, kp = gl.roundup(m, 16), gl.roundup(kv, 16)
    rng = np.random.default_rng(91)
    Wp = np.zeros((m16, kp))
    Wp[:m, :kv] = rng.standard_normal((m, kv))
    buf = np.full(_span(4, a0=kc, a1=mpad), np.nan)
    rows = np.full((mpad, kp), np.nan)                 # rows m16 .. mpad - 1 are read and thrown away
    rows[:m16] = Wp
    buf[:(kp // 16) * mpad * 16] = gl.gram_pack(rows, mpad, kp // 16)
    i, j = _ij(ldm)
    lower = (i >= j) & (i < m16)
    preset = rng.standard_normal((ldm, ldm))
    M0 = np.where(lower, preset, sentinels(ldm * ldm).reshape(ldm, ldm))
    dW, dM = _up(buf), _up(M0.T.reshape(-1))
    assert _lib().HMiGramLp(m, mpad, kc, kv, _ptr(dW), dW.numel(), _ptr(dM), dM.numel(), ldm) == 0
    got = _down(dM).reshape(ldm, ldm).T
    ref = np.zeros((ldm, ldm), dtype=LD)
    ab = np.zeros((ldm, ldm))
    ref[:m16, :m16], ab[:m16, :m16] = xr.mm(Wp, Wp.T), np.abs(Wp) @ np.abs(Wp).T
    r = hold("Gram LP", "LP product", got, ref + np.where(lower, preset, 0.0).astype(LD), (kp + 4) * U * (ab + np.abs(np.where(lower, preset, 0.0))), lower)
    assert np.all(is_sent(got)[~lower]), "the LP product wrote outside the lower triangle of the leading m16 x m16"
    print(f"\ngemm roles Gram LP: error / bound {r:.3f}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_buffers_smaller_than_their_forms_need():
    """one double short on each buffer in turn: the entry returns 1 and the destination keeps its bits"""
    op = CongOperands(144, 144, 2)
    lib = _lib()
    dLinv, dA, dT, dD = _up(op.linv_buf), _up(op.asrc_buf), _up(sentinels(op.t_len)), _up(sentinels(op.dst_len))
    s1 = lambda ll, al, tl, b0=op.b0: lib.HMiCongStep1(op.n, 1, op.maxloc, _ptr(dLinv), ll, op.npad, _ptr(dA), al, op.src_rows, b0, op.nb, _ptr(dT), tl)   # noqa: E731
    assert s1(dLinv.numel() - 1, dA.numel(), dT.numel()) == 1 and s1(dLinv.numel(), dA.numel() - 1, dT.numel()) == 1
    assert s1(dLinv.numel(), dA.numel(), op.nb * op.n16 * op.n16 - 1) == 1 and s1(dLinv.numel(), dA.numel(), dT.numel(), b0=op.src_rows - 1) == 1
    s2 = lambda ll, tl, dl, r0=op.row0: lib.HMiCongStep2(op.n, 1, op.maxloc, op.Bc, _ptr(dLinv), ll, op.npad, _ptr(dT), tl, op.nb, _ptr(dD), dl, r0, 0)   # noqa: E731
    assert s2(dLinv.numel() - 1, dT.numel(), dD.numel()) == 1 and s2(dLinv.numel(), dT.numel() - 1, dD.numel()) == 1
    assert s2(dLinv.numel(), dT.numel(), dD.numel() - 1) == 1 and s2(dLinv.numel(), dT.numel(), dD.numel(), r0=op.Lr - 1) == 1
    assert lib.HMiCongIRow(op.n, 1, op.maxloc, _ptr(dLinv), dLinv.numel(), op.npad, _ptr(dD), dD.numel() - 1, 0) == 1
    assert lib.HMiCongIRow(op.n, 1, op.maxloc, _ptr(dLinv), dLinv.numel(), op.npad, _ptr(dD), dD.numel(), op.Lr) == 1
    L = gl.layout(GRAM_N16, 1, 21)
    dW, dS = _up(np.zeros(_span(3, GRAM_N16, 1, 21))), _up(sentinels(3 * L["R"] ** 2))
    gs = lambda wl, sl, nz=3: lib.HMiGramSplits(GRAM_N16, 1, 21, 21, 3, 0, nz, _ptr(dW), wl, _ptr(dS), sl, 0, 1)   # noqa: E731
    assert gs(dW.numel() - 1, dS.numel()) == 1 and gs(dW.numel(), dS.numel() - 1) == 1 and gs(dW.numel(), dS.numel(), nz=4) == 1
    assert lib.HMiGramGathered(24, 20, 3, 1.0, 0, _ptr(dW), 32 * 24 - 1, _ptr(dS), dS.numel(), 1) == 1
    assert lib.HMiGramGathered(24, 20, 4, 1.0, 0, _ptr(dW), dW.numel(), _ptr(dS), dS.numel(), 1) == 1
    dM = _up(sentinels(100 * 100))
    assert lib.HMiGramLp(70, 128, 64, 37, _ptr(dW), _span(4, a0=64, a1=128) - 1, _ptr(dM), dM.numel(), 100) == 1
    assert lib.HMiGramLp(70, 128, 64, 37, _ptr(dW), dW.numel(), _ptr(dM), 79 * 100 + 80 - 1, 100) == 1
    for t in (dT, dD, dS, dM):
        assert np.all(is_sent(_down(t))), "a refused entry wrote to its destination"


# ---- launch form ----------------------------------------------------------------------------------------------------------------
def launch_form_hashes():
    """the outputs' hashes of the batch-9 congruence cases and of the nz = 16 Gram case (tests/gemm_roles_worker.py prints them
    from a process of its own)"""
    out = {}
    for n16, n in CONG_SIZES:
        out[f"cong {n16}"] = {k: digest(v) for k, v in cong_case(n16, n, 9, check=False).items()}
    out["gram"] = {str(k): digest(v) for k, v in gram_case(1, GRAM_ROWS[-1] - 3, ((16, 0, 16),), check=False).items()}
    return out


def test_one_tile_per_workgroup_and_persistent_forms_give_the_same_bits():
    """HDM_PERSIST is read once per process: a child process runs the batch-9 congruence cases and the nz = 16 Gram case with one
    workgroup per tile; this process ran them in the default (persistent) form"""
    here = launch_form_hashes()
    env = {k: v for k, v in os.environ.items() if not k.startswith("HDM_")}
    env["HDM_PERSIST"] = "0"
    r = subprocess.run([sys.executable, os.path.join(HERE, "gemm_roles_worker.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("GEMM_ROLES_WORKER_JSON ")]
    assert line, (r.stdout + r.stderr)[-2000:]
    there = json.loads(line[-1][len("GEMM_ROLES_WORKER_JSON "):])
    assert sorted(there) == sorted(here)
    for case in here:
        assert there[case] == here[case], f"{case}: HDM_PERSIST=0 gives other bits than the default form"
