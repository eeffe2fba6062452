"""tests/sparse_schur_cases.py is what tests/test_gpu_sparse_schur.py needs it to be, shown without a GPU:

- the model of the symbolic phase equals the code (HMiBspSymbolic, host only) on every pattern used: order, block rows, tiles,
  levels, dense-tail rows, update source pairs and the factor's block pattern;
- the block pattern is right whatever model and code say: against numpy's Cholesky factor of a diagonally dominant matrix with
  the permuted pattern, every nonzero block of the factor lies in the pattern and every tile of the pattern is a tile of the
  matrix or nonzero in the factor (closed, and nothing superfluous; no tile is left undecided);
- each family has the property the GPU tests use it for -- `filltail` has fill tiles, `band` and `blocks` have one block column
  per level, `arrow` has its five rows in the dense tail and fewer levels than block rows, m = 129 ends in a tile with one
  valid row, a renumbering changes the order;
- the envelope vectors are what set_envelope makes of them, and every family but `dense` has a block outside its row envelope;
- both references stay below 64 u of backward error on every case, and the LDL' finds as many negative pivots as there are
  negative signs: the premise of `e(gpu) <= 8 e(ref) + 16 u`."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_schur_cases as sc  # noqa: E402
import xprec_ref as xp  # noqa: E402

needs_ld = pytest.mark.skipif(not xp.HAVE_LD, reason=xp.NO_LD_REASON)
PATTERNS = sc.all_patterns()
ZERO_PATTERNS = [(f, m, r, rows) for f, m, r, rows, _ in sc.ZERO_PIVOT]


def _sym(family, m, renumbered, isolate=()):
    return sc.model(m, sc.pattern(family, m, renumbered, tuple(isolate)))


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------- model against code

@pytest.mark.parametrize("family,m,renumbered,isolate", [p + ((),) for p in PATTERNS] + ZERO_PATTERNS, ids=_ids)
def test_model_equals_the_symbolic_phase(family, m, renumbered, isolate):
    from hdsdp_amd import api
    pairs = sc.pattern(family, m, renumbered, tuple(isolate))
    s = sc.model(m, pairs)
    beg, idx = sc.lower_csc(m, pairs)
    rc, perm, stats, bptr, brow = api.bsp_symbolic(m, beg, idx, 1.0)
    assert rc == 0
    assert np.array_equal(perm, s.perm)
    assert list(stats) == [s.nb, s.ntiles, s.nlevels, s.tail, s.pairs], (list(stats), s.nb, s.ntiles, s.nlevels, s.tail, s.pairs)
    ptr, row = sc.block_csc(s.P)
    assert list(bptr) == ptr and list(brow) == row


def test_symbolic_phase_refuses_what_init_refuses():
    """one block row (m = 128), and a pattern with more tiles than the fraction allows; stats still say why"""
    from hdsdp_amd import api
    pairs = sc.pattern("band", 128, False)
    beg, idx = sc.lower_csc(128, pairs)
    rc, perm, stats, _, _ = api.bsp_symbolic(128, beg, idx, 1.0)
    assert rc == 1 and perm is None and stats[0] == 1
    pairs = sc.pattern("band", 640, False)
    beg, idx = sc.lower_csc(640, pairs)
    s = sc.model(640, pairs)
    rc, _, stats, _, _ = api.bsp_symbolic(640, beg, idx, 0.5)          # 9 of 15 tiles
    assert s.ntiles == 9 and rc == 1 and stats[1] == 9
    assert api.bsp_symbolic(640, beg, idx, 0.6)[0] == 0


# ---------------------------------------------------------------- the pattern against a factor

@pytest.mark.parametrize("family,m,renumbered", PATTERNS, ids=_ids)
def test_block_pattern_is_closed_and_carries_nothing_superfluous(family, m, renumbered):
    pairs = sc.pattern(family, m, renumbered)
    s = sc.model(m, pairs)
    B = sc.dominant(m, pairs, "pattern check")
    inv = np.argsort(s.perm)
    L = np.linalg.cholesky(B[np.ix_(inv, inv)])
    pad = s.nb * sc.BT - m
    Lp = np.pad(np.abs(L), ((0, pad), (0, pad)))
    big = Lp.reshape(s.nb, sc.BT, s.nb, sc.BT).max(axis=(1, 3))          # largest entry of every block of the factor
    nonzero = np.tril(big > 0.0)
    assert not (nonzero & ~s.P).any(), np.argwhere(nonzero & ~s.P)[:5]     # closed
    fill = s.P & ~s.P0
    # A fill tile with a nonzero entry in the factor is needed.  One that is all zero there would be undecided (superfluous, or
    # needed with every entry cancelled or underflowed): there is none.  (filltail's fill decays along its narrow band -- down
    # to 1e-149 in tile (7, 5) -- but the tile between the two tail tiles, (8, 7), holds entries of ordinary size.)
    undecided = fill & ~nonzero
    assert not undecided.any(), np.argwhere(undecided)[:5]
    if fill.any():
        print(f"    {family} m={m}: {int(fill.sum())} fill tiles, largest factor entry in each between "
              f"{big[fill].min():.3g} and {big[fill].max():.3g}")


# ---------------------------------------------------------------- family properties

def test_filltail_has_tiles_that_exist_only_as_fill():
    s = _sym("filltail", sc.FILLTAIL_M, False)
    assert (s.nb, s.tail) == (9, 140)
    assert (int(s.P0.sum()), s.ntiles) == (22, 30)                          # 8 fill tiles
    fill = s.P & ~s.P0
    assert fill[8, 7] or fill[8, 6]                                         # between the two tail tiles, or just before them
    assert int(fill.sum()) == 8
    print("filltail natural: tiles of the permuted matrix", int(s.P0.sum()), "tiles of the factor", s.ntiles)
    r = _sym("filltail", sc.FILLTAIL_M, True)
    print("filltail renumbered: tiles of the permuted matrix", int(r.P0.sum()), "tiles of the factor", r.ntiles)


@pytest.mark.parametrize("family,m,renumbered", [p for p in PATTERNS if p[0] in ("band", "blocks")], ids=_ids)
def test_band_and_blocks_have_one_block_column_per_level(family, m, renumbered):
    s = _sym(family, m, renumbered)
    assert s.nlevels == s.nb and s.tail == 0


@pytest.mark.parametrize("family,m,renumbered", [p for p in PATTERNS if p[0] == "arrow"], ids=_ids)
def test_arrow_sends_its_five_rows_to_the_tail(family, m, renumbered):
    s = _sym(family, m, renumbered)
    if s.nb >= 4:
        assert s.tail == 5 and s.nlevels < s.nb, (s.tail, s.nlevels, s.nb)
        assert s.ntiles == int(s.P0.sum())                                  # the shaft goes last: no fill


def test_sizes_reach_the_edges():
    assert 129 in sc.SWEEP_M and (129 + 127) // 128 == 2 and 129 - 128 == 1          # a last tile with one valid row
    assert {m % 128 for m in sc.SWEEP_M} >= {0, 1, 127}                                # no padding, one row, one row short
    assert sc.BIG_M["band"] % 128 == 1 and max(sc.BIG_M.values()) <= 1160


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_renumbering_changes_the_order(family):
    m = sc.BIG_M[family]
    assert sc.pattern(family, m, True) != sc.pattern(family, m, False)
    assert not np.array_equal(_sym(family, m, True).perm, _sym(family, m, False).perm)


@pytest.mark.parametrize("family,m,renumbered,rows,what", sc.ZERO_PIVOT, ids=_ids)
def test_zero_pivot_rows_lie_where_the_test_wants_them(family, m, renumbered, rows, what):
    s = _sym(family, m, renumbered, rows)
    p = [int(s.perm[r]) for r in rows]
    tiles = [q // sc.BT for q in p]
    levels = [int(s.level[t]) for t in tiles]
    if what == "same tile":
        assert tiles[0] == tiles[1]
    elif what == "different levels":
        assert levels[0] != levels[1]
    else:
        assert tiles[0] != tiles[1] and levels[0] == levels[1]
    assert p[0] != p[1]


# ---------------------------------------------------------------- envelopes

@pytest.mark.parametrize("nblk", sorted({(n + 127) // 128 for n in sc.ENV_N}))
def test_envelope_vectors(nblk):
    fams = sc.env_families_at(nblk)
    assert "dense" in fams and "diagonal" in fams
    seen = {}
    for f in fams:
        first = sc.env_first(f, nblk)
        c = sc.env_clamp(first)
        assert np.all(c >= 0) and np.all(c <= np.arange(nblk))
        if f == "unclamped":
            assert (first > np.arange(nblk)).sum() == 1 and (first < 0).sum() == 1
            twin = sc.env_first("band1", nblk)
            twin[1], twin[nblk - 2] = 1, 0
            assert np.array_equal(c, twin)
        else:
            assert np.array_equal(c, first)
            assert tuple(c) not in seen, (f, seen.get(tuple(c)))         # every family is a vector of its own at this nblk
            seen[tuple(c)] = f
        if f == "reachback":
            r = nblk // 2
            assert c[r] == c[r + 1] - 2
        # the column heights by their definition (tests/test_kkt_store_cpu.py: envelope_by_definition): block column k runs
        # down to the last block row whose envelope reaches it -- and that never rises from one column to the next
        colh = [max(b for b in range(k, nblk) if c[b] <= k) for k in range(nblk)]
        assert list(sc.env_colh(first)) == colh and all(colh[k] >= colh[k - 1] for k in range(1, nblk))
        outside = [(i, k) for i in range(nblk) for k in range(i) if k < c[i]]
        assert bool(outside) == (f != "dense"), f


@pytest.mark.parametrize("family,n,cond,grade", sc.env_cases(), ids=_ids)
def test_envelope_matrices_are_zero_outside_and_full_inside(family, n, cond, grade):
    c = sc.env_case(family, n, cond, grade)
    assert np.array_equal(c.A, c.A.T)
    low = np.tril(np.ones((n, n), dtype=bool))
    assert not c.A[low & ~c.inside].any()                                    # exactly 0.0 outside
    assert np.all(c.A[c.inside] != 0.0)                                      # dense inside
    br, bc = np.nonzero(np.tril(c.A))
    first = [int(np.min(bc[br // 128 == i]) // 128) for i in range(c.nblk)]
    assert first == list(c.clamped)


@needs_ld
@pytest.mark.parametrize("family,n,cond,grade", sc.env_cases(), ids=_ids)
def test_envelope_reference_is_below_the_cap(family, n, cond, grade):
    e, ef = sc.env_reference(family, n, cond, grade)
    print(f"    envelope {family} n={n} cond={cond:g} {grade}: e(scipy) = {e / sc.U:.2f} u, factor error {ef / sc.U:.2f} u")
    assert e <= sc.CAP


@pytest.mark.parametrize("n,row", [(600, 300), (600, 599), (600, 128), (257, 256), (1153, 1152)])
def test_not_positive_definite_cases_stop_where_they_should(n, row):
    nblk = (n + 127) // 128
    first = sc.env_first("band1" if nblk >= 3 else "dense", nblk)
    S = sc.not_pd(n, row, first)
    assert not np.tril(S)[~sc.env_mask(first, n) & np.tril(np.ones((n, n), dtype=bool))].any()
    _, info = sl.lapack.dpotrf(S, lower=1)
    assert info == row + 1


def test_the_recorded_report_covers_every_group_and_keeps_the_rule():
    """tests/golden/sparse_schur_report.txt: the SPARSE_REPORT lines of one run of tests/test_gpu_sparse_schur.py on an MI355X --
    a line for every group, each within the rule it was recorded under"""
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_schur_report.txt")
    rows = [json.loads(line.split(" ", 1)[1]) for line in open(path) if line.startswith("SPARSE_REPORT ")]
    groups = {r["group"] for r in rows}
    want = {f"tile sweep {f}" for f in sc.SWEEP_FAMILIES} | {f"tile conditioning {f} {o}" for f in sc.FAMILIES for o in ("natural", "renumbered")}
    want |= {f"tile filltail reuse {k}" for k in ("spd", "qd")} | {f"tile after a zero pivot {z[0]}" for z in sc.ZERO_PIVOT}
    want |= {f"envelope per-block substitution n={n}" for n in sc.ENV_N} | {"operators", "tile after a refusal"}
    assert want <= groups, sorted(want - groups)
    for n in sc.ENV_N:
        for kind in ("solve", "factor"):
            got = sum(r["cases"] for r in rows if r["group"].startswith(f"envelope {kind} n={n} "))
            assert got == len([c for c in sc.env_cases() if c[1] == n]), (n, kind, got)
    for r in rows:
        assert r["cases"] >= 1 and r["e_gpu_u"] <= 8.0 * r["e_ref_u"] + 16.0, r
        assert 0.0 <= r["worst_ratio"] <= 8.0 + 1.0, r                   # (e / max(e_ref, 16 u) <= 8 + 1 under the rule)


# ---------------------------------------------------------------- the references

def _tile_cases():
    out = [(f, m, r, "spd", 1e6, g) for f, m, r, g in sc.sweep_cases()]
    for f in sc.FAMILIES:
        out += [(f,) + c for c in sc.big_cases(f)]
    return out


@needs_ld
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_tile_references_are_below_the_cap(family):
    worst = {"spd": 0.0, "qd": 0.0}
    for f, m, r, kind, cond, grade in _tile_cases():
        if f != family:
            continue
        c = sc.tile_case(f, m, r, kind, cond, grade)
        assert np.array_equal(c.A, c.A.T)
        e, nneg = sc.tile_reference(f, m, r, kind, cond, grade)
        worst[kind] = max(worst[kind], e)
        assert e <= sc.CAP, (f, m, r, kind, cond, grade, e / sc.U)
        if kind == "qd":
            assert nneg == int(np.sum(c.s < 0)) and 0.2 * m < nneg < 0.45 * m
    print(f"    {family}: worst e(Cholesky) = {worst['spd'] / sc.U:.2f} u, worst e(LDL') = {worst['qd'] / sc.U:.2f} u")


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_quasi_definite_inertia(family):
    """cond 1e2: the eigenvalues are clear of zero, and as many are negative as there are negative signs"""
    m = sc.BIG_M[family]
    c = sc.tile_case(family, m, False, "qd", 1e2, "down")
    w = np.linalg.eigvalsh(c.A)
    assert np.min(np.abs(w)) > 1e-6 * np.max(np.abs(w))
    assert int(np.sum(w < 0)) == int(np.sum(c.s < 0))
