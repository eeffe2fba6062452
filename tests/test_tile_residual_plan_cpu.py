"""The work list of the tile form's twice-precision residual (csrc/tile_residual_plan.h) and the tile rows of the refined solve's
state rule (csrc/kkt_store.h: hdm_kkt_refine_source), without a device: the two headers are compiled alone with the host C++
compiler beside tests/tile_residual_plan_driver.cpp.

Patterns: sparse_schur_cases.pattern through HMiBspSymbolic (host code) -- band and arrow, natural and renumbered, at m = 129, 193,
257, 385 (a last tile with one valid row, a last quadrant with one valid row, an absent tile, three block rows), and filltail at
1040 (tiles that exist only as fill).  The expectations are written here from the plan's description:
one job per stored 64 x 64 quadrant below m in (tile, quadrant) order, two uses per job, one slot per use, the slots of a 64-row
block listed by (tile, quadrant, direct before transposed)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import sparse_schur_cases as sc  # noqa: E402

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

OFF, CONVERGED, STAGNATED, MAXSTEPS, NUMERICAL, NO_MATRIX, NOT_AVAILABLE = range(7)
MAT_NONE, MAT_DEVICE, MAT_COPY, MAT_TILES_M, MAT_TILES_COPY = range(5)
DENSE, CSC, TILES = range(3)

CASES = [(f, m, r) for f in ("band", "arrow") for m in (129, 193, 257, 385) for r in (False, True)] + [("filltail", 1040, False)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_residual_plan") / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "tile_residual_plan_driver.cpp")])
    return exe


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [row.split() for row in out.splitlines()]


def test_the_plan_header_compiles_alone(tmp_path):
    """host arithmetic only: tile_residual_plan.h by itself is a translation unit, without hipcc"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "tile_residual_plan.h"\nint main() { const int bptr[3] = {0, 2, 3}, brow[3] = {0, 1, 1};\n'
                   '    return hdm_tile_residual_plan(129, 2, bptr, brow).jobs.size() == 6 ? 0 : 1; }\n')   # 3 + 2 + 1
    exe = str(tmp_path / "alone")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


class Plan:
    """m, nb, ntiles, bptr, brow, perm; jobs (list of dicts), slot_ptr, slot_use, nrb"""


def plan_of(driver, family, m, renumbered):
    from hdsdp_amd import api
    beg, idx = sc.lower_csc(m, sc.pattern(family, m, renumbered))
    rc, perm, stats, bptr, brow = api.bsp_symbolic(m, beg, idx)
    assert rc == 0
    p = Plan()
    p.m, p.nb, p.ntiles, p.bptr, p.brow, p.perm = m, int(stats[0]), int(stats[1]), bptr, brow, perm
    rows = run(driver, [f"PLAN {m} {p.nb}", " ".join(str(int(v)) for v in bptr), " ".join(str(int(v)) for v in brow)])
    njobs, nslots, p.nrb = (int(v) for v in rows[0][1:])
    keys = ("tile", "qi", "qj", "rblk", "cblk", "slot_direct", "slot_trans", "diag")
    p.jobs = [dict(zip(keys, (int(v) for v in r[1:]))) for r in rows if r[0] == "J"]
    p.slot_ptr = [int(v) for v in next(r for r in rows if r[0] == "P")[1:]]
    p.slot_use = [int(v) for v in next(r for r in rows if r[0] == "U")[1:]]
    assert len(p.jobs) == njobs and len(p.slot_use) == nslots and p.nrb == 2 * p.nb and len(p.slot_ptr) == p.nrb + 1
    return p


def stored_quadrants(p):
    """(tile, quadrant number, I, J) of every stored quadrant whose first row and column are below m, in (tile, quadrant) order"""
    out = []
    for bj in range(p.nb):
        for t in range(p.bptr[bj], p.bptr[bj + 1]):
            bi = int(p.brow[t])
            for q in range(4):
                qi, qj = q & 1, q >> 1
                I, J = 2 * bi + qi, 2 * bj + qj
                if I >= J and 64 * I < p.m and 64 * J < p.m:
                    out.append((t, q, I, J))
    return out


@pytest.mark.parametrize("family,m,renumbered", CASES)
def test_jobs_slots_and_lists(driver, family, m, renumbered):
    p = plan_of(driver, family, m, renumbered)
    want = stored_quadrants(p)
    got = [(j["tile"], j["qi"] + 2 * j["qj"], j["rblk"], j["cblk"]) for j in p.jobs]
    assert got == want, "every stored quadrant below m in exactly one job, ascending tile then quadrant"
    assert all(0 <= j["tile"] < p.ntiles for j in p.jobs), "the trash tile is in no job"
    assert all(j["diag"] == (j["rblk"] == j["cblk"]) for j in p.jobs)
    # a diagonal tile has three quadrants, any other four (before the cut at m)
    per_tile = {}
    for t, q, I, J in want:
        per_tile.setdefault(t, []).append(q)
    for bj in range(p.nb):
        for t in range(p.bptr[bj], p.bptr[bj + 1]):
            full = [0, 1, 3] if p.brow[t] == bj else [0, 1, 2, 3]
            assert set(per_tile.get(t, [])) <= set(full)
            if 128 * (int(p.brow[t]) + 1) <= m:
                assert per_tile[t] == full
    # one writer per slot
    slots = [j["slot_direct"] for j in p.jobs] + [j["slot_trans"] for j in p.jobs]
    assert sorted(slots) == list(range(len(p.slot_use))), "every slot has exactly one writer"
    for k, j in enumerate(p.jobs):
        assert p.slot_use[j["slot_direct"]] == 2 * k and p.slot_use[j["slot_trans"]] == 2 * k + 1
    # every 64-row block's list: exactly the uses that land in it, by (tile, quadrant, direct before transposed)
    assert p.slot_ptr[0] == 0 and p.slot_ptr[-1] == len(p.slot_use)
    for R in range(p.nrb):
        uses = [(j["tile"], j["qi"] + 2 * j["qj"], u, 2 * k + u) for k, j in enumerate(p.jobs) for u in (0, 1)
                if (j["rblk"] if u == 0 else j["cblk"]) == R]
        uses.sort()
        assert p.slot_use[p.slot_ptr[R]:p.slot_ptr[R + 1]] == [w for _, _, _, w in uses], R
        if 64 * R >= m:
            assert p.slot_ptr[R] == p.slot_ptr[R + 1], "a block of padding has no slot"
    lengths = {p.slot_ptr[R + 1] - p.slot_ptr[R] for R in range(p.nrb) if 64 * R < m}
    if family == "band" and m == 257 and not renumbered:
        assert p.ntiles == 5 and len(lengths) > 1, "tile (2, 0) is absent: the lists differ in length"


@pytest.mark.parametrize("family,m,renumbered", CASES)
def test_numpy_execution_equals_the_assembled_product(driver, family, m, renumbered):
    """random tile contents (NaN in the trash tile and in every padding row and column), the plan executed in numpy with the
    kernel's predicates, against A @ x of the symmetric matrix assembled from the same tiles"""
    p = plan_of(driver, family, m, renumbered)
    rng = np.random.default_rng([m, len(family), int(renumbered)])
    npad = 128 * p.nb
    tiles = rng.standard_normal((p.ntiles + 1, 128, 128))        # [t, row, column]
    tiles[p.ntiles] = np.nan
    A = np.zeros((npad, npad))
    for bj in range(p.nb):
        for t in range(p.bptr[bj], p.bptr[bj + 1]):
            bi = int(p.brow[t])
            blk = np.tril(tiles[t]) if bi == bj else tiles[t]
            A[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128] = blk
    A = np.tril(A) + np.tril(A, -1).T
    A = A[:m, :m].copy()
    for t in range(p.ntiles):                                     # what lies past m is never to be read
        bi = int(p.brow[t])
        bj = int(np.searchsorted(p.bptr, t, side="right") - 1)
        r0, c0 = max(0, m - 128 * bi), max(0, m - 128 * bj)
        if r0 < 128:
            tiles[t, r0:, :] = np.nan
        if c0 < 128:
            tiles[t, :, c0:] = np.nan
        if bi == bj:
            tiles[t][np.triu_indices(128, 1)] = np.nan
    x = np.full(npad, np.nan)
    x[:m] = rng.standard_normal(m)
    slots = np.full((len(p.slot_use), 64), np.nan)
    for j in p.jobs:
        I, J = j["rblk"], j["cblk"]
        nr, nc = min(64, m - 64 * I), min(64, m - 64 * J)
        Q = np.zeros((64, 64))
        src = tiles[j["tile"], 64 * j["qi"]:64 * j["qi"] + 64, 64 * j["qj"]:64 * j["qj"] + 64]
        mask = np.zeros((64, 64), dtype=bool)
        mask[:nr, :nc] = True
        if j["diag"]:
            mask &= np.tri(64, dtype=bool)
        Q[mask] = src[mask]
        xJ, xI = np.zeros(64), np.zeros(64)
        xJ[:nc], xI[:nr] = x[64 * J:64 * J + nc], x[64 * I:64 * I + nr]
        slots[j["slot_direct"]] = Q @ xJ
        slots[j["slot_trans"]] = (np.tril(Q, -1) if j["diag"] else Q).T @ xI
    y = np.zeros(64 * p.nrb)
    for R in range(p.nrb):
        for s in range(p.slot_ptr[R], p.slot_ptr[R + 1]):
            y[64 * R:64 * R + 64] += slots[s]
    assert np.all(np.isfinite(y)), "a padding entry or the trash tile was read"
    want = A @ x[:m]
    assert np.allclose(y[:m], want, rtol=0.0, atol=1e-12 * float(np.max(np.abs(A) @ np.abs(x[:m])))), float(np.max(np.abs(y[:m] - want)))
    assert not np.any(y[m:])


# ---------------------------------------------------------------- the state rule's tile rows

def source(exe, lines):
    row = run(exe, lines + ["SOURCE"])[-1]
    keys = ("matrix", "why", "permute", "pivoted", "wants_copy", "wants_tile_copy", "cap", "switch")
    return dict(zip(keys, (int(v) for v in row)))


def tiles_factorised(mirror, cap=2, switch=1):
    lines = [f"INIT {TILES} 1", f"MIRROR {int(mirror)}"]
    if cap:
        lines.append(f"REFINE {cap}")
    if switch:
        lines.append("TILESW 1")
    return lines + ["START 0", "FINISH 0", "DO"]


def test_tile_operator_needs_the_cap_and_its_own_switch(driver):
    for mirror in (True, False):
        both = source(driver, tiles_factorised(mirror))
        assert both == dict(matrix=MAT_TILES_COPY if mirror else MAT_TILES_M, why=OFF, permute=0, pivoted=0, wants_copy=0,
                            wants_tile_copy=int(mirror), cap=2, switch=1), mirror
        cap_only = source(driver, tiles_factorised(mirror, switch=0))
        assert (cap_only["matrix"], cap_only["why"], cap_only["wants_tile_copy"]) == (MAT_NONE, NOT_AVAILABLE, 0), mirror
        switch_only = source(driver, tiles_factorised(mirror, cap=0))
        assert (switch_only["matrix"], switch_only["why"], switch_only["wants_tile_copy"], switch_only["cap"]) == (MAT_NONE, OFF, 0, 0), mirror
        # switched on after the factorisation: nothing was recorded
        late = source(driver, tiles_factorised(mirror, switch=0) + ["TILESW 1"])
        assert (late["matrix"], late["why"]) == (MAT_NONE, NO_MATRIX), mirror
        late = source(driver, tiles_factorised(mirror, cap=0) + ["REFINE 2"])
        assert (late["matrix"], late["why"]) == (MAT_NONE, NO_MATRIX), mirror
        assert source(driver, [f"INIT {TILES} 1", "REFINE 2", "TILESW 1"])["why"] == NO_MATRIX     # nothing factorised yet


def test_tile_source_validity(driver):
    # mirror off: the accumulation store in place, until a build that is no corrector build starts
    off = tiles_factorised(False)
    assert source(driver, off + ["START 1", "FINISH 1"])["matrix"] == MAT_TILES_M
    gone = source(driver, off + ["START 0"])
    assert (gone["matrix"], gone["why"]) == (MAT_NONE, NO_MATRIX)
    assert source(driver, off + ["START 0", "FINISH 0", "DO"])["matrix"] == MAT_TILES_M      # the next factorisation records it again
    # mirror on: the copy serves until the next factorisation, whatever is built meanwhile
    on = tiles_factorised(True)
    assert source(driver, on + ["START 0", "FINISH 0"])["matrix"] == MAT_TILES_COPY
    # either switch off frees the copy; on again it is NO_MATRIX until the next factorisation
    for off_cmd, on_cmd in (("TILESW 0", "TILESW 1"), ("REFINE 0", "REFINE 3")):
        s = source(driver, on + [off_cmd])
        assert (s["matrix"], s["wants_tile_copy"]) == (MAT_NONE, 0) and s["why"] == (NOT_AVAILABLE if off_cmd == "TILESW 0" else OFF)
        s = source(driver, on + [off_cmd, on_cmd])
        assert (s["matrix"], s["why"], s["wants_tile_copy"]) == (MAT_NONE, NO_MATRIX, 0)
        assert source(driver, on + [off_cmd, on_cmd, "DO"])["matrix"] == MAT_TILES_COPY
    # the switch does nothing to the other forms
    for form in (DENSE, CSC):
        base = [f"INIT {form} 0", "MIRROR 0", "REFINE 2", "START 0", "FINISH 0", "DO"]
        a, b = source(driver, base), source(driver, ["TILESW 1"] + base)
        assert a["matrix"] == MAT_DEVICE and {k: v for k, v in a.items() if k != "switch"} == {k: v for k, v in b.items() if k != "switch"}
