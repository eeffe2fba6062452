"""The geometry of the fp64 MFMA GEMM family (csrc/gemm_geom.h), without a device: the header is compiled alone with the host C++
compiler beside tests/gemm_geom_driver.cpp.

- tests/golden/gemm_geom_parent.json holds what the launcher of the commit before the header said about a grid of launches
  (tools/gemm_geom_fixture.py): the flops their MFMA instructions execute, per tile subset, and how far each operand's unmasked
  loads reach.  The header reproduces every integer.
- The other expected values are written here from the rules as they are stated, not from what the code gives: the tile list
  (row-major, stable sort, heaviest first), the K ranges, the MFMAs of a tile as a brute-force count over its live 16 x 16
  sub-tile pairs stage by stage, the four triangular K blocks (1280, 960, 1280, 1280), the blocked layout and its inverse, and
  the two work shares of congruence step 2 as one division of two integer sums."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

GENERIC, CONG1, CONG2, GRAM, CONG2D = range(5)
KLIM_NONE, KLIM_BY_M, KLIM_BY_N, KLIM_BAND = range(4)
EPI_SLAB = 2
DIAG_FULL, DIAG_SHORT, EDGE, SYMDIAG, MAIN = range(5)     # HdmTileKind
TILE, BK = 128, 16


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_geom") / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "gemm_geom_driver.cpp")])
    return exe


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "gemm_geom_parent.json")) as f:
        return json.load(f)


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [row.split() for row in out.split("\n")[:-1]]


def geom_of(c):
    """the launcher's adapter (gemm_f64.hip: tile_geom), from a fixture row"""
    npass = 2 if (c["second"] and c["role"] in (CONG2, GENERIC)) else 1
    return dict(M=c["M"], N=c["N"], K=c["K"], klimit=c["klimit"], lower_only=c["lower_only"], colmask=c["colmask"], role=c["role"],
                slab=int(c["epilogue"] == EPI_SLAB), batch=c["batch"], k_base=c["k_base"], k_chunk=c["k_chunk"], npass=npass)


def geom_line(g):
    return "GEOM " + " ".join(str(g[k]) for k in ("M", "N", "K", "klimit", "lower_only", "colmask", "role", "slab", "batch", "k_base",
                                                  "k_chunk", "npass"))


def step_geom(role, n, mask=0, batch=1):
    """the engine's launches on an n x n block: step 1, step 2 (its two kernels), and a Gram launch of K = n in splits of 48"""
    g = dict(M=n, N=n, K=n, lower_only=1, colmask=mask, role=role, slab=0, batch=batch, k_base=0, k_chunk=0, npass=1)
    if role == CONG1:
        g.update(klimit=KLIM_BAND)
    elif role in (CONG2, CONG2D):
        g.update(klimit=KLIM_BY_N, npass=2 if role == CONG2 else 1)
    else:
        g.update(klimit=KLIM_NONE, slab=1, batch=3, k_base=16, k_chunk=48)
    return g


# ---- the rules, restated ---------------------------------------------------------------------------
def ntiles(x):
    return (x + TILE - 1) // TILE


def selected(g, tm, tn):
    mask = g["colmask"] if ntiles(g["N"]) <= 64 else 0
    if (g["lower_only"] or g["klimit"] == KLIM_BAND) and tm < tn:
        return False
    return not (mask and not (mask >> tn) & 1)


def full_diag(g, tm, tn):
    return tm == tn and g["M"] - tm * TILE >= TILE - 15        # 8 sub-tile rows hold rows of the matrix


def weight(klimit, tm, tn):
    return {KLIM_NONE: 1, KLIM_BY_M: tm + 1, KLIM_BY_N: tn + 1, KLIM_BAND: tm - tn + 1}[klimit]


def tile_list(g, subset):
    tiles = [(tm, tn) for tm in range(ntiles(g["M"])) for tn in range(ntiles(g["N"]))
             if selected(g, tm, tn) and (subset == 0 or (subset == 1) == full_diag(g, tm, tn))]
    return sorted(tiles, key=lambda t: -weight(g["klimit"], *t))     # Python's sort is stable


def krange(g, tm, tn, z):
    kbeg, kend = 0, g["K"]
    if g["klimit"] in (KLIM_BY_M, KLIM_BAND):
        kend = min(g["K"], (tm + 1) * TILE)
    if g["klimit"] == KLIM_BY_N:
        kend = min(g["K"], (tn + 1) * TILE)
    if g["klimit"] == KLIM_BAND:
        kbeg = tn * TILE
    if g["slab"]:
        kbeg = g["k_base"] + z * g["k_chunk"]
        kend = min(kend, kbeg + g["k_chunk"])
    return kbeg, kend


def brute_mfmas(g, tm, tn, z):
    """16 x 16 x 4 products of tile (tm, tn), stage by stage over its live sub-tile pairs (I, J), I, J = 0..7.  A sub-tile is dead
    in a stage iff it is structurally zero there at the kernel's granularity: a wave owns every second sub-tile and stages run in
    pairs, so sub-tile X counts as X // 2 and stage s of a K block as s // 2."""
    role, M, N = g["role"], g["M"], g["N"]
    kbeg, kend = krange(g, tm, tn, z)
    stages = list(range(kbeg // BK, kend // BK))
    rv = min(8, (M - tm * TILE + 15) // 16)
    RV = max(4, rv)
    cells = None
    if role != CONG2D and g["lower_only"] and tm == tn:                      # diagonal tile, dealt in cells
        cells = [(i, j) for i in range(8 if rv == 8 else RV) for j in range(i + 1)]
    elif role != CONG2D and tm != tn and (tm + 1) * TILE > M and (tn + 1) * TILE <= N:   # bottom edge
        cells = [(i, j) for i in range(RV) for j in range(8)]
    if cells is not None or role == GRAM:
        # no triangular skipping; the stage count is run in pairs (an odd one ends with a stage of zeros)
        nst = len(stages) * g["npass"]
        return 4 * len(cells if cells is not None else range(64)) * (nst + nst % 2)

    def dead(s_abs, I, J):
        kb, s = divmod(s_abs, 8)                                             # K block, stage inside it
        if role == CONG1:        # A side: Linv rows of tile tm (k <= row); B side: A_L columns of tile tn (k >= column)
            return (kb == tm and I // 2 < s // 2) or (kb == tn and J // 2 > s // 2)
        if role == CONG2:        # B side of either product: rows of a lower triangular matrix in tile tn (k <= row)
            return kb == tn and J // 2 < s // 2
        return kb == tn and (I // 2 < s // 2 or J // 2 < s // 2)              # P + P^T: both operands, tm == tn

    return g["npass"] * sum(4 for s in stages for I in range(8) for J in range(8) if not dead(s, I, J))


# ---- tests -------------------------------------------------------------------------------------------
def test_the_header_reproduces_the_parent_launcher(driver, fixture):
    lines, want = [], []
    for c in fixture["host"]:
        lines.append(geom_line(geom_of(c)))
        lines += [f"LAUNCH {s}" for s in range(3)]
        per_launch = 2048 * (1 if c["epilogue"] == EPI_SLAB else c["batch"])
        want += [[str(v // per_launch)] for v in c["issued"]]
        assert all(v % per_launch == 0 for v in c["issued"])
        ops = {"A": (c["a_kmajor"], c["lda"], c["a_kblk"], c["strideA"], c["M"], 0), "B": (c["b_kmajor"], c["ldb"], c["b_kblk"], c["strideB"], c["N"], c["b_sky"]),
               "A2": (c["a_kmajor"], c["lda2"], BK, c["strideA2"], c["M"], 0), "B2": (c["b_kmajor"], c["ldb2"], BK, c["strideB2"], c["N"], 0)}
        for name, need in sorted(c["need"].items()):
            km, ld, kblk, stride, rows, sky = ops[name]
            lines.append(f"NEED {km} {ld} {kblk} {stride} {rows} {c['seg_rows']} {c['seg_extra']} {sky}")
            want.append([str(need)])
    assert len(fixture["host"]) >= 400 and len(want) > 3 * len(fixture["host"])
    assert run(driver, lines) == want


def test_fixture_covers_every_class_and_k_rule(driver, fixture):
    kinds, odd_even, masked = set(), set(), set()
    for c in fixture["host"]:
        g = geom_of(c)
        rows = run(driver, [geom_line(g)] + [f"TILE {tm} {tn} 0" for tm in range(ntiles(g["M"])) for tn in range(ntiles(g["N"]))]) if g["M"] <= 2000 else []
        for r in rows:
            if int(r[0]):
                kinds.add((g["role"], int(r[3]), int(r[5])))
                if g["slab"]:
                    odd_even.add(((int(r[2]) - int(r[1])) // BK) % 2)
        masked.add((g["colmask"] != 0, ntiles(g["N"]) > 64))
    for role in (CONG1, GRAM):
        assert {(role, k, 8) for k in (DIAG_FULL, MAIN)} <= kinds
        assert {(role, k, RV) for k in (DIAG_SHORT, EDGE) for RV in (4, 5)} <= kinds          # rv = 1 runs as 4
    assert {(CONG2, MAIN, 8), (CONG2, DIAG_SHORT, 5), (CONG2, EDGE, 4), (CONG2D, SYMDIAG, 8), (GENERIC, MAIN, 8)} <= kinds
    assert odd_even == {0, 1} and masked == {(False, False), (True, False), (False, True), (True, True)}
    assert {c["klimit"] for c in fixture["host"]} == {KLIM_NONE, KLIM_BY_M, KLIM_BY_N, KLIM_BAND}


def test_tile_list_is_the_rule(driver, fixture):
    lines, want = [], []
    for c in fixture["host"]:
        g = geom_of(c)
        lines.append(geom_line(g))
        for subset in range(3):
            lines.append(f"LIST {subset}")
            want.append([str(x) for t in tile_list(g, subset) for x in t])
    assert run(driver, lines) == want


@pytest.mark.parametrize("n", [128, 144, 384, 464])
def test_tile_mfmas_are_the_brute_force_count(driver, n):
    lines, want = [], []
    for role, subset in ((CONG1, 0), (CONG2, 2), (CONG2D, 1), (GRAM, 0)):
        for mask in (0, 0b0101):
            g = step_geom(role, n, mask)
            lines.append(geom_line(g))
            total = 0
            for z in range(g["batch"] if g["slab"] else 1):
                for tm, tn in tile_list(g, subset):
                    lines.append(f"TILE {tm} {tn} {z}")
                    kbeg, kend = krange(g, tm, tn, z)
                    mf = brute_mfmas(g, tm, tn, z)
                    want.append([kbeg, kend, mf])
                    total += mf
            lines.append(f"LAUNCH {subset}")
            want.append([total])
    got = run(driver, lines)
    assert [[int(r[1]), int(r[2]), int(r[6])] if len(r) > 1 else [int(r[0])] for r in got] == want


def test_tile_classes(driver):
    g = step_geom(CONG1, 464)                                                 # tiles 0..2 full, tile 3: 80 rows = 5 sub-tile rows
    rows = run(driver, [geom_line(g), "TILE 0 0 0", "TILE 3 3 0", "TILE 3 1 0", "TILE 2 0 0", "TILE 0 1 0",
                        geom_line(step_geom(CONG1, 144)), "TILE 1 1 0", "TILE 1 0 0",
                        geom_line(step_geom(CONG2D, 464)), "TILE 1 1 0", geom_line(step_geom(CONG2, 464)), "TILE 1 1 0", "TILE 2 1 0"])
    kind = [(int(r[0]), int(r[3]), int(r[4]), int(r[5])) for r in rows]
    assert kind == [(1, DIAG_FULL, 8, 8), (1, DIAG_SHORT, 5, 5), (1, EDGE, 5, 5), (1, MAIN, 8, 8), (0, MAIN, 8, 8),
                    (1, DIAG_SHORT, 1, 4), (1, EDGE, 1, 4), (1, SYMDIAG, 8, 8), (1, DIAG_FULL, 8, 8), (1, MAIN, 8, 8)]


def test_small_rules(driver):
    rows = run(driver, [f"RULES {x}" for x in (1, 3, 4, 7, 128, 129, 8256)] + ["MASK 5 64", "MASK 5 65", f"MASK {(1 << 63) | 1} 3", "TABLES"])
    assert [[int(v) for v in r] for r in rows] == [
        [1, 4, 1, 2, 2, 1], [1, 4, 1, 4, 2, 3], [1, 4, 1, 5, 2, 4], [1, 7, 1, 8, 2, 7], [1, 128, 1, 129, 2, 128], [2, 129, 1, 130, 2, 129],
        [65, 8256, 1, 8257, 2, 8256], [5], [0], [(1 << 63) | 1],
        [1280, 960, 1280, 1280, 2048]]        # 32 x (16 + 12 + 8 + 4), 32 x (16 + 9 + 4 + 1), 32 x (4 + 8 + 12 + 16), ...; 8 stages x 256


@pytest.mark.parametrize("nblk", [1, 8, 9, 125])
def test_blocked_layout_and_its_inverse(driver, nblk):
    pairs, starts = run(driver, [f"BLK {nblk}"])
    pairs = [int(v) for v in pairs]
    want = []
    sub = 0
    for bj in range(nblk):                     # sub-blocks are numbered column by column, bi = bj .. nblk - 1 inside a column
        assert int(starts[bj]) == sub
        for bi in range(bj, nblk):
            want += [sub, bj]
            sub += 1
    assert pairs == want and sub == nblk * (nblk + 1) // 2
    qs = sorted({0, 15, 16, 16 * nblk - 1, 16 * nblk, 16 * sub - 1} & set(range(16 * sub)))
    got = run(driver, [f"PBLOCK {q} {nblk}" for q in qs])
    for q, r in zip(qs, got):
        s = q // 16
        bj = max(b for b in range(nblk) if int(starts[b]) <= s)
        assert [int(v) for v in r] == [s, bj + s - int(starts[bj]), bj, 16 * bj + q % 16]


def test_dist_py_uses_the_same_numbering(driver):
    from hdsdp_amd.dist import ShardPlan
    plan = ShardPlan(40, 6, 1)                 # n16 = 48: three sub-blocks per edge
    r, c, pb, q, w = plan.blocked_index()
    pairs, _ = run(driver, [f"BLK {plan.nblk}"])
    subs = iter(int(v) for v in pairs[::2])
    sub_of = {(bi, bj): next(subs) for bj in range(plan.nblk) for bi in range(bj, plan.nblk)}
    assert all(int(p) == sub_of[(int(i) // 16, int(j) // 16)] * 16 + int(j) % 16 for i, j, p in zip(r, c, pb))


def test_both_shares_are_one_division_of_integer_sums(driver):
    lines, want = [], []
    for n in (128, 144, 384, 464, 2000, 8256):
        NT = ntiles(n)
        for mask in (0, 1, 0b0110, 0b1010, (1 << 63) | 1):
            eff = mask if NT <= 64 else 0
            cols = [tn for tn in range(NT) if not eff or (eff >> tn) & 1]
            # by output element: (i, j), i >= j, is 2 products x (j + 1) terms; the full diagonal tiles' part of it
            every = sum((n - j) * (j + 1) for tn in cols for j in range(tn * TILE, min(n, (tn + 1) * TILE)))
            diag = sum((min(n, (tn + 1) * TILE) - j) * (j + 1) for tn in cols if n - tn * TILE >= TILE - 15
                       for j in range(tn * TILE, min(n, (tn + 1) * TILE)))
            lines.append(f"DIAGSHARE {n} {n} {mask}")
            want.append((diag / every if every else 0.0).hex())
            # by tile: tile (tm, tn), tm >= tn, runs tn + 1 K blocks
            every = sum((NT - tn) * (tn + 1) for tn in range(NT))
            sel = sum((NT - tn) * (tn + 1) for tn in range(NT) if (eff >> tn) & 1)
            lines.append(f"MASKSHARE {NT} {mask}")
            want.append((sel / every if eff else 1.0).hex())
            assert every < 2 ** 53
    assert [float.fromhex(r[0]).hex() for r in run(driver, lines)] == want
