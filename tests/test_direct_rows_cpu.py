"""The rule of the direct rows (csrc/direct_rows.h), without a device: the header is compiled alone with the host C++ compiler
beside tests/direct_rows_driver.cpp.

Expected values are written here from the rule as the design states it, not from what the code gives:
which rows are direct, the local order (congruence rows ascending, then direct rows ascending), when the form is on, the terms
of a row -- off-diagonal entry (p, q), value v: c = v, x = w_p, y = w_q; diagonal entry: c = v / 2, x = y = w_p; rank one:
c = sigma / 2, x = y = u -- and the value of a transformed row, held to numpy's L^-1 A L^-T."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

ZERO, SPARSE, DENSE, SPR1, DSR1 = range(5)      # MiCoeffType
PATH_GEMM, PATH_R1, PATH_SPARSE = range(3)
UNSET = -1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("direct_rows") / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "direct_rows_driver.cpp")])
    return exe


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [row.split() for row in out.split("\n")[:-1]]


def part(exe, rows, on=1, kmax=8, table_bytes=1 << 30):
    line = f"PART {on} {kmax} {table_bytes} " + " ".join(f"{t} {k}" for t, k in rows)
    v = [int(x) for x in run(exe, [line])[0]]
    return dict(nCongruence=v[0], nDirect=v[1], nRankOne=v[2], nterms=v[3], order=v[4:])


def rule(exe, world=1, synthetic=0, streamed=0, natural=PATH_GEMM, force_gemm=0, force_path=0, n=4096, n16=4096, sw=UNSET):
    on, kmax = run(exe, [f"RULE {world} {synthetic} {streamed} {natural} {force_gemm} {force_path} {n} {n16} {sw}"])[0]
    return int(on), int(kmax)


def floor_and_kmax(exe, n16):
    kmax, floor = run(exe, [f"KMAX {n16}"])[0]
    return int(floor), int(kmax)


# ---- the partition and the order ----------------------------------------------------------------------
def test_partition_and_order_of_a_mixed_block(driver):
    rows = [(DENSE, 100), (SPR1, 3), (ZERO, 0), (SPARSE, 2), (SPARSE, 9), (DSR1, 50), (SPARSE, 8), (DENSE, 60)]
    p = part(driver, rows, kmax=8)
    # direct: the two rank-one rows (one term each) and the triplet rows of 2 and 8 entries; 9 entries is one too many; the zero
    # row is nobody's
    assert p == dict(nCongruence=3, nDirect=4, nRankOne=2, nterms=1 + 2 + 1 + 8, order=[0, 4, 7, 1, 3, 5, 6])


def test_partition_with_the_form_off_keeps_the_ascending_order(driver):
    rows = [(SPR1, 3), (ZERO, 0), (SPARSE, 2), (DENSE, 60)]
    assert part(driver, rows, on=0) == dict(nCongruence=3, nDirect=0, nRankOne=0, nterms=0, order=[0, 2, 3])


def test_partition_without_a_congruence_row_and_without_a_direct_row(driver):
    assert part(driver, [(SPARSE, 1), (DSR1, 7), (SPARSE, 3)], kmax=3) == dict(nCongruence=0, nDirect=3, nRankOne=1, nterms=5, order=[0, 1, 2])
    assert part(driver, [(SPARSE, 4), (DENSE, 7)], kmax=3) == dict(nCongruence=2, nDirect=0, nRankOne=0, nterms=0, order=[0, 1])


def test_k_forcing_moves_the_cut_and_rank_one_rows_are_direct_at_any_k(driver):
    rows = [(SPARSE, 1), (SPARSE, 2), (SPARSE, 3), (DSR1, 500), (SPR1, 400)]
    assert part(driver, rows, kmax=1)["order"] == [1, 2, 0, 3, 4]
    assert part(driver, rows, kmax=2)["order"] == [2, 0, 1, 3, 4]
    assert part(driver, rows, kmax=64)["order"] == [0, 1, 2, 3, 4]
    assert [int(run(driver, [f"NTERMS {t} {k} {kmax}"])[0][0]) for t, k, kmax in
            ((SPR1, 400, 1), (DSR1, 1, 1), (SPARSE, 2, 1), (SPARSE, 2, 2), (DENSE, 1, 64), (ZERO, 0, 64), (SPARSE, 0, 64))] == [1, 1, 0, 2, 0, 0, 0]


def test_the_table_cap_refuses_the_row_not_the_block(driver):
    # 16 bytes a term, a cap of three terms: the second two-entry row would make four, the one-entry row after it still fits
    rows = [(SPARSE, 2), (SPARSE, 2), (DENSE, 90), (SPARSE, 1), (SPR1, 5)]
    assert part(driver, rows, table_bytes=48) == dict(nCongruence=3, nDirect=2, nRankOne=0, nterms=3, order=[1, 2, 4, 0, 3])


# ---- when the form is on --------------------------------------------------------------------------------
def test_activation_rule_under_every_excluding_condition(driver):
    floor, kmax = floor_and_kmax(driver, 4096)
    assert floor >= 1 and kmax >= 1
    assert rule(driver) == (1, kmax)
    assert rule(driver, world=2) == (0, 0)
    assert rule(driver, synthetic=1) == (0, 0)
    assert rule(driver, streamed=1) == (0, 0)
    assert rule(driver, natural=PATH_R1) == (0, 0)
    assert rule(driver, natural=PATH_SPARSE) == (0, 0)
    assert rule(driver, force_gemm=1) == (0, 0)
    assert rule(driver, force_path=1) == (0, 0)
    assert rule(driver, sw=0) == (0, 0)
    # below the floor: off; at it: on, with the kmax of that size
    assert rule(driver, n=floor - 1, n16=(floor + 14) // 16 * 16) == (0, 0)
    assert rule(driver, n=floor, n16=(floor + 15) // 16 * 16) == (1, floor_and_kmax(driver, (floor + 15) // 16 * 16)[1])


def test_the_switch_forces_the_form_below_the_floor_with_its_own_kmax(driver):
    assert rule(driver, n=17, n16=32, sw=8) == (1, 8)
    assert rule(driver, n=4096, sw=3) == (1, 3)
    # ... and nothing else: every other excluding condition still holds
    assert rule(driver, n=17, n16=32, sw=8, world=2) == (0, 0)
    assert rule(driver, n=17, n16=32, sw=8, synthetic=1) == (0, 0)
    assert rule(driver, n=17, n16=32, sw=8, streamed=1) == (0, 0)
    assert rule(driver, n=17, n16=32, sw=8, force_gemm=1) == (0, 0)
    assert rule(driver, n=17, n16=32, sw=8, force_path=1) == (0, 0)
    assert rule(driver, n=17, n16=32, sw=8, natural=PATH_R1) == (0, 0)


# ---- the terms ---------------------------------------------------------------------------------------------
def packed(i, j, n):
    """packed index of (i, j), i >= j, of the lower triangle column by column"""
    return j * n - j * (j - 1) // 2 + (i - j)


def test_packed_index_decodes_to_row_and_column(driver):
    n = 7
    qs = [(i, j) for j in range(n) for i in range(j, n)]
    assert [packed(i, j, n) for i, j in qs] == list(range(n * (n + 1) // 2))
    got = run(driver, [f"DECODE {packed(i, j, n)} {n}" for i, j in qs])
    assert [(int(a), int(b)) for a, b in got] == qs


def terms(exe, type_, n, sign, slot, entries):
    w = run(exe, [f"TERMS {type_} {n} {float(sign).hex()} {slot} " + " ".join(f"{pk} {float(v).hex()}" for pk, v in entries)])[0]
    return [(float.fromhex(w[k]), int(w[k + 1]), int(w[k + 2])) for k in range(0, len(w), 3)]


def test_terms_of_a_row_with_diagonal_and_off_diagonal_entries(driver):
    n = 9
    entries = sorted([(packed(0, 0, n), 3.0), (packed(4, 1, n), -0.75), (packed(8, 8, n), 0.3), (packed(8, 0, n), 2.5)])
    got = terms(driver, SPARSE, n, 0.0, 0, entries)
    # ascending packed index: (0,0), (8,0), (4,1), (8,8); c = v / 2 on the diagonal, v off it
    assert got == [(1.5, 0, 0), (2.5, 8, 0), (-0.75, 4, 1), (0.15, 8, 8)]


def test_terms_of_both_rank_one_classes(driver):
    # one term, c = sigma / 2, x = y = the row's column of U (slot j is vector -1 - j); the stored entries play no part
    assert terms(driver, SPR1, 9, -2.5, 0, [(0, 1.0)]) == [(-1.25, -1, -1)]
    assert terms(driver, DSR1, 9, 7.0, 4, [(3, 1.0), (5, 2.0)]) == [(3.5, -5, -5)]


# ---- the value of a transformed row ------------------------------------------------------------------------
def value(exe, type_, n, sign, entries, u, Linv):
    f = lambda x: float(x).hex()
    line = (f"VALUE {type_} {n} {f(sign)} " + " ".join(f"{pk} {f(v)}" for pk, v in entries) + " | " + " ".join(f(x) for x in u) + " | " +
            " ".join(f(x) for x in np.asarray(Linv).T.ravel()))
    w = run(exe, [line])[0]
    return np.array([float.fromhex(x) for x in w]).reshape(n, n).T      # column-major out


@pytest.mark.parametrize("n", [17, 40])
def test_direct_value_is_the_congruence_transform(driver, n):
    rng = np.random.default_rng(1000 + n)
    L = np.tril(rng.standard_normal((n, n))) * 0.3 + np.diag(1.0 + rng.random(n))
    Linv = np.linalg.inv(L)
    Linv = np.tril(Linv)
    # a triplet row: diagonal and off-diagonal entries, the first and the last row / column among them
    pos = {(0, 0), (n - 1, n - 1), (n - 1, 0), (5, 2), (n - 2, 7), (9, 9), (16, 3)}
    entries = sorted((packed(i, j, n), float(rng.standard_normal())) for i, j in pos)
    A = np.zeros((n, n))
    for (i, j), (_, v) in zip(sorted(pos, key=lambda q: packed(q[0], q[1], n)), entries):
        A[i, j] = A[j, i] = v
    want = Linv @ A @ Linv.T
    got = value(driver, SPARSE, n, 0.0, entries, np.zeros(n), Linv)
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
    # both rank-one classes: sigma a a' with a sparse and with a dense factor, both signs
    for type_, sign, fill in ((SPR1, -1.7, 3), (DSR1, 2.3, n)):
        a = np.zeros(n)
        a[rng.choice(n, size=fill, replace=False)] = rng.standard_normal(fill)
        a /= np.linalg.norm(a)
        want = sign * (Linv @ np.outer(a, a) @ Linv.T)
        got = value(driver, type_, n, sign, [(0, 1.0)], Linv @ a, Linv)
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
