"""The rule of the refined Schur solve (csrc/refine_rule.h) and where its residual's matrix comes from (csrc/kkt_store.h:
hdm_kkt_refine_source), without a device: the two headers are compiled alone with the host C++ compiler beside
tests/refine_rule_driver.cpp.  The expected values are written here from the rules as DESIGN.md section 18 states them:

- tol = max(min(absTol, relTol |b|), 0.1 absTol), the reference's formula, with 1e-6 for a tolerance that was never set;
- the loop: CONVERGED (|r| < tol, strictly), STAGNATED (|r_k| >= 0.5 |r_k-1|; the iterate with the smaller residual goes back),
  MAXSTEPS (cap, clamped to 8), NUMERICAL (a residual that is not finite: the unrefined solution goes back);
- the source table:

    factorised source                      | residual reads      | until
    device M (mirror off; any CSC)         | device M in place   | a build that is no corrector build starts -> NO_MATRIX
    host M (dense + mirror, HFpLinsysNumeric) | the device copy  | the next factorisation; NO_MATRIX if refinement was off then
    nothing factorised                     | --                  | NO_MATRIX
    tile form                              | --                  | NOT_AVAILABLE

  permuted CSC: permute on the device; switched to the pivoted solver: its corrections, no permutation."""
import itertools
import math
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

OFF, CONVERGED, STAGNATED, MAXSTEPS, NUMERICAL, NO_MATRIX, NOT_AVAILABLE = range(7)
CURRENT, PREVIOUS, UNREFINED = range(3)
MAT_NONE, MAT_DEVICE, MAT_COPY = range(3)
DENSE, CSC, TILES = range(3)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("refine_rule") / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "refine_rule_driver.cpp")])
    return exe


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [row.split() for row in out.splitlines()]


def test_the_rule_header_compiles_alone(tmp_path):
    """no HIP call, no engine state: refine_rule.h by itself is a translation unit"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "refine_rule.h"\nint main() { return hdm_refine_clamp(3) == 3 ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


def test_step_cap_is_clamped(driver):
    rows = run(driver, [f"CLAMP {k}" for k in (-3, 0, 1, 3, 8, 9, 1000)])
    assert [int(r[0]) for r in rows] == [0, 0, 1, 3, 8, 8, 8]


def want_tol(rel, ab, bn):
    rel = rel if rel > 0 else 1e-6
    ab = ab if ab > 0 else 1e-6
    return max(min(ab, rel * bn), 0.1 * ab)


def test_tolerance_at_its_three_regimes_and_the_defaults(driver):
    """the Schur operator's own 5e-12 / 1e-12: a large right-hand side is held to absTol, a middling one to relTol |b|, a tiny one
    to 0.1 absTol; unset tolerances are the reference's 1e-6"""
    cases = [(5e-12, 1e-12, 10.0, 1e-12), (5e-12, 1e-12, 0.1, 5e-12 * 0.1), (5e-12, 1e-12, 1e-3, 0.1 * 1e-12),
             (5e-12, 1e-12, 0.2, 1e-12), (5e-12, 1e-12, 0.0, 0.1 * 1e-12),                         # (the first boundary: min takes either)
             (0.0, 0.0, 1.0, 1e-6), (-1.0, -1.0, 0.5, 1e-6 * 0.5), (0.0, 0.0, 1e-2, 0.1 * 1e-6),
             (0.0, 1e-9, 1.0, 1e-9), (1e-3, 0.0, 1e-4, 1e-7),
             (1e-30, 1e-30, 1.0, 1e-30)]
    rows = run(driver, [f"TOL {float(r).hex()} {float(a).hex()} {float(b).hex()}" for r, a, b, _ in cases])
    for (r, a, b, want), row in zip(cases, rows):
        got = float.fromhex(row[0])
        assert got == want_tol(r, a, b), (r, a, b, got)
        assert math.isclose(got, want, rel_tol=1e-15), (r, a, b, got, want)


def loop(driver, cap, tol, resid):
    """one refined solve fed the residual norms `resid` (the loop takes their squares; powers of two keep the roots exact)"""
    row = run(driver, [f"LOOP {cap} {float(tol).hex()} " + " ".join(float(r * r).hex() if math.isfinite(r) else repr(r) for r in resid)])[0]
    return dict(status=int(row[0]), keep=int(row[1]), steps=int(row[2]), solves=int(row[3]), resid0=float.fromhex(row[4]),
                resid=float.fromhex(row[5]), consumed=int(row[6]))


TOL = 2.0 ** -20


def test_converged_at_once_returns_the_unrefined_solve(driver):
    got = loop(driver, 3, TOL, [2.0 ** -21, 99.0])
    assert got == dict(status=CONVERGED, keep=CURRENT, steps=0, solves=0, resid0=2.0 ** -21, resid=2.0 ** -21, consumed=1)


def test_converged_is_strictly_below_the_tolerance(driver):
    got = loop(driver, 3, TOL, [TOL, 2.0 ** -30, 99.0])
    assert got == dict(status=CONVERGED, keep=CURRENT, steps=1, solves=1, resid0=TOL, resid=2.0 ** -30, consumed=2)


def test_converged_after_two_steps(driver):
    got = loop(driver, 3, TOL, [1.0, 2.0 ** -8, 2.0 ** -21, 99.0])
    assert got == dict(status=CONVERGED, keep=CURRENT, steps=2, solves=2, resid0=1.0, resid=2.0 ** -21, consumed=3)


def test_stagnation_returns_the_earlier_iterate_when_it_is_the_better_one(driver):
    got = loop(driver, 5, TOL, [1.0, 2.0 ** -8, 2.0 ** -7, 99.0])
    assert got == dict(status=STAGNATED, keep=PREVIOUS, steps=1, solves=2, resid0=1.0, resid=2.0 ** -8, consumed=3)
    # the very first correction is no better: what goes back is the unrefined solve, never something worse
    for r1 in (1.0, 4.0):
        got = loop(driver, 5, TOL, [1.0, r1, 99.0])
        assert got == dict(status=STAGNATED, keep=PREVIOUS, steps=0, solves=1, resid0=1.0, resid=1.0, consumed=2), r1


def test_stagnation_keeps_a_correction_that_still_gained(driver):
    for r1 in (0.75, 0.5):                       # 0.5 is the boundary: "not halved" includes exactly half
        got = loop(driver, 5, TOL, [1.0, r1, 99.0])
        assert got == dict(status=STAGNATED, keep=CURRENT, steps=1, solves=1, resid0=1.0, resid=r1, consumed=2), r1
    got = loop(driver, 5, TOL, [1.0, 0.4999999, 0.3, 99.0])
    assert got["status"] == STAGNATED and got["steps"] == 2 and got["consumed"] == 3


def test_maxsteps(driver):
    got = loop(driver, 2, TOL, [1.0, 0.25, 2.0 ** -4, 99.0])
    assert got == dict(status=MAXSTEPS, keep=CURRENT, steps=2, solves=2, resid0=1.0, resid=2.0 ** -4, consumed=3)
    got = loop(driver, 1, TOL, [1.0, 0.25, 99.0])
    assert got == dict(status=MAXSTEPS, keep=CURRENT, steps=1, solves=1, resid0=1.0, resid=0.25, consumed=2)
    # a cap above 8 is 8
    got = loop(driver, 50, 2.0 ** -200, [4.0 ** -k for k in range(12)])
    assert got["status"] == MAXSTEPS and got["steps"] == got["solves"] == 8 and got["consumed"] == 9 and got["resid"] == 4.0 ** -8


def test_a_residual_that_is_not_finite_returns_the_unrefined_solve(driver):
    for bad in (float("nan"), float("inf")):
        got = loop(driver, 3, TOL, [bad, 99.0])
        assert (got["status"], got["keep"], got["steps"], got["solves"], got["consumed"]) == (NUMERICAL, UNREFINED, 0, 0, 1)
        got = loop(driver, 3, TOL, [1.0, 2.0 ** -3, bad, 99.0])
        assert got == dict(status=NUMERICAL, keep=UNREFINED, steps=0, solves=2, resid0=1.0, resid=1.0, consumed=3)


# ---------------------------------------------------------------- where the residual's matrix comes from

def source(driver, lines):
    row = run(driver, lines + ["SOURCE"])[0]
    return dict(zip(("matrix", "why", "permute", "pivoted", "wants_copy", "cap"), (int(v) for v in row)))


def factorised(form, mirror, permuted, switched, refine_first=True):
    lines = [f"INIT {form} {int(permuted)}", f"MIRROR {int(mirror)}"]
    if refine_first:
        lines.append("REFINE 2")
    if switched:
        lines.append("PIVOTED")
    return lines + ["START 0", "FINISH 0", "DO"]


def states():
    for form in (DENSE, CSC, TILES):
        for mirror, permuted, switched in itertools.product((1, 0), repeat=3):
            if (permuted and form != CSC) or (switched and form == TILES):
                continue
            yield form, mirror, permuted, switched


def expected_source(form, mirror, permuted, switched):
    """the table, row by row"""
    if form == TILES:
        return dict(matrix=MAT_NONE, why=NOT_AVAILABLE, permute=0, pivoted=0, wants_copy=0, cap=2)
    host = form == DENSE and mirror
    return dict(matrix=MAT_COPY if host else MAT_DEVICE, why=OFF, permute=int(bool(permuted and not switched)), pivoted=int(switched),
                wants_copy=int(bool(host)), cap=2)


def test_source_table_row_by_row(driver):
    n = 0
    for s in states():
        assert source(driver, factorised(*s)) == expected_source(*s), s
        n += 1
    assert n == 4 + 8 + 2


def test_a_new_build_invalidates_the_device_matrix_and_a_corrector_build_does_not(driver):
    for s in states():
        want = expected_source(*s)
        assert source(driver, factorised(*s) + ["START 1", "FINISH 1"]) == want, s           # corrector: M is not touched
        after = source(driver, factorised(*s) + ["START 0"])
        if want["matrix"] == MAT_DEVICE:
            assert after == dict(want, matrix=MAT_NONE, why=NO_MATRIX, permute=0, pivoted=0), s
        else:
            assert after == want, s                                                            # the copy, or the tile form's answer
        # built and factorised again: the new matrix
        assert source(driver, factorised(*s) + ["START 0", "FINISH 0", "DO"]) == want, s


def test_no_matrix_when_refinement_was_off_at_factorisation_time(driver):
    for s in states():
        want = expected_source(*s)
        got = source(driver, factorised(*s, refine_first=False) + ["REFINE 2"])
        if want["matrix"] == MAT_COPY:           # no copy was taken
            assert got == dict(want, matrix=MAT_NONE, why=NO_MATRIX, permute=0, pivoted=0, wants_copy=0), s
            assert source(driver, factorised(*s, refine_first=False) + ["REFINE 2", "START 0", "FINISH 0", "DO"]) == want, s
        else:                                    # the device matrix is where it was
            assert got == want, s
        # switched off: OFF whatever the state; on again: the copy is gone until the next factorisation
        off = source(driver, factorised(*s) + ["REFINE 0"])
        assert (off["matrix"], off["why"], off["cap"], off["wants_copy"]) == (MAT_NONE, OFF, 0, 0), s
        again = source(driver, factorised(*s) + ["REFINE 0", "REFINE 5"])
        if want["matrix"] == MAT_COPY:
            assert (again["matrix"], again["why"], again["cap"]) == (MAT_NONE, NO_MATRIX, 5), s
        else:
            assert again == dict(want, cap=5), s


def test_nothing_factorised_a_stand_alone_matrix_and_the_small_pass(driver):
    assert source(driver, ["INIT 0 0", "REFINE 2"]) == dict(matrix=MAT_NONE, why=NO_MATRIX, permute=0, pivoted=0, wants_copy=0, cap=2)
    assert source(driver, ["INIT 0 0", "REFINE 2", "START 0", "FINISH 0"])["why"] == NO_MATRIX
    # HFpLinsysNumeric on an object that is no operator's: a host matrix
    assert source(driver, ["REFINE 3", "HOSTM"]) == dict(matrix=MAT_COPY, why=OFF, permute=0, pivoted=0, wants_copy=1, cap=3)
    assert source(driver, ["REFINE 3", "PIVOTED", "HOSTM"]) == dict(matrix=MAT_COPY, why=OFF, permute=0, pivoted=1, wants_copy=1, cap=3)
    assert source(driver, ["HOSTM", "REFINE 3"])["why"] == NO_MATRIX
    # the fused small pass writes M and its factor on the device in one launch
    got = source(driver, ["INIT 0 0", "REFINE 2", "START 0", "SMALL"])
    assert got == dict(matrix=MAT_DEVICE, why=OFF, permute=0, pivoted=0, wants_copy=0, cap=2)
    assert source(driver, ["INIT 0 0", "REFINE 2", "START 0", "SMALL", "START 0"])["why"] == NO_MATRIX
