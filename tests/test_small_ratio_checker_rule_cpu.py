"""The grouped ratio test's rules for the checker buffer (csrc/small_ratio_rule.h), without a device: the header is compiled alone
with the host C++ compiler and asked at its edges.  The expected values are written here from the rules as DESIGN.md section 26
states them:

- membership for a checker question, asked per launch: the dual-buffer rule, and a checker factor object of one 128-block
  (hdm_small_check_factor_ok).  No checker object or one of another shape: not a member now (its own path).  A checker that holds
  no factorisation: left out of the launch (its own call fails as it does per cone).  n = 1 stays outside;
- one slot per member, which records the buffer it answered.  A checker answer is served exactly once, only to the same question on
  the checker buffer, compared exactly, and only while HdmDualState::checker_epoch() and dS_writes() stand where the commit left
  them.  moves() is not part of it: the dual matrix is not read by a ratio test on the checker;
- the dual-buffer rule is unchanged, and never serves a checker answer."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

NOT_NOW, LEFT_OUT, TAKE = 0, 1, 2

DRIVER = r"""
#include "small_ratio_rule.h"
#include <cstdio>
#include <cstring>
int main() {
    char what[16];
    static_assert(HDM_RATIO_CHECKER_NOT_NOW == 0 && HDM_RATIO_CHECKER_LEFT_OUT == 1 && HDM_RATIO_CHECKER_TAKE == 2, "the three answers");
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "sort")) {
            int n, n16, whole, present, npad, nblk, factored;
            long mloc;
            if (scanf("%d %d %ld %d %d %d %d %d", &n, &n16, &mloc, &whole, &present, &npad, &nblk, &factored) != 8) return 2;
            HdmSmallRatioCone c;
            c.chk.on = true; c.chk.world = 1; c.chk.resident = true; c.chk.n16 = n16; c.chk.mloc = mloc;
            c.chk.fac_npad = 128; c.chk.fac_nblk = 1; c.n = n;
            const HdmLzSwitches sw = {whole != 0, true, true, true};
            HdmSmallRatioChecker k;
            k.present = present != 0; k.npad = npad; k.nblk = nblk; k.factored = factored != 0;
            printf("%d %d\n", (int) hdm_small_ratio_checker_sort(c, sw, k), hdm_small_ratio_member(c, sw) ? 1 : 0);
        } else if (!strcmp(what, "slot")) {
            // a slot that holds (tau 0.5, eye -0.25, y = 1, 2, 3) for buffer `held`, stored at moves 7, checker epoch 11, dS writes 5;
            // asked on `asked` with the given question and counters.  Prints: the checker rule's answer, the dual rule's answer
            int held, asked, valid, consumed, ny;
            unsigned long moves, checker, ds;
            double tau, eye, y[8];
            if (scanf("%d %d %d %d %lu %lu %lu %lf %lf %d", &held, &asked, &valid, &consumed, &moves, &checker, &ds, &tau, &eye, &ny) != 10 || ny > 8) return 2;
            for (int i = 0; i < ny; ++i) if (scanf("%lf", &y[i]) != 1) return 2;
            const double hy[3] = {1.0, 2.0, 3.0};
            HdmDualPoint h; h.tau = 0.5; h.eye = -0.25; h.y = hy; h.ny = 3;
            HdmRatioSlot s; s.valid = valid != 0; s.consumed = consumed != 0; s.buffer = held; s.moves = 7; s.checker = 11; s.dS_writes = 5;
            h.store(s.q);
            HdmDualPoint q; q.tau = tau; q.eye = eye; q.y = y; q.ny = ny;
            HdmRatioCheckerEpochs now; now.checker = checker; now.dS_writes = ds;
            const bool chk = asked != 0 && hdm_ratio_checker_slot_serves(s, q, now);
            const bool dual = asked == 0 && hdm_ratio_slot_serves(s, q, moves);
            printf("%d %d\n", chk ? 1 : 0, dual ? 1 : 0);
        } else if (!strcmp(what, "epochs")) {
            // which transitions move the two counters a checker answer is held to
            const double y[2] = {1.0, 2.0};
            HdmDualPoint p; p.tau = 1.0; p.eye = 0.0; p.y = y; p.ny = 2;
            HdmDualState st;
            auto show = [&] { const HdmRatioCheckerEpochs e = hdm_ratio_checker_epochs(st); printf(" %lu/%lu/%lu", e.checker, e.dS_writes, st.moves()); };
            show();
            st.checker_written(); show();
            st.dS_written(); show();
            st.S_assembled_at(p); show();
            st.S_factored(1); show();
            st.S_overwritten(); show();
            printf("\n");
        } else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("small_ratio_checker_rule")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, str(src)])
    return exe


def _run(exe, line):
    return subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout.split()


def sort(exe, n=10, n16=16, mloc=3, whole=1, present=1, npad=128, nblk=1, factored=1):
    s, dual = _run(exe, f"sort {n} {n16} {mloc} {whole} {present} {npad} {nblk} {factored}")
    return int(s), dual == "1"


def serves(exe, held=1, asked=1, valid=1, consumed=0, moves=7, checker=11, ds=5, tau=0.5, eye=-0.25, y=(1.0, 2.0, 3.0)):
    """(the checker rule serves, the dual rule serves)"""
    out = _run(exe, f"slot {held} {asked} {valid} {consumed} {moves} {checker} {ds} {tau!r} {eye!r} {len(y)} " + " ".join(repr(float(v)) for v in y))
    return out[0] == "1", out[1] == "1"


def test_the_rule_header_still_compiles_alone(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "small_ratio_rule.h"\nint main() { HdmSmallRatioChecker k; HdmRatioSlot s; return (k.present || s.buffer) ? 1 : 0; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


def test_checker_membership_at_its_edges(driver):
    """no checker, a checker of another shape, an unfactored one, n = 1, n16 = 128"""
    assert sort(driver) == (TAKE, True)
    assert sort(driver, present=0) == (NOT_NOW, True)                       # never had a checker: its own path
    assert sort(driver, npad=256) == (NOT_NOW, True)                        # another shape
    assert sort(driver, nblk=2) == (NOT_NOW, True)
    assert sort(driver, npad=256, nblk=2, factored=0) == (NOT_NOW, True)    # (shape is asked before the factorisation)
    assert sort(driver, factored=0) == (LEFT_OUT, True)                     # its own call fails, as per cone
    assert sort(driver, n=1) == (NOT_NOW, False)                            # the closed form stays outside
    assert sort(driver, n=2) == (TAKE, True)
    assert sort(driver, n=128, n16=128, mloc=8) == (TAKE, True)
    assert sort(driver, n=113, n16=128, mloc=8, factored=0) == (LEFT_OUT, True)
    assert sort(driver, n=128, n16=128, mloc=9) == (NOT_NOW, False)         # the dual rule's data bound holds here too
    assert sort(driver, n=129, n16=144, mloc=1) == (NOT_NOW, False)
    assert sort(driver, whole=0) == (NOT_NOW, False)                        # HDM_LANCZOS_WHOLE=0: no members on either buffer


def test_a_checker_answer_is_served_once_to_the_same_question_on_the_same_buffer(driver):
    assert serves(driver) == (True, False)
    assert serves(driver, consumed=1) == (False, False)                     # exactly once
    assert serves(driver, valid=0) == (False, False)
    assert serves(driver, held=1, asked=0) == (False, False)                # the other buffer misses ...
    assert serves(driver, held=0, asked=1) == (False, False)                # ... both ways


def test_one_ulp_away_is_another_question(driver):
    assert serves(driver, tau=0.5000000000000001)[0] is False
    assert serves(driver, eye=-0.25000000000000006)[0] is False
    for k in range(3):
        y = [1.0, 2.0, 3.0]
        y[k] = float.fromhex("0x1.0000000000001p+0") * y[k]
        assert serves(driver, y=y)[0] is False, k
    assert serves(driver, y=(1.0, 2.0))[0] is False
    assert serves(driver, y=(1.0, 2.0, float("nan")))[0] is False


def test_the_two_counters_hold_the_answer_and_moves_does_not(driver):
    """a checker_epoch move and a dS_writes move each miss; a moves() change alone still serves"""
    assert serves(driver, checker=12)[0] is False
    assert serves(driver, checker=10)[0] is False
    assert serves(driver, ds=6)[0] is False
    assert serves(driver, ds=4)[0] is False
    for moves in (0, 6, 8, 1000):
        assert serves(driver, moves=moves)[0] is True, moves


def test_the_dual_rule_is_unchanged(driver):
    """a dual answer is held to moves() and the question, and to nothing of the checker"""
    assert serves(driver, held=0, asked=0) == (False, True)
    assert serves(driver, held=0, asked=0, moves=8) == (False, False)
    assert serves(driver, held=0, asked=0, consumed=1) == (False, False)
    assert serves(driver, held=0, asked=0, tau=0.5000000000000001) == (False, False)
    assert serves(driver, held=0, asked=0, checker=99, ds=99) == (False, True)


def test_which_transitions_move_the_counters(driver):
    """checker_written moves the epoch only, dS_written the dS counter only; transitions of S move moves() and neither of the two"""
    assert _run(driver, "epochs") == ["0/0/0", "1/0/0", "1/1/0", "1/1/1", "1/1/2", "1/1/3"]
