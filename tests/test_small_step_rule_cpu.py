"""The two rules of the grouped step-and-check (csrc/small_step_rule.h), without a device: the header is compiled alone with the
host C++ compiler and asked at its edges.  The expected values are written here from the rules as DESIGN.md section 24 states
them:

- membership: the check set's population for the cone's dual factor object (switch on, world == 1, resident rows, n16 <= 128, the
  data bound, a factor object of one 128-block), a checker object of the same shape, and HDM_DIAG_SWEEP not 0; n = 1 is a member;
- a slot serves a step only if it is valid, holds exactly this dStep (==) and nothing has been written to the member's S, dS,
  checker buffer or checker factor since the commit; it serves any number of times while that holds;
- the dS counter moves whether or not the block tracks points (HDSDP_MI355X_AFFINE_S=0: mode 0), the checker's epoch with every
  commit into the checker buffer, and neither enters HdmDualState::moves()."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

DRIVER = r"""
#include "small_step_rule.h"
#include <cstdio>
#include <cstring>
static const double Y[2] = {1.0, 2.0}, Y2[2] = {1.5, 2.0};
int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "member")) {
            int on, world, resident, n16, npad, nblk, cpad, cblk, sweep;
            long mloc;
            if (scanf("%d %d %d %d %ld %d %d %d %d %d", &on, &world, &resident, &n16, &mloc, &npad, &nblk, &cpad, &cblk, &sweep) != 10) return 2;
            HdmSmallStepCone c;
            c.chk.on = on != 0; c.chk.world = world; c.chk.resident = resident != 0; c.chk.n16 = n16; c.chk.mloc = mloc;
            c.chk.fac_npad = npad; c.chk.fac_nblk = nblk; c.chk_npad = cpad; c.chk_nblk = cblk; c.diag_sweep = sweep != 0;
            printf("%d\n", hdm_small_step_member(c) ? 1 : 0);
        } else if (!strcmp(what, "slot")) {
            // a slot committed at step 0.25 on a state that had seen some transitions; then the named things happen, in order,
            // and the slot is asked `dStep` after each: prints one 0 / 1 per ask
            int valid, mode;
            double dStep;
            char ev[16];
            if (scanf("%d %lf %d", &valid, &dStep, &mode) != 3) return 2;
            HdmDualPoint p; p.tau = 1.0; p.eye = 0.0; p.y = Y; p.ny = 2;
            HdmDualPoint p2; p2.tau = 1.0; p2.eye = 0.0; p2.y = Y2; p2.ny = 2;
            HdmDualState st;
            st.S_assembled_at(p); st.S_factored(1);
            st.commit(hdm_dual_plan(st, p2, HDM_DUAL_DS, mode, 1), p2, HDM_DUAL_DS);
            st.checker_written();
            HdmStepSlot s; s.valid = valid != 0; s.dStep = 0.25; s.info = 0; s.at = hdm_step_epochs(st);
            printf("%d", hdm_step_slot_serves(s, dStep, hdm_step_epochs(st)) ? 1 : 0);
            while (scanf("%15s", ev) == 1 && strcmp(ev, ";")) {
                if (!strcmp(ev, "ask")) { }
                else if (!strcmp(ev, "S")) st.S_overwritten();                         // cone_axpy_check on the dual buffer, ...
                else if (!strcmp(ev, "Sline")) st.S_advanced_to(p2);
                else if (!strcmp(ev, "dS")) st.commit(hdm_dual_plan(st, p, HDM_DUAL_DS, mode, 1), p, HDM_DUAL_DS);   // cone_assemble
                else if (!strcmp(ev, "dSlaunch")) st.dS_written();                     // ratio_set_launch
                else if (!strcmp(ev, "Scheck")) st.commit(hdm_dual_plan(st, p2, HDM_DUAL_SCHECK, mode, 1), p2, HDM_DUAL_SCHECK);
                else if (!strcmp(ev, "factor")) st.checker_written();                  // cone_factor_check, the grouped commit
                else return 2;
                printf(" %d", hdm_step_slot_serves(s, dStep, hdm_step_epochs(st)) ? 1 : 0);
            }
            printf("\n");
        } else if (!strcmp(what, "counters")) {
            // moves(), dS_writes(), checker_epoch() after each writer, in mode `mode`
            int mode;
            if (scanf("%d", &mode) != 1) return 2;
            HdmDualPoint p; p.tau = 1.0; p.eye = 0.0; p.y = Y; p.ny = 2;
            HdmDualState st;
            auto show = [&] { printf(" %lu,%lu,%lu", st.moves(), st.dS_writes(), st.checker_epoch()); };
            show();
            st.commit(hdm_dual_plan(st, p, HDM_DUAL_DS, mode, 1), p, HDM_DUAL_DS); show();
            st.commit(hdm_dual_plan(st, p, HDM_DUAL_SCHECK, mode, 1), p, HDM_DUAL_SCHECK); show();
            st.dS_written(); show();
            st.checker_written(); show();
            st.commit(hdm_dual_plan(st, p, HDM_DUAL_S, mode, 1), p, HDM_DUAL_S); show();
            printf("\n");
        } else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("small_step_rule")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, str(src)])
    return exe


def _run(exe, line):
    return subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout.split()


def member(exe, on=1, world=1, resident=1, n16=16, mloc=3, npad=128, nblk=1, cpad=128, cblk=1, sweep=1):
    return _run(exe, f"member {on} {world} {resident} {n16} {mloc} {npad} {nblk} {cpad} {cblk} {sweep}") == ["1"]


def serves(exe, events="", valid=1, step=0.25, mode=1):
    """the slot's answers: at once, and after each of `events`"""
    return [v == "1" for v in _run(exe, f"slot {valid} {step!r} {mode} {events} ;")]


def test_the_rule_header_compiles_alone(tmp_path):
    """no HIP call, no engine state: small_step_rule.h by itself is a translation unit"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "small_step_rule.h"\nint main() { HdmStepSlot s; return hdm_step_slot_serves(s, 0.0, HdmStepEpochs()) ? 1 : 0; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


def test_padded_dimension_edges(driver):
    """n16 = 128 is the largest block of the register sweep; 144 is no small block at all, whatever the factor objects"""
    assert member(driver, n16=128, mloc=8) is True
    assert member(driver, n16=144, mloc=1) is False
    assert member(driver, n16=144, mloc=1, npad=256, nblk=2, cpad=256, cblk=2) is False
    assert member(driver, n16=16, mloc=0) is True                  # no rows: the launch stages no multipliers anyway


def test_the_data_bound_on_both_sides(driver):
    """the check rule's bound on the resident rows: 2^19 doubles for n16 <= 64, 2^17 above"""
    assert member(driver, n16=128, mloc=8) is True                 # 8 * 128^2 = 2^17
    assert member(driver, n16=128, mloc=9) is False
    assert member(driver, n16=64, mloc=128) is True                # 128 * 64^2 = 2^19
    assert member(driver, n16=64, mloc=129) is False
    assert member(driver, n16=80, mloc=20) is True                 # 20 * 80^2 = 128 000 <= 2^17
    assert member(driver, n16=80, mloc=21) is False


def test_the_diagonal_sweep_switch(driver):
    """with HDM_DIAG_SWEEP=0 the per-cone path factors with the LDS-panel kernel, whose bits the sweep's are not: no members"""
    assert member(driver, sweep=1) is True
    assert member(driver, sweep=0) is False


def test_kind_conditions(driver):
    """two ranks, rows not resident, the one-launch check switched off, a dual factor or a checker of another shape"""
    assert member(driver) is True
    for bad in (dict(world=2), dict(resident=0), dict(on=0), dict(npad=256), dict(nblk=2), dict(cpad=256, cblk=2), dict(cblk=2),
                dict(cpad=256)):
        assert member(driver, **bad) is False, bad


def test_the_same_step_serves_any_number_of_times(driver):
    assert serves(driver, "ask ask ask") == [True, True, True, True]


def test_a_step_one_ulp_away_misses(driver):
    up, down = float.fromhex("0x1.0000000000001p-2"), float.fromhex("0x1.fffffffffffffp-3")
    assert serves(driver, "ask", step=up) == [False, False]
    assert serves(driver, "ask", step=down) == [False, False]
    assert serves(driver, step=-0.25) == [False]
    assert serves(driver, step=float("nan")) == [False]


def test_an_empty_slot_serves_nothing(driver):
    assert serves(driver, "ask", valid=0) == [False, False]


@pytest.mark.parametrize("writer", ["S", "Sline", "dS", "dSlaunch", "Scheck", "factor"])
def test_each_writer_makes_the_slot_miss_for_good(driver, writer):
    """S (overwritten, or advanced along the line), dS (assembled, or written by the grouped ratio launch), the checker buffer, the
    checker factor: after any one of them the slot no longer serves, and asking again does not bring it back"""
    assert serves(driver, f"ask {writer} ask") == [True, True, False, False]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_a_rewritten_step_matrix_misses_in_every_tracking_mode(driver, mode):
    """mode 0 (HDSDP_MI355X_AFFINE_S=0) records no point of dS and moves() stands still; the dS counter moves all the same"""
    assert serves(driver, "dS", mode=mode) == [True, False]
    assert serves(driver, "dSlaunch", mode=mode) == [True, False]


def test_the_counters(driver):
    """(moves, dS writes, checker epoch) after: nothing; dS assembled; the checker buffer assembled; the grouped ratio launch's
    write; a checker factorisation; S assembled.  Tracking blocks count the dS point and S in moves(); mode 0 counts S alone
    there (as overwritten) -- and both count the two new counters alike"""
    assert _run(driver, "counters 1") == ["0,0,0", "1,1,0", "1,1,1", "1,2,1", "1,2,2", "2,2,2"]
    assert _run(driver, "counters 0") == ["0,0,0", "0,1,0", "0,1,1", "0,2,1", "0,2,2", "1,2,2"]
