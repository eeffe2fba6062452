"""The two rules of the grouped ratio test (csrc/small_ratio_rule.h), without a device: the header is compiled alone with the
host C++ compiler and asked at its edges.  The expected values are written here from the rules as DESIGN.md section 22 states
them:

- membership: the check set's population (switch on, world == 1, resident rows, n16 <= 128, the data bound, a factor object of one
  128-block), n >= 2, the Lanczos form of the block is the LDS-resident one-launch test (HDM_LANCZOS_WHOLE not 0), and
  mloc <= n16 * (n16 + 1): the multipliers are staged in the dynamic LDS the packed triangles use later;
- a slot serves an answer only if it is valid, not yet consumed, holds exactly this question (tau, eye and every multiplier
  compared with ==) and the member's dual state counts as many transitions as when the answer was stored;
- every transition of HdmDualState moves the counter."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

DRIVER = r"""
#include "small_ratio_rule.h"
#include <cstdio>
#include <cstring>
int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "member")) {
            int on, world, resident, n, n16, npad, nblk, whole, fused;
            long mloc;
            if (scanf("%d %d %d %d %d %ld %d %d %d %d", &on, &world, &resident, &n, &n16, &mloc, &npad, &nblk, &whole, &fused) != 10) return 2;
            HdmSmallRatioCone c;
            c.chk.on = on != 0; c.chk.world = world; c.chk.resident = resident != 0; c.chk.n16 = n16; c.chk.mloc = mloc;
            c.chk.fac_npad = npad; c.chk.fac_nblk = nblk; c.n = n;
            const HdmLzSwitches sw = {whole != 0, fused != 0, true, true};
            printf("%d %ld\n", hdm_small_ratio_member(c, sw) ? 1 : 0, hdm_small_ratio_lds_doubles(n16));
        } else if (!strcmp(what, "slot")) {
            // a slot that holds (tau 0.5, eye -0.25, y = 1, 2, 3) at counter 7, asked with the given question and counter
            int valid, consumed, ny;
            unsigned long moves;
            double tau, eye, y[8];
            if (scanf("%d %d %lu %lf %lf %d", &valid, &consumed, &moves, &tau, &eye, &ny) != 6 || ny > 8) return 2;
            for (int i = 0; i < ny; ++i) if (scanf("%lf", &y[i]) != 1) return 2;
            const double held[3] = {1.0, 2.0, 3.0};
            HdmDualPoint h; h.tau = 0.5; h.eye = -0.25; h.y = held; h.ny = 3;
            HdmRatioSlot s; s.valid = valid != 0; s.consumed = consumed != 0; s.moves = 7; h.store(s.q);
            HdmDualPoint q; q.tau = tau; q.eye = eye; q.y = y; q.ny = ny;
            printf("%d\n", hdm_ratio_slot_serves(s, q, moves) ? 1 : 0);
        } else if (!strcmp(what, "moves")) {
            const double y[2] = {1.0, 2.0};
            HdmDualPoint p; p.tau = 1.0; p.eye = 0.0; p.y = y; p.ny = 2;
            HdmDualState st;
            printf("%lu", st.moves());
            st.S_assembled_at(p); printf(" %lu", st.moves());
            st.S_advanced_to(p); printf(" %lu", st.moves());
            st.S_overwritten(); printf(" %lu", st.moves());
            st.data_changed(); printf(" %lu", st.moves());
            st.S_factored(1); printf(" %lu", st.moves());
            st.factor_stale(); printf(" %lu", st.moves());
            st.dS_assembled_at(p); printf(" %lu", st.moves());
            int psd = 0;
            (void) st.S_is_at(p); (void) st.S_factored_at(p, &psd); printf(" %lu\n", st.moves());      // questions move nothing
        } else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("small_ratio_rule")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, str(src)])
    return exe


def _run(exe, line):
    return subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout.split()


def member(exe, on=1, world=1, resident=1, n=10, n16=16, mloc=3, npad=128, nblk=1, whole=1, fused=1):
    m, lds = _run(exe, f"member {on} {world} {resident} {n} {n16} {mloc} {npad} {nblk} {whole} {fused}")
    return m == "1", int(lds)


def serves(exe, valid=1, consumed=0, moves=7, tau=0.5, eye=-0.25, y=(1.0, 2.0, 3.0)):
    return _run(exe, f"slot {valid} {consumed} {moves} {tau!r} {eye!r} {len(y)} " + " ".join(repr(float(v)) for v in y)) == ["1"]


def test_the_rule_header_compiles_alone(tmp_path):
    """no HIP call, no engine state: small_ratio_rule.h by itself is a translation unit"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "small_ratio_rule.h"\nint main() { return hdm_small_ratio_lds_doubles(16) == 272 ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


def test_dimension_one_and_two(driver):
    """n == 1 keeps its closed form; n == 2 is the smallest member"""
    assert member(driver, n=1)[0] is False
    assert member(driver, n=2)[0] is True


def test_padded_dimension_edges(driver):
    """n16 = 128 is the largest block whose triangles are LDS-resident; 144 is no small block at all"""
    assert member(driver, n=128, n16=128, mloc=8) == (True, 128 * 129)
    assert member(driver, n=113, n16=128, mloc=8)[0] is True
    assert member(driver, n=128, n16=128, mloc=9)[0] is False         # the check rule's data bound: 9 * 128^2 > 2^17
    assert member(driver, n=129, n16=144, mloc=1)[0] is False
    assert member(driver, n=144, n16=144, mloc=1, npad=256, nblk=2)[0] is False


def test_the_whole_switch(driver):
    """with HDM_LANCZOS_WHOLE=0 the per-cone path runs another form (FUSED, or QUEUED): there are no members"""
    assert member(driver, whole=1, fused=0)[0] is True
    assert member(driver, whole=0, fused=1)[0] is False
    assert member(driver, whole=0, fused=0)[0] is False


def test_kind_conditions(driver):
    """two ranks, rows not resident, the one-launch check switched off, a factor object of another shape"""
    assert member(driver)[0] is True
    for bad in (dict(world=2), dict(resident=0), dict(on=0), dict(npad=256), dict(nblk=2)):
        assert member(driver, **bad)[0] is False, bad


def test_the_multipliers_fit_the_triangles_region(driver):
    """mloc <= n16 (n16 + 1), stated beside the 2 * n16 (n16 + 1) / 2 doubles of the packed triangles: 272 rows at n16 = 16 (the
    check rule alone allows 2048 there), 512 at n16 = 32 by the data bound (1056 would fit), and no rows is a member too"""
    assert member(driver, n16=16, mloc=272) == (True, 272)
    assert member(driver, n16=16, mloc=273)[0] is False
    assert member(driver, n=20, n16=32, mloc=512) == (True, 1056)
    assert member(driver, n=20, n16=32, mloc=513)[0] is False
    assert member(driver, n16=16, mloc=0)[0] is True


def test_slot_same_question(driver):
    assert serves(driver) is True


def test_slot_one_component_different(driver):
    """tau, eye, each multiplier, the number of multipliers: any one of them differing by one ulp or more is another question"""
    assert serves(driver, tau=0.5000000000000001) is False
    assert serves(driver, eye=-0.25000000000000006) is False
    assert serves(driver, eye=0.25) is False
    for k in range(3):
        y = [1.0, 2.0, 3.0]
        y[k] = float.fromhex("0x1.0000000000001p+0") * y[k]
        assert serves(driver, y=y) is False, k
    assert serves(driver, y=(1.0, 2.0)) is False
    assert serves(driver, y=(1.0, 2.0, 3.0, 0.0)) is False
    assert serves(driver, y=(1.0, 2.0, float("nan"))) is False


def test_slot_counter_moved(driver):
    assert serves(driver, moves=8) is False
    assert serves(driver, moves=6) is False


def test_slot_already_consumed_or_empty(driver):
    assert serves(driver, consumed=1) is False
    assert serves(driver, valid=0) is False


def test_every_transition_of_the_dual_state_counts(driver):
    """S_assembled_at, S_advanced_to, S_overwritten, data_changed, S_factored, factor_stale, dS_assembled_at: one each; the
    questions (S_is_at, S_factored_at) none"""
    assert _run(driver, "moves") == ["0", "1", "2", "3", "4", "5", "6", "7", "7"]
