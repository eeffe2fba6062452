"""The grouped ratio test's two opt-ins (csrc/small_ratio_rule.h, csrc/engine_ratio_set.h, csrc/lanczos.hip:
hdm_grouped_fresh_kernel, csrc/small.hip: hdm_grouped_cuts_kernel): with HMiKKTSetGroupedRatioChecker the ratio set also answers a
ratio test on BUFFER_DUALCHECK, with HMiKKTSetGroupedRatioRest the rest of the safeguard -- fresh-start test and 10 % cuts -- runs
in the grouped launch.  The yardstick is, as in tests/test_gpu_grouped_ratio.py, the per-cone path of the same library with every
switch off, on a second set of cones made from the same data, compared with np.array_equal: step, step matrix, and a following
step-and-check plus barrier on the checker.  The independent yardstick is numpy's exact step from Scheck = S + dStep dS, with the
margins of _check_step there."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import line_search_model as lm  # noqa: E402
import grouped_cases  # noqa: E402
from grouped_cases import EXE, GROUPED, INSTANCES, _cone_of, _destroy, _lp_cone  # noqa: E402
from util import RATIO_TOL, y_of  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(HERE)
_rule = functools.partial(grouped_cases._rule, "ratio")
_golden_cones = functools.partial(grouped_cases._golden_cones, _rule)
instance = grouped_cases.instance_of(_golden_cones)
_set = functools.partial(grouped_cases._set, "ratio")
_two_sets = functools.partial(grouped_cases._two_sets, "ratio")
OPT_INS = ("HDSDP_MI355X_GRATIO_CHECKER", "HDSDP_MI355X_GRATIO_REST")
NO_DETAIL = {"on": False, "checker": False, "rest": False, "checker_launches": 0, "device_rests": 0, "device_cuts": 0, "fallbacks": 0}


def _ratio(c, dtau, dy, ada=0.0, checker=False):
    """a cone's own answer on the dual buffer or on the checker; NaN where its slot fails (no factor in place)"""
    from hdsdp_amd import api
    try:
        return c.ratio_test(dtau, dy, ada, buffer=api.BUFFER_DUALCHECK if checker else api.BUFFER_DUALVAR)
    except api.HDSDPError:
        return np.nan


_chk = functools.partial(_ratio, checker=True)


def _step_matrix(c):
    n = c.n
    out = np.zeros((n, n))
    c.build_primal_xsx(np.eye(n), out, dual_matrix=False)
    return out


def _half(steps):
    finite = [s for s in steps if np.isfinite(s) and s > 0.0]
    return 0.5 * min(finite) if finite else 0.5


def _after(cones, steps):
    """what the line search does with a step: the step matrix, and the barrier of the trial point S + step / 2 dS in the checker"""
    from hdsdp_amd import api
    half = _half(steps)
    out = []
    for c in cones:
        D = _step_matrix(c)
        ok = c.axpy_buffer_and_check(half, api.BUFFER_DUALCHECK)
        out.append((D, ok, c.log_barrier_of(api.BUFFER_DUALCHECK) if ok else np.nan))
    return out


def _same_after(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]), f"{what}: cone {k} step matrix differs at {int(np.count_nonzero(x[0] != y[0]))} places"
        assert x[1] == y[1] and np.array_equal(x[2], y[2], equal_nan=True), f"{what}: cone {k} trial point {x[1:]} against {y[1:]}"


def _same_steps(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(got, want, equal_nan=True), f"{what}: steps {got.tolist()} against the loop's {want.tolist()}"


def _check_step(step, a, S, dS, what):
    """tests/test_gpu_grouped_ratio.py: _check_step, the per-cone path's margins"""
    if np.isinf(a):
        assert step == np.inf or step > 1e6, (what, step)
        return
    assert 0.0 < step <= a * (1 + 1e-12), (what, step, a)                     # conservative
    assert step >= lm.ORACLE_STEP_FLOOR * a * (1 - RATIO_TOL), (what, step, a)
    assert lm.is_pd(S + step * dS) if step < a * (1 - 1e-9) else True, (what, step, a)


def _all_on(kkt, members, rest=True):
    assert kkt.set_grouped_ratio(True) == members
    assert kkt.set_grouped_ratio_checker(True) == members
    assert kkt.set_grouped_ratio_rest(rest) == (members if rest else 0)


def test_goldens_bit_identity_against_the_per_cone_path(instance):
    """truss1, blocks3, chain16, arrow128: a dual ratio test, step-and-check at half the smallest step, then two checker questions
    in a row -- one with dAdaRatio = 1 asked cone by cone, one with dAdaRatio = 0 through HMiKKTRatioTest(..., BUFFER_DUALCHECK).
    Every cone's step, step matrix and the following step-and-check and barrier equal the loop's; one launch per question with
    every member in it, members - 1 answers from slots"""
    from hdsdp_amd import api
    name, g, m, loop, grp, members = instance
    tau, y = float(g["tau"][0]), y_of(g)
    rng = np.random.default_rng(17)
    dys = [rng.uniform(-1.0, 1.0, m) * 1e-3 * (1.0 + np.abs(y)) for _ in range(3)]
    kkt = api.KKT(m, grp)
    try:
        assert kkt.grouped_ratio_detail() == NO_DETAIL
        _all_on(kkt, members)
        assert members >= 2 and members == INSTANCES[name][1] - (1 if name == "truss1_A" else 0)
        assert all(c.check_is_interior(tau, y) for c in grp) and all(c.check_is_interior(tau, y) for c in loop)
        got, want = [_ratio(c, 0.0, dys[0]) for c in grp], [_ratio(c, 0.0, dys[0]) for c in loop]
        _same_steps(got, want, name + " dual question")
        assert kkt.grouped_ratio_detail()["checker_launches"] == 0
        half = _half(want)
        assert all(c.axpy_buffer_and_check(half, api.BUFFER_DUALCHECK) for c in grp + loop)

        def question(k, ask, dtau, dy, ada):
            before, dbefore = kkt.grouped_ratio_info(), kkt.grouped_ratio_detail()
            got = ask(dtau, dy, ada)
            after, dafter = kkt.grouped_ratio_info(), kkt.grouped_ratio_detail()
            assert after["launches"] == before["launches"] + 1, (name, k, before, after)
            assert dafter["checker_launches"] == dbefore["checker_launches"] + 1, (name, k, dbefore, dafter)
            assert after["last_cones"] == members and after["left_out"] == 0, (name, k, after)
            assert after["from_slots"] == before["from_slots"] + members - 1, (name, k, before, after)
            want = [_chk(c, dtau, dy, ada) for c in loop]
            print(name, "checker question", k, "steps", np.asarray(got)[:4], dafter)
            _same_steps(got, want, f"{name} checker question {k}")
            _same_after(_after(grp, got), _after(loop, want), f"{name} checker question {k}")

        question(0, lambda *q: [_chk(c, *q) for c in grp], 0.0, dys[1], 1.0)            # the driver's Phase-A form
        question(1, lambda *q: list(kkt.ratio_test(*q, buffer=api.BUFFER_DUALCHECK)[0]), 0.01 * tau, dys[2], 0.0)
        assert kkt.grouped_ratio_detail()["fallbacks"] == kkt.grouped_ratio_info()["fallbacks"] == 0
    finally:
        kkt.destroy()


M_SHAPES = 40
SHAPES = [(2, [0, 5, 23]), (15, [1, 2, 3]), (16, list(range(M_SHAPES))), (17, list(range(4, 24))), (63, [0, 7, 9, 11, 22]),
          (64, [2, 8, 13, 21]), (65, [3, 4, 30]), (127, [1, 6, 12, 18, 24, 30, 36, 39]), (128, [0, 5, 10, 15, 20, 25, 30, 35]),
          (5, []), (12, [17])]
RD_SHAPES = -0.3


@pytest.mark.parametrize("how", ["per-cone step-and-check", "grouped step-and-check", "expert check"])
def test_seeded_shapes_with_the_checker_put_in_place_three_ways(how):
    """block dimensions 2, 15, 16, 17, 63, 64, 65, 127 and 128, a block no row touches, a block with one row, a block with forty.
    The checker is put at a trial point by the per-cone step-and-check, by the grouped one (every grouped switch on) or by the
    expert check on the checker (which writes one triangle of the buffer only); then three checker questions in a row (rows 1-3
    only, dTauStep, dAdaRatio).  Every step is the loop's bit for bit, and is held to numpy's exact step from the checker's matrix
    by the margins of the per-cone path"""
    from hdsdp_amd import api
    m = M_SHAPES
    loop, grp = _two_sets(31, m, SHAPES)
    rng = np.random.default_rng(33)
    y0 = np.random.default_rng(32).uniform(-0.02, 0.02, m)
    only = np.zeros(m)
    only[[1, 2, 3]] = [0.3, -0.2, 0.25]
    d0 = rng.uniform(-0.3, 0.3, m)
    questions = [(0.0, only, 0.0, "rows 1-3 only"), (0.05, rng.uniform(-0.3, 0.3, m), 0.0, "dTauStep"),
                 (0.0, rng.uniform(-0.3, 0.3, m), 0.5, "dAdaRatio")]
    try:
        for b in loop + grp:
            b[0].set_start(RD_SHAPES)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        _all_on(kkt, len(SHAPES))
        if how == "grouped step-and-check":
            assert kkt.set_grouped_check(True) == len(SHAPES) and kkt.set_grouped_step(True) == len(SHAPES)
        assert all(c.check_is_interior(1.0, y0) for c in gc + lc)
        if how == "expert check":
            yc = y0 + 0.05 * d0
            assert all(c.check_is_interior_expert(1.0, -1.0, yc, -RD_SHAPES, api.BUFFER_DUALCHECK) for c in gc + lc)
            model = [lm.T(C, A, 1.0, yc, -RD_SHAPES) for _, C, A in grp]
        else:
            got, want = [_ratio(c, 0.0, d0) for c in gc], [_ratio(c, 0.0, d0) for c in lc]
            _same_steps(got, want, f"{how}: dual question")
            half = _half(want)
            assert all(c.axpy_buffer_and_check(half, api.BUFFER_DUALCHECK) for c in gc + lc)
            if how == "grouped step-and-check":
                assert kkt.grouped_step_info()["launches"] == 1
            model = [lm.T(C, A, 1.0, y0, -RD_SHAPES) + half * lm.T(C, A, 0.0, d0, 0.0) for _, C, A in grp]
        for k, (dtau, dy, ada, label) in enumerate(questions):
            got = [_chk(c, dtau, dy, ada) for c in gc]
            info, detail = kkt.grouped_ratio_info(), kkt.grouped_ratio_detail()
            assert (detail["checker_launches"], info["last_cones"], info["left_out"]) == (k + 1, len(SHAPES), 0), (how, label, info, detail)
            want = [_chk(c, dtau, dy, ada) for c in lc]
            _same_steps(got, want, f"{how}, {label}")
            for (cone, C, A), Sc, step in zip(grp, model, got):
                n = C.shape[0]
                dS = lm.T(C, A, dtau, dy, ada * RD_SHAPES)
                D = _step_matrix(cone)
                assert np.max(np.abs(D - dS)) <= 1e-13 * max(np.max(np.abs(dS)), 1e-300), (n, label)
                a = lm.alpha_star(Sc, dS)
                print(f"{how}, {label}: n {n} step {step!r} exact {a!r} ratio {step / a if np.isfinite(a) else np.nan:.6f}")
                _check_step(step, a, Sc, dS, (how, n, label))
        # the line search goes on from the last question: the step-and-check and the barrier that follow are the loop's too
        _same_after(_after(gc, got), _after(lc, want), how)
        print(how, kkt.grouped_ratio_detail())
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_left_out_members_and_other_cones_in_one_operator():
    """four members, an n = 1 block, an n = 130 block and an LP cone.  One member's trial step was outside the cone -- its checker
    holds no factorisation: its call fails and it is left out --, one member never had a checker: its call fails and it is not
    asked; the other two are answered by one launch, the three other cones by their own paths: all as the loop answers"""
    from hdsdp_amd import api
    m = 8
    plan = [(24, [0, 1, 2]), (1, [1, 5]), (130, [2, 3, 4]), (40, [4, 5, 6, 7]), (33, [0, 3, 6]), (20, [1, 4, 7])]
    loop, grp = _two_sets(61, m, plan)
    lp_loop, lp_grp = _lp_cone(m, 9, 62), _lp_cone(m, 9, 62)
    rng = np.random.default_rng(63)
    y = rng.uniform(-0.02, 0.02, m)
    dys = [rng.uniform(-0.3, 0.3, m) for _ in range(3)]
    NEVER, OUTSIDE = 4, 5
    try:
        for c in [b[0] for b in loop + grp] + [lp_loop, lp_grp]:
            c.set_start(-0.2)
        gs, ls = [b[0] for b in grp], [b[0] for b in loop]
        cones, ref = gs[:3] + [lp_grp] + gs[3:], ls[:3] + [lp_loop] + ls[3:]
        kkt = api.KKT(m, cones)
        _all_on(kkt, 4)
        assert all(c.check_is_interior(1.0, y) for c in cones + ref)
        steps, _ = kkt.ratio_test(0.0, dys[0])
        want = [_ratio(c, 0.0, dys[0]) for c in ref]
        _same_steps(steps, want, "dual question")
        half = _half([s for k, s in enumerate(want) if k != 3])
        for k, (a, b) in enumerate(zip(gs, ls)):
            if k == NEVER:
                continue
            step = 1.5 * want[6] if k == OUTSIDE else half              # (cones[6] is gs[5])
            assert a.axpy_buffer_and_check(step, api.BUFFER_DUALCHECK) == b.axpy_buffer_and_check(step, api.BUFFER_DUALCHECK) == (k != OUTSIDE)
        for q, (dtau, ada) in enumerate(((0.0, 1.0), (-0.05, 0.0))):
            before = kkt.grouped_ratio_info()
            got = [_chk(c, dtau, dys[1 + q], ada) for c in gs]
            after = kkt.grouped_ratio_info()
            want = [_chk(c, dtau, dys[1 + q], ada) for c in ls]
            print("mixed, checker question", q, got, after)
            _same_steps(got, want, f"mixed, checker question {q}")
            assert np.isnan(got[NEVER]) and np.isnan(got[OUTSIDE]) and not np.any(np.isnan(np.delete(got, [NEVER, OUTSIDE])))
            assert (after["launches"], after["last_cones"], after["left_out"]) == (before["launches"] + 1, 2, 1), (before, after)
            assert after["from_slots"] == before["from_slots"] + 1
        assert kkt.grouped_ratio_detail()["checker_launches"] == 2
        kkt.destroy()
    finally:
        _destroy(loop, grp)
        lp_loop.destroy(); lp_grp.destroy()


def test_slot_transitions_of_a_checker_answer():
    """three members.  The same question a second time launches again; axpy_buffer_and_check, reduce_resi and set_perturb on one
    member make its stored answer miss while the others' are served; a dual-buffer ratio test in between replaces every slot.  The
    loop mirrors every test the launches ran: equal steps throughout"""
    from hdsdp_amd import api
    m = 7
    plan = [(11, [0, 1, 2]), (22, [2, 3]), (35, [4, 5, 6])]
    loop, grp = _two_sets(81, m, plan)
    rng = np.random.default_rng(82)
    y = rng.uniform(-0.02, 0.02, m)
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        _all_on(kkt, 3)
        assert all(c.check_is_interior(1.0, y) for c in gc + lc)
        d0 = rng.uniform(-0.3, 0.3, m)
        want = [_ratio(c, 0.0, d0) for c in lc]
        _same_steps([_ratio(c, 0.0, d0) for c in gc], want, "dual question")
        half = _half(want)
        assert all(c.axpy_buffer_and_check(half, api.BUFFER_DUALCHECK) for c in gc + lc)
        launches = kkt.grouped_ratio_info()["launches"]
        # the same question a second time to a cone whose answer is fetched: a launch for that cone alone
        q = (0.0, rng.uniform(-0.3, 0.3, m), 1.0)
        a, b = _chk(gc[0], *q), _chk(gc[0], *q)
        launches += 2
        info = kkt.grouped_ratio_info()
        assert (info["launches"], info["last_cones"], info["left_out"]) == (launches, 1, 2), info
        first = [_chk(c, *q) for c in lc]
        assert (a, b) == (first[0], _chk(lc[0], *q)), (a, b, first)
        assert _chk(gc[1], *q) == first[1] and _chk(gc[2], *q) == first[2]
        assert kkt.grouped_ratio_info()["launches"] == launches
        def step_again(c):                                         # (along the last question's step matrix: a short step stays inside)
            assert c.axpy_buffer_and_check(0.1 * half, api.BUFFER_DUALCHECK)

        changes = [("axpy_buffer_and_check", step_again),
                   ("reduce_resi", lambda c: c.reduce_resi(-0.04)), ("set_perturb", lambda c: c.set_perturb(0.05))]
        for label, change in changes:
            q = (0.0, rng.uniform(-0.3, 0.3, m), 0.5)
            a0 = _chk(gc[0], *q)                                   # every member's test runs
            first = [_chk(c, *q) for c in lc]
            launches += 1
            info = kkt.grouped_ratio_info()
            assert (info["launches"], info["last_cones"], info["left_out"]) == (launches, 3, 0), (label, info)
            assert a0 == first[0], (label, a0, first)
            change(gc[1]); change(lc[1])
            before = kkt.grouped_ratio_info()["from_slots"]
            a1 = _chk(gc[1], *q)                                   # not served: cone 0 (fetched) and cone 1 (changed) run again
            second = [_chk(lc[0], *q), _chk(lc[1], *q)]
            launches += 1
            info = kkt.grouped_ratio_info()
            assert (info["launches"], info["last_cones"], info["left_out"], info["from_slots"]) == (launches, 2, 1, before), (label, info)
            assert a1 == second[1], (label, a1, second)
            assert _chk(gc[2], *q) == first[2] and _chk(gc[0], *q) == second[0], label      # both served from their slots
            info = kkt.grouped_ratio_info()
            assert (info["launches"], info["from_slots"]) == (launches, before + 2), (label, info)
        # a dual-buffer question in between: one launch replaces every member's slot, and the checker question runs everywhere again
        q = (0.0, rng.uniform(-0.3, 0.3, m), 0.0)
        a0 = _chk(gc[0], *q)
        first = [_chk(c, *q) for c in lc]
        d1 = rng.uniform(-0.3, 0.3, m)
        b1 = _ratio(gc[1], 0.0, d1)
        mid = [_ratio(c, 0.0, d1) for c in lc]
        launches += 2
        info = kkt.grouped_ratio_info()
        assert (info["launches"], info["last_cones"], info["left_out"]) == (launches, 3, 0), info
        a1 = _chk(gc[1], *q)
        second = [_chk(c, *q) for c in lc]
        launches += 1
        info = kkt.grouped_ratio_info()
        assert (info["launches"], info["last_cones"], info["left_out"]) == (launches, 3, 0), info
        assert (a0, b1, a1) == (first[0], mid[1], second[1])
        assert _chk(gc[0], *q) == second[0] and _chk(gc[2], *q) == second[2] and kkt.grouped_ratio_info()["launches"] == launches
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_a_checker_launch_makes_the_step_sets_slot_miss():
    """ratio set and step set on one operator: a step-and-check answer stored for a member is not served once a checker ratio
    launch has rewritten that member's step matrix -- the step set launches again, and the flags are the loop's"""
    from hdsdp_amd import api
    m = 7
    plan = [(11, [0, 1, 2]), (22, [2, 3]), (35, [4, 5, 6])]
    loop, grp = _two_sets(83, m, plan)
    rng = np.random.default_rng(84)
    y = rng.uniform(-0.02, 0.02, m)
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        _all_on(kkt, 3)
        assert kkt.set_grouped_step(True) == 3
        assert all(c.check_is_interior(1.0, y) for c in gc + lc)
        d0, d1 = rng.uniform(-0.3, 0.3, m), rng.uniform(-0.3, 0.3, m)
        want = [_ratio(c, 0.0, d0) for c in lc]
        _same_steps([_ratio(c, 0.0, d0) for c in gc], want, "dual question")
        half = _half(want)
        assert gc[0].axpy_buffer_and_check(half, api.BUFFER_DUALCHECK) and all(c.axpy_buffer_and_check(half, api.BUFFER_DUALCHECK) for c in lc)
        s0 = kkt.grouped_step_info()
        assert gc[1].axpy_buffer_and_check(half, api.BUFFER_DUALCHECK)                    # served from its slot
        s1 = kkt.grouped_step_info()
        assert (s0["launches"], s1["launches"], s1["from_slots"]) == (1, 1, s0["from_slots"] + 1), (s0, s1)
        got, want = [_chk(c, 0.0, d1, 1.0) for c in gc], [_chk(c, 0.0, d1, 1.0) for c in lc]
        _same_steps(got, want, "checker question")
        flag = gc[1].axpy_buffer_and_check(half, api.BUFFER_DUALCHECK)                    # the same step: the step matrix is another
        s2 = kkt.grouped_step_info()
        assert s2["launches"] == 2 and s2["from_slots"] == s1["from_slots"], (s1, s2)
        assert [flag, gc[0].axpy_buffer_and_check(half), gc[2].axpy_buffer_and_check(half)] == [lc[k].axpy_buffer_and_check(half) for k in (1, 0, 2)]
        assert [c.log_barrier_of(api.BUFFER_DUALCHECK) for c in gc] == [c.log_barrier_of(api.BUFFER_DUALCHECK) for c in lc]
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def _n15_operator(m):
    """the n = 15 construction of tests/test_gpu_line_search.py as one of three members"""
    n = 15
    C15, A15 = lm.ratio_block(n, 11 + n)
    C15, A15 = lm.from_csc(n, m, *lm.to_csc([C15] + list(A15)))
    others = _set(91, m, [(20, [0, 1, 2]), (33, [1, 2, 3])])
    return [others[0], (_cone_of(n, m, C15, A15), C15, A15), others[1]]


@pytest.mark.parametrize("buffer,checker,rest", [("dual", False, True), ("checker", True, True), ("checker", True, False), ("dual", True, True)])
def test_the_rest_of_the_safeguard_on_the_device(buffer, checker, rest):
    """after a first test along e_4 the warm-started test along e_1 at y = 0.1 e_3 stops at the wrong Ritz value, a step past the
    exact one -- on the dual buffer after a check at that point, on the checker buffer after the expert check put the checker
    there.  With the rest's switch on the launch itself runs the fresh-start test and the cuts for that member: device rests >= 1,
    no host fallback, the step is the per-cone path's bit for bit, lies inside the cone and is not past the exact step.  With the
    rest's switch off (the checker's on) the host runs it: fallbacks >= 1, no device rest, the same step.  A question where nobody
    leaves the cone moves neither counter"""
    from hdsdp_amd import api
    m, Rd = 4, -0.5
    loop, grp = _n15_operator(m), _n15_operator(m)
    e = np.eye(m)
    yc = 0.1 * e[2]
    on_checker = buffer == "checker"
    ask = _chk if on_checker else _ratio
    try:
        for b in loop + grp:
            b[0].set_start(Rd)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_ratio(True) == 3
        assert kkt.set_grouped_ratio_checker(checker) == (3 if checker else 0)
        assert kkt.set_grouped_ratio_rest(rest) == (3 if rest else 0)
        detail = kkt.grouped_ratio_detail()
        assert (detail["on"], detail["checker"], detail["rest"]) == (True, checker, rest), detail
        assert all(c.check_is_interior(1.0, np.zeros(m)) for c in gc + lc)
        _same_steps([_ratio(c, 0.0, e[3]) for c in gc], [_ratio(c, 0.0, e[3]) for c in lc], "first test")       # nobody leaves the cone
        detail = kkt.grouped_ratio_detail()
        assert (detail["device_rests"], detail["device_cuts"], detail["fallbacks"]) == (0, 0, 0), detail
        if on_checker:
            assert all(c.check_is_interior_expert(1.0, -1.0, yc, -Rd, api.BUFFER_DUALCHECK) for c in gc + lc)
        else:
            assert all(c.check_is_interior(1.0, yc) for c in gc + lc)
        got = [ask(c, 0.0, e[0]) for c in gc]
        want = [ask(c, 0.0, e[0]) for c in lc]
        info, detail = kkt.grouped_ratio_info(), kkt.grouped_ratio_detail()
        C15, A15 = grp[1][1], grp[1][2]
        Sc = lm.T(C15, A15, 1.0, yc, -Rd)
        dS = lm.T(C15, A15, 0.0, e[0], 0.0)
        a = lm.alpha_star(Sc, dS)
        print(f"n = 15 member on the {buffer} buffer: step", got[1], "loop", want[1], "exact", a, info, detail)
        _same_steps(got, want, "warm-started test")
        assert (info["launches"], info["last_cones"]) == (2, 3), info
        assert detail["checker_launches"] == (1 if on_checker else 0), detail
        if rest:
            assert detail["device_rests"] >= 1 and detail["fallbacks"] == 0 and info["fallbacks"] == 0, (info, detail)
        else:
            assert detail["device_rests"] == 0 and detail["fallbacks"] >= 1 and info["fallbacks"] == detail["fallbacks"], (info, detail)
        assert 0.0 < got[1] <= a * (1 + 1e-12) and lm.is_pd(Sc + (1.0 - 1e-3) * got[1] * dS), (got[1], a)
        kkt.destroy()
    finally:
        _destroy(loop, grp)


@pytest.mark.parametrize("buffer", ["dual", "checker"])
def test_a_step_that_needs_a_cut_is_cut_on_the_device(buffer):
    """the block no constraint touches with dTauStep = -0.2: dS = -0.2 C against S = C + 0.3 I, every eigenvalue of the pencil
    within 2 % of the others.  The reference's estimate -- warm or fresh -- lands a little past the exact step, the safeguard cuts
    it by 10 % (tests/test_gpu_grouped_ratio.py records 0.9014 of the exact step from both paths): at least one cut is made on the
    device, no host fallback, and the step is the per-cone path's bit for bit"""
    from hdsdp_amd import api
    m = 12

    def make():
        # (the untouched block is block 9 of seed 31, the one that comment measured; the CPU oracle's recurrence from the fresh start
        # gives 1.0015 of the exact step for it, and the same again from the fresh start: one cut)
        return [grouped_cases._block("ratio", np.random.default_rng([31, k]), n, m, rows)
                for k, (n, rows) in ((9, (5, [])), (10, (12, [3])), (2, (16, list(range(m)))))]

    loop, grp = make(), make()
    rng = np.random.default_rng(35)
    y0 = rng.uniform(-0.02, 0.02, m)
    on_checker = buffer == "checker"
    ask = _chk if on_checker else _ratio
    try:
        for b in loop + grp:
            b[0].set_start(RD_SHAPES)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        _all_on(kkt, 3)
        assert all(c.check_is_interior(1.0, y0) for c in gc + lc)
        if on_checker:
            assert all(c.check_is_interior_expert(1.0, -1.0, y0, -RD_SHAPES, api.BUFFER_DUALCHECK) for c in gc + lc)
        dy = rng.uniform(-0.3, 0.3, m)
        got, want = [ask(c, -0.2, dy) for c in gc], [ask(c, -0.2, dy) for c in lc]
        info, detail = kkt.grouped_ratio_info(), kkt.grouped_ratio_detail()
        C, A = grp[0][1], grp[0][2]
        S, dS = lm.T(C, A, 1.0, y0, -RD_SHAPES), lm.T(C, A, -0.2, dy, 0.0)
        a = lm.alpha_star(S, dS)
        print(f"{buffer}: untouched block step {got[0]!r} loop {want[0]!r} exact {a!r} ratio {got[0] / a:.6f}", info, detail)
        _same_steps(got, want, "dTauStep = -0.2")
        assert detail["device_rests"] >= 1 and detail["device_cuts"] >= 1 and detail["fallbacks"] == 0, detail
        assert 0.0 < got[0] <= a * (1 + 1e-12) and lm.is_pd(S + (1.0 - 1e-3) * got[0] * dS), (got[0], a)
        # the next question, warm-started from what the launch left, is the loop's too
        dy = rng.uniform(-0.3, 0.3, m)
        _same_steps([ask(c, 0.05, dy) for c in gc], [ask(c, 0.05, dy) for c in lc], "the question after")
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_switches_and_lifetimes():
    """each opt-in acts only while the grouped ratio test is on; off again, or the set switched, both are off and what they made
    is freed; HKKTInit a second time turns everything off; a second operator over the same cones takes no member"""
    from hdsdp_amd import api
    m = 9
    plan = [(10, [0, 1]), (18, [2, 3, 4]), (31, [4, 5, 6])]
    loop, grp = _two_sets(71, m, plan)
    rng = np.random.default_rng(72)
    y = rng.uniform(-0.02, 0.02, m)
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        assert all(c.check_is_interior(1.0, y) for c in gc + lc)
        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_ratio_checker(True) == 0 and kkt.set_grouped_ratio_rest(True) == 0      # the set is not on
        assert kkt.grouped_ratio_detail() == NO_DETAIL
        _all_on(kkt, 3)
        assert kkt.grouped_ratio_detail() == dict(NO_DETAIL, on=True, checker=True, rest=True)
        assert sorted(kkt.grouped_ratio_info()) == sorted(["on", "members", "launches", "last_cones", "total_cones", "from_slots", "left_out", "fallbacks"])
        other = api.KKT(m, gc)                                            # a second operator over the same cones takes no member
        assert other.set_grouped_ratio(True) == 0 and other.set_grouped_ratio_checker(True) == 0 and other.set_grouped_ratio_rest(True) == 0
        assert other.grouped_ratio_detail() == NO_DETAIL
        other.destroy()

        def round_(label, launches):
            d = rng.uniform(-0.3, 0.3, m)
            want = [_ratio(c, 0.0, d) for c in lc]
            _same_steps([_ratio(c, 0.0, d) for c in gc], want, label + ": dual")
            half = _half(want)
            assert all(c.axpy_buffer_and_check(half, api.BUFFER_DUALCHECK) for c in gc + lc)
            d = rng.uniform(-0.3, 0.3, m)
            _same_steps([_chk(c, 0.0, d, 1.0) for c in gc], [_chk(c, 0.0, d, 1.0) for c in lc], label + ": checker")
            assert kkt.grouped_ratio_detail()["checker_launches"] == launches, (label, kkt.grouped_ratio_detail())

        round_("all on", 1)
        assert kkt.set_grouped_ratio_checker(False) == 0 and kkt.set_grouped_ratio_rest(False) == 0
        assert kkt.grouped_ratio_detail() == dict(NO_DETAIL, on=True, checker_launches=1)
        round_("opt-ins off", 1)                                          # the checker question is per cone again
        assert kkt.set_grouped_ratio_checker(True) == 3
        round_("checker on again", 2)
        assert kkt.set_grouped_ratio(False) == 0                           # the set off: both opt-ins go with it
        assert kkt.grouped_ratio_detail() == dict(NO_DETAIL, checker_launches=2)
        round_("set off", 2)
        assert kkt.set_grouped_ratio(True) == 3
        assert kkt.grouped_ratio_detail() == dict(NO_DETAIL, on=True, checker_launches=2)
        _all_on(kkt, 3)
        round_("all on again", 3)
        assert api.load_library().HKKTInit(kkt._k, m, len(gc), kkt._cone_arr) == 0
        assert kkt.grouped_ratio_detail() == NO_DETAIL
        round_("after a second HKKTInit", 0)
        kkt.destroy()
        round_ = None
    finally:
        _destroy(loop, grp)


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import functools, grouped_cases
from hdsdp_amd import api
blocks = grouped_cases._set("ratio", 5, 6, [(10, [0, 1]), (18, [2, 3, 4]), (31, [4, 5])])
kkt = api.KKT(6, [b[0] for b in blocks])
print("DETAIL", sorted(kkt.grouped_ratio_detail().items()))
print("INFO", kkt.grouped_ratio_info()["on"])
kkt.destroy()
for b in blocks:
    b[0].destroy()
"""


@pytest.mark.parametrize("names", [("HDSDP_MI355X_GROUPED_RATIO", OPT_INS[0]), ("HDSDP_MI355X_GROUPED_RATIO", OPT_INS[1]), OPT_INS],
                         ids=["ratio+checker", "ratio+rest", "opt-ins alone"])
def test_the_environment_switches_in_a_fresh_process(names, tmp_path):
    """read at HKKTInit: with the grouped ratio test's own switch each opt-in goes on and HKKTInit says so; without it HKKTInit
    prints why and does nothing"""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = {k: v for k, v in os.environ.items() if k not in GROUPED + OPT_INS}
    env.update({k: "1" for k in names})
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    detail = dict(eval(re.search(r"^DETAIL (.*)$", r.stdout, re.M).group(1)))
    with_set = "HDSDP_MI355X_GROUPED_RATIO" in names
    assert detail == dict(NO_DETAIL, on=with_set, checker=with_set and OPT_INS[0] in names, rest=with_set and OPT_INS[1] in names), (detail, out[-2000:])
    for k in OPT_INS:
        said = re.search(re.escape(k) + r"=1: (.*)", out)
        assert bool(said) == (k in names), out[-2000:]
        if said:
            print(said.group(0))
            assert ("3 of 3 cone(s)" in said.group(1)) == with_set and ("nothing to do" in said.group(1)) == (not with_set), said.group(0)


DRIVER_CASES = {"truss1": (8.999996, "6", "7"), "chain16": (74.932288321, "16", "16")}      # (truss1 has one 1 x 1 block)


@pytest.mark.parametrize("inst", sorted(DRIVER_CASES))
def test_unchanged_driver_with_all_six_grouped_switches(inst):
    """the reference's own driver with its SDP blocks handed to the engine's cones, once with no grouped switch and once with all
    six: both reach the optimum, HKKTInit names the members of both opt-ins, and the iteration numbers and the printed pObj / dObj
    are identical between the runs"""
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/sdpasolve_mi355x not built (make -C oracle drop needs the reference's sources at build time)")
    opt, nmembers, ncones = DRIVER_CASES[inst]
    clean = {k: os.environ.pop(k) for k in OPT_INS if k in os.environ}
    try:
        runs = [grouped_cases._drive(inst, ()), grouped_cases._drive(inst, GROUPED + OPT_INS)]
    finally:
        os.environ.update(clean)
    for out, its, pobj, dobj in runs:
        assert its and pobj and dobj, out[-3000:]
        assert abs(float(dobj[0]) - opt) <= 1e-4 * abs(opt), (dobj, opt)
        assert abs(float(pobj[0]) - float(dobj[0])) <= 1e-4 * abs(opt), (pobj, dobj)
    assert "GRATIO" not in runs[0][0]
    for k in OPT_INS:
        said = re.search(re.escape(k) + r"=1: (\d+) of (\d+) cone", runs[1][0])
        assert said, runs[1][0][-3000:]
        print(said.group(0))
        assert (said.group(1), said.group(2)) == (nmembers, ncones), said.group(0)
    print("iterations", runs[0][1][-1], runs[1][1][-1], "pObj", runs[0][2], runs[1][2], "dObj", runs[0][3], runs[1][3])
    assert runs[0][1] == runs[1][1], (runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2] and runs[0][3] == runs[1][3], (runs[0][2:], runs[1][2:])
