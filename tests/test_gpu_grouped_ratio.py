"""The grouped ratio test (csrc/small_ratio_rule.h, csrc/lanczos.hip: hdm_grouped_ratio_kernel, csrc/small.hip:
hdm_grouped_safeguard_kernel, csrc/engine_ratio_set.h): a ratio test on the dual buffer asked of one small
SDP cone of an operator runs every member's test in one pair of launches; the other members fetch their answers.  The yardstick
is the per-cone path of the same library, with the switch off, on a second set of cones made from the same data: the grouped
kernel forms the per-cone sweep's sums and runs the one-launch Lanczos test's own body, so step, step matrix and what follows
from them agree bit for bit -- np.array_equal, no tolerance.  An independent yardstick (numpy's eigenvalues in fp64) holds the
steps to the margins tests/test_gpu_line_search.py uses for the per-cone path."""
import functools
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import line_search_model as lm  # noqa: E402
import grouped_cases  # noqa: E402
from grouped_cases import EXE, INSTANCES, _check_goldens, _cone_of, _destroy, _lp_cone  # noqa: E402
from util import RATIO_TOL, load_golden, y_of  # noqa: E402

pytestmark = pytest.mark.gpu

_rule = functools.partial(grouped_cases._rule, "ratio")
_golden_cones = functools.partial(grouped_cases._golden_cones, _rule)
instance = grouped_cases.instance_of(_golden_cones)
_block = functools.partial(grouped_cases._block, "ratio")
_set = functools.partial(grouped_cases._set, "ratio")
_two_sets = functools.partial(grouped_cases._two_sets, "ratio")


def _drive(inst, grouped):
    return grouped_cases._drive(inst, ("HDSDP_MI355X_GROUPED_RATIO",) if grouped else ())
ZERO = {"on": False, "launches": 0, "last_cones": 0, "total_cones": 0, "from_slots": 0, "left_out": 0, "fallbacks": 0}


def _ratio(c, dtau, dy, ada=0.0):
    """a cone's own answer; NaN where its slot fails (no factor in place)"""
    from hdsdp_amd import api
    try:
        return c.ratio_test(dtau, dy, ada)
    except api.HDSDPError:
        return np.nan


def _step_matrix(c):
    """the step matrix of the last ratio test, observed through the primal direction's product with X = I"""
    n = c.n
    out = np.zeros((n, n))
    c.build_primal_xsx(np.eye(n), out, dual_matrix=False)
    return out


def _after(cones, steps):
    """what the line search does with a step: the step matrix, and the barrier of the trial point S + step / 2 dS in the checker"""
    from hdsdp_amd import api
    finite = [s for s in steps if np.isfinite(s) and s > 0.0]
    half = 0.5 * min(finite) if finite else 0.5
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


def test_goldens_bit_identity_against_the_per_cone_path(instance):
    """truss1, blocks3, chain16, arrow128: at the golden's point three different directions in a row (a fresh test, then
    warm-started ones; one with dTauStep and dAdaRatio), then a second point and a direction again: every cone's step, its step
    matrix and the barrier of the trial point S + step / 2 dS equal the loop's; one launch pair per question with every member
    in it, members - 1 answers from slots"""
    from hdsdp_amd import api
    name, g, m, loop, grp, members = instance
    tau, y = float(g["tau"][0]), y_of(g)
    rng = np.random.default_rng(7)
    dirs = [(0.0, rng.uniform(-1.0, 1.0, m) * 1e-3 * (1.0 + np.abs(y)), 0.0) for _ in range(2)]
    dirs.append((0.01 * tau, rng.uniform(-1.0, 1.0, m) * 1e-3 * (1.0 + np.abs(y)), 0.3))
    kkt = api.KKT(m, grp)
    try:
        assert kkt.grouped_ratio_info() == dict(ZERO, members=members)
        assert kkt.set_grouped_ratio(True) == (members if members >= 2 else 0)
        assert members >= 2 and members == INSTANCES[name][1] - (1 if name == "truss1_A" else 0)      # (truss1 has one 1 x 1 block)

        def question(k, dtau, dy, ada):
            before = kkt.grouped_ratio_info()
            got = [_ratio(c, dtau, dy, ada) for c in grp]
            after = kkt.grouped_ratio_info()
            assert after["launches"] == before["launches"] + 1, (name, k, before, after)
            assert after["last_cones"] == members and after["left_out"] == 0, (name, k, after)
            assert after["total_cones"] == before["total_cones"] + members
            assert after["from_slots"] == before["from_slots"] + members - 1, (name, k, before, after)
            want = [_ratio(c, dtau, dy, ada) for c in loop]
            print(name, "question", k, "steps", np.asarray(got)[:4], "fallbacks", after["fallbacks"])
            assert np.all(np.asarray(want) > 0.0)
            _same_steps(got, want, f"{name} question {k}")
            _same_after(_after(grp, got), _after(loop, want), f"{name} question {k}")
            return got

        assert all(c.check_is_interior(tau, y) for c in grp) and all(c.check_is_interior(tau, y) for c in loop)
        steps = [question(k, dtau, dy, ada) for k, (dtau, dy, ada) in enumerate(dirs)]
        # a second point: a quarter of the second direction's smallest step along it (dTauStep = dAdaRatio = 0 there) is inside every cone
        finite = [s for s in steps[1] if np.isfinite(s)]
        y2 = y + 0.25 * min(finite + [1.0]) * dirs[1][1]
        ok = [c.check_is_interior(tau, y2) for c in grp]
        assert ok == [c.check_is_interior(tau, y2) for c in loop]
        assert all(ok), ok
        question(3, *dirs[0])
        question(4, *dirs[2])
    finally:
        kkt.destroy()


def _check_step(step, a, S, dS, what):
    """tests/test_gpu_line_search.py: _check_step, the per-cone path's margins"""
    if np.isinf(a):
        assert step == np.inf or step > 1e6, (what, step)
        return
    assert 0.0 < step <= a * (1 + 1e-12), (what, step, a)                     # conservative
    assert step >= lm.ORACLE_STEP_FLOOR * a * (1 - RATIO_TOL), (what, step, a)
    assert lm.is_pd(S + step * dS) if step < a * (1 - 1e-9) else True, (what, step, a)


M_SHAPES = 40
SHAPES = [(2, [0, 5, 23]), (15, [1, 2, 3]), (16, list(range(M_SHAPES))), (17, list(range(4, 24))), (63, [0, 7, 9, 11, 22]),
          (64, [2, 8, 13, 21]), (65, [3, 4, 30]), (127, [1, 6, 12, 18, 24, 30, 36, 39]), (128, [0, 5, 10, 15, 20, 25, 30, 35]),
          (5, []), (12, [17])]
RD_SHAPES = -0.3


def _shape_directions(m):
    """a generic direction; one that is zero on the rows of most blocks (every owned multiplier zero: the sweep is told m = 0);
    one with dTauStep; one with dAdaRatio (the residual's share: dAdaRatio * Rd on the diagonal).
    dTauStep is positive: with a negative one the block no constraint touches has dS = dTauStep C against S = C + 0.3 I, all
    eigenvalues of L^-1 (-dS) L^-T within 2 % of each other -- the reference's estimate lands 0.15 % past the exact step there, the
    safeguard cuts it by 10 %, and the per-cone path itself answers 0.9014 of the exact step (measured with dTauStep = -0.2: 4.8322
    against 5.3610, the same bits from both paths): outside the spectra the 0.95 floor of tests/line_search_model.py was measured
    on, so not a case for that margin"""
    rng = np.random.default_rng(33)
    only = np.zeros(m)
    only[[1, 2, 3]] = [0.3, -0.2, 0.25]
    return [(0.0, rng.uniform(-0.3, 0.3, m), 0.0, "generic"), (0.0, only, 0.0, "rows 1-3 only"),
            (0.05, rng.uniform(-0.3, 0.3, m), 0.0, "dTauStep"), (0.0, rng.uniform(-0.3, 0.3, m), 0.5, "dAdaRatio")]


def test_seeded_shapes_against_the_loop_and_against_the_exact_step():
    """block dimensions 2, 15, 16, 17, 63, 64, 65, 127 and 128, a block no constraint touches, a block with one row beside the
    block with all forty; four directions in a row.  Every step equals the per-cone path's bit for bit, the step matrix equals
    numpy's to 1e-13, and the step is held to the exact one, 1 / lambda_max(L^-1 (-dS) L^-T) from numpy's eigenvalues, by the
    margins of tests/test_gpu_line_search.py: never past it, at least 0.95 (1 - 1e-6) of it, and inside the cone"""
    from hdsdp_amd import api
    m = M_SHAPES
    loop, grp = _two_sets(31, m, SHAPES)
    y0 = np.random.default_rng(32).uniform(-0.02, 0.02, m)
    try:
        for b in loop + grp:
            b[0].set_start(RD_SHAPES)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        assert all(_rule(n, len(rows)) for n, rows in SHAPES)
        assert kkt.set_grouped_ratio(True) == len(SHAPES)
        assert all(c.check_is_interior(1.0, y0) for c in gc + lc)
        for k, (dtau, dy, ada, label) in enumerate(_shape_directions(m)):
            got = [_ratio(c, dtau, dy, ada) for c in gc]
            info = kkt.grouped_ratio_info()
            assert (info["launches"], info["last_cones"], info["from_slots"]) == (k + 1, len(SHAPES), (k + 1) * (len(SHAPES) - 1)), info
            want = [_ratio(c, dtau, dy, ada) for c in lc]
            _same_steps(got, want, f"shapes, {label}")
            for (cone, C, A), step in zip(grp, got):
                n = C.shape[0]
                S = lm.T(C, A, 1.0, y0, -RD_SHAPES)
                dS = lm.T(C, A, dtau, dy, ada * RD_SHAPES)
                D = _step_matrix(cone)
                assert np.max(np.abs(D - dS)) <= 1e-13 * max(np.max(np.abs(dS)), 1e-300), (n, label)
                a = lm.alpha_star(S, dS)
                print(f"shapes {label}: n {n} step {step!r} exact {a!r} ratio {step / a if np.isfinite(a) else np.nan:.6f}")
                _check_step(step, a, S, dS, (n, label))
            _same_after(_after(gc, got), _after(lc, want), f"shapes, {label}")
        print("fallbacks", kkt.grouped_ratio_info()["fallbacks"])
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_members_and_others_in_one_operator():
    """two members, an n = 1 block (its closed form), a block the rule refuses (n = 130) and an LP cone: the three keep their own
    paths inside the same operator and every cone's answer is the loop's, cone by cone and through HMiKKTRatioTest (which is the
    plain loop while the switch is off); a second operator over the same cones takes no member while the first set is active"""
    from hdsdp_amd import api
    m = 8
    plan = [(24, [0, 1, 2]), (1, [1, 5]), (130, [2, 3, 4]), (40, [4, 5, 6, 7])]
    loop, grp = _two_sets(61, m, plan)
    lp_loop, lp_grp = _lp_cone(m, 9, 62), _lp_cone(m, 9, 62)
    rng = np.random.default_rng(63)
    y = rng.uniform(-0.02, 0.02, m)
    dys = [rng.uniform(-0.3, 0.3, m) for _ in range(4)]
    try:
        for c in [b[0] for b in loop + grp] + [lp_loop, lp_grp]:
            c.set_start(-0.2)
        cones = [grp[0][0], grp[1][0], grp[2][0], lp_grp, grp[3][0]]
        ref_cones = [loop[0][0], loop[1][0], loop[2][0], lp_loop, loop[3][0]]
        kkt = api.KKT(m, cones)
        assert kkt.grouped_ratio_info()["members"] == 2
        assert all(c.check_is_interior(1.0, y) for c in cones + ref_cones)
        steps, mn = kkt.ratio_test(0.0, dys[0])                    # switch off: the plain loop
        want = [_ratio(c, 0.0, dys[0]) for c in ref_cones]
        _same_steps(steps, want, "mixed, switch off")
        assert mn == min(want) and kkt.grouped_ratio_info()["launches"] == 0
        assert kkt.set_grouped_ratio(True) == 2
        for k, (dtau, ada) in enumerate(((0.0, 0.0), (-0.1, 0.4))):
            steps, mn = kkt.ratio_test(dtau, dys[1 + k], ada)
            want = [_ratio(c, dtau, dys[1 + k], ada) for c in ref_cones]
            _same_steps(steps, want, f"mixed, question {k}")
            assert mn == min(want)
            info = kkt.grouped_ratio_info()
            assert (info["launches"], info["last_cones"], info["total_cones"], info["from_slots"]) == (k + 1, 2, 2 * (k + 1), k + 1), info
        got = [_ratio(c, 0.0, dys[3]) for c in cones]                # cone by cone
        _same_steps(got, [_ratio(c, 0.0, dys[3]) for c in ref_cones], "mixed, cone by cone")
        assert kkt.grouped_ratio_info()["launches"] == 3
        # the checker buffer stays per cone
        assert grp[0][0].axpy_buffer_and_check(0.1 * got[0], api.BUFFER_DUALCHECK) and loop[0][0].axpy_buffer_and_check(0.1 * got[0], api.BUFFER_DUALCHECK)
        a = grp[0][0].ratio_test(0.0, dys[0], 0.0, buffer=api.BUFFER_DUALCHECK)
        assert a == loop[0][0].ratio_test(0.0, dys[0], 0.0, buffer=api.BUFFER_DUALCHECK) and kkt.grouped_ratio_info()["launches"] == 3
        other = api.KKT(m, cones)
        assert other.grouped_ratio_info()["members"] == 0 and other.set_grouped_ratio(True) == 0
        other.destroy()
        assert kkt.grouped_ratio_info()["members"] == 2
        kkt.destroy()
    finally:
        _destroy(loop, grp)
        lp_loop.destroy(); lp_grp.destroy()


def test_the_safeguard_inside_an_operator():
    """the n = 15 construction of tests/test_gpu_line_search.py (there on the checker buffer, here the same point and direction on
    the dual buffer) as one of three members: after a first test along e_4 the warm-started test along e_1 at y = 0.1 e_3 stops at
    the wrong Ritz value, a step past the exact one.  The grouped safeguard's factorisation fails for that member, the host runs
    the rest (fresh-start test, cuts) for it alone: the fallback counter moves, the step equals the per-cone path's, lies inside
    the cone and is not past the exact step; the other members' steps are the loop's"""
    from hdsdp_amd import api
    n, m, Rd = 15, 4, -0.5
    C15, A15 = lm.ratio_block(n, 11 + n)
    C15, A15 = lm.from_csc(n, m, *lm.to_csc([C15] + list(A15)))

    def make():
        others = _set(91, m, [(20, [0, 1, 2]), (33, [1, 2, 3])])
        return [others[0], (_cone_of(n, m, C15, A15), C15, A15), others[1]]

    loop, grp = make(), make()
    e = np.eye(m)
    yc = 0.1 * e[2]
    try:
        for b in loop + grp:
            b[0].set_start(Rd)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_ratio(True) == 3
        assert all(c.check_is_interior(1.0, np.zeros(m)) for c in gc + lc)
        _same_steps([_ratio(c, 0.0, e[3]) for c in gc], [_ratio(c, 0.0, e[3]) for c in lc], "first test")
        assert kkt.grouped_ratio_info()["fallbacks"] == 0
        assert all(c.check_is_interior(1.0, yc) for c in gc + lc)
        got = [_ratio(c, 0.0, e[0]) for c in gc]
        want = [_ratio(c, 0.0, e[0]) for c in lc]
        info = kkt.grouped_ratio_info()
        Sc = lm.T(C15, A15, 1.0, yc, -Rd)
        dS = lm.T(C15, A15, 0.0, e[0], 0.0)
        a = lm.alpha_star(Sc, dS)
        print("n = 15 member: step", got[1], "loop", want[1], "exact", a, "info", info)
        _same_steps(got, want, "warm-started test")
        assert (info["launches"], info["last_cones"]) == (2, 3), info
        assert info["fallbacks"] >= 1, info
        assert 0.0 < got[1] <= a * (1 + 1e-12) and lm.is_pd(Sc + (1.0 - 1e-3) * got[1] * dS), (got[1], a)
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_state_a_stored_answer_is_served_once_and_only_while_nothing_has_moved():
    """three members.  A question put to cone 0 runs all three tests; then something happens to cone 1 -- a check at a new point,
    set_perturb, reduce_resi, scal_by_constant -- and its stored answer is not served: the same question to cone 1 is a second
    pair of launches with cone 0 (its answer is fetched already: a second identical question is a second, warm-started test) and
    cone 1 in it and cone 2 left out, whose stored answer is then served.  The loop mirrors every test the launches ran: equal
    steps throughout.  A member without a factor is left out and fails alone"""
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
        assert kkt.set_grouped_ratio(True) == 3
        assert all(c.check_is_interior(1.0, y) for c in gc + lc)
        changes = [("check at a new point", lambda c: c.check_is_interior(1.05, 0.5 * y)), ("set_perturb", lambda c: c.set_perturb(0.05)),
                   ("reduce_resi", lambda c: c.reduce_resi(-0.04)), ("scal_by_constant", lambda c: c.scal_by_constant(0.5))]
        # a second identical question to a cone whose answer is fetched: a launch for that cone alone, the others keep theirs
        q = (0.0, rng.uniform(-0.3, 0.3, m), 0.0)
        a, b = _ratio(gc[0], *q), _ratio(gc[0], *q)
        info = kkt.grouped_ratio_info()
        assert (info["launches"], info["last_cones"], info["left_out"], info["total_cones"], info["from_slots"]) == (2, 1, 2, 4, 0), info
        first = [_ratio(c, *q) for c in lc]
        assert (a, b) == (first[0], _ratio(lc[0], *q)), (a, b, first)
        assert _ratio(gc[1], *q) == first[1] and _ratio(gc[2], *q) == first[2]
        info = kkt.grouped_ratio_info()
        assert (info["launches"], info["from_slots"]) == (2, 2), info
        launches = 2
        for label, change in changes:
            q = (0.0, rng.uniform(-0.3, 0.3, m), 0.0)
            a0 = _ratio(gc[0], *q)                                 # every member's test runs
            first = [_ratio(c, *q) for c in lc]
            info = kkt.grouped_ratio_info()
            launches += 1
            assert (info["launches"], info["last_cones"], info["left_out"]) == (launches, 3, 0), (label, info)
            assert a0 == first[0], (label, a0, first)
            change(gc[1]); change(lc[1])
            before = kkt.grouped_ratio_info()["from_slots"]
            a1 = _ratio(gc[1], *q)                                 # not served: cone 0 (fetched) and cone 1 (moved) run again
            second = [_ratio(lc[0], *q), _ratio(lc[1], *q)]
            info = kkt.grouped_ratio_info()
            launches += 1
            assert (info["launches"], info["last_cones"], info["left_out"], info["from_slots"]) == (launches, 2, 1, before), (label, info)
            assert a1 == second[1], (label, a1, second)
            assert _ratio(gc[2], *q) == first[2] and _ratio(gc[0], *q) == second[0], label      # both served from their slots
            info = kkt.grouped_ratio_info()
            assert (info["launches"], info["from_slots"]) == (launches, before + 2), (label, info)
        # a member whose dual matrix is not positive definite has no factor: left out, and its own call fails as it does per cone
        bad = y.copy()
        bad[3] = 60.0                                              # row 3 belongs to cone 1 alone
        assert [c.check_is_interior(1.0, bad) for c in gc] == [True, False, True] == [c.check_is_interior(1.0, bad) for c in lc]
        dy = rng.uniform(-0.3, 0.3, m)
        got = [_ratio(c, 0.0, dy) for c in gc]
        info = kkt.grouped_ratio_info()
        assert (info["launches"], info["last_cones"], info["left_out"]) == (launches + 1, 2, 1), info
        assert np.isnan(got[1])
        _same_steps(got, [_ratio(c, 0.0, dy) for c in lc], "a member without a factor")
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_lifetime():
    """a member destroyed before its operator; HKKTInit a second time on the same operator; the switch turned off and on; the
    operator destroyed and a former member asked on its own; the next operator: nothing fails, the answers are the loop's"""
    from hdsdp_amd import api
    m = 9
    plan = [(10, [0, 1]), (18, [2, 3, 4]), (31, [4, 5, 6]), (48, [6, 7, 8])]
    loop, grp = _two_sets(71, m, plan)
    rng = np.random.default_rng(72)
    y = rng.uniform(-0.02, 0.02, m)
    dys = [rng.uniform(-0.3, 0.3, m) for _ in range(7)]
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        assert all(c.check_is_interior(1.0, y) for c in gc + lc)
        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_ratio(True) == 4
        _same_steps([_ratio(c, 0.0, dys[0]) for c in gc], [_ratio(c, 0.0, dys[0]) for c in lc], "all four")
        gc[1].destroy(); lc[1].destroy()                                  # a member goes before its operator
        gc3, lc3 = [gc[0], gc[2], gc[3]], [lc[0], lc[2], lc[3]]
        assert kkt.grouped_ratio_info()["members"] == 3
        _same_steps([_ratio(c, 0.0, dys[1]) for c in gc3], [_ratio(c, 0.0, dys[1]) for c in lc3], "three left")
        info = kkt.grouped_ratio_info()
        assert (info["launches"], info["last_cones"]) == (2, 3), info
        assert kkt.set_grouped_ratio(False) == 0                           # off: per-cone tests, the counters stand still
        _same_steps([_ratio(c, 0.0, dys[2]) for c in gc3], [_ratio(c, 0.0, dys[2]) for c in lc3], "switch off")
        assert kkt.grouped_ratio_info()["launches"] == 2 and kkt.grouped_ratio_info()["on"] is False
        assert kkt.set_grouped_ratio(True) == 3                            # and on again
        _same_steps([_ratio(c, 0.0, dys[3]) for c in gc3], [_ratio(c, 0.0, dys[3]) for c in lc3], "switch on again")
        assert kkt.grouped_ratio_info()["launches"] == 3
        kkt.destroy()                                                     # the operator goes: a former member answers on its own
        _same_steps([_ratio(c, 0.0, dys[4]) for c in gc3], [_ratio(c, 0.0, dys[4]) for c in lc3], "after the operator")
        again = api.KKT(m, gc3)                                           # free for the next operator
        assert again.set_grouped_ratio(True) == 3
        _same_steps([_ratio(c, 0.0, dys[5]) for c in gc3], [_ratio(c, 0.0, dys[5]) for c in lc3], "next operator")
        assert again.grouped_ratio_info()["launches"] == 1
        again.destroy()
        twice = api.KKT(m, gc3)                                           # HKKTInit twice: the set is rebuilt, switched off
        assert twice.set_grouped_ratio(True) == 3
        assert api.load_library().HKKTInit(twice._k, m, len(gc3), twice._cone_arr) == 0
        assert twice.grouped_ratio_info() == dict(ZERO, members=3)
        assert twice.set_grouped_ratio(True) == 3
        _same_steps([_ratio(c, 0.0, dys[6]) for c in gc3], [_ratio(c, 0.0, dys[6]) for c in lc3], "after a second HKKTInit")
        assert twice.grouped_ratio_info()["launches"] == 1
        twice.destroy()
    finally:
        _destroy(loop, grp)


@pytest.mark.parametrize("name", ["arrow128_A", "chain16_A"])
def test_all_three_grouped_switches_together(name):
    """grouped check, grouped ratio test and grouped build on one operator: the check's launch writes the Dinv the ratio kernel
    reads as the triangular inverse and the build's inverse kernel reads afterwards; the ratio test leaves it alone, and M is the
    golden's"""
    from hdsdp_amd import api
    g = load_golden(name)
    m = int(g["mb_dims"][1])
    ncones = INSTANCES[name][1]
    cones, members = _golden_cones(name, m)
    loop, _ = _golden_cones(name, m)
    try:
        for c in cones + loop:
            c.set_start(float(g["Rd"][0]))
        kkt = api.KKT(m, cones)
        assert kkt.set_grouped_check(True) == ncones
        assert kkt.set_grouped_ratio(True) == members == ncones
        assert kkt.set_grouped_build(True) == ncones
        tau, y = float(g["tau"][0]), y_of(g)
        flags, _, every = kkt.check_is_interior(tau, y)
        assert every and flags.all() and all(c.check_is_interior(tau, y) for c in loop)
        dy = np.random.default_rng(9).uniform(-1.0, 1.0, m) * 1e-3 * (1.0 + np.abs(y))
        steps, mn = kkt.ratio_test(0.0, dy)
        _same_steps(steps, [_ratio(c, 0.0, dy) for c in loop], name)
        assert (kkt.grouped_check_info()["launches"], kkt.grouped_ratio_info()["launches"]) == (1, 1)
        _check_goldens(name, g, kkt, ncones)
        kkt.destroy()
    finally:
        for c in cones + loop:
            c.destroy()


# the optimum the driver prints, as tests/test_gpu_reference_driver.py expects it for the same files
DRIVER_CASES = {"truss1": (8.999996, "6", "7"), "chain16": (74.932288321, "16", "16")}      # (truss1 has one 1 x 1 block)


@pytest.mark.parametrize("inst", sorted(DRIVER_CASES))
def test_unchanged_driver_with_the_grouped_ratio_test_switched_on(inst):
    """the reference's own driver with its SDP blocks handed to the engine's cones (oracle/drop_attach.c), once without and once
    with HDSDP_MI355X_GROUPED_RATIO=1: both reach the optimum, HKKTInit names six of seven / all sixteen cones, and the iteration
    count and the printed final pObj / dObj are identical between the runs"""
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/sdpasolve_mi355x not built (make -C oracle drop needs the reference's sources at build time)")
    opt, nmembers, ncones = DRIVER_CASES[inst]
    runs = [_drive(inst, grouped) for grouped in (False, True)]
    for out, its, pobj, dobj in runs:
        assert its and pobj and dobj, out[-3000:]
        assert abs(float(dobj[0]) - opt) <= 1e-4 * abs(opt), (dobj, opt)
        assert abs(float(pobj[0]) - float(dobj[0])) <= 1e-4 * abs(opt), (pobj, dobj)
    assert "HDSDP_MI355X_GROUPED_RATIO" not in runs[0][0]
    said = re.search(r"HDSDP_MI355X_GROUPED_RATIO=1: (\d+) of (\d+) cone", runs[1][0])
    assert said, runs[1][0][-3000:]
    print(said.group(0))
    assert (said.group(1), said.group(2)) == (nmembers, ncones), said.group(0)
    print("iterations", runs[0][1][-1], runs[1][1][-1], "pObj", runs[0][2], runs[1][2], "dObj", runs[0][3], runs[1][3])
    assert runs[0][1] == runs[1][1], (runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2] and runs[0][3] == runs[1][3], (runs[0][2:], runs[1][2:])
