"""The grouped step-and-check (csrc/small_step_rule.h, csrc/small.hip: hdm_grouped_step_check_kernel, csrc/engine_step_set.h,
DESIGN.md section 24): "is S + dStep dS still inside?" asked of one small SDP cone of an operator on the checker buffer puts every
member's checker there in one launch; the other members answer from their slots.

Two yardsticks from the per-cone path of the same library, both without a tolerance (np.array_equal):

- a second set of cones made from the same data, asked one by one with the switch off: the flag, what the per-cone path WRITES
  of the checker buffer and the checker factor (the triangle i >= j of the n x n part of Scheck and of L, all of Dinv), the
  barrier of the checker and a ratio test on it.  The other triangle of a cone's dual buffer is never written by the one-launch
  check and holds whatever its allocation held, so S + dStep dS there differs between two cones of equal data;
- the same cone with the switch turned off: every element of Scheck (n16 x n16) and of L and Dinv (128 x 128, L's strict upper
  triangle included, which the grouped kernel reproduces: the rectangle copy's values and the padding's zeros).

An independent yardstick (numpy, fp64) holds the flag to the sign of lambda_min(S + dStep dS) and the barrier to slogdet."""
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
from grouped_cases import EXE, GROUPED, INSTANCES, ROOT, _check_goldens, _destroy, _drive, _lp_cone  # noqa: E402
from util import load_golden, y_of  # noqa: E402

pytestmark = pytest.mark.gpu

_rule = functools.partial(grouped_cases._rule, "step")
_golden_cones = functools.partial(grouped_cases._golden_cones, _rule)
instance = grouped_cases.instance_of(_golden_cones)
_block = functools.partial(grouped_cases._block, "step")
_set = functools.partial(grouped_cases._set, "step")
_two_sets = functools.partial(grouped_cases._two_sets, "step")
ZERO = {"on": False, "launches": 0, "last_cones": 0, "total_cones": 0, "from_slots": 0, "left_out": 0}


def _try(f, *a):
    """a cone's own answer; None where its slot fails"""
    from hdsdp_amd import api
    try:
        return f(*a)
    except api.HDSDPError:
        return None


def _ask(c, step):
    from hdsdp_amd import api
    return _try(c.axpy_buffer_and_check, step, api.BUFFER_DUALCHECK)


def _written(c):
    """what the per-cone path writes of the checker: (Scheck's and L's triangle i >= j inside n x n, Dinv); the arrays are
    column-major seen in C order, element (i, j) at [j, i]"""
    Sc, L, D = c.checker_state()
    n = c.n
    up = np.triu(np.ones((n, n), dtype=bool))
    return Sc[:n, :n][up], L[:n, :n][up], D


def _same_written(gc, lc, flags, what):
    """members' checkers against the loop's, where the per-cone factorisation stood; the buffer's contents in any case"""
    for k, (a, b, ok) in enumerate(zip(gc, lc, flags)):
        x, y = _written(a), _written(b)
        assert np.array_equal(x[0], y[0]), f"{what}: cone {k} checker buffer differs at {int(np.count_nonzero(x[0] != y[0]))} places"
        if ok:
            assert np.array_equal(x[1], y[1]), f"{what}: cone {k} L differs at {int(np.count_nonzero(x[1] != y[1]))} places"
            assert np.array_equal(x[2], y[2]), f"{what}: cone {k} Dinv differs at {int(np.count_nonzero(x[2] != y[2]))} places"


def _same_after(gc, lc, flags, q, what):
    """what the line search does next: the barrier of the checker, and a ratio test on it (along the same direction, so that dS
    holds the same bits afterwards)"""
    from hdsdp_amd import api
    for k, (a, b, ok) in enumerate(zip(gc, lc, flags)):
        if not ok:
            assert _try(a.log_barrier_of, api.BUFFER_DUALCHECK) is None and _try(b.log_barrier_of, api.BUFFER_DUALCHECK) is None, (what, k)
            continue
        assert a.log_barrier_of(api.BUFFER_DUALCHECK) == b.log_barrier_of(api.BUFFER_DUALCHECK), (what, k)
        ra, rb = (_try(c.ratio_test, q[0], q[1], q[2], api.BUFFER_DUALCHECK) for c in (a, b))
        assert ra is not None and np.array_equal(ra, rb), f"{what}: cone {k} ratio test on the checker {ra} against {rb}"


def _same_cone_every_element(kkt, gc, step, members, what):
    """the members' checkers as the grouped launch left them against the same cones' per-cone path: every element"""
    flags = [_ask(c, step) for c in gc]
    grouped = [c.checker_state() for c in gc]
    assert kkt.set_grouped_step(False) == 0
    assert flags == [_ask(c, step) for c in gc], what
    for k, (c, g3) in enumerate(zip(gc, grouped)):
        for name, x, y in zip(("Scheck", "L", "Dinv"), g3, c.checker_state()):
            if name == "Scheck" or flags[k]:
                assert np.array_equal(x, y, equal_nan=True), f"{what}: cone {k} {name} differs at {int(np.count_nonzero(x != y))} places"
    assert kkt.set_grouped_step(True) == members
    return flags


def test_goldens_bit_identity_against_the_per_cone_path(instance):
    """truss1, blocks3, chain16, arrow128: after a ratio test at the golden's point, the steps 0.5, 0.98 and 1.5 x the smallest
    step (the last puts at least one cone outside): one launch per question with every member in it and members - 1 answers from
    slots; the question again: no launch; 0.8 x the step: one launch.  Flags, checker contents, barrier and the ratio test on the
    checker equal the loop's"""
    from hdsdp_amd import api
    name, g, m, loop, grp, members = instance
    tau, y = float(g["tau"][0]), y_of(g)
    q = (0.0, np.random.default_rng(7).uniform(-1.0, 1.0, m) * 1e-3 * (1.0 + np.abs(y)), 0.0)
    kkt = api.KKT(m, grp)
    try:
        assert kkt.grouped_step_info() == dict(ZERO, members=members)
        assert members == INSTANCES[name][1]
        assert all(c.check_is_interior(tau, y) for c in grp) and all(c.check_is_interior(tau, y) for c in loop)
        steps = [c.ratio_test(*q) for c in grp]
        assert steps == [c.ratio_test(*q) for c in loop]
        smin = min(steps)
        assert 0.0 < smin < 1e6, steps
        assert kkt.set_grouped_step(True) == members

        def question(step, what, launches=1):
            before = kkt.grouped_step_info()
            got = [_ask(c, step) for c in grp]
            after = kkt.grouped_step_info()
            assert after["launches"] == before["launches"] + launches, (what, before, after)
            if launches:
                assert after["last_cones"] == members and after["left_out"] == 0, (what, after)
                assert after["total_cones"] == before["total_cones"] + members
            assert after["from_slots"] == before["from_slots"] + members - launches, (what, before, after)
            want = [_ask(c, step) for c in loop]
            print(name, what, "step", step, "inside", int(np.sum([bool(f) for f in got])), "of", len(got))
            assert got == want and None not in got, (what, got, want)
            _same_written(grp, loop, got, f"{name} {what}")
            return got

        for f in (0.5, 0.98, 1.5):
            flags = question(f * smin, f"{f} x the smallest step")
            assert all(flags) if f < 1.0 else not all(flags), (f, flags)
            assert question(f * smin, f"{f} x, again", launches=0) == flags
            _same_after(grp, loop, flags, q, f"{name} {f} x")          # (rewrites dS: the next question is a launch)
        flags = question(0.8 * 1.5 * smin, "the retry with 0.8 x")
        _same_cone_every_element(kkt, grp, 0.4 * smin, members, name)
    finally:
        kkt.destroy()


def _full(c, raw):
    """a device matrix whose triangle i >= j is valid (column-major seen in C order) as a full symmetric n x n matrix"""
    n = c.n
    M = raw[:n, :n].T
    return np.tril(M) + np.tril(M, -1).T


def _step_matrix(c):
    """the step matrix of the last ratio test, observed through the primal direction's product with X = I"""
    out = np.zeros((c.n, c.n))
    c.build_primal_xsx(np.eye(c.n), out, dual_matrix=False)
    return out


def _first_bad_pivot(M):
    """index of the first non-positive pivot of a right-looking Cholesky of M in fp64, or -1"""
    M = M.copy()
    for k in range(M.shape[0]):
        if not M[k, k] > 0.0:
            return k
        col = M[k + 1:, k] / M[k, k]
        M[k + 1:, k + 1:] -= np.outer(col, M[k + 1:, k])
    return -1


M_SHAPES = 40
ALL40 = list(range(M_SHAPES))
# the sweep's chunk edges (16 k, 16 k + 1), the identity padding (n < 128), n = 1; no rows, one row, a few, all forty
SHAPES = [(1, []), (2, [7]), (15, [1, 2, 3]), (16, ALL40), (17, [11]), (21, ALL40), (64, ALL40), (65, []), (112, [5]),
          (113, [0, 9, 18, 27, 36]), (127, [20]), (128, [0, 5, 10, 15, 20, 25, 30, 35])]
RD_SHAPES = -0.3


def _pivot_directions(m):
    """(dTauStep, dy, dAdaRatio, inside step, outside step, chunk of the first bad pivot there).  dy is small beside the identity
    and objective terms; the rows' share of S itself, sum y_i A_i with |y_i| <= 0.02, has norm about 0.5 on the forty-row blocks.
    first: dS = -C - ..., S + a dS = (1 - a) C + 0.3 I - ...: at a = 1.3 the first pivot is 0.3 - 0.3 * 6 (n = 1: * 2) < 0.
    last:  dS = 10 Rd I - ... = -3 I - ..., S + a dS = C + (0.3 - 3 a) I - ...: at a = 0.93 the leading block without the last row
           is 1.5 I or more plus that 0.5, the last diagonal entry 2 + 0.3 - 2.79 < 0, and the last pivot is not above it.
    inside: a = 0.5 gives 0.5 C + 0.3 I and C - 1.2 I, both 1.3 I or more."""
    rng = np.random.default_rng(33)
    return [(-1.0, rng.uniform(-1e-3, 1e-3, m), 0.0, 0.5, 1.3, "first"), (0.0, rng.uniform(-1e-3, 1e-3, m), 10.0, 0.5, 0.93, "last")]


def test_seeded_shapes_inside_and_outside_with_the_bad_pivot_in_the_first_and_in_the_last_chunk():
    """n = 1, 2, 15, 16, 17, 21, 64, 65, 112, 113, 127 and 128 in one operator, with no rows, one row, a few or forty: an inside
    step, an outside step whose first bad pivot falls in the first chunk of the sweep, and one where it falls in the last chunk
    (where numpy finds it is asserted).  Against the loop's cones what the per-cone path writes, against the same cone with the
    switch off every element"""
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
        assert kkt.set_grouped_step(True) == len(SHAPES)
        assert all(c.check_is_interior(1.0, y0) for c in gc + lc)
        for dtau, dy, ada, inside, outside, chunk in _pivot_directions(m):
            assert [c.ratio_test(dtau, dy, ada) for c in gc] == [c.ratio_test(dtau, dy, ada) for c in lc]
            for step, want_in in ((inside, True), (outside, False)):
                launches = kkt.grouped_step_info()["launches"]
                got = [_ask(c, step) for c in gc]
                info = kkt.grouped_step_info()
                assert (info["launches"], info["last_cones"], info["left_out"]) == (launches + 1, len(SHAPES), 0), info
                want = [_ask(c, step) for c in lc]
                assert got == want, (chunk, step, got, want)
                _same_written(gc, lc, got, f"shapes, {chunk} chunk, step {step}")
                _same_after(gc, lc, got, (dtau, dy, ada), f"shapes, {chunk} chunk, step {step}")
                assert _same_cone_every_element(kkt, gc, step, len(SHAPES), f"shapes, {chunk} chunk, step {step}") == got
                for (cone, C, A), flag in zip(loop, got):
                    n = cone.n
                    bad = _first_bad_pivot(_full(cone, cone.checker_state()[0]))
                    if want_in:
                        assert flag is True and bad == -1, (n, chunk, step, flag, bad)
                    else:
                        last0 = 16 * ((n - 1) // 16)
                        assert flag is False and (0 <= bad < 16 if chunk == "first" else bad >= last0), (n, chunk, step, flag, bad)
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_numpy_yardstick_flag_is_the_sign_of_the_smallest_eigenvalue_and_the_barrier_is_slogdet():
    """with S from dual_matrix() and dS from build_primal_xsx(I, dual_matrix=False): the flag equals lambda_min(S + dStep dS) > 0
    at 0.5 and 1.5 x the exact step 1 / lambda_max(L^-1 (-dS) L^-T), and the barrier of the checker equals numpy's slogdet to
    1e-12 relative"""
    from hdsdp_amd import api
    m = M_SHAPES
    grp = _set(31, m, SHAPES)
    y0 = np.random.default_rng(32).uniform(-0.02, 0.02, m)
    dy = np.random.default_rng(34).uniform(-0.3, 0.3, m)
    try:
        gc = [b[0] for b in grp]
        for c in gc:
            c.set_start(RD_SHAPES)
        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_step(True) == len(SHAPES)
        assert all(c.check_is_interior(1.0, y0) for c in gc)
        for c in gc:
            c.ratio_test(-0.2, dy, 0.5)
        mats = [(_full(c, c.dual_matrix()), _step_matrix(c)) for c in gc]
        exact = [lm.alpha_star(S, dS) for S, dS in mats]
        a = min(exact)
        assert np.isfinite(a) and a > 0.0, exact
        for f in (0.5, 1.5):
            flags, every, rc = kkt.axpy_buffer_and_check(f * a)
            assert rc == 0 and kkt.grouped_step_info()["last_cones"] == len(SHAPES)
            for c, (S, dS), flag in zip(gc, mats, flags):
                T = S + f * a * dS
                lam = float(np.linalg.eigvalsh(T)[0])
                print(f"n {c.n} step {f} x exact: lambda_min {lam:.3e} flag {bool(flag)}")
                assert abs(lam) > 1e-9 * np.max(np.abs(T)) and bool(flag) == (lam > 0.0), (c.n, f, lam, flag)
                if flag:
                    sign, ref = np.linalg.slogdet(T)
                    ld = c.log_barrier_of(api.BUFFER_DUALCHECK)
                    print(f"    barrier {ld!r} slogdet {ref!r} relative {abs(ld - ref) / abs(ref):.2e}")
                    assert sign > 0 and abs(ld - ref) <= 1e-12 * abs(ref), (c.n, ld, ref)
            assert every == bool(np.all(flags)) and (every if f < 1.0 else not every)
        kkt.destroy()
    finally:
        _destroy(grp)


def test_a_member_that_has_never_had_a_ratio_test_fails_alone():
    """three members, a ratio test on the first and the last only: the middle one has no step matrix.  Its own call fails as the
    per-cone path's does, the others answer in one launch of two, and it is counted in left_out"""
    from hdsdp_amd import api
    m = 7
    loop, grp = _two_sets(81, m, [(11, [0, 1, 2]), (22, [2, 3]), (35, [4, 5, 6])])
    rng = np.random.default_rng(82)
    y, dy = rng.uniform(-0.02, 0.02, m), rng.uniform(-0.3, 0.3, m)
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        assert all(c.check_is_interior(1.0, y) for c in gc + lc)
        for k in (0, 2):
            assert gc[k].ratio_test(0.0, dy) == lc[k].ratio_test(0.0, dy)
        assert kkt.set_grouped_step(True) == 3
        assert _ask(gc[1], 0.1) is None and _ask(lc[1], 0.1) is None
        assert kkt.grouped_step_info()["launches"] == 0
        got = [_ask(c, 0.1) for c in gc]
        info = kkt.grouped_step_info()
        assert (info["launches"], info["last_cones"], info["left_out"], info["from_slots"]) == (1, 2, 1, 1), info
        assert got == [_ask(c, 0.1) for c in lc] and got[1] is None and got[0] is not None and got[2] is not None
        flags, every, rc = kkt.axpy_buffer_and_check(0.1)
        assert rc != 0 and not every and flags.tolist() == [bool(got[0]), False, bool(got[2])]
        _same_written([gc[0], gc[2]], [lc[0], lc[2]], [got[0], got[2]], "the two with a step matrix")
        assert gc[1].ratio_test(0.0, dy) == lc[1].ratio_test(0.0, dy)      # now it has one: it is launched alone
        assert _ask(gc[1], 0.1) == _ask(lc[1], 0.1)
        info = kkt.grouped_step_info()
        assert (info["launches"], info["last_cones"], info["left_out"]) == (2, 1, 2), info
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_members_and_others_in_one_operator():
    """three members (one of them n = 1), a block the data bound refuses (n = 120 with nine rows), an n = 130 block and an LP cone:
    the three others keep their own paths inside the same operator and every cone's answer is the loop's, through
    HMiKKTAddStepToBufferAndCheck (the plain loop while the switch is off) and cone by cone; BUFFER_DUALVAR never launches; a
    second operator over the same cones takes no member while the first set is active"""
    from hdsdp_amd import api
    m = 12
    plan = [(24, [0, 1, 2]), (1, [1, 5]), (130, [2, 3, 4]), (40, [4, 5, 6, 7]), (120, list(range(3, 12)))]
    loop, grp = _two_sets(61, m, plan)
    lp_loop, lp_grp = _lp_cone(m, 9, 62), _lp_cone(m, 9, 62)
    rng = np.random.default_rng(63)
    y, dy = rng.uniform(-0.02, 0.02, m), rng.uniform(-0.3, 0.3, m)
    try:
        for c in [b[0] for b in loop + grp] + [lp_loop, lp_grp]:
            c.set_start(-0.2)
        cones = [grp[0][0], grp[1][0], grp[2][0], lp_grp, grp[3][0], grp[4][0]]
        ref_cones = [loop[0][0], loop[1][0], loop[2][0], lp_loop, loop[3][0], loop[4][0]]
        assert [_rule(n, len(rows)) for n, rows in plan] == [True, True, False, True, False]
        kkt = api.KKT(m, cones)
        assert kkt.grouped_step_info()["members"] == 3
        assert all(c.check_is_interior(1.0, y) for c in cones + ref_cones)
        steps = [c.ratio_test(0.0, dy) for c in cones]
        assert steps == [c.ratio_test(0.0, dy) for c in ref_cones]
        smin = min(steps)
        assert 0.0 < smin < 1e6
        for k, f in enumerate((0.5, 1.5)):
            flags, every, rc = kkt.axpy_buffer_and_check(f * smin)         # switch off: the plain loop
            want = [_ask(c, f * smin) for c in ref_cones]
            assert rc == 0 and flags.tolist() == want and every == all(want) and every == (f < 1.0), (f, flags, want)
        assert kkt.grouped_step_info() == dict(ZERO, members=3)
        assert kkt.set_grouped_step(True) == 3
        for k, f in enumerate((0.6, 1.4, 0.3)):
            flags, every, rc = kkt.axpy_buffer_and_check(f * smin)
            want = [_ask(c, f * smin) for c in ref_cones]
            assert rc == 0 and flags.tolist() == want and every == all(want) and every == (f < 1.0), (f, flags, want)
            info = kkt.grouped_step_info()
            assert (info["launches"], info["last_cones"], info["total_cones"], info["from_slots"]) == (k + 1, 3, 3 * (k + 1), 2 * (k + 1)), info
        sdp = [0, 1, 2, 4, 5]
        _same_written([cones[k] for k in sdp if k != 2], [ref_cones[k] for k in sdp if k != 2], [True] * 4, "mixed")
        got = [_ask(c, 0.3 * smin) for c in cones]                          # cone by cone: the members' slots serve
        assert got == [True] * 6 and kkt.grouped_step_info()["launches"] == 3
        for k in sdp:
            assert cones[k].log_barrier_of(api.BUFFER_DUALCHECK) == ref_cones[k].log_barrier_of(api.BUFFER_DUALCHECK), k
        other = api.KKT(m, cones)
        assert other.grouped_step_info()["members"] == 0 and other.set_grouped_step(True) == 0
        other.destroy()
        assert kkt.grouped_step_info()["members"] == 3
        # the dual buffer: S itself moves, per cone
        flags, every, rc = kkt.axpy_buffer_and_check(0.2 * smin, api.BUFFER_DUALVAR)
        assert rc == 0 and flags.tolist() == [c.axpy_buffer_and_check(0.2 * smin, api.BUFFER_DUALVAR) for c in ref_cones]
        assert kkt.grouped_step_info()["launches"] == 3
        for k in sdp:
            a, b = cones[k].dual_matrix(), ref_cones[k].dual_matrix()
            up = np.triu(np.ones(a.shape, dtype=bool))
            assert np.array_equal(a[up], b[up]), k
        kkt.destroy()
    finally:
        _destroy(loop, grp)
        lp_loop.destroy(); lp_grp.destroy()


def test_every_writer_invalidates_and_the_next_call_launches_that_member_alone():
    """three members at a step all slots serve; then something is written under cone 1 -- its step matrix (a ratio test on the dual
    buffer), its dual matrix (a check at a new point), its checker (the expert check on the checker buffer; the primal recovery),
    or the perturbation followed by a ratio test -- and the same step asked of cone 1 is a launch with cone 1 alone in it, the
    other two left out; the answers and the checkers are the loop's"""
    from hdsdp_amd import api
    m = 7
    loop, grp = _two_sets(83, m, [(11, [0, 1, 2]), (22, [2, 3]), (35, [4, 5, 6])])
    rng = np.random.default_rng(84)
    y = rng.uniform(-0.02, 0.02, m)
    dy, dy2 = rng.uniform(-0.3, 0.3, m), rng.uniform(-0.3, 0.3, m)

    def perturb_then_ratio(c):
        c.set_perturb(0.05)
        return c.ratio_test(0.0, dy2)

    changes = [("a ratio test on the dual buffer", lambda c: c.ratio_test(0.01, dy2, 0.2)),
               ("a check at a new point", lambda c: c.check_is_interior(1.05, 0.5 * y)),
               ("the expert check on the checker", lambda c: c.check_is_interior_expert(1.0, 1.0, -0.4 * y, 0.3, api.BUFFER_DUALCHECK)),
               ("the primal recovery", lambda c: c.get_primal(0.5, 0.3 * y, dy2) is not None),
               ("set_perturb and a ratio test", perturb_then_ratio)]
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_step(True) == 3
        assert all(c.check_is_interior(1.0, y) for c in gc + lc)
        assert [c.ratio_test(0.0, dy) for c in gc] == [c.ratio_test(0.0, dy) for c in lc]
        launches = 0
        for k, (label, change) in enumerate(changes):
            step = 0.05 + 0.01 * k
            got = [_ask(c, step) for c in gc]
            launches += 1
            info = kkt.grouped_step_info()
            assert (info["launches"], info["last_cones"], info["left_out"]) == (launches, 3, 0), (label, info)
            assert got == [_ask(c, step) for c in lc] and None not in got, label
            assert change(gc[1]) == change(lc[1]), label
            before = kkt.grouped_step_info()["from_slots"]
            a1 = _ask(gc[1], step)
            launches += 1
            info = kkt.grouped_step_info()
            assert (info["launches"], info["last_cones"], info["left_out"], info["from_slots"]) == (launches, 1, 2, before), (label, info)
            assert a1 == _ask(lc[1], step) and a1 is not None, label
            _same_written(gc, lc, [got[0], a1, got[2]], label)
            assert [_ask(c, step) for c in gc] == [got[0], a1, got[2]]      # all three served
            info = kkt.grouped_step_info()
            assert (info["launches"], info["from_slots"]) == (launches, before + 3), (label, info)
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_lifetime():
    """a member destroyed before its operator; the switch turned off and on; the operator destroyed and a former member asked on
    its own; the next operator; HKKTInit a second time on the same operator; two operators over disjoint cones, both on: nothing
    fails, the answers are the loop's"""
    from hdsdp_amd import api
    m = 9
    plan = [(10, [0, 1]), (18, [2, 3, 4]), (31, [4, 5, 6]), (48, [6, 7, 8]), (5, [])]
    loop, grp = _two_sets(71, m, plan)
    rng = np.random.default_rng(72)
    y, dy = rng.uniform(-0.02, 0.02, m), rng.uniform(-0.3, 0.3, m)
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        assert all(c.check_is_interior(1.0, y) for c in gc + lc)
        assert [c.ratio_test(0.0, dy) for c in gc] == [c.ratio_test(0.0, dy) for c in lc]

        def same(a, b, step, what):
            got = [_ask(c, step) for c in a]
            assert got == [_ask(c, step) for c in b] and None not in got, what
            _same_written(a, b, got, what)

        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_step(True) == 5
        same(gc, lc, 0.11, "all five")
        gc[1].destroy(); lc[1].destroy()                                  # a member goes before its operator
        gc3, lc3 = [gc[0], gc[2], gc[3], gc[4]], [lc[0], lc[2], lc[3], lc[4]]
        assert kkt.grouped_step_info()["members"] == 4
        same(gc3, lc3, 0.12, "four left")
        info = kkt.grouped_step_info()
        assert (info["launches"], info["last_cones"]) == (2, 4), info
        assert kkt.set_grouped_step(False) == 0                            # off: per-cone checks, the counters stand still
        same(gc3, lc3, 0.13, "switch off")
        assert kkt.grouped_step_info()["launches"] == 2 and kkt.grouped_step_info()["on"] is False
        assert kkt.set_grouped_step(True) == 4                             # and on again: no slot survives the switch
        same(gc3, lc3, 0.13, "switch on again")
        assert kkt.grouped_step_info()["launches"] == 3
        kkt.destroy()                                                     # the operator goes: a former member answers on its own
        same(gc3, lc3, 0.14, "after the operator")
        again = api.KKT(m, gc3)                                           # free for the next operator
        assert again.set_grouped_step(True) == 4
        same(gc3, lc3, 0.15, "next operator")
        assert again.grouped_step_info()["launches"] == 1
        again.destroy()
        twice = api.KKT(m, gc3)                                           # HKKTInit twice: the set is rebuilt, switched off
        assert twice.set_grouped_step(True) == 4
        assert api.load_library().HKKTInit(twice._k, m, len(gc3), twice._cone_arr) == 0
        assert twice.grouped_step_info() == dict(ZERO, members=4)
        assert twice.set_grouped_step(True) == 4
        same(gc3, lc3, 0.16, "after a second HKKTInit")
        assert twice.grouped_step_info()["launches"] == 1
        twice.destroy()
        one, two = api.KKT(m, gc3[:2]), api.KKT(m, gc3[2:])               # two operators, both on, each with its own members
        assert one.set_grouped_step(True) == 2 and two.set_grouped_step(True) == 2
        same(gc3, lc3, 0.17, "two operators")
        for op in (one, two):
            info = op.grouped_step_info()
            assert (info["launches"], info["last_cones"], info["from_slots"]) == (1, 2, 1), info
        one.destroy(); two.destroy()
    finally:
        _destroy(loop, grp)


@pytest.mark.parametrize("name", ["arrow128_A", "chain16_A"])
def test_all_four_grouped_switches_together(name):
    """grouped check, grouped ratio test, grouped step-and-check and grouped build on one operator: the step launch writes the
    checker's factor and leaves the dual factor, whose Dinv the build's inverse kernel reads, alone: M is the golden's"""
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
        assert kkt.set_grouped_ratio(True) == ncones
        assert kkt.set_grouped_step(True) == members == ncones
        assert kkt.set_grouped_build(True) == ncones
        tau, y = float(g["tau"][0]), y_of(g)
        flags, _, every = kkt.check_is_interior(tau, y)
        assert every and flags.all() and all(c.check_is_interior(tau, y) for c in loop)
        dy = np.random.default_rng(9).uniform(-1.0, 1.0, m) * 1e-3 * (1.0 + np.abs(y))
        steps, mn = kkt.ratio_test(0.0, dy)
        assert steps.tolist() == [c.ratio_test(0.0, dy) for c in loop]
        for f in (0.7, 1.3):
            flags, every, rc = kkt.axpy_buffer_and_check(f * mn)
            assert rc == 0 and flags.tolist() == [_ask(c, f * mn) for c in loop] and every == (f < 1.0)
            _same_written(cones, loop, flags, f"{name} {f}")
        assert (kkt.grouped_check_info()["launches"], kkt.grouped_ratio_info()["launches"], kkt.grouped_step_info()["launches"]) == (1, 1, 2)
        _check_goldens(name, g, kkt, ncones)
        kkt.destroy()
    finally:
        for c in cones + loop:
            c.destroy()


# ---- HDSDP_MI355X_AFFINE_S=0 in a child process: no block tracks points, a rewritten dS must still be noticed ---------------
def _untracked_worker():
    from hdsdp_amd import api
    m = 7
    loop, grp = _two_sets(85, m, [(11, [0, 1, 2]), (22, [2, 3]), (35, [4, 5, 6])])
    rng = np.random.default_rng(86)
    y = rng.uniform(-0.02, 0.02, m)
    dys = [rng.uniform(-0.3, 0.3, m) for _ in range(3)]
    for b in loop + grp:
        b[0].set_start(-0.1)
    gc, lc = [b[0] for b in grp], [b[0] for b in loop]
    kkt = api.KKT(m, gc)
    assert kkt.set_grouped_step(True) == 3
    assert all(c.check_is_interior(1.0, y) for c in gc + lc)
    launches = 0
    for k, dy in enumerate(dys):
        if k == 2:
            assert kkt.set_grouped_ratio(True) == 3                        # the grouped ratio launch rewrites dS too
        assert [c.ratio_test(0.0, dy) for c in gc] == [c.ratio_test(0.0, dy) for c in lc]
        got = [_ask(c, 0.2) for c in gc]                                  # the same step every time: only dS has changed
        launches += 1
        info = kkt.grouped_step_info()
        assert (info["launches"], info["last_cones"]) == (launches, 3), (k, info)
        assert got == [_ask(c, 0.2) for c in lc] and None not in got, (k, got)
        _same_written(gc, lc, got, f"untracked, direction {k}")
    kkt.destroy()
    print("untracked worker: ok", launches)


def test_untracked_blocks_do_not_serve_a_stale_step_matrix():
    """HDSDP_MI355X_AFFINE_S=0: the dual state records no point of a step matrix, so only the dS counter tells that a ratio test
    has rewritten it -- per cone and through the grouped ratio launch.  The same step after each of three directions is a launch
    each time, and the checkers are the loop's"""
    env = dict(os.environ, HDSDP_MI355X_AFFINE_S="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "untracked"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "untracked worker: ok 3" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- the unchanged driver ---------------------------------------------------------------------------------------------------
# the optimum the driver prints, as tests/test_gpu_reference_driver.py expects it for the same files; every block is a member
DRIVER_CASES = {"truss1": (8.999996, "7", "7"), "chain16": (74.932288321, "16", "16")}


@pytest.mark.parametrize("inst", sorted(DRIVER_CASES))
def test_unchanged_driver_with_the_grouped_step_and_check_switched_on(inst):
    """the reference's own driver with its SDP blocks handed to the engine's cones (oracle/drop_attach.c): without any grouped
    switch, with HDSDP_MI355X_GROUPED_STEP=1 alone, and with all four grouped switches.  All reach the optimum, HKKTInit names
    every cone a member, and the iteration count and the printed final pObj / dObj are identical between the runs: the driver
    never reads the checkers the grouped launch moved behind the cone its loop broke at"""
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/sdpasolve_mi355x not built (make -C oracle drop needs the reference's sources at build time)")
    opt, nmembers, ncones = DRIVER_CASES[inst]
    runs = [_drive(inst, on) for on in ((), GROUPED[3:], GROUPED)]
    for out, its, pobj, dobj in runs:
        assert its and pobj and dobj, out[-3000:]
        assert abs(float(dobj[0]) - opt) <= 1e-4 * abs(opt), (dobj, opt)
        assert abs(float(pobj[0]) - float(dobj[0])) <= 1e-4 * abs(opt), (pobj, dobj)
    assert "HDSDP_MI355X_GROUPED_STEP" not in runs[0][0]
    for out, its, pobj, dobj in runs[1:]:
        said = re.search(r"HDSDP_MI355X_GROUPED_STEP=1: (\d+) of (\d+) cone", out)
        assert said, out[-3000:]
        print(said.group(0))
        assert (said.group(1), said.group(2)) == (nmembers, ncones), said.group(0)
        print("iterations", runs[0][1][-1], its[-1], "pObj", runs[0][2], pobj, "dObj", runs[0][3], dobj)
        assert runs[0][1] == its, (runs[0][1], its)
        assert runs[0][2] == pobj and runs[0][3] == dobj, (runs[0][2:], pobj, dobj)


if __name__ == "__main__":
    if sys.argv[1:] == ["untracked"]:
        sys.path.insert(0, ROOT)
        _untracked_worker()
