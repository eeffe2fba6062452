"""The grouped interior check (csrc/small_check_rule.h, csrc/small.hip: hdm_grouped_check_kernel, csrc/engine_check_set.h,
DESIGN.md section 19): a point question put to one small SDP cone of an operator answers all of them in one launch.  The
yardstick is the per-cone path of the same library on a second set of cones made from the same data: the grouped kernel runs
the one-launch check's own body, so dual matrix, log det, flag and a following ratio test agree bit for bit -- no tolerance."""
import functools
import os
import re

import numpy as np
import pytest

import grouped_cases
from grouped_cases import EXE, INSTANCES, _destroy, _lp_cone
from util import load_golden, y_of

pytestmark = pytest.mark.gpu

_rule = functools.partial(grouped_cases._rule, "check")
_golden_cones = functools.partial(grouped_cases._golden_cones, _rule)
instance = grouped_cases.instance_of(_golden_cones)
_block = functools.partial(grouped_cases._block, "check")
_set = functools.partial(grouped_cases._set, "check")
_two_sets = functools.partial(grouped_cases._two_sets, "check")
_check_goldens = functools.partial(grouped_cases._check_goldens, full=True)


def _drive(inst, grouped):
    return grouped_cases._drive(inst, ("HDSDP_MI355X_GROUPED_CHECK",) if grouped else ())


def _ask(cones, tau, y, dtau, dy, stop_at_first_failure=False):
    """the driver's questions at one point, cone by cone: interior, then the barrier at that point, then the dual matrix and a
    ratio test along (dtau, dy); one tuple per cone"""
    flags = []
    for c in cones:
        flags.append(c.check_is_interior(tau, y))
        if stop_at_first_failure and not flags[-1]:
            return flags
    out = []
    for c, ok in zip(cones, flags):
        ld = c.log_barrier(tau, y) if ok else np.nan
        S = c.dual_matrix()
        step = c.ratio_test(dtau, dy) if ok else np.nan
        out.append((ok, ld, S, step))
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0], f"{what}: cone {k} flag {x[0]} against {y[0]}"
        assert np.array_equal(x[1], y[1], equal_nan=True), f"{what}: cone {k} log det {x[1]!r} against {y[1]!r}"
        # (dual_matrix() copies the whole buffer; the check writes the lower triangle of S -- the upper one of the C-order view --
        # and the other triangle of a buffer is whatever its allocation held: two cones' never agree on that)
        bad = np.argwhere(np.triu(x[2]) != np.triu(y[2]))
        assert bad.size == 0, f"{what}: cone {k} dual matrix differs at {len(bad)} places of its written triangle, first {bad[:3].tolist()}"
        assert np.array_equal(x[3], y[3], equal_nan=True), f"{what}: cone {k} ratio test {x[3]!r} against {y[3]!r}"


def _full(D):
    """dual_matrix() is column-major seen in C order; the lower triangle of S is what the check writes"""
    U = np.triu(D)
    return U + np.triu(D, 1).T


def _points(g, m):
    tau, y = float(g["tau"][0]), y_of(g)
    rng = np.random.default_rng(5)
    dy = rng.uniform(-1.0, 1.0, m) * 1e-3 * (1.0 + np.abs(y))
    return [(tau, y, 0.0, dy), (tau, 0.75 * y, 0.0, -dy), (1.25 * tau, y, 0.01, dy)]


def test_bit_identity_against_the_per_cone_path(instance):
    """truss1, blocks3, chain16, arrow128 at the golden's point and two more (one with another tau): every cone's dual matrix,
    log det, flag and following ratio-test step equal the per-cone path's; one launch per new point with every member in it,
    and members - 1 of the loop's interior calls answered from state"""
    from hdsdp_amd import api
    name, g, m, loop, grp, members = instance
    kkt = api.KKT(m, grp)
    try:
        assert kkt.grouped_check_info() == {"on": False, "members": members, "launches": 0, "last_cones": 0, "total_cones": 0,
                                            "from_state": 0, "left_out": 0}
        assert kkt.set_grouped_check(True) == (members if members >= 2 else 0)
        on = members >= 2
        for k, (tau, y, dtau, dy) in enumerate(_points(g, m)):
            before = kkt.grouped_check_info()
            flags = [c.check_is_interior(tau, y) for c in grp]
            after = kkt.grouped_check_info()
            if k == 0:
                assert all(flags), "the golden's point is interior"
            if on:
                assert after["launches"] == before["launches"] + 1, (name, k, before, after)
                assert after["last_cones"] == members and after["left_out"] == 0
                assert after["total_cones"] == before["total_cones"] + members
                assert after["from_state"] == before["from_state"] + members - 1
            else:
                assert after["launches"] == 0
            got = _ask(grp, tau, y, dtau, dy)
            if on:     # the interior calls again, the barriers: all from state, no further launch
                last = kkt.grouped_check_info()
                assert last["launches"] == after["launches"] and last["from_state"] >= after["from_state"] + members
            _same(got, _ask(loop, tau, y, dtau, dy), f"{name} point {k}")
    finally:
        kkt.destroy()


M_SHAPES = 40
SHAPES = [(1, [0, 5, 23]), (15, [1, 2, 3]), (16, list(range(M_SHAPES))), (17, list(range(4, 24))), (63, [0, 7, 9, 11, 22]),
          (64, [2, 8, 13, 21]), (65, [3, 4, 30]), (127, [1, 6, 12, 18, 24, 30, 36, 39]), (128, [0, 5, 10, 15, 20, 25, 30, 35]),
          (5, []), (12, [17])]


def test_shapes_where_the_body_or_the_table_can_go_wrong():
    """block dimensions 1, 15, 16, 17, 63, 64, 65, 127 and 128 (eight rows at n16 = 128, what the rule admits), a block no
    constraint touches, and a block with one row beside the block with all forty (the launch's LDS is sized by another member):
    each against the per-cone path bit for bit, and log det against numpy's slogdet of the dual matrix to 1e-12 relative"""
    from hdsdp_amd import api
    m = M_SHAPES
    loop, grp = _two_sets(31, m, SHAPES)
    rng = np.random.default_rng(32)
    y0 = rng.uniform(-0.02, 0.02, m)
    dy = rng.uniform(-1e-3, 1e-3, m)
    try:
        for b in loop + grp:
            b[0].set_start(-0.3)
        kkt = api.KKT(m, [b[0] for b in grp])
        assert all(_rule(n, len(rows)) for n, rows in SHAPES)
        assert kkt.set_grouped_check(True) == len(SHAPES)
        for k, (tau, y) in enumerate(((0.9, y0), (1.0, 0.5 * y0), (1.3, -y0))):
            got = _ask([b[0] for b in grp], tau, y, 0.0, dy)
            info = kkt.grouped_check_info()
            assert info["launches"] == k + 1 and info["last_cones"] == len(SHAPES), info
            _same(got, _ask([b[0] for b in loop], tau, y, 0.0, dy), f"shapes point {k}")
            for (ok, ld, D, _), (_, C, A) in zip(got, grp):
                n = C.shape[0]
                S = tau * C - np.tensordot(y, A, axes=1) + 0.3 * np.eye(n)
                assert ok == bool(np.all(np.linalg.eigvalsh(S) > 0))
                assert np.max(np.abs(_full(D) - S)) <= 1e-13 * np.max(np.abs(S))
                if ok:
                    sign, ref = np.linalg.slogdet(_full(D))
                    assert sign > 0 and abs(ld - ref) <= 1e-12 * abs(ref), (n, ld, ref)
        kkt.destroy()
    finally:
        _destroy(loop, grp)


def test_two_members_are_a_set_and_one_is_not():
    from hdsdp_amd import api
    m = 6
    plan = [(9, [0, 1, 2]), (20, [2, 3, 4, 5])]
    loop, grp = _two_sets(41, m, plan)
    y = np.random.default_rng(42).uniform(-0.02, 0.02, m)
    dy = 1e-3 * np.ones(m)
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        kkt = api.KKT(m, [b[0] for b in grp])
        assert kkt.set_grouped_check(True) == 2
        got = _ask([b[0] for b in grp], 1.0, y, 0.0, dy)
        info = kkt.grouped_check_info()
        assert (info["launches"], info["last_cones"], info["members"]) == (1, 2, 2), info
        _same(got, _ask([b[0] for b in loop], 1.0, y, 0.0, dy), "two members")
        kkt.destroy()
        one = api.KKT(m, [grp[0][0]])
        assert one.set_grouped_check(True) == 0 and one.grouped_check_info()["on"] is False
        assert grp[0][0].check_is_interior(1.1, y)
        assert one.grouped_check_info()["launches"] == 0
        one.destroy()
    finally:
        _destroy(loop, grp)


def test_a_non_interior_member():
    """y makes exactly one member's S indefinite (numpy says so).  First set of cones: its flag is 0, the others are 1 with their
    log det and usable factors (a ratio test succeeds on each).  Second pair of sets: the per-cone loop BREAKS at the indefinite
    cone as the reference's does, the grouped form has moved the cones behind the break as well; at a good point asked next every
    cone has the per-cone path's bits, those behind the break included"""
    from hdsdp_amd import api
    m = 10
    plan = [(14, [0, 1, 2]), (33, [3, 4]), (20, [0, 5, 6, 7]), (65, [8, 9])]       # row 4 belongs to cone 1 alone
    first = _set(51, m, plan)
    loop, grp = _two_sets(51, m, plan)
    rng = np.random.default_rng(52)
    good = rng.uniform(-0.02, 0.02, m)
    bad = good.copy()
    bad[4] = 60.0
    dy = rng.uniform(-1e-3, 1e-3, m)
    try:
        for b in first + loop + grp:
            b[0].set_start(-0.2)
        pd = [bool(np.all(np.linalg.eigvalsh(1.0 * C - np.tensordot(bad, A, axes=1) + 0.2 * np.eye(C.shape[0])) > 0)) for _, C, A in grp]
        assert pd == [True, False, True, True]
        kkt = api.KKT(m, [b[0] for b in first])
        assert kkt.set_grouped_check(True) == 4
        flags, logdets, every = kkt.check_is_interior(1.0, bad)
        assert flags.tolist() == pd and not every
        assert np.isnan(logdets[1]) and np.all(np.isfinite(logdets[[0, 2, 3]]))
        info = kkt.grouped_check_info()
        assert (info["launches"], info["last_cones"]) == (1, 4), info
        for k in (0, 2, 3):
            cone, C, A = first[k]
            S = 1.0 * C - np.tensordot(bad, A, axes=1) + 0.2 * np.eye(C.shape[0])
            ref = np.linalg.slogdet(S)[1]
            assert abs(logdets[k] - ref) <= 1e-12 * abs(ref)
            assert cone.log_barrier(1.0, bad) == logdets[k]
            assert cone.ratio_test(0.0, dy) > 0.0
        with pytest.raises(api.HDSDPError):
            first[1][0].log_barrier(1.0, bad)
        assert kkt.grouped_check_info()["launches"] == 1
        kkt.destroy()
        # the break: the loop stops at cone 1 and never asks cones 2 and 3 at the bad point
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_check(True) == 4
        assert _ask(gc, 1.0, bad, 0.0, dy, stop_at_first_failure=True) == [True, False]
        assert _ask(lc, 1.0, bad, 0.0, dy, stop_at_first_failure=True) == [True, False]
        assert all(np.array_equal(np.triu(gc[k].dual_matrix()), np.triu(lc[k].dual_matrix())) for k in (0, 1))
        for k in (2, 3):          # behind the break: the grouped form has put them at the bad point, the loop has not touched them
            C, A = grp[k][1], grp[k][2]
            S = 1.0 * C - np.tensordot(bad, A, axes=1) + 0.2 * np.eye(C.shape[0])
            assert np.max(np.abs(_full(gc[k].dual_matrix()) - S)) <= 1e-13 * np.max(np.abs(S))
        got = _ask(gc, 1.1, good, 0.0, dy)
        assert all(x[0] for x in got)
        _same(got, _ask(lc, 1.1, good, 0.0, dy), "good point after the bad one")
        assert kkt.grouped_check_info()["launches"] == 2
        kkt.destroy()
    finally:
        _destroy(first, loop, grp)


def test_mixed_operator():
    """two members, a cone the rule refuses (n = 130) and an LP cone: two members; HMiKKTCheckIsInterior agrees with the per-cone
    loop on every cone, the non-members through their own slots; and a second operator over the same cones takes none of the
    cones the first one's active set holds"""
    from hdsdp_amd import api
    m = 8
    plan = [(24, [0, 1, 2]), (130, [2, 3, 4]), (40, [4, 5, 6, 7])]
    loop, grp = _two_sets(61, m, plan)
    lp_loop, lp_grp = _lp_cone(m, 9, 62), _lp_cone(m, 9, 62)
    y = np.random.default_rng(63).uniform(-0.02, 0.02, m)
    try:
        for c in [b[0] for b in loop + grp] + [lp_loop, lp_grp]:
            c.set_start(-0.2)
        cones = [grp[0][0], grp[1][0], lp_grp, grp[2][0]]
        ref_cones = [loop[0][0], loop[1][0], lp_loop, loop[2][0]]
        kkt = api.KKT(m, cones)
        assert kkt.grouped_check_info()["members"] == 2
        plain = kkt.check_is_interior(0.8, y)                      # switch off: the plain loop
        assert kkt.grouped_check_info()["launches"] == 0
        assert kkt.set_grouped_check(True) == 2
        for tau in (1.0, 1.2):
            flags, logdets, every = kkt.check_is_interior(tau, y)
            want_f = [c.check_is_interior(tau, y) for c in ref_cones]
            want_l = [c.log_barrier(tau, y) for c in ref_cones]
            assert flags.tolist() == want_f and every == all(want_f) and all(want_f)
            assert np.array_equal(logdets, np.asarray(want_l)), (logdets, want_l)
            assert np.array_equal(np.triu(grp[1][0].dual_matrix()), np.triu(loop[1][0].dual_matrix()))
        info = kkt.grouped_check_info()
        assert (info["launches"], info["last_cones"], info["total_cones"]) == (2, 2, 4), info
        ref_plain = [c.check_is_interior(0.8, y) for c in ref_cones], [c.log_barrier(0.8, y) for c in ref_cones]
        again = kkt.check_is_interior(0.8, y)
        for got in (plain, again):
            assert got[0].tolist() == ref_plain[0] and np.array_equal(got[1], np.asarray(ref_plain[1]))
        # a second operator over the same cones while the first set is active: no member for it, and the first keeps its own
        other = api.KKT(m, cones)
        assert other.grouped_check_info()["members"] == 0 and other.set_grouped_check(True) == 0
        other.destroy()
        assert kkt.grouped_check_info()["members"] == 2
        flags, _, _ = kkt.check_is_interior(0.9, y)
        assert flags.all() and kkt.grouped_check_info()["launches"] == 4
        kkt.destroy()
    finally:
        _destroy(loop, grp)
        lp_loop.destroy(); lp_grp.destroy()


def test_lifetime():
    """a member destroyed before its operator; the switch turned off and on; the operator destroyed and a former member asked on
    its own: nothing fails, and the answers are the per-cone path's"""
    from hdsdp_amd import api
    m = 9
    plan = [(10, [0, 1]), (18, [2, 3, 4]), (31, [4, 5, 6]), (48, [6, 7, 8])]
    loop, grp = _two_sets(71, m, plan)
    rng = np.random.default_rng(72)
    ys = [rng.uniform(-0.02, 0.02, m) for _ in range(5)]
    dy = rng.uniform(-1e-3, 1e-3, m)
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_check(True) == 4
        _same(_ask(gc, 1.0, ys[0], 0.0, dy), _ask(lc, 1.0, ys[0], 0.0, dy), "all four")
        gc[1].destroy(); lc[1].destroy()                                  # a member goes before its operator
        gc3, lc3 = [gc[0], gc[2], gc[3]], [lc[0], lc[2], lc[3]]
        info = kkt.grouped_check_info()
        assert info["members"] == 3
        _same(_ask(gc3, 1.0, ys[1], 0.0, dy), _ask(lc3, 1.0, ys[1], 0.0, dy), "three left")
        info = kkt.grouped_check_info()
        assert (info["launches"], info["last_cones"]) == (2, 3), info
        assert kkt.set_grouped_check(False) == 0                           # off: per-cone launches, the counters stand still
        _same(_ask(gc3, 1.0, ys[2], 0.0, dy), _ask(lc3, 1.0, ys[2], 0.0, dy), "switch off")
        assert kkt.grouped_check_info()["launches"] == 2 and kkt.grouped_check_info()["on"] is False
        assert kkt.set_grouped_check(True) == 3                            # and on again
        _same(_ask(gc3, 1.0, ys[3], 0.0, dy), _ask(lc3, 1.0, ys[3], 0.0, dy), "switch on again")
        assert kkt.grouped_check_info()["launches"] == 3
        kkt.destroy()                                                     # the operator goes: a former member answers on its own
        _same(_ask(gc3, 1.0, ys[4], 0.0, dy), _ask(lc3, 1.0, ys[4], 0.0, dy), "after the operator")
        again = api.KKT(m, gc3)                                           # and is free for the next operator
        assert again.set_grouped_check(True) == 3
        _same(_ask(gc3, 0.9, ys[0], 0.0, dy), _ask(lc3, 0.9, ys[0], 0.0, dy), "next operator")
        assert again.grouped_check_info()["launches"] == 1
        again.destroy()
    finally:
        _destroy(loop, grp)


@pytest.mark.parametrize("name", ["arrow128_A", "chain16_A"])
def test_with_the_grouped_build(name):
    """both switches on: the grouped inverse kernel reads the Dinv the grouped check's launch wrote; test_gpu_grouped_build.py's
    golden comparison, same bars"""
    from hdsdp_amd import api
    g = load_golden(name)
    m = int(g["mb_dims"][1])
    ncones = INSTANCES[name][1]
    cones, members = _golden_cones(name, m)
    try:
        for c in cones:
            c.set_start(float(g["Rd"][0]))
        kkt = api.KKT(m, cones)
        assert kkt.set_grouped_check(True) == members == ncones
        assert kkt.set_grouped_build(True) == ncones
        flags, _, every = kkt.check_is_interior(float(g["tau"][0]), y_of(g))
        assert every and flags.all()
        info = kkt.grouped_check_info()
        assert (info["launches"], info["last_cones"]) == (1, ncones), info
        _check_goldens(name, g, kkt, ncones)
        kkt.destroy()
    finally:
        for c in cones:
            c.destroy()


def test_state_transitions():
    """set_perturb / reduce_resi on one member: only that member is launched at the old y, the others are left out and the counter
    says so; scal_by_constant on every cone: all members are launched"""
    from hdsdp_amd import api
    m = 7
    plan = [(11, [0, 1, 2]), (22, [2, 3]), (35, [4, 5, 6])]
    loop, grp = _two_sets(81, m, plan)
    y = np.random.default_rng(82).uniform(-0.02, 0.02, m)
    dy = 1e-3 * np.ones(m)
    try:
        for b in loop + grp:
            b[0].set_start(-0.1)
        gc, lc = [b[0] for b in grp], [b[0] for b in loop]
        kkt = api.KKT(m, gc)
        assert kkt.set_grouped_check(True) == 3
        _same(_ask(gc, 1.0, y, 0.0, dy), _ask(lc, 1.0, y, 0.0, dy), "start")
        assert kkt.grouped_check_info()["launches"] == 1
        for step, change in enumerate((lambda c: c.set_perturb(0.05), lambda c: c.reduce_resi(-0.04))):
            change(gc[1]); change(lc[1])
            assert gc[0].check_is_interior(1.0, y) and kkt.grouped_check_info()["launches"] == 1 + step      # unchanged: from state
            assert gc[1].check_is_interior(1.0, y)
            info = kkt.grouped_check_info()
            assert (info["launches"], info["last_cones"], info["left_out"]) == (2 + step, 1, 2), info
            _same(_ask(gc, 1.0, y, 0.0, dy), _ask(lc, 1.0, y, 0.0, dy), f"after change {step}")
            assert kkt.grouped_check_info()["launches"] == 2 + step
        for c in gc + lc:
            c.scal_by_constant(0.5)
        _same(_ask(gc, 1.0, y, 0.0, dy), _ask(lc, 1.0, y, 0.0, dy), "after scal_by_constant")
        info = kkt.grouped_check_info()
        assert (info["launches"], info["last_cones"], info["left_out"]) == (4, 3, 0), info
        kkt.destroy()
    finally:
        _destroy(loop, grp)


# the optimum the driver prints, as tests/test_gpu_reference_driver.py expects it for the same files
DRIVER_CASES = {"truss1": (8.999996, "7"), "chain16": (74.932288321, "16")}


@pytest.mark.parametrize("inst", sorted(DRIVER_CASES))
def test_unchanged_driver_with_the_grouped_check_switched_on(inst):
    """the reference's own driver with its SDP blocks handed to the engine's cones (oracle/drop_attach.c), once without and once
    with HDSDP_MI355X_GROUPED_CHECK=1: both reach the optimum tests/test_gpu_reference_driver.py expects, HKKTInit names all
    seven / all sixteen cones, and the iteration count and the printed final pObj / dObj are identical between the runs"""
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/sdpasolve_mi355x not built (make -C oracle drop needs the reference's sources at build time)")
    opt, ncones = DRIVER_CASES[inst]
    runs = [_drive(inst, grouped) for grouped in (False, True)]
    for out, its, pobj, dobj in runs:
        assert its and pobj and dobj, out[-3000:]
        assert abs(float(dobj[0]) - opt) <= 1e-4 * abs(opt), (dobj, opt)
        assert abs(float(pobj[0]) - float(dobj[0])) <= 1e-4 * abs(opt), (pobj, dobj)
    assert "HDSDP_MI355X_GROUPED_CHECK" not in runs[0][0]
    said = re.search(r"HDSDP_MI355X_GROUPED_CHECK=1: (\d+) of (\d+) cone", runs[1][0])
    assert said, runs[1][0][-3000:]
    print(said.group(0))
    assert said.group(1) == said.group(2) == ncones, said.group(0)
    print("iterations", runs[0][1][-1], runs[1][1][-1], "pObj", runs[0][2], runs[1][2], "dObj", runs[0][3], runs[1][3])
    assert runs[0][1] == runs[1][1], (runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2] and runs[0][3] == runs[1][3], (runs[0][2:], runs[1][2:])
