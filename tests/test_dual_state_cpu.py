"""The rule that answers a dual-matrix request (csrc/dual_state.h: hdm_dual_plan, HdmDualState), without a device: the header is
compiled alone with the host C++ compiler beside tests/dual_state_driver.cpp, and the plan is checked for cases derived from
the rule as it is stated, not from what the code gives:

- a request for the point S holds is answered by nothing (into S) or a copy (into the checker);
- p = pS + alpha pD + delta e_eye is answered by S + alpha dS (+ delta I): alpha from the largest |pD| multiplier, else tau; tau and
  every multiplier within 8e-15 (|p| + |pS| + |alpha pD|); the identity coefficient free; a non-finite alpha misses;
- a request for S is swept afresh once 16 updates in place have been chained; the checker is not;
- mode 1 short-cuts the exact point only, mode 0 and sharded blocks (world > 1) nothing; a step matrix is always swept;
- every transition that forgets something forces the request that relied on it into a sweep.

Each case also names the assembly counter it counts as (HMiGetAssembleCounts's order)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

S, CHECK, DS = 0, 1, 2                                            # targets
NONE, COPY, AXPY, AXPY_EYE, SWEEP = range(5)                      # actions
HELD, COPIED, LINE, OFF_LINE, REFRESH, STEP, UNTRACKED = range(7)    # counters, in HMiGetAssembleCounts's order
TOL, CHAIN = 8e-15, 16


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dual_state") / "driver")
    # (no contraction into fused multiply-adds: the test's own arithmetic below is plain IEEE double)
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "dual_state_driver.cpp")])
    return exe


def _pt(p):
    tau, eye, y = p
    return " ".join(float(v).hex() for v in (tau, eye, *y))


class Script:
    """one fresh state per script; queries come back in order"""

    def __init__(self):
        self.lines, self.kinds = [], []

    def at(self, cmd, p):                      # S, D, ADV
        self.lines.append(f"{cmd} {_pt(p)}")
        return self

    def do(self, cmd, *a):                     # OVER, DATA, STALE, FAC r
        self.lines.append(" ".join([cmd] + [str(x) for x in a]))
        return self

    def plan(self, target, mode, p, world=1, commit=False):
        self.lines.append(f"{'DO' if commit else 'PLAN'} {target} {mode} {world} {_pt(p)}")
        self.kinds.append("plan")
        return self

    def facat(self, p):
        self.lines.append(f"FACAT {_pt(p)}")
        self.kinds.append("fac")
        return self

    def run(self, exe, env=None):
        out = subprocess.run([exe], input="\n".join(self.lines) + "\n", capture_output=True, text=True, check=True, env=env).stdout
        rows = out.splitlines()
        assert len(rows) == len(self.kinds), out
        res = []
        for kind, row in zip(self.kinds, rows):
            t = row.split()
            if kind == "fac":
                res.append((int(t[0]), int(t[1])))
            else:
                res.append({"action": int(t[0]), "alpha": float.fromhex(t[1]), "delta": float.fromhex(t[2]), "counter": int(t[3]),
                            "tracked": int(t[4]), "line_missed": int(t[5]), "off_line": int(t[6]), "worst": float.fromhex(t[7]),
                            "worst_at": int(t[8])})
        return res


def _is(r, action, counter):
    return r["action"] == action and r["counter"] == counter


# pS, pD and points on their line in numbers that are exact in binary, so "on the line" holds to the last bit
Y0, DY = (1.0, 2.0, 4.0), (0.5, -1.0, 0.25)                 # the largest |pD| multiplier is component 1 of y: index 3
PS = (1.0, 0.5, Y0)
PD = (0.0, 0.0, DY)


def along(a, ps=PS, pd=PD, deye=0.0):
    return (ps[0] + a * pd[0], ps[1] + a * pd[1] + deye, tuple(y + a * d for y, d in zip(ps[2], pd[2])))


def held():
    return Script().at("S", PS).at("D", PD)


def test_the_same_point_is_nothing_or_a_copy(driver):
    for mode in (1, 2):
        a, b = held().plan(S, mode, PS).plan(CHECK, mode, PS).run(driver)
        assert _is(a, NONE, HELD) and _is(b, COPY, COPIED), (mode, a, b)
    # the point is the whole point: tau, the identity coefficient, every multiplier
    for q in ((1.5, 0.5, Y0), (1.0, 0.25, Y0), (1.0, 0.5, (1.0, 2.0, 4.5))):
        a, = held().plan(S, 1, q).run(driver)
        assert _is(a, SWEEP, OFF_LINE), (q, a)
    # a NaN is the same as nothing, itself included
    nan = (1.0, 0.5, (1.0, float("nan"), 4.0))
    a, b = Script().at("S", nan).at("D", PD).plan(S, 2, nan).plan(CHECK, 2, nan).run(driver)
    assert _is(a, SWEEP, OFF_LINE) and _is(b, SWEEP, OFF_LINE), (a, b)


def test_a_point_on_the_line_is_s_plus_alpha_ds(driver):
    for target in (S, CHECK):
        a, b = held().plan(target, 2, along(0.5)).plan(target, 2, along(-0.25)).run(driver)
        assert _is(a, AXPY, LINE) and a["alpha"] == 0.5 and a["delta"] == 0.0 and a["tracked"] == 1, a
        assert _is(b, AXPY, LINE) and b["alpha"] == -0.25 and b["delta"] == 0.0, b


def test_the_identity_coefficient_is_free(driver):
    a, = held().plan(S, 2, along(0.5, deye=0.25)).run(driver)
    assert _is(a, AXPY_EYE, LINE) and a["alpha"] == 0.5 and a["delta"] == 0.25, a
    # a direction with an identity part of its own (the ratio test's dAdaRatio * Rd): delta is what alpha does not explain
    pd = (0.0, 0.5, DY)
    a, b = Script().at("S", PS).at("D", pd).plan(S, 2, along(0.5, pd=pd)).plan(S, 2, along(0.5, pd=pd, deye=-1.0)).run(driver)
    assert _is(a, AXPY, LINE) and a["delta"] == 0.0, a
    assert _is(b, AXPY_EYE, LINE) and b["delta"] == -1.0, b


def _off_by(rel, k, a=0.5):
    """along(a) with multiplier k moved off the line by about `rel` of the rule's scale; returns the point and the distance as the
    rule measures it: |(p - pS) - alpha pD| / (|p| + |pS| + |alpha pD|)"""
    tau, eye, y = along(a)
    y = list(y)
    e = a * DY[k]
    y[k] = y[k] + rel * (abs(y[k]) + abs(Y0[k]) + abs(e))
    measured = abs((y[k] - Y0[k]) - e) / (abs(y[k]) + abs(Y0[k]) + abs(e))
    return (tau, eye, tuple(y)), measured


def test_the_tolerance_is_8e_15_of_the_rules_own_scale(driver):
    for k in (0, 2):                                # not the component alpha is taken from
        near, e_near = _off_by(7e-15, k)
        far, e_far = _off_by(9e-15, k)
        assert 6e-15 < e_near < TOL < e_far < 1e-14, (e_near, e_far)
        a, b = held().plan(S, 2, near).plan(S, 2, far).run(driver)
        assert _is(a, AXPY, LINE) and a["alpha"] == 0.5 and a["line_missed"] == 0, (k, a)
        assert _is(b, SWEEP, OFF_LINE) and b["line_missed"] == 1 and b["off_line"] == 1 and b["worst_at"] == 2 + k, (k, b)
        assert b["worst"] == e_far and a["worst"] == e_near, (k, a, b)
    # tau is held to the line like a multiplier
    tau_line = (-0.5, 0.0, DY)
    on = along(0.5, pd=tau_line)
    off = (on[0] * (1 + 1e-13), on[1], on[2])
    a, b = Script().at("S", PS).at("D", tau_line).plan(S, 2, on).plan(S, 2, off).run(driver)
    assert _is(a, AXPY, LINE) and a["alpha"] == 0.5, a
    assert _is(b, SWEEP, OFF_LINE) and b["off_line"] == 1 and b["worst_at"] == 0, b


def test_alpha_comes_from_the_largest_multiplier_else_tau(driver):
    # moving the component alpha is read from moves alpha, and every OTHER component is then off the line
    tau, eye, y = along(0.5)
    a, = held().plan(S, 2, (tau, eye, (y[0], y[1] - 0.25, y[2]))).run(driver)
    assert _is(a, SWEEP, OFF_LINE) and a["alpha"] == 0.75 and a["off_line"] == 2, a
    # no multiplier in pD: alpha from tau
    only_tau = (-0.5, 0.0, (0.0, 0.0, 0.0))
    q = along(0.25, pd=only_tau)
    a, b = (Script().at("S", PS).at("D", only_tau).plan(S, 2, q).plan(S, 2, (q[0], q[1], (1.0, 2.0, 4.5))).run(driver))
    assert _is(a, AXPY, LINE) and a["alpha"] == 0.25, a
    assert _is(b, SWEEP, OFF_LINE) and b["line_missed"] == 1 and b["worst_at"] == 4, b
    # pD all zero: alpha is 0; only the identity coefficient may move
    zero = (0.0, 0.0, (0.0, 0.0, 0.0))
    a, b = (Script().at("S", PS).at("D", zero).plan(S, 2, (1.0, 0.75, Y0)).plan(S, 2, (1.0, 0.5, (1.0, 2.0, 4.5))).run(driver))
    assert _is(a, AXPY_EYE, LINE) and a["alpha"] == 0.0 and a["delta"] == 0.25, a
    assert _is(b, SWEEP, OFF_LINE) and b["alpha"] == 0.0 and b["line_missed"] == 1, b
    # an alpha that is not finite misses
    tiny = (0.0, 0.0, (1e-300, 0.0, 0.0))
    a, = Script().at("S", PS).at("D", tiny).plan(S, 2, (1.0, 0.5, (1e10, 2.0, 4.0))).run(driver)
    assert _is(a, SWEEP, OFF_LINE) and a["line_missed"] == 1 and a["alpha"] == float("inf"), a


def _chained(links):
    s = held()
    for k in range(1, links + 1):
        s.plan(S, 2, along(k / 32.0), commit=True)
    return s


def test_a_chain_is_refreshed_at_16_links_for_s_only(driver):
    nxt = along(17 / 32.0)
    *links, a, b = _chained(CHAIN - 1).plan(S, 2, nxt).plan(CHECK, 2, nxt).run(driver)
    assert all(_is(r, AXPY, LINE) and r["alpha"] == 1 / 32.0 for r in links), links     # each link from where S then stands
    assert _is(a, AXPY, LINE) and _is(b, AXPY, LINE), (a, b)
    *links, a, b = _chained(CHAIN).plan(S, 2, nxt).plan(CHECK, 2, nxt).run(driver)
    assert len(links) == CHAIN and all(_is(r, AXPY, LINE) for r in links)
    assert _is(a, SWEEP, REFRESH) and a["line_missed"] == 0, a
    assert _is(b, AXPY, LINE) and b["alpha"] == 1 / 32.0, b
    # the refresh sweep starts a new chain at the refreshed point
    *_, a, b, c = _chained(CHAIN).plan(S, 2, nxt, commit=True).plan(S, 2, nxt).plan(S, 2, along(18 / 32.0)).run(driver)
    assert _is(a, SWEEP, REFRESH) and _is(b, NONE, HELD) and _is(c, AXPY, LINE), (a, b, c)
    # updates of the checker buffer are no links: S does not move
    s = held()
    for k in range(1, 2 * CHAIN):
        s.plan(CHECK, 2, along(k / 64.0), commit=True)
    *_, a = s.plan(S, 2, PS).run(driver)
    assert _is(a, NONE, HELD), a


def test_modes_world_and_the_step_matrix(driver):
    on = along(0.5)
    # mode 1: the exact point only (the line is not even looked at)
    a, b, c = held().plan(S, 1, PS).plan(CHECK, 1, PS).plan(S, 1, on).run(driver)
    assert _is(a, NONE, HELD) and _is(b, COPY, COPIED), (a, b)
    assert _is(c, SWEEP, OFF_LINE) and c["line_missed"] == 0 and c["tracked"] == 1, c
    # mode 0 and a sharded block: every request is a sweep of an untracked block, the point S holds included
    for mode, world in ((0, 1), (2, 2), (1, 8)):
        rs = held().plan(S, mode, PS, world).plan(CHECK, mode, PS, world).plan(S, mode, on, world).plan(DS, mode, PD, world).run(driver)
        assert all(r["tracked"] == 0 and r["action"] == SWEEP for r in rs), (mode, world, rs)
        assert [r["counter"] for r in rs] == [UNTRACKED, UNTRACKED, UNTRACKED, STEP], (mode, world, rs)
    # a step matrix is always swept, the direction dS holds included
    for mode in (1, 2):
        a, b = held().plan(DS, mode, PD).plan(DS, mode, PS).run(driver)
        assert _is(a, SWEEP, STEP) and _is(b, SWEEP, STEP) and a["tracked"] == 1, (mode, a, b)


def test_every_transition_forces_the_sweep_it_must(driver):
    on = along(0.5)
    # nothing known; S known but no direction
    a, b = Script().plan(S, 2, PS).plan(CHECK, 2, PS).run(driver)
    assert _is(a, SWEEP, OFF_LINE) and _is(b, SWEEP, OFF_LINE), (a, b)
    a, b = Script().at("D", PD).plan(S, 2, on).run(driver) + Script().at("S", PS).plan(S, 2, on).run(driver)
    assert _is(a, SWEEP, OFF_LINE) and _is(b, SWEEP, OFF_LINE) and b["line_missed"] == 0, (a, b)
    # a sweep into S records its point, a sweep of a step matrix its direction: then the line is there
    a, b, c, d = Script().plan(S, 2, PS, commit=True).plan(DS, 2, PD, commit=True).plan(S, 2, PS).plan(CHECK, 2, on).run(driver)
    assert _is(a, SWEEP, OFF_LINE) and _is(b, SWEEP, STEP) and _is(c, NONE, HELD) and _is(d, AXPY, LINE), (a, b, c, d)
    # dS assembled at another direction (a new ratio test, the primal recovery): a point on the OLD line sweeps
    a, = held().plan(DS, 2, (0.0, 0.0, (0.25, 1.0, -0.5)), commit=True).plan(S, 2, on).run(driver)[1:]
    assert _is(a, SWEEP, OFF_LINE) and a["line_missed"] == 1, a
    # S advanced along the line: it stands at the new point, the old one is a step back along the same line
    a, b, c = held().plan(S, 2, on, commit=True).plan(S, 2, on).plan(S, 2, PS).run(driver)
    assert _is(a, AXPY, LINE) and _is(b, NONE, HELD) and _is(c, AXPY, LINE) and c["alpha"] == -0.5, (a, b, c)
    # ... while a short-cut or a sweep into the checker leaves S where it was
    a, b, c = held().plan(CHECK, 2, on, commit=True).plan(CHECK, 2, (3.0, 0.5, Y0), commit=True).plan(S, 2, PS).run(driver)
    assert _is(a, AXPY, LINE) and _is(b, SWEEP, OFF_LINE) and _is(c, NONE, HELD), (a, b, c)
    # S written by someone else: the point it held and the line through it are gone, until S is assembled again
    a, b, c, d, e = (held().do("OVER").plan(S, 2, PS).plan(CHECK, 2, PS).plan(S, 2, on)
                     .plan(S, 2, PS, commit=True).plan(S, 2, on).run(driver))
    assert all(_is(r, SWEEP, OFF_LINE) for r in (a, b, c, d)) and _is(e, AXPY, LINE), (a, b, c, d, e)
    # the data under S and dS changed: both gone, and a new S alone brings no line back
    a, b, c, d = held().do("DATA").plan(S, 2, PS).plan(S, 2, on).plan(S, 2, PS, commit=True).plan(S, 2, on).run(driver)
    assert all(_is(r, SWEEP, OFF_LINE) for r in (a, b, c, d)) and d["line_missed"] == 0, (a, b, c, d)
    # a sweep of an untracked block into S leaves no point behind (a tracking reader would have to assemble)
    a, b = held().plan(S, 0, on, commit=True).plan(S, 2, PS).run(driver)
    assert _is(a, SWEEP, UNTRACKED) and _is(b, SWEEP, OFF_LINE), (a, b)


def test_the_factor_is_held_only_while_s_stands_where_it_was_factored(driver):
    on = along(0.5)
    assert Script().facat(PS).run(driver) == [(0, -1)]
    assert Script().at("S", PS).facat(PS).run(driver) == [(0, -1)]                      # assembled, not factored
    for psd in (1, 0):
        assert Script().at("S", PS).do("FAC", psd).facat(PS).facat(on).run(driver) == [(1, psd), (0, -1)]
    fac = lambda: Script().at("S", PS).at("D", PD).do("FAC", 1)  # noqa: E731
    assert fac().do("STALE").facat(PS).run(driver) == [(0, -1)]
    assert fac().do("OVER").facat(PS).run(driver) == [(0, -1)]
    assert fac().do("DATA").facat(PS).run(driver) == [(0, -1)]
    assert fac().at("S", PS).facat(PS).run(driver) == [(0, -1)]                         # S assembled again: a new matrix
    assert fac().at("ADV", on).facat(on).facat(PS).run(driver) == [(0, -1), (0, -1)]
    assert fac().at("D", (0.0, 0.0, (1.0, 1.0, 1.0))).facat(PS).run(driver) == [(1, 1)]      # dS does not move S
    # through the plan: what moves S takes the factor along, what does not leaves it
    assert fac().plan(S, 2, PS, commit=True).plan(CHECK, 2, on, commit=True).facat(PS).run(driver)[-1] == (1, 1)
    assert fac().plan(S, 2, on, commit=True).facat(on).run(driver)[-1] == (0, -1)
    assert fac().plan(S, 1, on, commit=True).facat(on).run(driver)[-1] == (0, -1)


def test_the_mode_rule(driver):
    def modes(env_value):
        env = {k: v for k, v in os.environ.items() if k != "HDSDP_MI355X_AFFINE_S"}
        if env_value is not None:
            env["HDSDP_MI355X_AFFINE_S"] = env_value
        # 16 MiB of owned constraint data, 4 mloc n (n + 1) bytes: 64 x 256 x 257 x 4 = 16.06 MiB, 63 rows fall short
        out = subprocess.run([driver], input="MODE 64 256\nMODE 63 256\nMODE 2000 2000\nMODE 10 100\n", capture_output=True, text=True,
                             check=True, env=env).stdout
        return [int(v) for v in out.split()]
    assert 64 * 256 * 257 * 4 >= 16 << 20 > 63 * 256 * 257 * 4
    assert modes(None) == [2, 1, 2, 1]
    for v in ("0", "1", "2"):
        assert modes(v) == [int(v)] * 4


def test_the_debug_line_of_a_miss(driver):
    far, e_far = _off_by(9e-15, 2)
    script = "\n".join([f"S {_pt(PS)}", f"D {_pt(PD)}", f"MISS {CHECK} 2 1 {_pt(far)}"]) + "\n"
    out = subprocess.run([driver], input=script, capture_output=True, text=True, check=True).stdout
    assert out.startswith("[hdsdp_mi355x affine] miss (checker): alpha 5.000000e-01, 1 of 5 components off the tested line, "
                          "worst relative %.3e at 4; d tau 0.000e+00, d eye 0.000e+00," % e_far), out
