"""The line search's device quantities against the host fp64 model (tests/line_search_model.py, itself pinned to the oracle
by tests/test_line_search_model.py):

- the dual matrix cone_assemble hands out -- a cache of S = T(pS) and dS = T(pD), with short-cuts -- after every request of
  the reference's line search, corrector and primal recovery, in each HDSDP_MI355X_AFFINE_S mode (child processes:
  tests/line_search_worker.py), with the assembly counters showing which short-cut answered;
- the ratio test against the exact largest step alpha* at every Lanczos kernel form;
- the interior decision and the log-barrier against matrices whose spectrum is known."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)
import line_search_model as lm  # noqa: E402
from util import RATIO_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = ("257x64", "300x60")          # 16 MiB of constraint data or more: short-cut mode 2 by default
SMALL = "100x10"                    # one-launch small check, mode 1 by default


def _run(mode):
    # (HDSDP_MI355X_LIB is kept: it names the library build under test)
    env = {k: v for k, v in os.environ.items()
           if not (k.startswith("HDM_") or k.startswith("HDSDP_MI355X_")) or k == "HDSDP_MI355X_LIB"}
    if mode is not None:
        env["HDSDP_MI355X_AFFINE_S"] = mode
    r = subprocess.run([sys.executable, os.path.join(HERE, "line_search_worker.py")], capture_output=True, text=True,
                       timeout=300, env=env)
    if r.returncode != 0:
        pytest.fail(f"worker (mode {mode}) exited with {r.returncode}:\n" + (r.stdout + r.stderr)[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("LINE_SEARCH_JSON ")]
    assert line, (r.stdout + r.stderr)[-2000:]
    return json.loads(line[-1][len("LINE_SEARCH_JSON "):])


@pytest.fixture(scope="module")
def runs():
    return {mode: _run(mode) for mode in ("0", "1", "2")}


def _bad(out):
    bad = []
    for key in BIG + (SMALL,):
        bad += [f"{key}: {b}" for b in out[key]["bad"]]
    bad += out["phase_a"]["bad"] + out["downstream"]["bad"]
    return bad


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_every_dual_matrix_request_is_the_models(runs, mode):
    """after every call: raw S, the interior decision and both log-barriers within 1e-13 of the model (a stale state is off
    by O(1)); X of the primal recovery; M and the vectors of a Schur build from a short-cut S against the oracle's formulas"""
    out = runs[mode]
    assert not _bad(out), _bad(out)
    for key in BIG + (SMALL,):
        assert out[key]["err"]["S"] <= 1e-13
        assert out[key]["e"]["primal_err"] <= 1e-10, (key, out[key]["e"])       # X returned, and the model's
    assert out["phase_a"]["primal_err"] <= 1e-10, out["phase_a"]      # X where S(y) is interior (mcp100's recovery point)


def test_mode_2_takes_every_short_cut_it_claims(runs):
    """the counters show that the branches the sequences aim at actually ran in mode 2 (per request where it matters)"""
    out = runs["2"]
    for key in BIG:
        r = out[key]
        assert r["a"]["counts"][0] >= 1 and r["a"]["counts"][1] >= 1 and r["a"]["counts"][2] >= 5, (key, r["a"])
        assert r["b"]["counts"][2] >= 3, (key, r["b"])                       # S + alpha dS + delta I
        assert r["c"]["counts"][2] >= 16 and r["c"]["counts"][4] >= 1, (key, r["c"])   # the refresh after 16 links
        assert r["d"]["far"][3] == 1 and r["d"]["far"][2] == 0, (key, r["d"])
        assert r["d"]["near"][2] == 1 and r["d"]["near"][3] == 0, (key, r["d"])
        for case in ("scal", "axpy", "toggle", "primal"):           # invalidated: the on-line request sweeps
            assert r["e"][case][3] == 1 and r["e"][case][2] == 0, (key, case, r["e"])
        assert max(r["c"]["drift"]) <= 1e-13
    assert out["downstream"]["counts"][2] >= 1, out["downstream"]
    assert out["phase_a"]["counts"][2] == 0 and out["phase_a"]["counts"][3] == 1, out["phase_a"]


def test_mode_0_and_1_never_short_cut_along_a_line(runs):
    for mode in ("0", "1"):
        for key in BIG + (SMALL,):
            for seq in "abcde":
                c = runs[mode][key][seq]["counts"]
                assert c[2] == 0 and c[4] == 0, (mode, key, seq, c)
                if mode == "0":
                    assert c[0] == 0 and c[1] == 0, (mode, key, seq, c)


def test_the_three_modes_agree(runs):
    for key in BIG + (SMALL,):
        steps = [runs[mode][key]["a"]["step"] for mode in ("0", "1", "2")]
        assert max(abs(s - steps[0]) for s in steps) <= 1e-8 * abs(steps[0]), (key, steps)
    for k in ("M", "ASinv"):
        assert all(runs[mode]["downstream"]["errs"][k] <= 1e-10 for mode in ("0", "1", "2"))


# ---- the ratio test against the exact step ----------------------------------------------------------------------------
RATIO_SIZES = [1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1000, 2047, 2048, 2049, 2304]
ORACLE_MAX_N = 1000        # the oracle's recurrence on the host (seconds per call past this)
KNOWN = {"rank-one": 0.5, "near-degenerate pair": 1.0, "dS = -S": 1.0, "psd": np.inf}


def _check_step(step, a, S, dS, what):
    if np.isinf(a):
        assert step == np.inf or step > 1e6, (what, step)
        return
    assert 0.0 < step <= a * (1 + 1e-12), (what, step, a)                     # conservative
    assert step >= lm.ORACLE_STEP_FLOOR * a * (1 - RATIO_TOL), (what, step, a)
    assert lm.is_pd(S + step * dS) if step < a * (1 - 1e-9) else True, (what, step, a)


def _vs_oracle(got, want, a, what):
    """the device runs the oracle's recurrence: the same step at RATIO_TOL -- unless the recurrence's own step is past alpha*,
    where the device's safeguard (cone_ratio_test) must have replaced it by a step inside (checked by _check_step)"""
    if want > a * (1 + 1e-12):
        assert got < want, (what, got, want, a)
    else:
        assert abs(got - want) <= RATIO_TOL * abs(want) or (got > 1e6 and want > 1e6), (what, got, want, a)


@pytest.mark.parametrize("n", RATIO_SIZES)
def test_ratio_test_is_conservative_and_close_to_the_exact_step(n):
    import oracle_py
    from hdsdp_amd import api
    m = 4
    if n == 1:
        mats = [np.array([[3.0]]), np.array([[1.5]]), np.array([[-2.0]]), np.array([[0.25]]), np.array([[3.0]])]
    else:
        C, A = lm.ratio_block(n, 11 + n)
        mats = [C] + list(A)
    beg, idx, val = lm.to_csc([M for M in mats])
    C, A = lm.from_csc(n, m, beg, idx, val)
    cone = api.SDPCone.from_csc(n, m, beg, idx, val)
    blk = oracle_py.Block(n, m, beg, idx, val) if 1 < n <= ORACLE_MAX_N else None
    try:
        cone.set_start(0.0)
        assert cone.check_is_interior(1.0, np.zeros(m))
        S = lm.T(C, A, 1.0, np.zeros(m), 0.0)
        Lf = blk.factor(blk.assemble_S(1.0, np.zeros(m), 0.0))[0] if blk else None
        if n == 1:      # -s0 / d0 exactly, or inf for a step matrix that is >= 0
            for dy, want in ((np.eye(m)[0], 2.0), (np.eye(m)[1], np.inf), (np.eye(m)[3], 1.0), (np.zeros(m), np.inf)):
                got = cone.ratio_test(0.0, dy, 0.0)
                assert got == want, (dy, got, want)
            return
        for dtau, dy, ada, name in lm.ratio_directions(m):
            dS = lm.T(C, A, dtau, dy, 0.0)
            a = KNOWN[name] if (name in KNOWN and n >= 1000) else lm.alpha_star(S, dS)
            if name == "dtau and ada" and n > 257:
                continue
            got = cone.ratio_test(dtau, dy, ada)
            _check_step(got, a, S, dS, (n, name))
            if blk is not None:
                _vs_oracle(got, blk.ratio_test(Lf, dtau, dy, 0.0), a, (n, name))
        if n <= 257:
            # (a fresh cone and oracle: the Lanczos warm start left by dS = -S is rounding noise, see ratio_directions)
            cone.destroy()
            blk.close()
            cone = api.SDPCone.from_csc(n, m, beg, idx, val)
            blk = oracle_py.Block(n, m, beg, idx, val)
            # the residual's share, with ada != 0: S = C - Rd I, dS = dtau C - sum dy A + ada Rd I
            Rd = -0.5
            cone.set_start(Rd)
            assert cone.check_is_interior(1.0, np.zeros(m))
            S2 = lm.T(C, A, 1.0, np.zeros(m), -Rd)
            Lf2 = blk.factor(blk.assemble_S(1.0, np.zeros(m), Rd))[0]

            def on_S2(dtau, dy, ada, name):
                dS = lm.T(C, A, dtau, dy, ada * Rd)
                a = lm.alpha_star(S2, dS)
                got = cone.ratio_test(dtau, dy, ada)
                _check_step(got, a, S2, dS, (n, "Rd", name))
                _vs_oracle(got, blk.ratio_test(Lf2, dtau, dy, ada * Rd), a, (n, "Rd", name))
            on_S2(0.0, np.eye(m)[3], 0.0, "dS = -C")
            # the checker's factor (BUFFER_DUALCHECK): a trial point, then the step from it
            yc = 0.1 * np.eye(m)[2]
            assert cone.check_is_interior_expert(1.0, -1.0, yc, -Rd, api.BUFFER_DUALCHECK)
            Sc = lm.T(C, A, 1.0, yc, -Rd)
            dS = lm.T(C, A, 0.0, np.eye(m)[0], 0.0)
            a = lm.alpha_star(Sc, dS)
            got = cone.ratio_test(0.0, np.eye(m)[0], 0.0, buffer=api.BUFFER_DUALCHECK)
            _check_step(got, a, Sc, dS, (n, "checker"))
            want = blk.ratio_test(blk.factor(blk.assemble_S(1.0, yc, Rd))[0], 0.0, np.eye(m)[0], 0.0)
            if n == 15:
                # the reference's recurrence, warm-started, stops at the wrong Ritz value here (1/0.678 for a largest
                # eigenvalue 1/0.614): the case that keeps the safeguard of cone_ratio_test under test
                assert want > a * 1.05, (want, a)
            _vs_oracle(got, want, a, (n, "checker"))
            on_S2(*lm.ratio_directions(m)[-2])          # back on S's factor: dtau and ada with Rd != 0
    finally:
        cone.destroy()
        if blk is not None:
            blk.close()


# ---- the interior decision and the log-barrier on a known spectrum ----------------------------------------------------
# m = 1 (A_1 = I): the one-launch small check for n16 <= 128; m = 12 puts n = 100 and 128 past the small check's resident
# limit, onto the blocked factor, which every n >= 129 takes anyway
SPECTRUM_CASES = [(n, 1) for n in (1, 2, 16, 17, 100, 128, 129, 255, 257, 1000, 2049)] + [(100, 12), (128, 12)]


@pytest.mark.parametrize("n,m", SPECTRUM_CASES, ids=[f"{n}x{m}" for n, m in SPECTRUM_CASES])
def test_interior_decision_and_barrier_on_a_known_spectrum(n, m):
    from hdsdp_amd import api
    rng = np.random.default_rng(100 + n)
    lam = np.geomspace(1.0, 1e6, n) if n > 1 else np.array([1e3])
    Q = lm.householder_q(rng, n)
    C = (Q * lam) @ Q.T
    C = 0.5 * (C + C.T)
    extra = [lm.random_sym(rng, n, 0.5) for _ in range(m - 1)]
    beg, idx, val = lm.to_csc([C, np.eye(n)] + extra)
    C, A = lm.from_csc(n, m, beg, idx, val)
    cone = api.SDPCone.from_csc(n, m, beg, idx, val)
    try:
        cone.set_start(0.0)
        lmin, lmax = float(lam[0]), float(lam[-1])
        e0 = np.eye(m)[0]
        for buf in (api.BUFFER_DUALVAR, api.BUFFER_DUALCHECK):
            def interior(y):
                if buf == api.BUFFER_DUALVAR:
                    return cone.check_is_interior(1.0, y)
                return cone.check_is_interior_expert(1.0, -1.0, y, 0.0, api.BUFFER_DUALCHECK)

            # S = C - y_1 I: spectrum lam - y_1
            assert interior(np.zeros(m)), (n, buf)
            ld = cone.log_barrier(1.0) if buf == api.BUFFER_DUALVAR else cone.log_barrier_of(buf)
            ref = float(np.sum(np.log(lam)))
            assert abs(ld - ref) <= 1e-11 * max(1.0, abs(ref)), (n, buf, ld, ref)
            span = lmax - lmin if n > 1 else lmax
            for shift, want in ((1e-8, True), (-1e-8, False), (1e-12, True)):
                y = (lmin - shift * span) * e0
                c0 = api.assemble_counts()
                ok = interior(y)
                # the path that decided: the one-launch small check assembles S itself, the blocked factor asks cone_assemble
                swept = sum(api.assemble_counts()) - sum(c0)
                small = (n + 15) // 16 * 16 <= 128 and m == 1
                assert (swept == 0) if small else (swept >= 1), (n, m, buf, swept)
                assert ok == want == lm.is_pd(lm.T(C, A, 1.0, y, 0.0)), (n, m, buf, shift, ok)
            for bad in (np.nan, np.inf):
                yb = np.zeros(m)
                yb[0] = bad
                assert not interior(yb), (n, buf, bad)
            assert interior(np.zeros(m)), (n, buf)                 # and back
    finally:
        cone.destroy()
