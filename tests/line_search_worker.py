"""child process of tests/test_gpu_line_search.py: the line search's dual-matrix requests, in sequences that walk every
answer cone_assemble (csrc/engine_cone.h) can give -- the same point, a copy, S + alpha dS (+ delta I) on the last ratio test's
line, the 16-link refresh, a sweep -- and every place that must invalidate what it remembers.  After every call the raw S,
the interior decision and the log-barrier are compared with the host fp64 model (tests/line_search_model.py).  The library
reads HDSDP_MI355X_AFFINE_S once per process, so the parent runs this once per mode; it prints one JSON line: per sequence
the worst errors, the assembly counters each step advanced, and the chain's drift."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)
import line_search_model as lm  # noqa: E402
from util import load_golden, y_of  # noqa: E402
from hdsdp_amd import api  # noqa: E402

BUFFER_DUALVAR, BUFFER_DUALCHECK = api.BUFFER_DUALVAR, api.BUFFER_DUALCHECK


class Probe:
    """one device cone beside its model; every request goes through here and is checked at once"""

    def __init__(self, n, m, seed, density=0.3, y0=None):
        rng = np.random.default_rng(seed)
        mats = [lm.random_sym(rng, n, density)] + [lm.random_sym(rng, n, density) for _ in range(m)]
        self.y0 = 0.05 + 0.1 * rng.random(m) if y0 is None else y0    # every component well away from zero (sequence d)
        self.dy = rng.standard_normal(m)
        # C is shifted so that C - sum y_i A_i (no residual term) is positive definite near y0, with a margin of the spectrum's
        # width: the primal recovery (sequence e) needs that matrix to be interior
        ev = np.linalg.eigvalsh(mats[0] - np.tensordot(self.y0, np.stack(mats[1:]), axes=1))
        mats[0] = mats[0] + (abs(float(ev[0])) + float(ev[-1] - ev[0])) * np.eye(n)
        self.csc = lm.to_csc(mats)
        self.n, self.m = n, m
        self.C, self.A = lm.from_csc(n, m, *self.csc)
        self.cone = api.SDPCone.from_csc(n, m, *self.csc)
        self.Rd = -0.25 * float(ev[-1] - ev[0])
        self.perturb = 0.0
        self.cone.set_start(self.Rd)
        self.p = None                      # (tau, y, eye) the device's S should hold
        self.dS = None
        self.err = {"S": 0.0, "logdet": 0.0, "checker_logdet": 0.0}
        self.bad = []

    def eye(self):
        return -self.Rd + self.perturb

    def model(self, tau, y, eye=None):
        return lm.T(self.C, self.A, tau, y, self.eye() if eye is None else eye)

    def check_S(self, what, alpha=0.0):
        D = lm.dev_lower(self.cone.dual_matrix())
        S = self.model(*self.p)
        den = float(np.max(np.abs(S))) + (abs(alpha) * float(np.max(np.abs(self.dS))) if self.dS is not None else 0.0)
        e = float(np.max(np.abs(D - S))) / den
        self.err["S"] = max(self.err["S"], e)
        if e > 1e-13:
            self.bad.append(f"{what}: S off the model by {e:.3e}")
        return S

    def check_logdet(self, got, S, key, what):
        ev = np.linalg.eigvalsh(S)
        ref = float(np.sum(np.log(ev)))
        e = abs(got - ref) / max(1.0, abs(ref))
        self.err[key] = max(self.err[key], e)
        if e > 1e-11:
            self.bad.append(f"{what}: log det {got!r} vs {ref!r}")

    def interior(self, tau, y, what, alpha=0.0):
        """the driver's "interior?" then "barrier" at the point just checked, then the same point again"""
        ok = self.cone.check_is_interior(tau, y)
        self.p = (tau, np.array(y), self.eye())
        S = self.check_S(what, alpha)
        want = lm.is_pd(S)
        if ok != want:
            self.bad.append(f"{what}: interior {ok}, model {want}")
        if ok:
            self.check_logdet(self.cone.log_barrier(tau), S, "logdet", what)
            self.check_logdet(self.cone.log_barrier(tau, y), S, "logdet", what + " (asked again)")
            self.check_S(what + " (asked again)", alpha)
        return ok

    def checker(self, tau, y, what):
        """the same kind of point into the checker buffer (the reference's trial points: HConeCheckIsInteriorExpert)"""
        ok = self.cone.check_is_interior_expert(tau, -1.0, y, -self.Rd, BUFFER_DUALCHECK)
        S = self.model(tau, y)
        if ok != lm.is_pd(S):
            self.bad.append(f"{what}: checker interior {ok}")
        if ok:
            self.check_logdet(self.cone.log_barrier_of(BUFFER_DUALCHECK), S, "checker_logdet", what)
        self.check_S(what + " (S untouched)")
        return ok

    def ratio(self, dtau, dy, ada=0.0):
        step = self.cone.ratio_test(dtau, dy, ada)
        self.dS = lm.T(self.C, self.A, dtau, dy, ada * self.Rd)
        self.check_S("after the ratio test")
        return step


def counts():
    return np.asarray(api.assemble_counts(), dtype=np.int64)


def run(label, fn, out):
    c0 = counts()
    extra = fn() or {}
    out[label] = {"counts": (counts() - c0).tolist(), **extra}


def line_search(P):
    """a: the reference's line search (interface/hdsdp_algo.c): check at y0, ratio test, trial points along the line, the same
    point again, an on-line point into the checker"""
    tau, y0, dy = 1.0, P.y0, P.dy
    assert P.interior(tau, y0, "a: start")
    step = P.ratio(0.0, dy)
    top = min(step, 1.0)
    for f in (0.9, 0.5, 0.3, 0.1):
        P.interior(tau, y0 + f * top * dy, f"a: trial {f}", f * top)
    P.checker(tau, y0 + 0.2 * top * dy, "a: checker on the line")
    P.checker(tau, y0 + 0.1 * top * dy, "a: checker at S's point")
    dtau = -0.05
    step = P.ratio(dtau, 0.5 * dy)
    P.interior(tau + 0.5 * min(step, 1.0) * dtau, y0 + 0.1 * top * dy + 0.5 * min(step, 1.0) * 0.5 * dy, "a: tau moves", 0.5)
    return {"step": step}


def eye_moves(P):
    """b: the identity coefficient moves between the ratio test and the request (reduce_resi, set_perturb, the corrector)"""
    rng = np.random.default_rng(7)
    tau, y = P.p[0], P.p[1]
    step = min(P.ratio(0.0, P.dy), 1.0)
    Rd0 = P.Rd

    def trial(q, what, a):
        # (a point outside leaves no factor for the next ratio test: go back to the last interior one, as the driver does)
        y_prev = P.p[1]
        if not P.interior(tau, q, what, a):
            P.interior(tau, y_prev, what + ", back")
    def reduced(frac):
        # the residual cut so that the current point keeps `frac` of its distance to the boundary
        lam = float(np.linalg.eigvalsh(lm.T(P.C, P.A, tau, P.p[1], 0.0))[0])
        return -(-lam + frac * (P.eye() + lam) - P.perturb)
    P.Rd = reduced(0.6)
    P.cone.reduce_resi(P.Rd)
    trial(y + 0.1 * step * P.dy, "b: residual reduced", 0.1 * step)
    y = P.p[1]
    step = min(P.ratio(0.0, P.dy), 1.0)
    P.perturb = 1e-3 * abs(Rd0)
    P.cone.set_perturb(P.perturb)
    trial(y + 0.1 * step * P.dy, "b: perturbation", 0.1 * step)
    y = P.p[1]
    d1, d2, b = rng.standard_normal(P.m), rng.standard_normal(P.m), 0.7
    step = min(P.ratio(0.0, b * d2 - d1), 1.0)
    P.Rd = reduced(0.8)
    P.cone.reduce_resi(P.Rd)
    a = 0.1 * step
    trial(y + a * b * d2 - a * d1, "b: corrector point, residual reduced", a)     # formed in another association
    P.perturb = 0.0
    P.cone.set_perturb(0.0)
    P.interior(tau, P.p[1], "b: perturbation back to zero")


def chain(P, links=20):
    """c: in-place updates along one line, across the 16-link refresh; the last one against a fresh sweep"""
    tau, y = P.p[0], P.p[1]
    step = min(P.ratio(0.0, P.dy), 1.0)
    # (no component of y may come near zero on the way: the short-cut's match is relative per component)
    h = min(0.4 * step, 0.5 * float(np.min(np.abs(y))) / float(np.max(np.abs(P.dy)))) / links
    drift = []
    for k in range(1, links + 1):
        P.interior(tau, y + k * h * P.dy, f"c: link {k}", k * h)
        D = lm.dev_lower(P.cone.dual_matrix())
        S = P.model(*P.p)
        drift.append(float(np.max(np.abs(D - S))) / (float(np.max(np.abs(S))) + k * h * float(np.max(np.abs(P.dS)))))
    last = lm.dev_lower(P.cone.dual_matrix())
    P.cone.scal_by_constant(1.0)                                   # (exact: forgets the point, changes nothing)
    P.interior(tau, P.p[1], "c: fresh sweep")
    fresh = lm.dev_lower(P.cone.dual_matrix())
    e = float(np.max(np.abs(last - fresh))) / float(np.max(np.abs(fresh)))
    if e > 1e-13:
        P.bad.append(f"c: chain end vs fresh sweep {e:.3e}")
    return {"drift": drift, "chain_vs_sweep": e}


def tolerance_edge(P):
    """d: one component off the tested line by 1e-12 relative (must sweep) and by 4e-15 (short-cut); both exact"""
    tau, y = P.p[0], P.p[1]
    step = min(P.ratio(0.0, P.dy), 1.0)
    k = int(np.argmin(np.abs(P.dy)))            # not the component the short-cut takes alpha from
    res = {}
    for rel, key in ((1e-12, "far"), (4e-15, "near")):
        q = y + 0.2 * step * P.dy
        q[k] *= 1.0 + rel
        c0 = counts()
        P.interior(tau, q, f"d: off the line by {rel:g}", 0.2 * step)
        res[key] = (counts() - c0).tolist()
        P.ratio(0.0, P.dy)
        y = P.p[1]
    return res


def invalidation(P):
    """e: what must make the next request assemble, between a ratio test and an on-line request"""
    res = {}
    tau = P.p[0]

    def online(what):
        # S re-established at the current point (a sweep where the state was forgotten), then the ratio test of the line
        y = P.p[1]
        assert P.interior(tau, y, f"e: {what}: current point")
        step = min(P.ratio(0.0, P.dy), 1.0)
        return y, step

    # scal_by_constant
    y, step = online("scal")
    P.cone.scal_by_constant(1.25)
    P.C = P.C * 1.25
    c0 = counts()
    P.interior(tau, y + 0.3 * step * P.dy, "e: after scal_by_constant", 0.3 * step)
    res["scal"] = (counts() - c0).tolist()
    # HMiConeAddStepToBufferAndCheck on S: S moves without a point being named
    y, step = online("axpy")
    ok = P.cone.axpy_buffer_and_check(0.2 * step, BUFFER_DUALVAR)
    P.p = (tau, y + 0.2 * step * P.dy, P.eye())
    S = P.check_S("e: after S += step dS", 0.2 * step)
    if ok != lm.is_pd(S):
        P.bad.append("e: axpy-and-check decision")
    c0 = counts()
    P.interior(tau, y + 0.35 * step * P.dy, "e: after axpy_buffer_and_check", 0.35 * step)
    res["axpy"] = (counts() - c0).tolist()
    # the sweep-copy toggle
    y, step = online("toggle")
    P.cone.use_sweep_copy(False)
    c0 = counts()
    P.interior(tau, y + 0.3 * step * P.dy, "e: after use_sweep_copy(0)", 0.3 * step)
    res["toggle"] = (counts() - c0).tolist()
    P.cone.use_sweep_copy(True)
    # primal recovery replaces dS; then a point on the OLD line
    y, step = online("primal")
    mu = 0.7
    pdy = 0.01 * np.cos(np.arange(P.m))
    X = P.cone.get_primal(mu, y, pdy)
    Sp = lm.T(P.C, P.A, 1.0, y, 0.0)
    assert lm.is_pd(Sp), "the recovery point must be interior (see Probe)"
    Xm = lm.primal_X(Sp, lm.T(P.C, P.A, 0.0, -pdy, 0.0), mu)
    ex = float(np.max(np.abs(X - Xm))) / float(np.max(np.abs(Xm))) if X is not None else float("inf")
    res["primal_err"] = ex
    if not ex <= 1e-10:
        P.bad.append(f"e: primal X off by {ex:.3e}")
    c0 = counts()
    P.interior(tau, y + 0.3 * step * P.dy, "e: old line after get_primal", 0.3 * step)
    res["primal"] = (counts() - c0).tolist()
    return res


def phase_a_case(out):
    """e, last case: the fused Phase-A pass writes S itself (small rank-one block: mcp100)"""
    g = load_golden("mcp100_A")
    n, m = int(g["dims"][0]), int(g["dims"][1])
    C, A = lm.from_csc(n, m, g["csc_beg"], g["csc_idx"], g["csc_val"])
    cone = api.SDPCone.from_csc(n, m, g["csc_beg"], g["csc_idx"], g["csc_val"])
    Rd, tau, y = float(g["Rd"][0]), float(g["tau"][0]), y_of(g)
    cone.set_start(Rd)
    kkt = api.KKT(m, [cone])
    bad = []
    try:
        # the primal recovery at the golden's recovery point, against the definition
        mu, py, pdy = float(g["pr_mu"][0]), g["pr_y"], g["pr_dy"]
        X = cone.get_primal(mu, py, pdy)
        Xm = lm.primal_X(lm.T(C, A, 1.0, py, 0.0), lm.T(C, A, 0.0, -pdy, 0.0), mu)
        primal_err = float(np.max(np.abs(X - Xm))) / float(np.max(np.abs(Xm))) if X is not None else float("inf")
        assert cone.check_is_interior(tau, y)
        dy = 0.01 * np.sin(np.arange(m) + 0.5)
        step = min(cone.ratio_test(0.0, dy, 0.0), 1.0)
        assert kkt.phase_a_eligible()
        y2 = y + 0.5 * step * dy + 1e-3 * np.cos(np.arange(m))
        ok, ld, *_ = kkt.phase_a(tau, y2, g["b"])
        S2 = lm.T(C, A, tau, y2, -Rd)
        if ok != lm.is_pd(S2) or (ok and abs(ld - lm.logdet(S2)) > 1e-11 * max(1.0, abs(ld))):
            bad.append("phase A: decision or log det")
        c0 = counts()
        q = y + 0.3 * step * dy
        ok = cone.check_is_interior(tau, q)
        S = lm.T(C, A, tau, q, -Rd)
        D = lm.dev_lower(cone.dual_matrix())
        e = float(np.max(np.abs(D - S))) / float(np.max(np.abs(S)))
        if e > 1e-13 or ok != lm.is_pd(S):
            bad.append(f"phase A: old line after the pass: S off by {e:.3e}")
        if ok and abs(cone.log_barrier(tau) - lm.logdet(S)) > 1e-11 * max(1.0, abs(lm.logdet(S))):
            bad.append("phase A: old line after the pass: log det")
        out["phase_a"] = {"counts": (counts() - c0).tolist(), "err": e, "bad": bad, "primal_err": primal_err}
    finally:
        kkt.destroy()
        cone.destroy()


def downstream(out, mode):
    """f: two cones in one operator, S from a short-cut, then the Schur build against the pinned oracle's formulas"""
    import oracle_py
    from util import check_close, lower_mask
    m = 40
    P0 = Probe(257, m, 31)
    Ps = [P0, Probe(180, m, 32, y0=P0.y0)]
    tau = 1.0
    for P in Ps:
        assert P.interior(tau, P.y0, "f: start")
    dy = Ps[0].dy
    for P in Ps:
        P.dy = dy
    steps = [min(P.ratio(0.0, dy), 1.0) for P in Ps]
    a = 0.4 * min(steps)
    c0 = counts()
    y0 = P0.y0
    for P in Ps:
        P.interior(tau, y0 + a * dy, "f: trial", a)
    cnt = (counts() - c0).tolist()
    kkt = api.KKT(m, [P.cone for P in Ps])
    res = {"counts": cnt}
    try:
        kkt.build_up(api.KKT_TYPE_HOMOGENEOUS)
        ex = kkt.export()
        ref = None
        for P in Ps:
            blk = oracle_py.Block(P.n, m, *P.csc)
            try:
                Sinv = np.linalg.inv(P.model(*P.p))
                r = blk.kkt_build(np.ascontiguousarray(0.5 * (Sinv + Sinv.T)), P.Rd, 2)
            finally:
                blk.close()
            ref = r if ref is None else {k: ref[k] + r[k] for k in ref}
        msk = lower_mask(m)
        errs = {}
        try:
            errs["M"] = check_close(kkt.M[msk], ref["M"][msk], "M")
            for k in ("ASinv", "ASinvRdSinv", "ASinvCSinv"):
                errs[k] = check_close(ex[k], ref[k], k)
            for k in ("CSinv", "CSinvCSinv", "CSinvRdSinv", "TraceSinv"):
                errs[k] = check_close([ex[k]], [ref[k]], k)
        except AssertionError as exc:
            res["bad"] = [str(exc)]
        res["errs"] = errs
    finally:
        kkt.destroy()
        for P in Ps:
            res.setdefault("bad", []).extend(P.bad)
            P.cone.destroy()
    out["downstream"] = res


def main():
    mode = os.environ.get("HDSDP_MI355X_AFFINE_S", "default")
    out = {"mode": mode}
    for n, m, seed in ((257, 64, 1), (300, 60, 2), (100, 10, 3)):
        P = Probe(n, m, seed)
        r = {}
        print(f"line_search_worker: {n} x {m}", file=sys.stderr, flush=True)
        run("a", lambda: line_search(P), r)
        run("b", lambda: eye_moves(P), r)
        run("c", lambda: chain(P), r)
        run("d", lambda: tolerance_edge(P), r)
        run("e", lambda: invalidation(P), r)
        r["err"], r["bad"] = P.err, P.bad
        out[f"{n}x{m}"] = r
        P.cone.destroy()
    phase_a_case(out)
    downstream(out, mode)
    print("LINE_SEARCH_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
