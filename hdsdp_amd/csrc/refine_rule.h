// refine_rule.h -- the rule of the refined Schur solve: its tolerance, when the loop stops and which iterate it hands back.
// Pure host arithmetic: no HIP call, no engine state.  The engine performs it (engine_linsys.h: lin_solve_refined) on residuals
// formed in twice the working precision (refine.hip); where the residual's matrix comes from is kkt_store.h's
// hdm_kkt_refine_source.  tests/test_refine_rule_cpu.py compiles this header and kkt_store.h alone.
//
// The loop: solve, form r0 = b - M x0.  |r0| < tol: CONVERGED with 0 steps, x0 as it is.  Otherwise step k solves M d = r with the
// same factor, x <- x + d, forms the new residual and stops at
//   CONVERGED   |r_k| < tol
//   STAGNATED   |r_k| >= 0.5 |r_k-1|: the iterate with the smaller residual is returned (the previous one is kept for that)
//   MAXSTEPS    k reached the cap
//   NUMERICAL   |r_k| is not finite: the unrefined solution is returned (HFpLinsysSolve's NaN escalation sees what it saw before)
// Unlike the reference's Cholesky-preconditioned CG (hdsdp_linsolver.c:1446-1588) a solve that stops short of tol is no failure:
// 1e-12 absolute cannot be reached in fp64 once u |M| |x| exceeds it.  The status says what happened.
#pragma once
#include <algorithm>
#include <cmath>

enum HdmRefineStatus {
    HDM_REFINE_OFF = 0,         // refinement is off: the solve ran as it always did
    HDM_REFINE_CONVERGED,
    HDM_REFINE_STAGNATED,
    HDM_REFINE_MAXSTEPS,
    HDM_REFINE_NUMERICAL,
    HDM_REFINE_NO_MATRIX,       // the factorised matrix is no longer (or was never) at hand: the solve ran unrefined
    HDM_REFINE_NOT_AVAILABLE    // the storage form's refined solve is not switched on (tile form, kkt_store.h): the solve ran unrefined
};

constexpr int HDM_REFINE_STEP_CAP = 8;
constexpr double HDM_REFINE_DEFAULT_TOL = 1e-6;      // the reference's defaults (hdsdp_linsolver.c:1314-1315)
constexpr double HDM_REFINE_STAGNATION = 0.5;

static inline int hdm_refine_clamp(int maxSteps) { return maxSteps <= 0 ? 0 : std::min(maxSteps, HDM_REFINE_STEP_CAP); }

// the reference's formula (hdsdp_linsolver.c:1486-1487); a tolerance that was never set (<= 0) takes the default
static inline double hdm_refine_tol(double relTol, double absTol, double rhsNorm) {
    if (!(relTol > 0.0)) relTol = HDM_REFINE_DEFAULT_TOL;
    if (!(absTol > 0.0)) absTol = HDM_REFINE_DEFAULT_TOL;
    return std::max(std::min(absTol, relTol * rhsNorm), 0.1 * absTol);
}

enum HdmRefineKeep { HDM_REFINE_KEEP_CURRENT = 0, HDM_REFINE_KEEP_PREVIOUS, HDM_REFINE_KEEP_UNREFINED };

// One refined solve.  first() takes |r0|^2, next() the squared residual norm after each correction; both return true while another
// correction is to be made.  Afterwards: status, keep (which iterate goes back to the caller), steps (corrections IN that iterate),
// solves (correction solves made), resid0 and resid (of the returned iterate).
struct HdmRefineLoop {
    int cap = 0;
    double tol = 0.0;
    HdmRefineStatus status = HDM_REFINE_OFF;
    HdmRefineKeep keep = HDM_REFINE_KEEP_CURRENT;
    int steps = 0, solves = 0;
    double resid0 = 0.0, resid = 0.0;

    HdmRefineLoop(int maxSteps, double tolerance) : cap(hdm_refine_clamp(maxSteps)), tol(tolerance) {}

    bool first(double norm2) {
        resid0 = resid = std::sqrt(norm2);
        if (!std::isfinite(resid0)) return stop(HDM_REFINE_NUMERICAL, HDM_REFINE_KEEP_UNREFINED);
        if (resid0 < tol) return stop(HDM_REFINE_CONVERGED, HDM_REFINE_KEEP_CURRENT);
        if (cap == 0) return stop(HDM_REFINE_MAXSTEPS, HDM_REFINE_KEEP_CURRENT);
        return true;
    }
    bool next(double norm2) {
        const double prev = resid, now = std::sqrt(norm2);
        solves += 1;
        if (!std::isfinite(now)) { steps = 0; resid = resid0; return stop(HDM_REFINE_NUMERICAL, HDM_REFINE_KEEP_UNREFINED); }
        if (now < prev) { steps = solves; resid = now; }
        if (now < tol) return stop(HDM_REFINE_CONVERGED, HDM_REFINE_KEEP_CURRENT);
        if (now >= HDM_REFINE_STAGNATION * prev) return stop(HDM_REFINE_STAGNATED, now < prev ? HDM_REFINE_KEEP_CURRENT : HDM_REFINE_KEEP_PREVIOUS);
        if (solves >= cap) return stop(HDM_REFINE_MAXSTEPS, HDM_REFINE_KEEP_CURRENT);
        return true;
    }

private:
    bool stop(HdmRefineStatus s, HdmRefineKeep k) { status = s; keep = k; return false; }
};
