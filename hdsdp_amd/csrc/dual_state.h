// dual_state.h -- where a block's dual matrix S and step matrix dS stand, and how a request for a dual matrix is answered.
// S = T(pS) and dS = T(pD) for the linear map T(tau, y, eye) = tau C - sum y_i A_i + eye I.  The reference's line searches and
// correctors ask for the dual matrix twice at the same point (interior check, then barrier) and at points y + alpha dy along the
// direction whose dS the ratio test has just assembled: each a 32 GB sweep over all m constraint matrices at n = m = 2000 (6 ms,
// 344 such requests per headline solve, 14 % of a whole solve's device time).  A request for T(p) is compared with what the
// buffers hold, component by component, and answered by nothing, a copy, or S + alpha dS (+ delta I) -- one pass over n^2 --
// where that is what it is; anything else takes the sweep.
// Pure host arithmetic on at most m + 2 doubles: no HIP call, no engine state.  The engine performs what hdm_dual_plan says and
// commits it (engine_cone.h: cone_assemble); every other writer of S, dS or the factor names what it did through one of
// HdmDualState's transitions.  tests/test_dual_state_cpu.py compiles this header alone.
#pragma once
#include "env_switches.h"
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

// ---- constants ------------------------------------------------------------------------------
// A point counts as on the line pS + alpha pD when tau and every multiplier agree to 8e-15 relative: the driver forms its trial
// points in another association than pS + alpha pD, and the differences measured on a whole solve reach 4e-15 (a 1.8e-15 bound
// turned 157 of 345 such requests of the headline solve into 15.6 GB sweeps for one or two components at 2e-15:
// HDSDP_MI355X_AFFINE_DEBUG=1 prints every miss).
constexpr double HDM_DUAL_LINE_TOL = 8e-15;
// updates of S in place before a request for S is swept afresh, so that the rounding of a chain of S + alpha dS stays bounded
constexpr int HDM_DUAL_CHAIN_MAX = 16;
// "a sweep costs something": 16 MiB of owned constraint data or more, i.e. from about n = m = 160 on.  From here on a block
// tracks lines by default (hdm_dual_mode) and gets a zero-suppressed sweep copy (row_store_rule.h: hdm_sweep_copy_rule).
constexpr long HDM_SWEEP_COSTS_BYTES = 16L << 20;
static inline bool hdm_sweep_costs(long mloc, long n) { return mloc * n * (n + 1) * 4 >= HDM_SWEEP_COSTS_BYTES; }

// ---- mode -----------------------------------------------------------------------------------
// 0: every request is swept.  1: only the exact case -- the same point again -- is short-cut, so every number is the one a sweep
// would have produced.  2: also points on the line through the last ratio test's direction (S + alpha dS); the results then
// differ from a sweep's in the last bits (as a sweep's differ from the reference's own summation order).
// Default: 2 where a sweep costs something, and 1 on small blocks, where the sweep is free and the end game of a badly
// conditioned instance can turn on the last bits (gpp100 through the reference's driver in mode 2: same dual objective, a primal
// estimate 3e-4 further away).  HDSDP_MI355X_AFFINE_S=0/1/2 overrides (read time: env_switches.h).
static inline int hdm_dual_mode(long mloc, long n) {
    const int env = hdm_env_int<ENV_AFFINE_S>().value_or(-1);
    return env >= 0 ? env : (hdm_sweep_costs(mloc, n) ? 2 : 1);
}
static inline bool hdm_dual_debug() { return hdm_env_on<ENV_AFFINE_DEBUG>(); }

// ---- counters -------------------------------------------------------------------------------
// how a request was answered (HMiGetAssembleCounts and the exit table of engine_stats.h index them in this order)
enum HdmAsmCount {
    HDM_ASM_HELD = 0,          // the buffer already held the point
    HDM_ASM_COPY,              // a copy of S
    HDM_ASM_LINE,              // S + alpha dS (+ delta I) on the last ratio test's line
    HDM_ASM_SWEEP_OFF_LINE,    // a sweep for a dual matrix: the point was not on that line, or no point / no line was known
    HDM_ASM_SWEEP_REFRESH,     // a sweep because HDM_DUAL_CHAIN_MAX updates in a row are refreshed
    HDM_ASM_SWEEP_STEP,        // a sweep for a step matrix (every ratio test)
    HDM_ASM_SWEEP_UNTRACKED,   // sweeps of blocks that do not track points (mode 0, sharded)
    HDM_ASM_N
};

// ---- point ----------------------------------------------------------------------------------
// the argument of T: tau, the identity coefficient, and a view of the owned multipliers
struct HdmDualPoint {
    double tau = 0.0, eye = 0.0;
    const double *y = nullptr;
    int ny = 0;
    int size() const { return ny + 2; }
    double comp(int i) const { return i == 0 ? tau : i == 1 ? eye : y[i - 2]; }   // stored order: tau, eye, multipliers
    bool same_as(const std::vector<double> &p) const {                            // exactly: a NaN is the same as nothing
        if ((int) p.size() != size()) return false;
        for (int i = 0; i < size(); ++i)
            if (comp(i) != p[i]) return false;
        return true;
    }
    void store(std::vector<double> &p) const {
        p.resize((size_t) size());
        for (int i = 0; i < size(); ++i) p[i] = comp(i);
    }
};

enum HdmDualTarget { HDM_DUAL_S = 0, HDM_DUAL_SCHECK, HDM_DUAL_DS };
enum HdmDualAction { HDM_DUAL_NONE = 0, HDM_DUAL_COPY_FROM_S, HDM_DUAL_AXPY, HDM_DUAL_AXPY_EYE, HDM_DUAL_SWEEP };

struct HdmDualPlan {
    HdmDualAction action = HDM_DUAL_SWEEP;
    double alpha = 0.0, delta = 0.0;   // AXPY: target = S + alpha dS; AXPY_EYE: + delta I
    HdmAsmCount counter = HDM_ASM_SWEEP_UNTRACKED;
    bool tracked = false;              // the block records the points of what it assembles
    // the line test, where it ran and missed (HDSDP_MI355X_AFFINE_DEBUG: hdm_dual_print_miss)
    bool line_missed = false;
    int off_line = 0;                  // components off the line
    double worst = 0.0;                // worst relative distance of a component from the line ...
    int worst_at = -1;                 // ... and its index (0: tau; 2 + q: multiplier q)
};

// ---- state ----------------------------------------------------------------------------------
class HdmDualState {
    std::vector<double> pS, pD;          // tau, eye, then the owned multipliers
    bool pS_ok = false, pD_ok = false;
    int aff_chain = 0;                   // updates of S in place since its last full assembly
    bool fac_ok = false; int fac_psd = 0;   // the dual factor object holds the factorisation of S = T(pS) (result: fac_psd)
    unsigned long n_moves = 0;           // transitions so far: whoever keeps something derived from S, dS or the factor compares it
    // Two counters the transitions above do not give (small_step_rule.h: a stored step-and-check answer is served only while
    // neither has moved): every rewrite of dS, whether or not the block tracks points (dS_assembled_at is a tracking block's alone),
    // and every write of the checker buffer or the checker factor object, which no transition names.  Neither enters moves().
    unsigned long n_dS_writes = 0, n_checker = 0;
    friend HdmDualPlan hdm_dual_plan(const HdmDualState &, const HdmDualPoint &, HdmDualTarget, int, int);
    friend void hdm_dual_print_miss(FILE *, const HdmDualState &, const HdmDualPoint &, HdmDualTarget, const HdmDualPlan &);

public:
    bool S_is_at(const HdmDualPoint &p) const { return pS_ok && p.same_as(pS); }
    // S = T(p) and its factor are in place (the one-launch small check: the reference's line search asks "interior?" and then
    // for the barrier at the point it has just checked)
    bool S_factored_at(const HdmDualPoint &p, int *psd) const {
        if (!(fac_ok && S_is_at(p))) return false;
        if (psd) *psd = fac_psd;
        return true;
    }

    // every transition below counts here; a value read after one and found again later says that none has happened in between
    // (small_ratio_rule.h: a stored ratio-test answer is served only then)
    unsigned long moves() const { return n_moves; }
    unsigned long dS_writes() const { return n_dS_writes; }
    unsigned long checker_epoch() const { return n_checker; }
    // dS rewritten by a path that does not go through commit (the grouped ratio launch); Scheck or the checker factor object
    // written (cone_small_check on the checker, cone_factor_check, cone_axpy_check, the primal recovery, the grouped step launch)
    void dS_written() { n_dS_writes += 1; }
    void checker_written() { n_checker += 1; }

    // Transitions, named for what happened.  Whatever moves S leaves its factor behind.
    // S assembled at p: a sweep of a tracking block, or the one-launch small check (which assembles S itself)
    void S_assembled_at(const HdmDualPoint &p) { n_moves += 1; p.store(pS); pS_ok = true; aff_chain = 0; fac_ok = false; }
    // dS assembled at p (every ratio test, the primal recovery: a request on the OLD line is then off the new one)
    void dS_assembled_at(const HdmDualPoint &p) { n_moves += 1; p.store(pD); pD_ok = true; }
    // S advanced along the line to p: S <- S + alpha dS (+ delta I) in place
    void S_advanced_to(const HdmDualPoint &p) { n_moves += 1; p.store(pS); aff_chain += 1; fac_ok = false; }
    // S written by someone else, at a point this state is not told: the next request assembles it.
    //  * S += step dS without a point being named (cone_axpy_check on the dual buffer);
    //  * the fused Phase-A pass writes S itself (HMiKKTPhaseA);
    //  * a sweep of a block that does not track points.
    void S_overwritten() { n_moves += 1; pS_ok = false; fac_ok = false; }
    // the data under S and dS changed: both are T of nothing known, no short-cut from them.
    //  * the objective was rescaled (cone_scal): S and dS were assembled with the old one;
    //  * the sweep copy was switched (HMiConeUseSweepCopy): the next request is assembled, not short-cut.
    void data_changed() { n_moves += 1; pS_ok = pD_ok = false; fac_ok = false; }
    // S factored with result r, in the dual factor object, by a path that keeps the result (the one-launch small check)
    void S_factored(int psd) { n_moves += 1; fac_ok = true; fac_psd = psd; }
    // the factor no longer follows S: S moves and its factor does not (cone_update), or the factor object is being rewritten by
    // a path that does not record its result (cone_factor_S)
    void factor_stale() { n_moves += 1; fac_ok = false; }

    // what performing `plan` for a request of T(p) into `target` did to the buffers
    void commit(const HdmDualPlan &plan, const HdmDualPoint &p, HdmDualTarget target) {
        if (target == HDM_DUAL_DS) dS_written();                              // in every mode: tracking decides what is REMEMBERED of it
        if (target == HDM_DUAL_SCHECK) checker_written();
        switch (plan.action) {
        case HDM_DUAL_NONE: case HDM_DUAL_COPY_FROM_S: break;                 // S stays; the checker buffer is not tracked
        case HDM_DUAL_AXPY: case HDM_DUAL_AXPY_EYE: if (target == HDM_DUAL_S) S_advanced_to(p); break;
        case HDM_DUAL_SWEEP:
            if (target == HDM_DUAL_S) { if (plan.tracked) S_assembled_at(p); else S_overwritten(); }
            // (pD is only ever recorded by a tracking block, and whether a block tracks never changes)
            else if (target == HDM_DUAL_DS && plan.tracked) dS_assembled_at(p);
            break;
        }
    }
};

// ---- the rule -------------------------------------------------------------------------------
// How a request for T(p) into `target` is answered, given what the buffers hold.  `mode`: hdm_dual_mode; `world`: ranks the
// block's rows are dealt over -- a sharded block does not track points (every rank would have to agree on every decision).
inline HdmDualPlan hdm_dual_plan(const HdmDualState &st, const HdmDualPoint &p, HdmDualTarget target, int mode, int world) {
    HdmDualPlan r;
    r.tracked = mode > 0 && world == 1;
    auto sweep = [&](HdmAsmCount k) { r.action = HDM_DUAL_SWEEP; r.counter = k; return r; };
    if (target == HDM_DUAL_DS) return sweep(HDM_ASM_SWEEP_STEP);              // a new direction: nothing to derive it from
    if (!r.tracked) return sweep(HDM_ASM_SWEEP_UNTRACKED);
    if (!st.pS_ok) return sweep(HDM_ASM_SWEEP_OFF_LINE);                      // (no point known yet: a first assembly)
    if (p.same_as(st.pS)) {                                                   // S already is T(p): nothing, or a copy into the other buffer
        r.action = (target == HDM_DUAL_S) ? HDM_DUAL_NONE : HDM_DUAL_COPY_FROM_S;
        r.counter = (target == HDM_DUAL_S) ? HDM_ASM_HELD : HDM_ASM_COPY;
        return r;
    }
    if (!st.pD_ok || mode < 2) return sweep(HDM_ASM_SWEEP_OFF_LINE);
    // Is p = pS + alpha pD + delta e_eye for some alpha, delta?  alpha from the largest multiplier component of pD (tau if it
    // has none), checked on tau and every multiplier to HDM_DUAL_LINE_TOL; the identity coefficient is free: the driver's trial
    // points move y along the tested direction with the residual held, and its corrector ends at y + a (b d2 - d1) with the
    // residual reduced (interface/hdsdp_algo.c:911-921) -- the tested direction plus a multiple of the identity, which costs n
    // additions on top of S + alpha dS.
    const int np = p.size();
    int kmax = -1;
    for (int i = 2; i < np; ++i) if (st.pD[i] != 0.0 && (kmax < 0 || fabs(st.pD[i]) > fabs(st.pD[kmax]))) kmax = i;
    if (kmax < 0 && st.pD[0] != 0.0) kmax = 0;
    if (kmax >= 0) r.alpha = (p.comp(kmax) - st.pS[kmax]) / st.pD[kmax];
    bool hit = std::isfinite(r.alpha);
    for (int i = 0; i < np; ++i) {
        if (i == 1) continue;
        const double d = p.comp(i) - st.pS[i], e = r.alpha * st.pD[i];
        const double sc = fabs(p.comp(i)) + fabs(st.pS[i]) + fabs(e);
        if (fabs(d - e) > HDM_DUAL_LINE_TOL * sc) { hit = false; r.off_line += 1; }
        if (sc > 0.0 && fabs(d - e) / sc > r.worst) { r.worst = fabs(d - e) / sc; r.worst_at = i; }
    }
    r.delta = (p.eye - st.pS[1]) - r.alpha * st.pD[1];
    if (!hit) { r.line_missed = true; return sweep(HDM_ASM_SWEEP_OFF_LINE); }
    if (target == HDM_DUAL_S && st.aff_chain >= HDM_DUAL_CHAIN_MAX) return sweep(HDM_ASM_SWEEP_REFRESH);
    r.action = (r.delta == 0.0) ? HDM_DUAL_AXPY : HDM_DUAL_AXPY_EYE;
    r.counter = HDM_ASM_LINE;
    return r;
}

// HDSDP_MI355X_AFFINE_DEBUG=1: one line per request that missed the last ratio test's line (plan.line_missed)
inline void hdm_dual_print_miss(FILE *f, const HdmDualState &st, const HdmDualPoint &p, HdmDualTarget target, const HdmDualPlan &r) {
    double dd = 0.0, pp = 0.0, dp = 0.0;
    for (int i = 2; i < p.size(); ++i) { const double d = p.comp(i) - st.pS[i]; dd += d * d; pp += st.pD[i] * st.pD[i]; dp += d * st.pD[i]; }
    fprintf(f, "[hdsdp_mi355x affine] miss (%s): alpha %.6e, %d of %d components off the tested line, worst relative %.3e at %d; "
               "d tau %.3e, d eye %.3e, |d y| %.3e, |pD y| %.3e, cos %.9f\n", target == HDM_DUAL_S ? "S" : "checker", r.alpha, r.off_line,
            p.size(), r.worst, r.worst_at, p.tau - st.pS[0], p.eye - st.pS[1], sqrt(dd), sqrt(pp), (dd > 0 && pp > 0) ? dp / sqrt(dd * pp) : 0.0);
}
