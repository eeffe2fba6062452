// small_step_rule.h -- which cones the grouped step-and-check (small.hip: hdm_grouped_step_check_kernel, engine_step_set.h)
// answers, and when a stored answer may be served: two rules, stated once.  Pure host arithmetic: no HIP call, no engine state.
// The step set of an operator asks the first per cone at HKKTInit, the hook in cone_axpy_check asks the second per call.
// tests/test_small_step_rule_cpu.py compiles this header alone.  DESIGN.md section 24.
#pragma once
#include "dual_state.h"
#include "small_check_rule.h"

// ---- membership -----------------------------------------------------------------------------------------------------------
// The kernel forms S + dStep dS and runs the register sweep HdmChol::factor runs on a one-block object: the check set's population
// (for the cone's dual factor object), a checker object of the same shape -- one 128-block, whose Dinv the sweep writes -- and
// HDM_DIAG_SWEEP in its default position: with HDM_DIAG_SWEEP=0 the per-cone path runs another kernel, whose bits the sweep's are
// not.  The launch's dynamic LDS is hdm_small_check_lds_bytes(0) whatever the block's rows: no multipliers are staged.  n = 1 is
// a member like any other.
struct HdmSmallStepCone {
    HdmSmallCheckCone chk;     // the cone as the check rule sees it, with its DUAL factor object's shape
    int chk_npad = 0, chk_nblk = 0;   // the CHECKER factor object the launch would write (HdmChol::npad, ::nblk)
    bool diag_sweep = true;    // HDM_DIAG_SWEEP
};

static inline bool hdm_small_step_member(const HdmSmallStepCone &c) {
    if (!hdm_small_check_eligible(c.chk)) return false;       // one device, resident rows, n16 <= 128, the data bound, a one-block factor
    if (!hdm_small_check_factor_ok(c.chk_npad, c.chk_nblk)) return false;
    return c.diag_sweep;
}

// ---- the slot -------------------------------------------------------------------------------------------------------------
// The question is (dStep, whichBuffer == BUFFER_DUALCHECK); its answer -- Scheck = S + dStep dS, the checker's factor, the flag --
// is a function of S, dS and dStep alone, and asking again changes nothing (no warm start, unlike a ratio test).  So a slot serves
// any number of times, while
//   * dStep is exactly the one it holds (==: a NaN is the same as nothing), and
//   * nothing has been written to the member's S, dS, Scheck or checker factor since the commit: the three counters of
//     HdmDualState stand where they stood -- moves() for S (every writer of S names a transition), dS_writes() for dS in every
//     tracking mode, checker_epoch() for the checker buffer and the checker factor object.
struct HdmStepEpochs {
    unsigned long moves = 0, dS_writes = 0, checker = 0;
    bool operator==(const HdmStepEpochs &o) const { return moves == o.moves && dS_writes == o.dS_writes && checker == o.checker; }
};
static inline HdmStepEpochs hdm_step_epochs(const HdmDualState &st) { return {st.moves(), st.dS_writes(), st.checker_epoch()}; }

struct HdmStepSlot {
    bool valid = false;
    double dStep = 0.0;
    int info = 0;              // the sweep's report: 0, or the first non-positive pivot + 1
    HdmStepEpochs at;          // the member's counters after the launch was committed
};

static inline bool hdm_step_slot_serves(const HdmStepSlot &s, double dStep, const HdmStepEpochs &now) {
    return s.valid && s.dStep == dStep && s.at == now;
}
