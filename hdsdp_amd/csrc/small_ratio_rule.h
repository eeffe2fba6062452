// small_ratio_rule.h -- which cones the grouped ratio test (lanczos.hip: hdm_grouped_ratio_kernel, small.hip:
// hdm_grouped_safeguard_kernel, engine_ratio_set.h) answers, and when a stored answer may be served: two rules, stated once.
// Pure host arithmetic: no HIP call, no engine state.  The ratio set of an operator asks the first per cone at HKKTInit, the hook
// in cone_ratio_test asks the second per call.  tests/test_small_ratio_rule_cpu.py compiles this header alone.  DESIGN.md section 22.
// The same two rules for a question on the checker buffer stand below them (DESIGN.md section 26;
// tests/test_small_ratio_checker_rule_cpu.py).
#pragma once
#include "dual_state.h"
#include "lanczos_rule.h"
#include "small_check_rule.h"
#include <vector>

// ---- membership -----------------------------------------------------------------------------------------------------------
// The kernel's dynamic LDS is the region the one-launch Lanczos test packs its two lower triangles into: 2 * n16 * (n16 + 1) / 2
// doubles.  Before the triangles are packed the same region stages the member's multipliers for the step-matrix sum, so
//     mloc <= n16 * (n16 + 1)
// (272 rows at n16 = 16, 16 512 at n16 = 128; the check rule's data bound keeps mloc <= 2048, so this bound is the binding one
// only for n16 <= 32: 2^19 / 16^2 = 2048 > 272 and 2^19 / 32^2 = 512 <= 1056).
static inline long hdm_small_ratio_lds_doubles(int n16) { return (long) n16 * (n16 + 1); }

struct HdmSmallRatioCone {
    HdmSmallCheckCone chk;     // the cone as the check rule sees it, with its DUAL factor object's shape
    int n = 0;                 // block dimension (n == 1 keeps its closed form in cone_ratio_test)
};

// `sw`: the process's Lanczos switches (hdm_lz_switches()); the other arguments of the form rule mean nothing up to n16 = 256
static inline bool hdm_small_ratio_member(const HdmSmallRatioCone &c, const HdmLzSwitches &sw) {
    if (!hdm_small_check_eligible(c.chk)) return false;       // one device, resident rows, n16 <= 128, a one-block factor
    if (c.n < 2) return false;
    if (hdm_lz_form(c.chk.n16, sw, true, false, 0) != LZ_FORM_WHOLE_RESIDENT) return false;
    return c.chk.mloc <= hdm_small_ratio_lds_doubles(c.chk.n16);
}

// ---- the slot -------------------------------------------------------------------------------------------------------------
// What a member keeps of the last grouped launch it was in: the question (dTauStep, eye = dAdaRatio * Rd, the owned components of
// dy), the answer, and the value HdmDualState::moves() had after the launch was committed.  An answer is served
//   * exactly once (`consumed`),
//   * only to the same question, compared component by component and exactly, as HdmDualPoint::same_as compares,
//   * only while nothing has moved under it: any transition of the member's dual state since the commit changes the counter.
// A member has ONE slot; it also records the buffer the launch answered on (0: the dual buffer, else the checker buffer), and a
// launch for either buffer replaces it.  An answer is never served to a question on the other buffer.
struct HdmRatioSlot {
    bool valid = false, consumed = false;
    int buffer = 0;            // the buffer the answer is for: 0 BUFFER_DUALVAR, 1 BUFFER_DUALCHECK
    unsigned long moves = 0;   // dual-buffer answer: HdmDualState::moves() after the commit
    unsigned long checker = 0, dS_writes = 0;   // checker-buffer answer: checker_epoch() and dS_writes() after the commit
    std::vector<double> q;     // stored order of a point: tau, eye, multipliers
    double step = 0.0;
    int rc = 0;                // the retcode the member's own call returns with the step
};

static inline bool hdm_ratio_slot_serves(const HdmRatioSlot &s, const HdmDualPoint &q, unsigned long moves_now) {
    return s.valid && !s.consumed && s.buffer == 0 && s.moves == moves_now && q.same_as(s.q);
}

// ---- the checker buffer (HMiKKTSetGroupedRatioChecker) ---------------------------------------------------------------------
// Membership for a question on BUFFER_DUALCHECK, asked per launch: the dual-buffer rule, and a checker factor object of the shape
// the step rule asks for (small_step_rule.h: hdm_small_check_factor_ok(chk_npad, chk_nblk): one 128-block, whose Dinv the launch
// reads as the triangular inverse).  A member without a checker object, or with one of another shape, is not a member now and takes
// its own path; one whose checker does not hold a factorisation is left out of the launch, and its own call fails as it does per
// cone.  (cone_set.h's HdmSetSort has the same three values; this header does not need that one.)
enum HdmRatioCheckerSort { HDM_RATIO_CHECKER_NOT_NOW = 0, HDM_RATIO_CHECKER_LEFT_OUT, HDM_RATIO_CHECKER_TAKE };
struct HdmSmallRatioChecker {
    bool present = false;      // the cone has a checker factor object
    int npad = 0, nblk = 0;    // its shape (HdmChol::npad, ::nblk)
    bool factored = false;     // it holds the factorisation of the trial point
};
static inline HdmRatioCheckerSort hdm_small_ratio_checker_sort(const HdmSmallRatioCone &c, const HdmLzSwitches &sw,
                                                               const HdmSmallRatioChecker &k) {
    if (!hdm_small_ratio_member(c, sw)) return HDM_RATIO_CHECKER_NOT_NOW;       // n == 1 stays outside, as on the dual buffer
    if (!k.present || !hdm_small_check_factor_ok(k.npad, k.nblk)) return HDM_RATIO_CHECKER_NOT_NOW;
    return k.factored ? HDM_RATIO_CHECKER_TAKE : HDM_RATIO_CHECKER_LEFT_OUT;
}

// The checker slot rule.  The answer is a function of the checker factor, the question and the member's warm-start state.  It is
// served exactly once, only to the same question on the checker buffer, compared exactly, and only while checker_epoch() and
// dS_writes() stand where the commit left them: every writer of the checker buffer or the checker factor object moves the first,
// every ratio test of this cone (per cone or grouped, on either buffer) rewrites dS and so moves the second -- "no other ratio test
// on this cone since" is what keeps the warm-start state the answer's.  moves() is deliberately NOT compared: S is not read by a
// ratio test on the checker, so a transition of S alone leaves the answer what the per-cone path would compute.
struct HdmRatioCheckerEpochs { unsigned long checker = 0, dS_writes = 0; };
static inline HdmRatioCheckerEpochs hdm_ratio_checker_epochs(const HdmDualState &st) { return {st.checker_epoch(), st.dS_writes()}; }
static inline bool hdm_ratio_checker_slot_serves(const HdmRatioSlot &s, const HdmDualPoint &q, const HdmRatioCheckerEpochs &now) {
    return s.valid && !s.consumed && s.buffer != 0 && s.checker == now.checker && s.dS_writes == now.dS_writes && q.same_as(s.q);
}
