// small_ratio_rule.h -- which cones the grouped ratio test (lanczos.hip: hdm_grouped_ratio_kernel, small.hip:
// hdm_grouped_safeguard_kernel, engine_ratio_set.h) answers, and when a stored answer may be served: two rules, stated once.
// Pure host arithmetic: no HIP call, no engine state.  The ratio set of an operator asks the first per cone at HKKTInit, the hook
// in cone_ratio_test asks the second per call.  tests/test_small_ratio_rule_cpu.py compiles this header alone.  DESIGN.md section 22.
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
struct HdmRatioSlot {
    bool valid = false, consumed = false;
    unsigned long moves = 0;
    std::vector<double> q;     // stored order of a point: tau, eye, multipliers
    double step = 0.0;
    int rc = 0;                // the retcode the member's own call returns with the step
};

static inline bool hdm_ratio_slot_serves(const HdmRatioSlot &s, const HdmDualPoint &q, unsigned long moves_now) {
    return s.valid && !s.consumed && s.moves == moves_now && q.same_as(s.q);
}
