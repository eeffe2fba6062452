// engine_step_set.h -- the step set of an operator: a step-and-check asked of one small SDP cone on the checker buffer is run for
// all of them in one launch.  Implementation header of engine.hip: included exactly once, there, in this order (the pieces share
// the anonymous namespace and the engine's thread-local context `g`).
// The rules are small_step_rule.h's (membership, and when a stored answer may be served), the kernel small.hip's
// (hdm_grouped_step_check_kernel: S + dStep dS into the checker buffer and the diagonal-block sweep's own steps, one workgroup per
// table entry), the counters dual_state.h's; the struct (MiStepSet) is engine_cone.h's, next to the cones it names; members,
// lifetimes and the protocol of switch, launch and answer are cone_set.h's (DESIGN.md sections 23 and 25).  This file is the
// kind's own: its rule, its table entry and its commit.  DESIGN.md section 24.

// the cone as small_step_rule.h sees it.  `checker`: the checker object the launch would write; nullptr: not made yet -- it is
// made by HdmChol::init(n) like the dual factor object, whose shape then stands for it
HdmSmallStepCone step_set_desc(const MiCone *c, const HdmChol *checker) {
    HdmSmallStepCone d;
    const HdmChol *dual = dual_chol(c);
    d.chk = small_check_desc(c, dual);
    d.chk_npad = checker ? checker->npad : dual->npad;
    d.chk_nblk = checker ? checker->nblk : dual->nblk;
    d.diag_sweep = hdm_env_on<ENV_DIAG_SWEEP>();
    return d;
}
bool MiStepSet::eligible(const MiCone *c) const { return hdm_small_step_member(step_set_desc(c, c->checker.get())); }
void MiStepSet::empty() {
    slots.assign(members.size(), HdmStepSlot());
    made_dS.assign(members.size(), 0);
    ds_at_on.assign(members.size(), 0);
}

const char *MiStepSet::prepare(size_t k, MiCone *c) {
    HdmChol *ch = nullptr;
    if (cone_checker(c, &ch) != HDSDP_RETCODE_OK) return set_lacks("a member's checker object");
    // a step buffer the switch makes holds zeros, not a step matrix: the member has one once its dS counter has moved
    made_dS[k] = c->dS.get() ? 0 : 1;
    ds_at_on[k] = c->dual.dS_writes();
    return cone_make_dS(c) != hipSuccess ? set_lacks("a step matrix") : nullptr;
}
const char *MiStepSet::alloc_tables() {
    if (table.alloc(members.size(), hipHostMallocMapped) != hipSuccess) return set_lacks("the table");
    if (words.alloc(members.size(), hipHostMallocMapped) != hipSuccess) return set_lacks("the report words");
    return nullptr;
}

// the member in slot k has a step matrix: its buffer was there before the switch, or has been written since
bool step_set_has_dS(const MiStepSet *ss, size_t k) {
    const MiCone *c = ss->members[k];
    return c->dS.get() && (!ss->made_dS[k] || c->dual.dS_writes() != ss->ds_at_on[k]);
}
// (the rule is asked again: neither the switch nor the objects' shapes change under a set.)  A member without a step matrix is
// left out: its own call fails as it does today
HdmSetSort MiStepSet::sort(size_t k, MiCone *c, const double &) {
    if (!c->checker || !eligible(c)) return HDM_SET_NOT_NOW;
    return step_set_has_dS(this, k) ? HDM_SET_TAKE : HDM_SET_LEFT_OUT;
}
bool MiStepSet::serves(size_t k, MiCone *c, const double &dStep) { return hdm_step_slot_serves(slots[k], dStep, hdm_step_epochs(c->dual)); }
void MiStepSet::fill(int place, size_t k, MiCone *c, const double &dStep) {
    HdmChol *ch = c->checker.get();
    HdmGroupedStepArgs a = {};
    a.n = c->n; a.n16 = c->n16; a.S = c->S.get(); a.dS = c->dS.get(); a.dStep = dStep; a.Scheck = c->Scheck.get();
    a.L = ch->L.get(); a.Dinv = ch->Dinv.get(); a.info = words.dev() + k;
    words.get()[k] = -1;                                        // "nothing reported"
    // the launch writes the checker buffer and the checker's factor: what they hold is known again when it has reported
    slots[k].valid = false;
    ch->factored = false; ch->have_inv = false; ch->logdet_ok = false;
    c->dual.checker_written();
    table.get()[place] = a;
}
int MiStepSet::fire(int nl, const double &) {
    return (hdm_grouped_step_check(table.get(), table.dev(), nl, g.stream) || hipStreamSynchronize(g.stream) != hipSuccess) ? 1 : 0;
}
void MiStepSet::commit(int, size_t k, MiCone *c, const double &dStep) {
    HdmChol *ch = c->checker.get();
    int info = words.get()[k];
    if (info < 0) return;                                       // the launch has not reported for this member: its slot stays empty
    if (info > c->n) info = 0;                                  // (as HdmChol::factor: no pivot fails inside the identity padding)
    // what cone_factor_check leaves: the factor stands or not, no inverse, no log det (the barrier takes the diagonal)
    ch->factored = (info == 0); ch->have_inv = false; ch->logdet_ok = false;
    c->dual.checker_written();
    HdmStepSlot &slot = slots[k];
    slot.dStep = dStep; slot.info = info;
    slot.at = hdm_step_epochs(c->dual);
    slot.valid = true;
}

bool step_set_answer(MiCone *c, double dStep, int *isInterior, hdsdp_retcode *rc) {
    MiStepSet *ss = set_of<MiStepSet>(c->in_step);
    const int at = c->in_step.slot;
    if (at < 0 || at >= (int) ss->slots.size() || !ss->table || !ss->words) return false;
    *rc = HDSDP_RETCODE_FAILED;
    // (no step matrix yet: the call fails as the per-cone path's does)
    if (!step_set_has_dS(ss, (size_t) at) || !ss->answer((size_t) at, c, dStep)) return true;
    if (isInterior) *isInterior = (ss->slots[(size_t) at].info == 0);
    *rc = HDSDP_RETCODE_OK;
    return true;
}
