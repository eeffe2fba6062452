// engine_step_set.h -- the step set of an operator: a step-and-check asked of one small SDP cone on the checker buffer is run for
// all of them in one launch.  Implementation header of engine.hip: included exactly once, there, in this order (the pieces share
// the anonymous namespace and the engine's thread-local context `g`).
// The rules are small_step_rule.h's (membership, and when a stored answer may be served), the kernel small.hip's
// (hdm_grouped_step_check_kernel: S + dStep dS into the checker buffer and the diagonal-block sweep's own steps, one workgroup per
// table entry), the counters dual_state.h's; the struct (MiStepSet) is engine_cone.h's, next to the cones it names; who is a
// member for how long is cone_set.h's.  This file says which cones of an operator are eligible, keeps the
// table and the slots, and makes the launch.  DESIGN.md section 24.

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
// a member: an SDP cone of this engine (not a device-group cone, not an LP cone, not a host cone) the rule admits
MiCone *step_set_eligible(const hdsdp_cone *hc) {
    MiCone *c = own_cone_with_factor(hc);
    return (c && hdm_small_step_member(step_set_desc(c, c->checker.get()))) ? c : nullptr;
}

// HKKTInit: membership only, by cone_set.h's rules (the operator initialised last has a cone no ACTIVE set holds)
void step_set_init(hdsdp_kkt *HKKT, MiKKTPriv *pv) {
    MiStepSet &ss = pv->stp;
    ss.release();
    ss.reset_counters(); ss.from_slots = 0;
    for (int i = 0; i < HKKT->nCones; ++i)
        if (MiCone *c = step_set_eligible(HKKT->cones[i])) ss.adopt(c);
    ss.slots.assign(ss.members.size(), HdmStepSlot());
}

// the switch: returns the number of members (0: off, or fewer than two members).  Turning it on makes everything a launch needs.
int step_set_switch(MiKKTPriv *pv, int on) {
    MiStepSet &ss = pv->stp;
    ss.on = false;
    ss.table.reset(); ss.words.reset();
    ss.from_slots = 0;
    for (HdmStepSlot &s : ss.slots) s = HdmStepSlot();
    const int k = ss.count();
    if (!on || k < 2) return 0;
    auto stays = [&](const char *what) {
        (void) hipGetLastError();
        ss.table.reset(); ss.words.reset();
        fprintf(stderr, "[hdsdp_mi355x] grouped step-and-check: no memory for %s; the per-cone checks stay\n", what);
        return 0;
    };
    ss.made_dS.assign(ss.members.size(), 0);
    ss.ds_at_on.assign(ss.members.size(), 0);
    for (size_t q = 0; q < ss.members.size(); ++q) {
        MiCone *c = ss.members[q];
        if (!c) continue;
        HdmChol *ch = nullptr;
        if (cone_checker(c, &ch) != HDSDP_RETCODE_OK) return stays("a member's checker object");
        // a step buffer the switch makes holds zeros, not a step matrix: the member has one once its dS counter has moved
        ss.made_dS[q] = c->dS.get() ? 0 : 1;
        ss.ds_at_on[q] = c->dual.dS_writes();
        if (cone_make_dS(c) != hipSuccess) return stays("a step matrix");
    }
    if (ss.table.alloc(ss.members.size(), hipHostMallocMapped) != hipSuccess) return stays("the table");
    if (ss.words.alloc(ss.members.size(), hipHostMallocMapped) != hipSuccess) return stays("the report words");
    ss.on = true;
    return k;
}

// the member at place k has a step matrix: its buffer was there before the switch, or has been written since
bool step_set_has_dS(const MiStepSet *ss, size_t k) {
    const MiCone *c = ss->members[k];
    return c->dS.get() && (!ss->made_dS[k] || c->dual.dS_writes() != ss->ds_at_on[k]);
}

// One launch and one synchronisation for every member that has a step matrix and whose slot does not already serve dStep.  Returns
// nonzero when the launch could not be made or did not finish.
int step_set_launch(MiStepSet *ss, double dStep) {
    HdmGroupedStepArgs *tab = ss->table.get();
    int *rep = ss->words.get();
    ss->launch_begin();
    int left_out = 0;
    for (size_t k = 0; k < ss->members.size(); ++k) {
        MiCone *c = ss->members[k];
        if (!c) continue;
        HdmChol *ch = c->checker.get();
        // (the rule is asked again: neither the switch nor the objects' shapes change under a set)
        if (!ch || !hdm_small_step_member(step_set_desc(c, ch))) continue;
        if (!step_set_has_dS(ss, k)) { left_out += 1; continue; }       // its own call fails as it does today
        HdmStepSlot &slot = ss->slots[k];
        if (hdm_step_slot_serves(slot, dStep, hdm_step_epochs(c->dual))) { left_out += 1; continue; }
        HdmGroupedStepArgs a = {};
        a.n = c->n; a.n16 = c->n16; a.S = c->S.get(); a.dS = c->dS.get(); a.dStep = dStep; a.Scheck = c->Scheck.get();
        a.L = ch->L.get(); a.Dinv = ch->Dinv.get(); a.info = ss->words.dev() + k;
        rep[k] = -1;                                            // "nothing reported"
        // the launch writes the checker buffer and the checker's factor: what they hold is known again when it has reported
        slot.valid = false;
        ch->factored = false; ch->have_inv = false; ch->logdet_ok = false;
        c->dual.checker_written();
        tab[ss->launch_take(k)] = a;
    }
    ss->last_left_out = left_out;
    const int nl = (int) ss->launched.size();
    if (nl == 0) return 0;
    if (hdm_grouped_step_check(tab, ss->table.dev(), nl, g.stream) || hipStreamSynchronize(g.stream) != hipSuccess) return 1;
    ss->launch_made();
    for (int s = 0; s < nl; ++s) {
        const size_t k = (size_t) ss->launched[(size_t) s];
        MiCone *c = ss->members[k];
        HdmChol *ch = c->checker.get();
        int info = rep[k];
        if (info < 0) continue;                                 // the launch has not reported for this member: its slot stays empty
        if (info > c->n) info = 0;                              // (as HdmChol::factor: no pivot fails inside the identity padding)
        // what cone_factor_check leaves: the factor stands or not, no inverse, no log det (the barrier takes the diagonal)
        ch->factored = (info == 0); ch->have_inv = false; ch->logdet_ok = false;
        c->dual.checker_written();
        HdmStepSlot &slot = ss->slots[k];
        slot.dStep = dStep; slot.info = info;
        slot.at = hdm_step_epochs(c->dual);
        slot.valid = true;
    }
    return 0;
}

bool step_set_answer(MiCone *c, double dStep, int *isInterior, hdsdp_retcode *rc) {
    MiStepSet *ss = step_set_of(c);
    const int at = c->in_step.slot;
    if (at < 0 || at >= (int) ss->slots.size() || !ss->table || !ss->words) return false;
    *rc = HDSDP_RETCODE_FAILED;
    if (!step_set_has_dS(ss, (size_t) at)) return true;         // no step matrix yet: the call fails as the per-cone path's does
    HdmStepSlot &slot = ss->slots[(size_t) at];
    if (hdm_step_slot_serves(slot, dStep, hdm_step_epochs(c->dual))) ss->from_slots += 1;
    else if (step_set_launch(ss, dStep) || !hdm_step_slot_serves(slot, dStep, hdm_step_epochs(c->dual))) return true;
    if (isInterior) *isInterior = (slot.info == 0);
    *rc = HDSDP_RETCODE_OK;
    return true;
}

// HMiKKTAddStepToBufferAndCheck: every cone of cones[] in order, no early exit, through its own coneAxpyBufferAndCheck slot -- the
// members of an active set reach the grouped launch through the first of them that is asked
hdsdp_retcode step_all_cones(hdsdp_kkt *HKKT, double dStep, int whichBuffer, int *flags, int *all) {
    hdsdp_retcode first = HDSDP_RETCODE_OK;
    int every = 1;
    for (int i = 0; i < HKKT->nCones; ++i) {
        hdsdp_cone *hc = HKKT->cones[i];
        int in = 0;
        const hdsdp_retcode rc = hc->coneAxpyBufferAndCheck(hc->coneData, dStep, whichBuffer, &in);
        if (rc != HDSDP_RETCODE_OK) { in = 0; if (first == HDSDP_RETCODE_OK) first = rc; }
        if (flags) flags[i] = in;
        every &= in ? 1 : 0;
    }
    if (all) *all = every;
    return first;
}
