// engine_ratio_set.h -- the ratio set of an operator: a ratio test asked of one small SDP cone on the dual buffer is run for all
// of them in one pair of launches.  Implementation header of engine.hip: included exactly once, there, in this order (the pieces
// share the anonymous namespace and the engine's thread-local context `g`).
// The rules are small_ratio_rule.h's (membership, and when a stored answer may be served), the kernels lanczos.hip's
// (hdm_grouped_ratio_kernel: step matrix + the one-launch Lanczos test's body, one workgroup per table entry) and small.hip's
// (hdm_grouped_safeguard_kernel), the book-keeping dual_state.h's; the struct (MiRatioSet) is engine_cone.h's, next to the cones it
// names; who is a member for how long is cone_set.h's.  This file says which cones of an operator are
// eligible, keeps the table and the slots, and makes the launch.  DESIGN.md section 22.

// the cone as small_ratio_rule.h sees it, with its dual factor object
HdmSmallRatioCone ratio_set_desc(const MiCone *c) {
    HdmSmallRatioCone d;
    d.chk = small_check_desc(c, dual_chol(c));
    d.n = c->n;
    return d;
}
// a member: an SDP cone of this engine (not a device-group cone, not an LP cone, not a host cone) the rule admits
MiCone *ratio_set_eligible(const hdsdp_cone *hc) {
    MiCone *c = own_cone_with_factor(hc);
    return (c && hdm_small_ratio_member(ratio_set_desc(c), hdm_lz_switches())) ? c : nullptr;
}

// HKKTInit: membership only, by cone_set.h's rules (the operator initialised last has a cone no ACTIVE set holds)
void ratio_set_init(hdsdp_kkt *HKKT, MiKKTPriv *pv) {
    MiRatioSet &rs = pv->rat;
    rs.release();
    rs.reset_counters(); rs.from_slots = rs.fallbacks = 0;
    for (int i = 0; i < HKKT->nCones; ++i)
        if (MiCone *c = ratio_set_eligible(HKKT->cones[i])) rs.adopt(c);
    rs.slots.assign(rs.members.size(), HdmRatioSlot());
}

void ratio_set_drop_answer(MiCone *c) {
    MiRatioSet *rs = ratio_set_of(c);
    const int slot = c->in_ratio.slot;
    if (rs && slot >= 0 && slot < (int) rs->slots.size()) rs->slots[(size_t) slot].valid = false;
}

// the switch: returns the number of members (0: off, or fewer than two members).  Turning it on makes everything a launch needs.
int ratio_set_switch(MiKKTPriv *pv, int on) {
    MiRatioSet &rs = pv->rat;
    rs.on = false;
    rs.table.reset(); rs.ybuf.reset();
    rs.from_slots = 0;
    for (HdmRatioSlot &s : rs.slots) s = HdmRatioSlot();
    const int k = rs.count();
    if (!on || k < 2) return 0;
    auto stays = [&](const char *what) {
        (void) hipGetLastError();
        rs.table.reset(); rs.ybuf.reset();
        fprintf(stderr, "[hdsdp_mi355x] grouped ratio test: no memory for %s; the per-cone tests stay\n", what);
        return 0;
    };
    long ytot = 0;
    rs.yoff.assign(rs.members.size(), 0);
    for (size_t q = 0; q < rs.members.size(); ++q) {
        MiCone *c = rs.members[q];
        if (!c) continue;
        rs.yoff[q] = ytot;
        ytot += std::max(1, c->mloc);
        if (cone_make_dS(c) != hipSuccess) return stays("a step matrix");
        if (cone_make(c->lanczos, c->n) != HDSDP_RETCODE_OK) return stays("a member's Lanczos buffers");
    }
    if (rs.table.alloc(rs.members.size(), hipHostMallocMapped) != hipSuccess) return stays("the table");
    if (rs.ybuf.alloc((size_t) ytot, hipHostMallocMapped) != hipSuccess) return stays("the multipliers");
    rs.on = true;
    return k;
}

// the member's question: dTauStep, eye = dAdaRatio * its own Rd, dy gathered through its own own[] into `yo`; *any: one of them is non-zero
HdmDualPoint ratio_set_question(const MiCone *c, double dTauStep, const double *dy, double dAdaRatio, double *yo, bool *any) {
    return cone_point(c, dTauStep, dAdaRatio * c->Rd, dy, yo, any);
}

// One pair of launches and one synchronisation for every member whose dual factor stands and whose slot does not already hold an
// unconsumed answer to this question.  Returns nonzero when the launches could not be made or did not finish.
int ratio_set_launch(MiRatioSet *rs, double dTauStep, const double *dy, double dAdaRatio) {
    HdmGroupedRatioArgs *tab = rs->table.get();
    rs->launch_begin();
    int left_out = 0;
    std::vector<HdmDualPoint> pts;
    for (size_t k = 0; k < rs->members.size(); ++k) {
        MiCone *c = rs->members[k];
        if (!c) continue;
        HdmChol *ch = dual_chol(c);
        // (the rule is asked again: neither the switches nor the factor object's shape change under a set)
        if (!hdm_small_ratio_member(ratio_set_desc(c), hdm_lz_switches()) || !c->lanczos || !c->dS.get()) continue;
        if (!ch->factored) { left_out += 1; continue; }         // its own call fails as it does today
        double *yo = rs->ybuf.get() + rs->yoff[k];
        HdmRatioSlot &slot = rs->slots[k];
        bool any = false;
        const HdmDualPoint p = ratio_set_question(c, dTauStep, dy, dAdaRatio, yo, &any);
        // an answer nobody has fetched yet stands if it is this question's and nothing has moved under it
        if (hdm_ratio_slot_serves(slot, p, c->dual.moves())) { left_out += 1; continue; }
        HdmGroupedRatioArgs a = {};
        a.n = c->n; a.n16 = c->n16; a.m = any ? c->mloc : 0; a.fresh = c->lanczos->nComputed == 0 ? 1 : 0;
        a.A = c->rows.resident(); a.astride = c->astride; a.C = c->Cfull.get();
        a.y = rs->ybuf.dev() + rs->yoff[k]; a.tau = p.tau; a.eye = p.eye;
        a.dS = c->dS.get(); a.S = c->S.get(); a.Linv = ch->Dinv.get();
        a.V = c->lanczos->V.get(); a.warm = c->lanczos->warm.get(); a.start = c->lanczos->startd.get();
        a.out = c->lanczos->scal_h.dev() + LZ_MB_WHOLE;
        double *r = c->lanczos->scal_h.get() + LZ_MB_WHOLE;
        r[0] = 0.0; r[1] = 0.0; r[2] = -1.0; r[3] = -1.0;       // "nothing reported"
        slot.valid = false;
        tab[rs->launch_take(k)] = a;
        pts.push_back(p);
    }
    rs->last_left_out = left_out;
    const int nl = (int) rs->launched.size();
    if (nl == 0) return 0;
    if (hdm_grouped_ratio(tab, rs->table.dev(), nl, g.stream) || hdm_grouped_safeguard(rs->table.dev(), nl, g.stream) ||
        hipStreamSynchronize(g.stream) != hipSuccess) return 1;
    rs->launch_made();
    const bool dbg = hdm_env_int<ENV_RATIO_DEBUG>().value_or(0) != 0;
    for (int s = 0; s < nl; ++s) {
        const size_t k = (size_t) rs->launched[(size_t) s];
        MiCone *c = rs->members[k];
        HdmRatioSlot &slot = rs->slots[k];
        const HdmDualPoint &p = pts[(size_t) s];
        const double *r = c->lanczos->scal_h.get() + LZ_MB_WHOLE;
        g_asm_counts[HDM_ASM_SWEEP_STEP].fetch_add(1, std::memory_order_relaxed);
        c->dual.dS_written();                                   // in every tracking mode (small_step_rule.h)
        if (hdm_dual_mode(c->mloc, c->n) > 0) c->dual.dS_assembled_at(p);       // (a member is on one device: it tracks points unless mode 0)
        if (r[2] < 0.0 || r[3] < 0.0) continue;                 // the launch has not reported for this member: its slot stays empty
        slot.rc = HDSDP_RETCODE_OK;
        slot.step = r[0];
        if (r[2] != 0.0) slot.rc = HDSDP_RETCODE_FAILED;        // the Lanczos test failed: this member's own call says so
        else {
            c->lanczos->nComputed += 1;
            if (dbg) fprintf(stderr, "[hdsdp_mi355x ratio] n %d: %d Lanczos steps, step %.6e (grouped)\n", c->n, (int) r[1], slot.step);
            if (r[3] != 0.0) {
                // the step left the cone: the rest of the safeguard on the host, for this cone alone (its fresh-start test reads
                // the factor's Linv, which the per-cone path would have made before its own test)
                HdmChol *ch = dual_chol(c);
                rs->fallbacks += 1;
                slot.rc = ch->invert_factor(g.stream) ? HDSDP_RETCODE_FAILED : ratio_safeguard_rest(c, ch, 0, &slot.step);
            }
        }
        p.store(slot.q);
        slot.moves = c->dual.moves();
        slot.valid = true; slot.consumed = false;
    }
    return 0;
}

bool ratio_set_answer(MiCone *c, double dTauStep, const double *dy, double dAdaRatio, double *maxStep, hdsdp_retcode *rc) {
    MiRatioSet *rs = ratio_set_of(c);
    const int at = c->in_ratio.slot;
    if (at < 0 || at >= (int) rs->slots.size() || !rs->table || !c->lanczos || !c->dS.get()) return false;
    HdmRatioSlot &slot = rs->slots[(size_t) at];
    std::vector<double> yq((size_t) std::max(1, c->mloc));
    const HdmDualPoint q = ratio_set_question(c, dTauStep, dy, dAdaRatio, yq.data(), nullptr);
    const bool held = hdm_ratio_slot_serves(slot, q, c->dual.moves());
    if (held) rs->from_slots += 1;
    else if (ratio_set_launch(rs, dTauStep, dy, dAdaRatio) || !hdm_ratio_slot_serves(slot, q, c->dual.moves())) {
        *rc = HDSDP_RETCODE_FAILED;
        return true;
    }
    slot.consumed = true;
    *rc = (hdsdp_retcode) slot.rc;
    if (slot.rc == HDSDP_RETCODE_OK) *maxStep = slot.step;
    return true;
}

// HMiKKTRatioTest: every cone of cones[] in order, no early exit, through its own coneRatioTest slot -- the members of an active
// set reach the grouped launch through the first of them that is asked
hdsdp_retcode ratio_all_cones(hdsdp_kkt *HKKT, double dTauStep, const double *dy, double dAdaRatio, int whichBuffer, double *steps, double *minStep) {
    hdsdp_retcode first = HDSDP_RETCODE_OK;
    double mn = INFINITY;
    for (int i = 0; i < HKKT->nCones; ++i) {
        hdsdp_cone *hc = HKKT->cones[i];
        double step = NAN;
        const hdsdp_retcode rc = hc->coneRatioTest(hc->coneData, dTauStep, (double *) dy, dAdaRatio, whichBuffer, &step);
        if (rc != HDSDP_RETCODE_OK) { step = NAN; if (first == HDSDP_RETCODE_OK) first = rc; }
        else if (step < mn) mn = step;
        if (steps) steps[i] = step;
    }
    if (minStep) *minStep = mn;
    return first;
}
