// engine_check_set.h -- the check set of an operator: a point question put to one small SDP cone is answered for all of them
// in one launch.  Implementation header of engine.hip: included exactly once, there, in this order (the pieces share the
// anonymous namespace and the engine's thread-local context `g`).
// The rule is small_check_rule.h's, the kernel small.hip's (hdm_grouped_check_kernel: the one-launch check's body, one
// workgroup per table entry), the book-keeping dual_state.h's; the struct (MiCheckSet) is engine_cone.h's, next to the cones it
// names; who is a member for how long is cone_set.h's.  This file says which cones of an operator are
// eligible, keeps the table, and makes the launch.  DESIGN.md section 19.

// a member: an SDP cone of this engine (not a device-group cone, not an LP cone, not a host cone) whose own one-launch check on
// the dual buffer would run -- a sharded cone fails the rule by world != 1
MiCone *check_set_eligible(const hdsdp_cone *hc) {
    MiCone *c = own_cone_with_factor(hc);
    return (c && hdm_small_check_eligible(small_check_desc(c, dual_chol(c)))) ? c : nullptr;
}

// HKKTInit: membership only, by cone_set.h's rules (the operator initialised last has a cone no ACTIVE set holds)
void check_set_init(hdsdp_kkt *HKKT, MiKKTPriv *pv) {
    MiCheckSet &cs = pv->chk;
    cs.release();
    cs.reset_counters(); cs.from_state = 0;
    for (int i = 0; i < HKKT->nCones; ++i)
        if (MiCone *c = check_set_eligible(HKKT->cones[i])) cs.adopt(c);
}

// the switch: returns the number of members (0: off, or fewer than two members)
int check_set_switch(MiKKTPriv *pv, int on) {
    MiCheckSet &cs = pv->chk;
    cs.on = false;
    cs.table.reset();
    cs.from_state = 0;
    const int k = cs.count();
    if (!on || k < 2) return 0;
    if (cs.table.alloc(cs.members.size(), hipHostMallocMapped) != hipSuccess) {
        (void) hipGetLastError();
        fprintf(stderr, "[hdsdp_mi355x] grouped interior check: no pinned memory for the table; the per-cone checks stay\n");
        return 0;
    }
    cs.on = true;
    return k;
}

// One launch for every member that does not stand at (tau, y_host) with its own identity coefficient.
int check_set_launch(MiCheckSet *cs, double tau, const double *y_host) {
    HdmSmallCheckArgs *tab = cs->table.get();
    cs->launch_begin();
    int left_out = 0, max_m = 0;
    std::vector<HdmDualPoint> pts;
    for (size_t k = 0; k < cs->members.size(); ++k) {
        MiCone *c = cs->members[k];
        if (!c) continue;
        // (the rule is asked again: whether the check is switched on and the factor object's shape do not change under a
        // set, so this holds for every member -- a cone for which it did not would be left to its own path)
        HdmChol *ch = dual_chol(c);
        if (!hdm_small_check_eligible(small_check_desc(c, ch)) || small_check_block(c)) continue;
        const HdmDualPoint p = small_check_point(c, tau, y_host, cone_eye(c));
        if (c->dual.S_factored_at(p, nullptr)) { left_out += 1; continue; }
        tab[cs->launch_take(k)] = small_check_args(c, ch, p, 0);
        c->dual.S_overwritten();          // the launch writes S: what it holds is known again when the launch has reported
        max_m = std::max(max_m, c->mloc);
        pts.push_back(p);
    }
    cs->last_left_out = left_out;
    const int nl = (int) cs->launched.size();
    if (nl == 0) return 0;
    if (hdm_grouped_check(tab, cs->table.dev(), nl, max_m, g.stream) || hipStreamSynchronize(g.stream) != hipSuccess) return 1;
    cs->launch_made();
    for (int s = 0; s < nl; ++s) {
        MiCone *c = cs->members[(size_t) cs->launched[(size_t) s]];
        (void) small_check_commit(c, dual_chol(c), pts[(size_t) s], 0);
    }
    return 0;
}

// HMiKKTCheckIsInterior: every cone of cones[] in order, no early exit, through its own slots -- the members of an active set
// reach the grouped launch through the first of them that is asked
hdsdp_retcode check_all_cones(hdsdp_kkt *HKKT, double tau, const double *y, int *flags, double *logdets, int *all) {
    hdsdp_retcode first = HDSDP_RETCODE_OK;
    int every = 1;
    for (int i = 0; i < HKKT->nCones; ++i) {
        hdsdp_cone *hc = HKKT->cones[i];
        int in = 0;
        double ld = NAN;
        hdsdp_retcode rc = hc->coneInteriorCheck(hc->coneData, tau, (double *) y, &in);
        if (rc == HDSDP_RETCODE_OK && in) {
            rc = hc->coneGetBarrier(hc->coneData, tau, (double *) y, 0, &ld);
            if (rc != HDSDP_RETCODE_OK) ld = NAN;
        } else in = 0;
        if (rc != HDSDP_RETCODE_OK && first == HDSDP_RETCODE_OK) first = rc;
        if (flags) flags[i] = in;
        if (logdets) logdets[i] = in ? ld : NAN;
        every &= in;
    }
    if (all) *all = every;
    return first;
}
