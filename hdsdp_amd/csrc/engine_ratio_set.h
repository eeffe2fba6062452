// engine_ratio_set.h -- the ratio set of an operator: a ratio test asked of one small SDP cone on the dual buffer is run for all
// of them in one pair of launches.  Implementation header of engine.hip: included exactly once, there, in this order (the pieces
// share the anonymous namespace and the engine's thread-local context `g`).
// The rules are small_ratio_rule.h's (membership, and when a stored answer may be served), the kernels lanczos.hip's
// (hdm_grouped_ratio_kernel: step matrix + the one-launch Lanczos test's body, one workgroup per table entry) and small.hip's
// (hdm_grouped_safeguard_kernel), the book-keeping dual_state.h's; the struct (MiRatioSet) is engine_cone.h's, next to the cones it
// names; members, lifetimes and the protocol of switch, launch and answer are cone_set.h's (DESIGN.md sections 23 and 25).  This
// file is the kind's own: its rule, its table entry and its commit.  DESIGN.md section 22.

// the cone as small_ratio_rule.h sees it, with its dual factor object
HdmSmallRatioCone ratio_set_desc(const MiCone *c) {
    HdmSmallRatioCone d;
    d.chk = small_check_desc(c, dual_chol(c));
    d.n = c->n;
    return d;
}
bool MiRatioSet::eligible(const MiCone *c) const { return hdm_small_ratio_member(ratio_set_desc(c), hdm_lz_switches()); }
void MiRatioSet::empty() {
    slots.assign(members.size(), HdmRatioSlot());
    yoff.assign(members.size(), 0);
    ytot = 0;
}
void ratio_set_drop_answer(MiCone *c) {
    MiRatioSet *rs = set_of<MiRatioSet>(c->in_ratio);
    const int slot = c->in_ratio.slot;
    if (rs && slot >= 0 && slot < (int) rs->slots.size()) rs->slots[(size_t) slot].valid = false;
}

const char *MiRatioSet::prepare(size_t k, MiCone *c) {
    yoff[k] = ytot;
    ytot += std::max(1, c->mloc);
    if (cone_make_dS(c) != hipSuccess) return set_lacks("a step matrix");
    if (cone_make(c->lanczos, c->n) != HDSDP_RETCODE_OK) return set_lacks("a member's Lanczos buffers");
    return nullptr;
}
const char *MiRatioSet::alloc_tables() {
    if (table.alloc(members.size(), hipHostMallocMapped) != hipSuccess) return set_lacks("the table");
    if (ybuf.alloc((size_t) ytot, hipHostMallocMapped) != hipSuccess) return set_lacks("the multipliers");
    return nullptr;
}

// (the rule is asked again: neither the switches nor the factor object's shape change under a set.)  A member whose dual factor
// does not stand is left out: its own call fails as it does today
HdmSetSort MiRatioSet::sort(size_t, MiCone *c, const MiRatioQ &) {
    if (!eligible(c) || !c->lanczos || !c->dS.get()) return HDM_SET_NOT_NOW;
    return dual_chol(c)->factored ? HDM_SET_TAKE : HDM_SET_LEFT_OUT;
}
// the member's question: dTauStep, eye = dAdaRatio * its own Rd, dy in its own own[] order in its part of `ybuf`
static HdmDualPoint ratio_set_asked(const MiRatioSet *rs, size_t k, const MiCone *c, const MiRatioQ &q) {
    return HdmDualPoint{q.dTauStep, q.dAdaRatio * c->Rd, rs->ybuf.get() + rs->yoff[k], c->mloc};
}
// dy is gathered to where the launch reads it; an answer nobody has fetched yet stands if it is this question's and nothing has
// moved under it
bool MiRatioSet::serves(size_t k, MiCone *c, const MiRatioQ &q) {
    const HdmDualPoint p = cone_point(c, q.dTauStep, q.dAdaRatio * c->Rd, q.dy, ybuf.get() + yoff[k]);
    return hdm_ratio_slot_serves(slots[k], p, c->dual.moves());
}
void MiRatioSet::fill(int place, size_t k, MiCone *c, const MiRatioQ &q) {
    const HdmDualPoint p = ratio_set_asked(this, k, c, q);
    const HdmChol *ch = dual_chol(c);
    bool any = false;                                           // one of the gathered multipliers is non-zero
    for (int i = 0; i < p.ny; ++i) any |= (p.y[i] != 0.0);
    HdmGroupedRatioArgs a = {};
    a.n = c->n; a.n16 = c->n16; a.m = any ? c->mloc : 0; a.fresh = c->lanczos->nComputed == 0 ? 1 : 0;
    a.A = c->rows.resident(); a.astride = c->astride; a.C = c->Cfull.get();
    a.y = ybuf.dev() + yoff[k]; a.tau = p.tau; a.eye = p.eye;
    a.dS = c->dS.get(); a.S = c->S.get(); a.Linv = ch->Dinv.get();
    a.V = c->lanczos->V.get(); a.warm = c->lanczos->warm.get(); a.start = c->lanczos->startd.get();
    a.out = c->lanczos->scal_h.dev() + LZ_MB_WHOLE;
    double *r = c->lanczos->scal_h.get() + LZ_MB_WHOLE;
    r[0] = 0.0; r[1] = 0.0; r[2] = -1.0; r[3] = -1.0;           // "nothing reported"
    slots[k].valid = false;
    table.get()[place] = a;
}
// two kernels, one synchronisation
int MiRatioSet::fire(int nl, const MiRatioQ &) {
    return (hdm_grouped_ratio(table.get(), table.dev(), nl, g.stream) || hdm_grouped_safeguard(table.dev(), nl, g.stream) ||
            hipStreamSynchronize(g.stream) != hipSuccess) ? 1 : 0;
}
void MiRatioSet::commit(int, size_t k, MiCone *c, const MiRatioQ &q) {
    HdmRatioSlot &slot = slots[k];
    const HdmDualPoint p = ratio_set_asked(this, k, c, q);
    const double *r = c->lanczos->scal_h.get() + LZ_MB_WHOLE;
    g_asm_counts[HDM_ASM_SWEEP_STEP].fetch_add(1, std::memory_order_relaxed);
    c->dual.dS_written();                                       // in every tracking mode (small_step_rule.h)
    if (hdm_dual_mode(c->mloc, c->n) > 0) c->dual.dS_assembled_at(p);       // (a member is on one device: it tracks points unless mode 0)
    if (r[2] < 0.0 || r[3] < 0.0) return;                       // the launch has not reported for this member: its slot stays empty
    slot.rc = HDSDP_RETCODE_OK;
    slot.step = r[0];
    if (r[2] != 0.0) slot.rc = HDSDP_RETCODE_FAILED;            // the Lanczos test failed: this member's own call says so
    else {
        c->lanczos->nComputed += 1;
        if (hdm_env_int<ENV_RATIO_DEBUG>().value_or(0) != 0)
            fprintf(stderr, "[hdsdp_mi355x ratio] n %d: %d Lanczos steps, step %.6e (grouped)\n", c->n, (int) r[1], slot.step);
        if (r[3] != 0.0) {
            // the step left the cone: the rest of the safeguard on the host, for this cone alone (its fresh-start test reads
            // the factor's Linv, which the per-cone path would have made before its own test)
            HdmChol *ch = dual_chol(c);
            fallbacks += 1;
            slot.rc = ch->invert_factor(g.stream) ? HDSDP_RETCODE_FAILED : ratio_safeguard_rest(c, ch, 0, &slot.step);
        }
    }
    p.store(slot.q);
    slot.moves = c->dual.moves();
    slot.valid = true; slot.consumed = false;
}

bool ratio_set_answer(MiCone *c, double dTauStep, const double *dy, double dAdaRatio, double *maxStep, hdsdp_retcode *rc) {
    MiRatioSet *rs = set_of<MiRatioSet>(c->in_ratio);
    const int at = c->in_ratio.slot;
    if (at < 0 || at >= (int) rs->slots.size() || !rs->table || !c->lanczos || !c->dS.get()) return false;
    HdmRatioSlot &slot = rs->slots[(size_t) at];
    *rc = HDSDP_RETCODE_FAILED;
    if (!rs->answer((size_t) at, c, MiRatioQ{dTauStep, dy, dAdaRatio})) return true;
    slot.consumed = true;
    *rc = (hdsdp_retcode) slot.rc;
    if (slot.rc == HDSDP_RETCODE_OK) *maxStep = slot.step;
    return true;
}
