// engine_ratio_set.h -- the ratio set of an operator: a ratio test asked of one small SDP cone on the dual buffer is run for all
// of them in one pair of launches.  Implementation header of engine.hip: included exactly once, there, in this order (the pieces
// share the anonymous namespace and the engine's thread-local context `g`).
// The rules are small_ratio_rule.h's (membership, and when a stored answer may be served), the kernels lanczos.hip's
// (hdm_grouped_ratio_kernel: step matrix + the one-launch Lanczos test's body, one workgroup per table entry) and small.hip's
// (hdm_grouped_safeguard_kernel), the book-keeping dual_state.h's; the struct (MiRatioSet) is engine_cone.h's, next to the cones it
// names; members, lifetimes and the protocol of switch, launch and answer are cone_set.h's (DESIGN.md sections 23 and 25).  This
// file is the kind's own: its rule, its table entry and its commit.  DESIGN.md section 22.
// Two opt-ins go through the same hooks: a question on the checker buffer differs in the rule asked (sort,
// serves), in two pointers of the table entry (fill) and in what the slot records (commit); the safeguard's rest on the device is
// two more kernels behind the same synchronisation (fire: hdm_grouped_fresh_kernel, hdm_grouped_cuts_kernel), a second table
// entry (fill) and a branch of the commit.

// the cone as small_ratio_rule.h sees it, with its dual factor object
HdmSmallRatioCone ratio_set_desc(const MiCone *c) {
    HdmSmallRatioCone d;
    d.chk = small_check_desc(c, dual_chol(c));
    d.n = c->n;
    return d;
}
// ... and its checker factor object
HdmSmallRatioChecker ratio_set_checker_desc(const MiCone *c) {
    HdmSmallRatioChecker k;
    if (const HdmChol *ch = c->checker.get()) { k.present = true; k.npad = ch->npad; k.nblk = ch->nblk; k.factored = ch->factored; }
    return k;
}
// the factor object a question on `whichBuffer` reads
HdmChol *ratio_set_factor(const MiCone *c, int whichBuffer) { return whichBuffer == 0 ? dual_chol(c) : c->checker.get(); }
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
// The opt-ins' switches.  Each acts only while the set is on, and makes everything a launch then needs: a launch allocates nothing.
int MiRatioSet::turn_checker(int on_) {
    checker_on = on_ && on;
    return checker_on ? 1 : 0;
}
int MiRatioSet::turn_rest(int on_) {
    rest_on = false;
    rest_table.reset(); rest_words.reset();
    if (!on_ || !on) return 0;
    const char *lacks = nullptr;
    for (size_t k = 0; k < members.size() && !lacks; ++k)
        if (MiCone *c = members[k]; c && cone_make(c->lanczos_fresh, c->n) != HDSDP_RETCODE_OK) lacks = set_lacks("a member's fresh-start Lanczos buffers");
    if (!lacks && rest_table.alloc(members.size(), hipHostMallocMapped) != hipSuccess) lacks = set_lacks("the rest's table");
    if (!lacks && rest_words.alloc((size_t) HDM_GROUPED_REST_WORDS * members.size(), hipHostMallocMapped) != hipSuccess) lacks = set_lacks("the rest's report words");
    if (lacks) {
        rest_table.reset(); rest_words.reset();
        fprintf(stderr, "[hdsdp_mi355x] grouped ratio test: no memory for %s; the safeguard's rest stays on the host\n", lacks);
        return 0;
    }
    rest_on = true;
    return 1;
}

// (the rule is asked again: neither the switches nor the factor object's shape change under a set.)  A member whose factor -- the
// dual factor, or for a checker question the checker's -- does not stand is left out: its own call fails as it does today.  A
// checker question is asked of small_ratio_rule.h's checker rule, per launch: a member without a checker object of the right
// shape is not a member now
HdmSetSort MiRatioSet::sort(size_t, MiCone *c, const MiRatioQ &q) {
    if (!c->lanczos || !c->dS.get() || (rest_on && !c->lanczos_fresh)) return HDM_SET_NOT_NOW;
    if (q.whichBuffer == 0) {
        if (!eligible(c)) return HDM_SET_NOT_NOW;
        return dual_chol(c)->factored ? HDM_SET_TAKE : HDM_SET_LEFT_OUT;
    }
    switch (hdm_small_ratio_checker_sort(ratio_set_desc(c), hdm_lz_switches(), ratio_set_checker_desc(c))) {
    case HDM_RATIO_CHECKER_TAKE: return HDM_SET_TAKE;
    case HDM_RATIO_CHECKER_LEFT_OUT: return HDM_SET_LEFT_OUT;
    default: return HDM_SET_NOT_NOW;
    }
}
// the member's question: dTauStep, eye = dAdaRatio * its own Rd, dy in its own own[] order in its part of `ybuf`
static HdmDualPoint ratio_set_asked(const MiRatioSet *rs, size_t k, const MiCone *c, const MiRatioQ &q) {
    return HdmDualPoint{q.dTauStep, q.dAdaRatio * c->Rd, rs->ybuf.get() + rs->yoff[k], c->mloc};
}
// dy is gathered to where the launch reads it; an answer nobody has fetched yet stands if it is this question's, on this buffer,
// and nothing has moved under it (what "nothing" is differs by buffer: small_ratio_rule.h)
bool MiRatioSet::serves(size_t k, MiCone *c, const MiRatioQ &q) {
    const HdmDualPoint p = cone_point(c, q.dTauStep, q.dAdaRatio * c->Rd, q.dy, ybuf.get() + yoff[k]);
    return q.whichBuffer == 0 ? hdm_ratio_slot_serves(slots[k], p, c->dual.moves())
                              : hdm_ratio_checker_slot_serves(slots[k], p, hdm_ratio_checker_epochs(c->dual));
}
void MiRatioSet::fill(int place, size_t k, MiCone *c, const MiRatioQ &q) {
    const HdmDualPoint p = ratio_set_asked(this, k, c, q);
    // (the per-cone path builds the factor's Linv with invert_factor and sets have_inv; this reads Dinv, the same bits for a
    // one-block factor, and leaves the flags alone)
    const HdmChol *ch = ratio_set_factor(c, q.whichBuffer);
    bool any = false;                                           // one of the gathered multipliers is non-zero
    for (int i = 0; i < p.ny; ++i) any |= (p.y[i] != 0.0);
    HdmGroupedRatioArgs a = {};
    a.n = c->n; a.n16 = c->n16; a.m = any ? c->mloc : 0; a.fresh = c->lanczos->nComputed == 0 ? 1 : 0;
    a.A = c->rows.resident(); a.astride = c->astride; a.C = c->Cfull.get();
    a.y = ybuf.dev() + yoff[k]; a.tau = p.tau; a.eye = p.eye;
    a.dS = c->dS.get(); a.S = q.whichBuffer == 0 ? c->S.get() : c->Scheck.get(); a.Linv = ch->Dinv.get();
    a.V = c->lanczos->V.get(); a.warm = c->lanczos->warm.get(); a.start = c->lanczos->startd.get();
    a.out = c->lanczos->scal_h.dev() + LZ_MB_WHOLE;
    double *r = c->lanczos->scal_h.get() + LZ_MB_WHOLE;
    r[0] = 0.0; r[1] = 0.0; r[2] = -1.0; r[3] = -1.0;           // "nothing reported"
    slots[k].valid = false;
    table.get()[place] = a;
    if (!rest_on) return;
    HdmLanczos *lf = c->lanczos_fresh.get();
    HdmGroupedRestArgs b = {};
    b.V = lf->V.get(); b.warm = lf->warm.get(); b.start = lf->startd.get();
    b.fresh_out = lf->scal_h.dev() + LZ_MB_WHOLE;
    b.rest = rest_words.dev() + HDM_GROUPED_REST_WORDS * k;
    double *f = lf->scal_h.get() + LZ_MB_WHOLE, *w = rest_words.get() + HDM_GROUPED_REST_WORDS * k;
    f[0] = 0.0; f[1] = 0.0; f[2] = -1.0;
    w[0] = 0.0; w[1] = -1.0; w[2] = 0.0; w[3] = 0.0;            // "nothing reported"
    rest_table.get()[place] = b;
}
// two kernels -- four with the rest on the device --, one synchronisation
int MiRatioSet::fire(int nl, const MiRatioQ &q) {
    if (hdm_grouped_ratio(table.get(), table.dev(), nl, g.stream) || hdm_grouped_safeguard(table.dev(), nl, g.stream)) return 1;
    if (rest_on && (hdm_grouped_fresh(table.get(), table.dev(), rest_table.get(), rest_table.dev(), nl, g.stream) ||
                    hdm_grouped_cuts(table.dev(), rest_table.dev(), nl, g.stream))) return 1;
    if (hipStreamSynchronize(g.stream) != hipSuccess) return 1;
    if (q.whichBuffer != 0) checker_launches += 1;
    return 0;
}
void MiRatioSet::commit(int, size_t k, MiCone *c, const MiRatioQ &q) {
    HdmRatioSlot &slot = slots[k];
    const HdmDualPoint p = ratio_set_asked(this, k, c, q);
    const double *r = c->lanczos->scal_h.get() + LZ_MB_WHOLE;
    const bool dbg = hdm_env_int<ENV_RATIO_DEBUG>().value_or(0) != 0;
    g_asm_counts[HDM_ASM_SWEEP_STEP].fetch_add(1, std::memory_order_relaxed);
    c->dual.dS_written();                                       // in every tracking mode (small_step_rule.h)
    if (hdm_dual_mode(c->mloc, c->n) > 0) c->dual.dS_assembled_at(p);       // (a member is on one device: it tracks points unless mode 0)
    if (r[2] < 0.0 || r[3] < 0.0) return;                       // the launch has not reported for this member: its slot stays empty
    slot.rc = HDSDP_RETCODE_OK;
    slot.step = r[0];
    if (r[2] != 0.0) slot.rc = HDSDP_RETCODE_FAILED;            // the Lanczos test failed: this member's own call says so
    else {
        c->lanczos->nComputed += 1;
        if (dbg) fprintf(stderr, "[hdsdp_mi355x ratio] n %d: %d Lanczos steps, step %.6e (grouped)\n", c->n, (int) r[1], slot.step);
        if (r[3] != 0.0 && rest_on) {
            // the step left the cone, and the launch has run the rest of the safeguard for this member: the fresh-start test on
            // its lanczos_fresh object (left as the host's call leaves it) and the cuts
            const double *w = rest_words.get() + HDM_GROUPED_REST_WORDS * k;
            if (w[1] < 0.0) return;                             // ... or has not reported: the slot stays empty
            device_rests += 1;
            device_cuts += (long) w[2];
            c->lanczos_fresh->nComputed = std::isfinite(w[3]) ? 1 : 0;
            if (dbg) fprintf(stderr, "[hdsdp_mi355x ratio] n %d: step %.6e left the cone, safeguarded to %.6e (fresh start %.6e)\n", c->n,
                             slot.step, w[0], w[3]);
            slot.step = (w[1] != 0.0) ? w[0] : 0.0;
        } else if (r[3] != 0.0) {
            // the step left the cone: the rest of the safeguard on the host, for this cone alone (its fresh-start test reads
            // the factor's Linv, which the per-cone path would have made before its own test)
            HdmChol *ch = ratio_set_factor(c, q.whichBuffer);
            fallbacks += 1;
            slot.rc = ch->invert_factor(g.stream) ? HDSDP_RETCODE_FAILED : ratio_safeguard_rest(c, ch, q.whichBuffer, &slot.step);
        }
    }
    // what the answer is held to, after the transitions above (small_ratio_rule.h: which of them count differs by buffer)
    p.store(slot.q);
    slot.buffer = q.whichBuffer == 0 ? 0 : 1;
    slot.moves = c->dual.moves();
    const HdmRatioCheckerEpochs at = hdm_ratio_checker_epochs(c->dual);
    slot.checker = at.checker; slot.dS_writes = at.dS_writes;
    slot.valid = true; slot.consumed = false;
}

bool ratio_set_answer(MiCone *c, double dTauStep, const double *dy, double dAdaRatio, int whichBuffer, double *maxStep, hdsdp_retcode *rc) {
    MiRatioSet *rs = set_of<MiRatioSet>(c->in_ratio);
    const int at = c->in_ratio.slot;
    if (at < 0 || at >= (int) rs->slots.size() || !rs->table || !c->lanczos || !c->dS.get()) return false;
    const MiRatioQ q = {dTauStep, dy, dAdaRatio, whichBuffer};
    // (a checker question of a member whose checker object is of another shape: its own path)
    if (whichBuffer != 0 && rs->sort((size_t) at, c, q) == HDM_SET_NOT_NOW) return false;
    HdmRatioSlot &slot = rs->slots[(size_t) at];
    *rc = HDSDP_RETCODE_FAILED;
    if (!rs->answer((size_t) at, c, q)) {
        // (the one unanswered member that does not fail: its test ran, its step left the cone, and the rest's launches have not
        // reported for it -- it takes its own path)
        const double *r = c->lanczos->scal_h.get() + LZ_MB_WHOLE;
        return !(rs->rest_on && r[2] == 0.0 && r[3] > 0.0 && rs->rest_words.get()[HDM_GROUPED_REST_WORDS * (size_t) at + 1] < 0.0);
    }
    slot.consumed = true;
    *rc = (hdsdp_retcode) slot.rc;
    if (slot.rc == HDSDP_RETCODE_OK) *maxStep = slot.step;
    return true;
}
