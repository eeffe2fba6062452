// engine_check_set.h -- the check set of an operator: a point question put to one small SDP cone is answered for all of them
// in one launch.  Implementation header of engine.hip: included exactly once, there, in this order (the pieces share the
// anonymous namespace and the engine's thread-local context `g`).
// The rule is small_check_rule.h's, the kernel small.hip's (hdm_grouped_check_kernel: the one-launch check's body, one
// workgroup per table entry), the book-keeping dual_state.h's; the struct (MiCheckSet) is engine_cone.h's, next to the cones it
// names; members, lifetimes and the protocol of switch, launch and answer are cone_set.h's (DESIGN.md sections 23 and 25).  This
// file is the kind's own: its rule, its table entry and its commit.  DESIGN.md section 19.

// a member: an SDP cone whose own one-launch check on the dual buffer would run -- a sharded cone fails the rule by world != 1
bool MiCheckSet::eligible(const MiCone *c) const { return hdm_small_check_eligible(small_check_desc(c, dual_chol(c))); }
void MiCheckSet::empty() {}                                       // (the stored answer is the member's dual state)
const char *MiCheckSet::prepare(size_t, MiCone *) { return nullptr; }
const char *MiCheckSet::alloc_tables() { return table.alloc(members.size(), hipHostMallocMapped) != hipSuccess ? set_lacks("the table") : nullptr; }

// (the rule is asked again: whether the check is switched on and the factor object's shape do not change under a set, so this
// holds for every member -- a cone for which it did not would be left to its own path)
HdmSetSort MiCheckSet::sort(size_t, MiCone *c, const MiCheckQ &) {
    return (eligible(c) && !small_check_block(c)) ? HDM_SET_TAKE : HDM_SET_NOT_NOW;
}
// the member stands at (tau, y) with its own identity coefficient (y gathered into its block, where the launch reads it)
bool MiCheckSet::serves(size_t, MiCone *c, const MiCheckQ &q) {
    return c->dual.S_factored_at(small_check_point(c, q.tau, q.y, cone_eye(c)), nullptr);
}
// the point `serves` gathered
static HdmDualPoint check_set_asked(const MiCone *c, const MiCheckQ &q) { return HdmDualPoint{q.tau, cone_eye(c), c->chk.get(), c->mloc}; }
void MiCheckSet::fill(int place, size_t, MiCone *c, const MiCheckQ &q) {
    table.get()[place] = small_check_args(c, dual_chol(c), check_set_asked(c, q), 0);
    c->dual.S_overwritten();              // the launch writes S: what it holds is known again when the launch has reported
}
int MiCheckSet::fire(int nl, const MiCheckQ &) {
    int max_m = 0;
    for (int s = 0; s < nl; ++s) max_m = std::max(max_m, members[(size_t) launched[(size_t) s]]->mloc);
    return (hdm_grouped_check(table.get(), table.dev(), nl, max_m, g.stream) || hipStreamSynchronize(g.stream) != hipSuccess) ? 1 : 0;
}
void MiCheckSet::commit(int, size_t, MiCone *c, const MiCheckQ &q) { (void) small_check_commit(c, dual_chol(c), check_set_asked(c, q), 0); }
