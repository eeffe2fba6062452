// engine_grouped.h -- the grouped Schur build: every eligible small SDP cone of an operator built in three launches
// Implementation header of engine.hip: included exactly once, there, in this order (the pieces share the anonymous namespace
// and the engine's thread-local context `g`).
// The rule and the plan are grouped_plan.h's (pure host arithmetic), the kernels small.hip's; this file says which cones of an
// operator the engine may group, keeps the plan's device copies and the staging buffers in MiKKTPriv::grp, and performs one
// grouped pass.  DESIGN.md section 17.

// what only the engine can say about a cone (grouped_plan.h: HdmGroupedCone::kind_ok): an SDP cone of this engine on one device,
// not synthetic, not streamed, its A_L forms resident -- and a one-block dual factor, whose Dinv is the triangular inverse
bool grouped_kind_ok(const hdsdp_cone *hc) {
    const MiCone *c = own_cone_with_factor(hc);
    if (!c || c->world != 1 || c->synthetic || c->rows.streamed() || !c->rows.resident()) return false;
    const HdmChol &ch = *dual_chol(c);
    return ch.nblk == 1 && ch.npad == SMALL_P;
}

// HKKTInit: the eligible cones of this operator
void grouped_init_plan(hdsdp_kkt *HKKT, MiKKTPriv *pv) {
    MiGrouped &gr = pv->grp;
    gr.desc.assign((size_t) HKKT->nCones, HdmGroupedCone());
    gr.n_eligible = 0;
    for (int i = 0; i < HKKT->nCones; ++i) {
        const hdsdp_cone *hc = HKKT->cones[i];
        HdmGroupedCone &d = gr.desc[(size_t) i];
        if (!(d.kind_ok = grouped_kind_ok(hc))) continue;
        const MiCone *c = (const MiCone *) hc->coneData;
        d.n = c->n; d.mloc = c->mloc; d.rows = c->own.data();
        gr.n_eligible += hdm_grouped_eligible(d) ? 1 : 0;
    }
    gr.on = gr.planned = gr.dev_ready = false;
    gr.plan = HdmGroupedPlan();
    gr.max_n16 = 0;
}
// the lists, when the switch is first turned on
void grouped_make_plan(hdsdp_kkt *HKKT, MiKKTPriv *pv) {
    MiGrouped &gr = pv->grp;
    if (gr.planned) return;
    gr.plan = hdm_grouped_plan(HKKT->nRow, gr.desc);
    gr.planned = true;
    for (int i : gr.plan.cones) gr.max_n16 = std::max(gr.max_n16, ((const MiCone *) HKKT->cones[i]->coneData)->n16);
}

template <typename T> static int grouped_upload(HdmBuf<T> &dst, const std::vector<T> &src) {
    if (dst.alloc(std::max<size_t>(1, src.size())) != hipSuccess) return 1;
    return (!src.empty() && hdm_memcpy_h2d_sync(dst.get(), src.data(), sizeof(T) * src.size()) != hipSuccess) ? 1 : 0;
}

// the plan's device copies and the staging buffers (once per operator, when the switch is first turned on)
int grouped_make_device(MiKKTPriv *pv) {
    MiGrouped &gr = pv->grp;
    const HdmGroupedPlan &p = gr.plan;
    if (gr.dev_ready) return 0;
    if (grouped_upload(gr.jobs, p.jobs) || grouped_upload(gr.m_row, p.m_row) || grouped_upload(gr.m_col, p.m_col) ||
        grouped_upload(gr.m_ptr, p.m_ptr) || grouped_upload(gr.m_slot, p.m_slot) || grouped_upload(gr.m_idx, p.m_idx) ||
        grouped_upload(gr.v_row, p.v_row) || grouped_upload(gr.v_ptr, p.v_ptr) || grouped_upload(gr.v_slot, p.v_slot) ||
        grouped_upload(gr.v_idx, p.v_idx))
        return 1;
    if (gr.cones_host.alloc(p.cones.size()) != hipSuccess || gr.cones_dev.alloc(p.cones.size()) != hipSuccess ||
        gr.X.alloc((size_t) std::max(1L, p.x_doubles)) != hipSuccess || gr.G.alloc((size_t) std::max(1L, p.g_doubles)) != hipSuccess ||
        gr.V.alloc((size_t) std::max(1L, p.v_doubles)) != hipSuccess)
        return 1;
    gr.dev_ready = true;
    return 0;
}

// the switch: returns the number of cones that will be grouped
int grouped_set(hdsdp_kkt *HKKT, MiKKTPriv *pv, int on) {
    MiGrouped &gr = pv->grp;
    gr.on = false;
    if (!on || gr.n_eligible < HDM_GROUPED_MIN_CONES) return 0;
    grouped_make_plan(HKKT, pv);
    if (!gr.plan.used()) return 0;
    if (grouped_make_device(pv)) {
        (void) hipGetLastError();
        fprintf(stderr, "[hdsdp_mi355x] grouped Schur build: out of device memory for the plan and the staging buffers; the per-cone builders stay\n");
        return 0;
    }
    gr.on = true;
    return (int) gr.plan.cones.size();
}

// One grouped pass: the grouped cones' contributions to M and to the accumulators, where the per-cone builders put theirs.
// The cones' factor objects are read, nothing of a cone is written.
hdsdp_retcode grouped_build(hdsdp_kkt *HKKT, MiKKTPriv *pv, int typeKKT) {
    MiGrouped &gr = pv->grp;
    const HdmGroupedPlan &p = gr.plan;
    const int nc = (int) p.cones.size();
    for (int s = 0; s < nc; ++s) {
        const MiCone *c = (const MiCone *) HKKT->cones[p.cones[(size_t) s]]->coneData;
        const HdmChol &ch = *dual_chol(c);
        if (!ch.factored) {
            fprintf(stderr, "[hdsdp_mi355x] BuildSchur: the dual matrix has no valid Cholesky factor\n");
            return HDSDP_RETCODE_FAILED;
        }
        HdmGroupedConeDev &d = gr.cones_host.get()[s];
        d.n = c->n; d.n16 = c->n16; d.mloc = c->mloc; d.pad = 0;
        d.W = ch.Dinv.get(); d.A = c->rows.resident(); d.C = c->Cfull.get(); d.Rd = c->Rd;
        d.xoff = p.xoff[(size_t) s]; d.goff = p.goff[(size_t) s]; d.voff = p.voff[(size_t) s];
    }
    // (the pinned block is free to be rewritten: every build ends in kkt_pull's synchronisation)
    HIP_RC(hipMemcpyAsync(gr.cones_dev.get(), gr.cones_host.get(), sizeof(HdmGroupedConeDev) * (size_t) nc, hipMemcpyHostToDevice, g.stream));
    HdmGroupedArgs a = {};
    a.cones = gr.cones_dev.get(); a.ncones = nc; a.jobs = gr.jobs.get(); a.njobs = (int) p.jobs.size();
    a.max_n16 = gr.max_n16; a.typeKKT = typeKKT;
    a.X = gr.X.get(); a.G = gr.G.get(); a.V = gr.V.get();
    HdmGroupedScatterArgs sc = {};
    sc.cones = a.cones; sc.ncones = nc;
    sc.nM = (long) p.m_row.size(); sc.m_row = gr.m_row.get(); sc.m_col = gr.m_col.get(); sc.m_ptr = gr.m_ptr.get();
    sc.m_slot = gr.m_slot.get(); sc.m_idx = gr.m_idx.get();
    sc.nV = (int) p.v_row.size(); sc.v_row = gr.v_row.get(); sc.v_ptr = gr.v_ptr.get(); sc.v_slot = gr.v_slot.get(); sc.v_idx = gr.v_idx.get();
    sc.G = gr.G.get(); sc.V = gr.V.get(); sc.vecs = pv->vecs.get(); sc.m = HKKT->nRow; sc.typeKKT = typeKKT;
    if (hdm_grouped_inverses(a, g.stream)) return HDSDP_RETCODE_FAILED;
    gr.last_launches += 1;
    if (hdm_grouped_jobs(a, g.stream)) return HDSDP_RETCODE_FAILED;
    gr.last_launches += 1;
    if (hdm_grouped_scatter(sc, kkt_view(HKKT), g.stream)) return HDSDP_RETCODE_FAILED;
    gr.last_launches += 1;
    gr.last_cones = nc; gr.last_jobs = a.njobs;
    return HDSDP_RETCODE_OK;
}
