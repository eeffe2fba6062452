// engine_build_small.h -- the rank-one and the sparse-gather Schur builders, cone destruction and the cone shell (vtable)
// Implementation header of engine.hip: included exactly once, there, in this order (the pieces share the anonymous namespace
// and the engine's thread-local context `g`); split out of a 3 300-line file in round 3, nothing else changed.

#define TRACE_STEP(msg)                                                                                          \
    do {                                                                                                         \
        if (stat_trace()) {                                                                                      \
            const hipError_t e_ = hipDeviceSynchronize();                                                        \
            fprintf(stderr, "[hdsdp_mi355x trace]     %s (n %d, rows %d, m %d) -> %s\n", msg, c->n, c->mloc, m, \
                    e_ == hipSuccess ? "ok" : hipGetErrorName(e_));                                              \
        }                                                                                                        \
    } while (0)
hdsdp_retcode build_r1_path(MiCone *c, hdsdp_kkt *kkt, MiKKTPriv *pv, int typeKKT) {
    // all (non-zero) constraints are rank one: A_i = s_i a_i a_i'  (reference strategy M2)
    MiLin *l = (MiLin *) c->dualFactor->chol;
    HdmChol &ch = l->ch;
    const int m = kkt->nRow;
    const int n16 = c->n16, m16 = c->mloc16;
    RC(ch.invert_factor(g.stream));
    TRACE_STEP("r1 step 1");
    HdmGemmArgs u = {};  // U = Linv * Avec
    u.A = ch.Linv.get(); u.lda = ch.npad; u.B = c->Avec.get(); u.ldb = n16; u.b_kmajor = 1; u.C = c->U.get(); u.ldc = n16;
    u.M = n16; u.N = m16; u.K = n16; u.batch = 1; u.alpha = 1.0; u.klimit = HDM_KLIM_BY_M; u.epilogue = HDM_EPI_STORE;
    RC(hdm_launch_gemm(u, g.stream));
    TRACE_STEP("r1 step 2");
    HdmGemmArgs v = {};  // V = Linv^T * U = S^-1 * Avec
    v.A = ch.Linv.get(); v.lda = ch.npad; v.a_kmajor = 1; v.B = c->U.get(); v.ldb = n16; v.b_kmajor = 1; v.C = c->V.get(); v.ldc = n16;
    v.M = n16; v.N = m16; v.K = n16; v.batch = 1; v.alpha = 1.0; v.epilogue = HDM_EPI_STORE;
    RC(hdm_launch_gemm(v, g.stream));
    TRACE_STEP("r1 step 3");
    if (typeKKT == KKT_TYPE_CORRECTOR) {
        // ASinv_i = s_i a_i' S^-1 a_i = s_i <u_i,u_i>; ASinvRdSinv_i = Rd s_i |v_i|^2
        hipLaunchKernelGGL(mi_col_dot_kernel, dim3((c->mloc + 3) / 4), dim3(256), 0, g.stream, c->U.get(), c->U.get(), (long) n16,
                           n16, c->sgn.get(), c->rows_own.get(), c->mloc, pv->vecs.get());
    TRACE_STEP("r1 step 4");
        if (c->Rd != 0.0) RC(hdm_r1_colnorm(c->V.get(), n16, n16, c->sgn.get(), c->rows_own.get(), c->mloc, c->Rd, pv->vecs.get() + m, g.stream));
        return HDSDP_RETCODE_OK;
    }
    HdmGemmArgs gq = {};  // Gr1 = U^T U
    gq.A = c->U.get(); gq.lda = n16; gq.a_kmajor = 1; gq.B = c->U.get(); gq.ldb = n16; gq.b_kmajor = 1; gq.C = c->Gr1.get(); gq.ldc = m16;
    gq.M = m16; gq.N = m16; gq.K = n16; gq.batch = 1; gq.alpha = 1.0; gq.lower_only = 1; gq.epilogue = HDM_EPI_STORE;
    RC(hdm_launch_gemm(gq, g.stream));
    TRACE_STEP("r1 step 5");
    RC(hdm_r1_hadamard(c->Gr1.get(), m16, c->sgn.get(), c->rows_own.get(), c->mloc, kkt_view(kkt), pv->vecs.get(), g.stream));
    TRACE_STEP("r1 step 6");
    if (c->Rd != 0.0) {
        RC(hdm_r1_colnorm(c->V.get(), n16, n16, c->sgn.get(), c->rows_own.get(), c->mloc, c->Rd, pv->vecs.get() + m, g.stream));
    TRACE_STEP("r1 step 7");
        // TraceSinv = |Linv|_F^2
        hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, ch.Linv.get(), (long) ch.npad, ch.Linv.get(),
                           (long) ch.npad, c->n, 0, 1.0, pv->vecs.get() + 3 * m);
    TRACE_STEP("r1 step 8");
    }
    if (typeKKT == KKT_TYPE_HOMOGENEOUS && c->rank == 0) {
        // Ct = Linv C Linv^T (full);  ASinvCSinv_i = s_i u_i' Ct u_i;  CSinv = tr Ct; CSinvCSinv = |Ct|_F^2;
        // CSinvRdSinv = Rd <Ct, Linv Linv^T>
        HdmGemmArgs k1 = {};
        k1.A = ch.Linv.get(); k1.lda = ch.npad; k1.B = c->Cfull.get(); k1.ldb = n16; k1.C = c->W.get(); k1.ldc = n16;
        k1.M = n16; k1.N = n16; k1.K = n16; k1.batch = 1; k1.alpha = 1.0; k1.klimit = HDM_KLIM_BY_M;
        RC(hdm_launch_gemm(k1, g.stream));
    TRACE_STEP("r1 step 9");
        HdmGemmArgs k2 = {};
        k2.A = c->W.get(); k2.lda = n16; k2.B = ch.Linv.get(); k2.ldb = ch.npad; k2.C = c->Ct.get(); k2.ldc = n16;
        k2.M = n16; k2.N = n16; k2.K = n16; k2.batch = 1; k2.alpha = 1.0; k2.klimit = HDM_KLIM_BY_N;
        RC(hdm_launch_gemm(k2, g.stream));
    TRACE_STEP("r1 step 10");
        HdmGemmArgs w = {};  // W = Ct * U
        w.A = c->Ct.get(); w.lda = n16; w.B = c->U.get(); w.ldb = n16; w.b_kmajor = 1; w.C = c->W.get(); w.ldc = n16;
        w.M = n16; w.N = m16; w.K = n16; w.batch = 1; w.alpha = 1.0;
        RC(hdm_launch_gemm(w, g.stream));
    TRACE_STEP("r1 step 11");
        hipLaunchKernelGGL(mi_col_dot_kernel, dim3((c->mloc + 3) / 4), dim3(256), 0, g.stream, c->U.get(), c->W.get(), (long) n16,
                           n16, c->sgn.get(), c->rows_own.get(), c->mloc, pv->vecs.get() + 2 * m);
    TRACE_STEP("r1 step 12");
        hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, c->Ct.get(), (long) n16, nullptr, 0L, c->n, 1,
                           1.0, pv->vecs.get() + 3 * m + 1);
    TRACE_STEP("r1 step 13");
        hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, c->Ct.get(), (long) n16, c->Ct.get(), (long) n16,
                           c->n, 0, 1.0, pv->vecs.get() + 3 * m + 2);
    TRACE_STEP("r1 step 14");
        if (c->Rd != 0.0) {
            HdmGemmArgs q = {};  // Xinv := Linv Linv^T
            q.A = ch.Linv.get(); q.lda = ch.npad; q.B = ch.Linv.get(); q.ldb = ch.npad; q.C = c->Xinv.get(); q.ldc = n16;
            q.M = n16; q.N = n16; q.K = n16; q.batch = 1; q.alpha = 1.0;
            RC(hdm_launch_gemm(q, g.stream));
    TRACE_STEP("r1 step 15");
            hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, c->Ct.get(), (long) n16, c->Xinv.get(),
                               (long) n16, c->n, 0, c->Rd, pv->vecs.get() + 3 * m + 3);
    TRACE_STEP("r1 step 16");
        }
    }
    HIP_RC(hipGetLastError());
    return HDSDP_RETCODE_OK;
}

hdsdp_retcode build_sparse_path(MiCone *c, hdsdp_kkt *kkt, MiKKTPriv *pv, int typeKKT) {
    // every constraint is a short triplet list: gather from X = S^-1 (reference strategy M5, and the corrector /
    // HSD components that the reference evaluates with the same gathers, hdsdp_conic_sdp.c:923-1056)
    MiLin *l = (MiLin *) c->dualFactor->chol;
    HdmChol &ch = l->ch;
    const int m = kkt->nRow;
    const long ldx = ch.npad;
    RC(ch.inverse_full(c->Xinv.get(), ldx, g.stream));
    RC(hdm_sparse_dot(c->sp_rp.get(), c->sp_ti.get(), c->sp_tj.get(), c->sp_tv.get(), c->Xinv.get(), ldx, c->mloc, c->rows_own.get(), 1.0, pv->vecs.get(), g.stream));
    if (c->Rd != 0.0) {
        HdmGemmArgs q = {};  // Y = X X^T = S^-2
        q.A = c->Xinv.get(); q.lda = ldx; q.B = c->Xinv.get(); q.ldb = ldx; q.C = c->Yinv.get(); q.ldc = ldx;
        q.M = c->n16; q.N = c->n16; q.K = c->n16; q.batch = 1; q.alpha = 1.0; q.epilogue = HDM_EPI_STORE;
        RC(hdm_launch_gemm(q, g.stream));
        RC(hdm_sparse_dot(c->sp_rp.get(), c->sp_ti.get(), c->sp_tj.get(), c->sp_tv.get(), c->Yinv.get(), ldx, c->mloc, c->rows_own.get(), c->Rd,
                          pv->vecs.get() + m, g.stream));
    }
    if (typeKKT == KKT_TYPE_CORRECTOR) return HDSDP_RETCODE_OK;
    if (c->Rd != 0.0)
        hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, c->Xinv.get(), ldx, nullptr, 0L, c->n, 1, 1.0,
                           pv->vecs.get() + 3 * m);
    RC(hdm_sparse_pairs(c->sp_rp.get(), c->sp_ti.get(), c->sp_tj.get(), c->sp_tv.get(), c->Xinv.get(), ldx, c->mloc, c->rows_own.get(), kkt_view(kkt), g.stream));
    if (typeKKT == KKT_TYPE_HOMOGENEOUS) {
        HdmGemmArgs w = {};  // W = X C,  Ct = W X = X C X
        w.A = c->Xinv.get(); w.lda = ldx; w.B = c->Cfull.get(); w.ldb = c->n16; w.C = c->W.get(); w.ldc = ldx;
        w.M = c->n16; w.N = c->n16; w.K = c->n16; w.batch = 1; w.alpha = 1.0; w.epilogue = HDM_EPI_STORE;
        RC(hdm_launch_gemm(w, g.stream));
        HdmGemmArgs x = {};
        x.A = c->W.get(); x.lda = ldx; x.B = c->Xinv.get(); x.ldb = ldx; x.C = c->Ct.get(); x.ldc = ldx;
        x.M = c->n16; x.N = c->n16; x.K = c->n16; x.batch = 1; x.alpha = 1.0; x.epilogue = HDM_EPI_STORE;
        RC(hdm_launch_gemm(x, g.stream));
        RC(hdm_sparse_dot(c->sp_rp.get(), c->sp_ti.get(), c->sp_tj.get(), c->sp_tv.get(), c->Ct.get(), ldx, c->mloc, c->rows_own.get(), 1.0,
                          pv->vecs.get() + 2 * m, g.stream));
        hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, c->Cfull.get(), (long) c->n16, c->Xinv.get(), ldx, c->n,
                           0, 1.0, pv->vecs.get() + 3 * m + 1);
        hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, c->Cfull.get(), (long) c->n16, c->Ct.get(), ldx, c->n, 0,
                           1.0, pv->vecs.get() + 3 * m + 2);
        if (c->Rd != 0.0)
            hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, c->Cfull.get(), (long) c->n16, c->Yinv.get(), ldx,
                               c->n, 0, c->Rd, pv->vecs.get() + 3 * m + 3);
    }
    HIP_RC(hipGetLastError());
    return HDSDP_RETCODE_OK;
}

void cone_destroy_data(void **pcd) {
    if (!pcd || !*pcd) return;
    MiCone *c = (MiCone *) *pcd;
    HFpLinsysDestroy(&c->dualFactor);
    for (hipEvent_t e : c->piece_ev) if (e) (void) hipEventDestroy(e);
    for (hipEvent_t e : c->pe_s2) if (e) (void) hipEventDestroy(e);
    for (hipEvent_t e : c->pe_ga) if (e) (void) hipEventDestroy(e);
    for (hipEvent_t e : c->pe_gb) if (e) (void) hipEventDestroy(e);
    if (c->pe_s1) (void) hipEventDestroy(c->pe_s1);
    delete c;
    *pcd = nullptr;
}

hdsdp_cone *new_cone_shell(MiCone *c, int iCone) {
    hdsdp_cone *h = (hdsdp_cone *) calloc(1, sizeof(hdsdp_cone));
    h->iCone = iCone;
    h->cone = HDSDP_CONETYPE_DENSE_SDP;
    h->coneData = c;
    h->coneDestroyData = cone_destroy_data;
    h->coneSetStart = cone_setstart;
    h->coneUpdate = cone_update;
    h->coneGetSymNnz = cone_getsymnnz;
    h->coneAddSymNz = cone_add_sym_nz;
    h->coneGetKKTMap = cone_get_kkt_map;
    h->coneGetDim = cone_getdim;
    h->coneBuildSchur = cone_build_schur;
    h->coneBuildSchurFixed = cone_build_schur_fixed;
    h->coneBuildPrimalDirection = cone_build_primal_dir;
    h->coneInteriorCheck = cone_interior;
    h->coneRatioTest = cone_ratio_test;
    h->conePRecover = cone_precover;
    h->coneInteriorCheckExpert = cone_interior_expert;
    h->coneAxpyBufferAndCheck = cone_axpy_check;
    h->coneReduceResi = cone_reduce_resi;
    h->coneSetPerturb = cone_set_perturb;
    h->getstat = cone_getstat;
    h->coneView = cone_view;
    h->coneGetCoeffNorm = cone_coeff_norm;
    h->coneGetObjNorm = cone_obj_norm;
    h->coneScal = cone_scal;
    h->coneATimesXpy = cone_a_times_x;
    h->coneTraceCX = cone_trace_cx;
    h->coneXDotS = cone_x_dot_s;
    h->coneDRecover = cone_get_dual;
    h->coneGetBarrier = cone_barrier;
    return h;
}
