// engine_build_small.h -- the rank-one and the sparse-gather Schur builders, cone destruction, the cone shell (vtable) and the way
// back from a shell to the engine's own cone (own_cone_data, own_cone_with_factor)
// Implementation header of engine.hip: included exactly once, there, in this order (the pieces share the anonymous namespace
// and the engine's thread-local context `g`).

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
    HdmChol &ch = *dual_chol(c);
    const int m = kkt->nRow;
    const int n16 = c->n16, m16 = c->mloc16;
    RC(ch.invert_factor(g.stream));
    TRACE_STEP("r1 step 1");
    const HdmOperand Linv = hdm_mmajor(ch.Linv.get(), ch.npad), LinvT = hdm_kmajor(ch.Linv.get(), ch.npad), Ut = hdm_kmajor(c->U.get(), n16);
    // U = Linv * Avec
    RC(hdm_launch_gemm(hdm_gemm_product(c->U.get(), n16, n16, m16, n16, 1.0, Linv, hdm_kmajor(c->Avec.get(), n16), 0.0, hdm_klimit(HDM_KLIM_BY_M)), g.stream));
    TRACE_STEP("r1 step 2");
    // V = Linv^T * U = S^-1 * Avec
    RC(hdm_launch_gemm(hdm_gemm_product(c->V.get(), n16, n16, m16, n16, 1.0, LinvT, Ut), g.stream));
    TRACE_STEP("r1 step 3");
    if (typeKKT == KKT_TYPE_CORRECTOR) {
        // ASinv_i = s_i a_i' S^-1 a_i = s_i <u_i,u_i>; ASinvRdSinv_i = Rd s_i |v_i|^2
        hipLaunchKernelGGL(mi_col_dot_kernel, dim3((c->mloc + 3) / 4), dim3(256), 0, g.stream, c->U.get(), c->U.get(), (long) n16,
                           n16, c->sgn.get(), c->rows_own.get(), c->mloc, pv->vecs.get());
    TRACE_STEP("r1 step 4");
        if (c->Rd != 0.0) RC(hdm_r1_colnorm(c->V.get(), n16, n16, c->sgn.get(), c->rows_own.get(), c->mloc, c->Rd, pv->vecs.get() + m, g.stream));
        return HDSDP_RETCODE_OK;
    }
    // Gr1 = U^T U
    RC(hdm_launch_gemm(hdm_gemm_product(c->Gr1.get(), m16, m16, m16, n16, 1.0, Ut, Ut, 0.0, hdm_lower()), g.stream));
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
        // W = Linv * C   (C symmetric)
        RC(hdm_launch_gemm(hdm_gemm_product(c->W.get(), n16, n16, n16, n16, 1.0, Linv, hdm_mmajor(c->Cfull.get(), n16), 0.0, hdm_klimit(HDM_KLIM_BY_M)), g.stream));
    TRACE_STEP("r1 step 9");
        // Ct = W * Linv^T
        RC(hdm_launch_gemm(hdm_gemm_product(c->Ct.get(), n16, n16, n16, n16, 1.0, hdm_mmajor(c->W.get(), n16), Linv, 0.0, hdm_klimit(HDM_KLIM_BY_N)), g.stream));
    TRACE_STEP("r1 step 10");
        // W = Ct * U
        RC(hdm_launch_gemm(hdm_gemm_product(c->W.get(), n16, n16, m16, n16, 1.0, hdm_mmajor(c->Ct.get(), n16), Ut), g.stream));
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
            // Xinv := Linv Linv^T
            RC(hdm_launch_gemm(hdm_gemm_product(c->Xinv.get(), n16, n16, n16, n16, 1.0, Linv, Linv), g.stream));
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
    HdmChol &ch = *dual_chol(c);
    const int m = kkt->nRow;
    const long ldx = ch.npad;
    const int n16 = c->n16;
    const HdmOperand X = hdm_mmajor(c->Xinv.get(), ldx);
    RC(ch.inverse_full(c->Xinv.get(), ldx, g.stream));
    RC(hdm_sparse_dot(c->sp_rp.get(), c->sp_ti.get(), c->sp_tj.get(), c->sp_tv.get(), c->Xinv.get(), ldx, c->mloc, c->rows_own.get(), 1.0, pv->vecs.get(), g.stream));
    if (c->Rd != 0.0) {
        // Y = X X^T = S^-2
        RC(hdm_launch_gemm(hdm_gemm_product(c->Yinv.get(), ldx, n16, n16, n16, 1.0, X, X), g.stream));
        RC(hdm_sparse_dot(c->sp_rp.get(), c->sp_ti.get(), c->sp_tj.get(), c->sp_tv.get(), c->Yinv.get(), ldx, c->mloc, c->rows_own.get(), c->Rd,
                          pv->vecs.get() + m, g.stream));
    }
    if (typeKKT == KKT_TYPE_CORRECTOR) return HDSDP_RETCODE_OK;
    if (c->Rd != 0.0)
        hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, c->Xinv.get(), ldx, nullptr, 0L, c->n, 1, 1.0,
                           pv->vecs.get() + 3 * m);
    RC(hdm_sparse_pairs(c->sp_rp.get(), c->sp_ti.get(), c->sp_tj.get(), c->sp_tv.get(), c->Xinv.get(), ldx, c->mloc, c->rows_own.get(), kkt_view(kkt), g.stream));
    if (typeKKT == KKT_TYPE_HOMOGENEOUS) {
        // W = X C,  Ct = W X = X C X
        RC(hdm_launch_gemm(hdm_gemm_product(c->W.get(), ldx, n16, n16, n16, 1.0, X, hdm_mmajor(c->Cfull.get(), n16)), g.stream));
        RC(hdm_launch_gemm(hdm_gemm_product(c->Ct.get(), ldx, n16, n16, n16, 1.0, hdm_mmajor(c->W.get(), ldx), X), g.stream));
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
    delete c;                 // (its links leave their sets: cone_set.h)
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
// ... and back: the cone behind a shell this function made, nullptr behind any other (a device-group cone -- cone_data answers
// for those too --, an LP cone, a host cone); and the same with a dual factor object: what the grouped build, the check set and
// the ratio set may look at
MiCone *own_cone_data(const hdsdp_cone *cone) { return (cone && cone->coneBuildSchur == cone_build_schur) ? (MiCone *) cone->coneData : nullptr; }
MiCone *own_cone_with_factor(const hdsdp_cone *cone) { MiCone *c = own_cone_data(cone); return (c && c->dualFactor) ? c : nullptr; }
