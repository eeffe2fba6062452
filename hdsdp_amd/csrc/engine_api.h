// engine_api.h -- exported C ABI, second part: the HMi* cone entries, the device group entries, the fused Phase-A pass, call statistics
// Implementation header of engine.hip: included exactly once, there, in this order (inside extern "C"); split out of a 3 300-line file in round 3, nothing else changed.

hdsdp_retcode HMiConeCreateSDP(hdsdp_cone **pCone, int iCone, int nRow, int nCol, const int *coneMatBeg,
                               const int *coneMatIdx, const double *coneMatElem, int rank, int world) {
    return cone_create_csc(pCone, iCone, nRow, nCol, coneMatBeg, coneMatIdx, coneMatElem, rank, world);
}
hdsdp_retcode HMiConeCreateSDP64(hdsdp_cone **pCone, int iCone, int nRow, int nCol, const int64_t *coneMatBeg,
                                 const int *coneMatIdx, const double *coneMatElem, int rank, int world) {
    return cone_create_csc(pCone, iCone, nRow, nCol, coneMatBeg, coneMatIdx, coneMatElem, rank, world);
}

// ---------------------------------------------------------------- LP cone (engine_lp.h)
hdsdp_retcode HMiConeCreateLP(hdsdp_cone **pCone, int iCone, int nRow, int nCol, const int *coneMatBeg, const int *coneMatIdx,
                              const double *coneMatElem) {
    return lp_cone_create(pCone, iCone, nRow, nCol, coneMatBeg, coneMatIdx, coneMatElem);
}
int HMiConeLPSetSchurPath(hdsdp_cone *cone, int path) {
    if (!cone || cone->coneBuildSchur != lp_build_schur || path < 0 || path > 2) return 1;
    MiLPCone *c = (MiLPCone *) cone->coneData;
    if (lp_set_path(c, path)) {
        fprintf(stderr, "[hdsdp_mi355x] HMiConeLPSetSchurPath(%d): the %s path cannot be set up (pair list of %.2f GiB, cap %.2f)\n", path,
                path == 2 ? "sparse" : "dense", (double) lp_sparse_bytes(c) / LP_PAIR_CAP, 1.0);
        return 1;
    }
    return 0;
}
int HMiConeLPGetSchurPath(hdsdp_cone *cone, double *costDense, double *costSparse, int64_t *pairBytes) {
    if (!cone || cone->coneBuildSchur != lp_build_schur) return -1;
    const MiLPCone *c = (const MiLPCone *) cone->coneData;
    if (costDense) *costDense = c->cost_dense;
    if (costSparse) *costSparse = c->cost_sparse;
    if (pairBytes) *pairBytes = lp_sparse_bytes(c);
    return c->path;
}

// ---------------------------------------------------------------- column-by-column ingest (64-bit totals)
struct HMiConeBuilder_s : MiConeBuilder {};
hdsdp_retcode HMiConeBuilderBegin(HMiConeBuilder **pBuilder, int iCone, int nRow, int nCol, int rank, int world) {
    if (!pBuilder || nRow < 1 || nCol < 1 || nCol > 65535 || world < 1 || rank < 0 || rank >= world) return HDSDP_RETCODE_FAILED;
    HMiConeBuilder_s *b = new HMiConeBuilder_s();
    b->iCone = iCone; b->rank = rank; b->world = world;
    b->blk.n = nCol; b->blk.m = nRow;
    b->blk.rows.assign((size_t) nRow, MiCoeff());
    b->seen.assign((size_t) nRow + 1, 0);
    *pBuilder = b;
    return HDSDP_RETCODE_OK;
}
hdsdp_retcode HMiConeBuilderAddColumn(HMiConeBuilder *b, int iCol, int64_t nnz, const int *packedIdx, const double *val) {
    if (!b || iCol < 0 || iCol > b->blk.m || nnz < 0 || (nnz > 0 && (!packedIdx || !val))) return HDSDP_RETCODE_FAILED;
    if (b->seen[iCol]) { fprintf(stderr, "[hdsdp_mi355x] HMiConeBuilderAddColumn: column %d was given before\n", iCol); return HDSDP_RETCODE_FAILED; }
    MiCoeff &dst = (iCol == 0) ? b->blk.obj : b->blk.rows[iCol - 1];
    if (mi_coeff_build(dst, b->blk.n, (long) nnz, packedIdx, val)) {
        fprintf(stderr, "[hdsdp_mi355x] HMiConeBuilderAddColumn: column %d has a packed index outside [0, n(n+1)/2) or too many entries\n", iCol);
        return HDSDP_RETCODE_FAILED;
    }
    b->seen[iCol] = 1;
    return HDSDP_RETCODE_OK;
}
int64_t HMiConeBuilderStored(const HMiConeBuilder *b) {
    if (!b) return 0;
    int64_t t = b->blk.obj.stored;
    for (const MiCoeff &c : b->blk.rows) t += c.stored;
    return t;
}
hdsdp_retcode HMiConeBuilderFinish(HMiConeBuilder **pBuilder, hdsdp_cone **pCone) {
    if (!pBuilder || !*pBuilder || !pCone) return HDSDP_RETCODE_FAILED;
    HMiConeBuilder_s *b = *pBuilder;
    mi_block_plan(b->blk);                       // (columns never given are zero matrices)
    const hdsdp_retcode rc = cone_from_block(pCone, b->iCone, b->blk, b->rank, b->world);
    delete b;
    *pBuilder = nullptr;
    return rc;
}
void HMiConeBuilderAbort(HMiConeBuilder **pBuilder) {
    if (pBuilder && *pBuilder) { delete *pBuilder; *pBuilder = nullptr; }
}

hdsdp_retcode HMiConeCreateSynthetic(hdsdp_cone **pCone, int iCone, int nCol, int nRow, int rank, int world) {
    if (!pCone || nRow < 1 || nCol < 1 || world < 1 || rank < 0 || rank >= world) return HDSDP_RETCODE_FAILED;
    if (group_configure_from_env()) return HDSDP_RETCODE_FAILED;
    if (ensure_ctx()) return HDSDP_RETCODE_FAILED;
    if (rank == 0 && world == 1 && group_wants_synthetic(nRow, nCol))
        return group_create_cone(pCone, iCone, nRow, nCol, nullptr, true);
    MiCone *c = nullptr;
    hdsdp_retcode rc = make_synth_cone(&c, nCol, nRow, rank, world);
    if (rc != HDSDP_RETCODE_OK) return rc;
    *pCone = new_cone_shell(c, iCone);
    return HDSDP_RETCODE_OK;
}

void HMiConeDestroy(hdsdp_cone **pCone) {
    if (!pCone || !*pCone) return;
    if ((*pCone)->coneDestroyData) (*pCone)->coneDestroyData(&(*pCone)->coneData);
    free(*pCone);
    *pCone = nullptr;
}
void HMiConeSetStart(hdsdp_cone *cone, double v) { cone->coneSetStart(cone->coneData, v); }
void HMiConeUpdate(hdsdp_cone *cone, double tau, double *y) { cone->coneUpdate(cone->coneData, tau, y); }
hdsdp_retcode HMiConeCheckIsInterior(hdsdp_cone *cone, double tau, double *y, int *isInterior) {
    return cone->coneInteriorCheck(cone->coneData, tau, y, isInterior);
}
hdsdp_retcode HMiConeGetLogBarrier(hdsdp_cone *cone, double tau, double *y, int whichBuffer, double *logdet) {
    return cone->coneGetBarrier(cone->coneData, tau, y, whichBuffer, logdet);
}
hdsdp_retcode HMiConeRatioTest(hdsdp_cone *cone, double dTauStep, double *dy, double dAdaRatio, int whichBuffer,
                               double *maxStep) {
    return cone->coneRatioTest(cone->coneData, dTauStep, dy, dAdaRatio, whichBuffer, maxStep);
}
void HMiLanczosStartVector(int n, double *v) { hdm_lanczos_start_vector(n, v); }
hdsdp_retcode HMiConeCheckIsInteriorExpert(hdsdp_cone *cone, double dCCoef, double dACoefScal, double *dACoef, double dEyeCoef,
                                           int whichBuffer, int *isInterior) {
    return cone->coneInteriorCheckExpert(cone->coneData, dCCoef, dACoefScal, dACoef, dEyeCoef, whichBuffer, isInterior);
}
hdsdp_retcode HMiConeAddStepToBufferAndCheck(hdsdp_cone *cone, double dStep, int whichBuffer, int *isInterior) {
    return cone->coneAxpyBufferAndCheck(cone->coneData, dStep, whichBuffer, isInterior);
}
double HMiConeGetCoeffNorm(hdsdp_cone *cone, int whichNorm) { return cone->coneGetCoeffNorm(cone->coneData, whichNorm); }
double HMiConeGetObjNorm(hdsdp_cone *cone, int whichNorm) { return cone->coneGetObjNorm(cone->coneData, whichNorm); }
void HMiConeScalByConstant(hdsdp_cone *cone, double dScal) { cone->coneScal(cone->coneData, dScal); }
void HMiConeComputeATimesXpy(hdsdp_cone *cone, double *dConePrimal, double *dATimesX) {
    cone->coneATimesXpy(cone->coneData, dConePrimal, dATimesX);
}
double HMiConeComputeXDotS(hdsdp_cone *cone, double *dConePrimal) { return cone->coneXDotS(cone->coneData, dConePrimal); }
double HMiConeComputeTraceCX(hdsdp_cone *cone, double *dConePrimal) { return cone->coneTraceCX(cone->coneData, dConePrimal); }
void HMiConeGetDual(hdsdp_cone *cone, double *dConeDual, double *dConeDual2) {
    cone->coneDRecover(cone->coneData, dConeDual, dConeDual2);
}
void HMiConeDetectFeature(hdsdp_cone *cone, double *rowRHS, int coneIntFeatures[20], double coneDblFeatures[20]) {   // hdsdp_conic.c:423-428
    cone->getstat(cone->coneData, rowRHS, coneIntFeatures, coneDblFeatures);
}
void HMiConeReduceResi(hdsdp_cone *cone, double dResiReduction) { cone->coneReduceResi(cone->coneData, dResiReduction); }
void HMiConeSetPerturb(hdsdp_cone *cone, double dDualPerturb) { cone->coneSetPerturb(cone->coneData, dDualPerturb); }
void HMiConeGetPrimal(hdsdp_cone *cone, double dBarrierMu, double *dRowDual, double *dRowDualStep, double *dConePrimal,
                      double *dConePrimal2) {
    cone->conePRecover(cone->coneData, dBarrierMu, dRowDual, dRowDualStep, dConePrimal, dConePrimal2);
}
void HMiConeGetPresolve(hdsdp_cone *cone, int *coefType, int *coefRank, int *coefNnz, int *kktPerm, int *kktStrategy,
                        int *objType) {
    MiCone *c = cone_data(cone);
    if (!c) return;                   // (not an SDP cone of the engine: no presolve)
    for (int i = 0; i < c->m && !c->synthetic; ++i) {
        if (coefType) coefType[i] = c->blk.rows[i].type;
        if (coefRank) coefRank[i] = c->blk.rows[i].rank;
        if (coefNnz) coefNnz[i] = c->blk.rows[i].nnz;
        if (kktPerm) kktPerm[i] = c->blk.perm[i];
        if (kktStrategy) kktStrategy[i] = c->blk.strategy[i];
    }
    if (objType) *objType = c->synthetic ? MI_COEFF_DENSE : c->blk.obj.type;
}
hdsdp_retcode HMiPresolveCSC(int nRow, int nCol, const int *coneMatBeg, const int *coneMatIdx,
                             const double *coneMatElem, int *coefType, int *coefRank, int *coefNnz, int *kktPerm,
                             int *kktStrategy, int *objType) {
    if (nRow < 1 || nCol < 1 || !coneMatBeg) return HDSDP_RETCODE_FAILED;
    MiBlockData blk;
    if (mi_block_from_csc(blk, nRow, nCol, coneMatBeg, coneMatIdx, coneMatElem)) return HDSDP_RETCODE_FAILED;
    for (int i = 0; i < nRow; ++i) {
        if (coefType) coefType[i] = blk.rows[i].type;
        if (coefRank) coefRank[i] = blk.rows[i].rank;
        if (coefNnz) coefNnz[i] = blk.rows[i].nnz;
        if (kktPerm) kktPerm[i] = blk.perm[i];
        if (kktStrategy) kktStrategy[i] = blk.strategy[i];
    }
    if (objType) *objType = blk.obj.type;
    return HDSDP_RETCODE_OK;
}
hdsdp_retcode HMiConeGetDualMatrix(hdsdp_cone *cone, double *S) {
    MiCone *c = cone_data(cone);
    if (!c) return HDSDP_RETCODE_FAILED;
    if (hipMemcpy2DAsync(S, sizeof(double) * c->n, c->S.get(), sizeof(double) * c->n16, sizeof(double) * c->n, c->n,
                         hipMemcpyDeviceToHost, g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    return hipStreamSynchronize(g.stream) == hipSuccess ? HDSDP_RETCODE_OK : HDSDP_RETCODE_FAILED;
}
hdsdp_retcode HMiConeGetChecker(hdsdp_cone *cone, double *Scheck, double *L, double *Dinv) {
    MiCone *c = own_cone_data(cone);
    if (!c || !c->checker || !hdm_small_check_factor_ok(c->checker->npad, c->checker->nblk)) return HDSDP_RETCODE_FAILED;
    const HdmChol &ch = *c->checker;
    const size_t np2 = sizeof(double) * (size_t) ch.npad * ch.npad;
    if (Scheck && hipMemcpyAsync(Scheck, c->Scheck.get(), sizeof(double) * (size_t) c->n16 * c->n16, hipMemcpyDeviceToHost, g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    if (L && hipMemcpyAsync(L, ch.L.get(), np2, hipMemcpyDeviceToHost, g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    if (Dinv && hipMemcpyAsync(Dinv, ch.Dinv.get(), np2, hipMemcpyDeviceToHost, g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    return hipStreamSynchronize(g.stream) == hipSuccess ? HDSDP_RETCODE_OK : HDSDP_RETCODE_FAILED;
}
hdsdp_retcode HMiConeGetTraces(hdsdp_cone *cone, double *trA) {
    MiCone *c = cone_data(cone);
    if (!c || c->trA.empty()) return HDSDP_RETCODE_FAILED;
    memcpy(trA, c->trA.data(), sizeof(double) * c->m);
    return HDSDP_RETCODE_OK;
}
int HMiConeGetPath(hdsdp_cone *cone) { const MiCone *c = cone_data(cone); return c ? c->path : -1; }
void HMiConeGetDirectRows(hdsdp_cone *cone, int *nDirect, int *nRankOne, int *nCongruence, int *kmax) {
    const MiCone *c = own_cone_data(cone);
    const bool on = c && c->dr_n > 0;
    if (nDirect) *nDirect = on ? c->dr_n : 0;
    if (nRankOne) *nRankOne = on ? c->dr_r1 : 0;
    if (nCongruence) *nCongruence = on ? c->mloc - c->dr_n : 0;
    if (kmax) *kmax = on ? c->dr_kmax : 0;
}
int HMiConeUseSweepCopy(hdsdp_cone *cone, int on) {
    MiCone *c = cone_data(cone);
    if (!c || ensure_ctx()) return 1;
    c->dual.data_changed();          // the next request is assembled, not short-cut
    if (!on) { c->rows.use_sweep_copy(false); return 0; }   // (the copy stays: switching it on again costs nothing)
    if (c->rows.make_sweep_copy(1.0)) return 1;
    return c->rows.sweep_copy_in_use() ? 0 : 1;
}
int HMiConeGetStreaming(hdsdp_cone *cone, int *batchRows) {
    const MiCone *c = cone_data(cone);
    const bool on = c && c->rows.streamed();
    if (batchRows) *batchRows = on ? c->rows.batch() : 0;
    return on ? 1 : 0;
}
int HMiConeSweepInfo(hdsdp_cone *cone, int64_t *values, int64_t *positions) {
    const MiCone *c = cone_data(cone);
    const bool on = c && c->rows.sweep_copy_in_use();
    if (values) *values = on ? (int64_t) c->rows.sweep_copy().nnz : 0;
    if (positions) *positions = on ? (int64_t) c->rows.sweep_copy().sky * c->rows.sweep_copy().m : 0;
    return on ? 1 : 0;
}
// the work plan (work_plan.h): what the engine would plan here and now -- host only, no context, no device -- and what a cone holds
int HMiWorkPlanQuery(int n, int m, int world, int rank, int64_t *out, int cap) {
    if (n < 1 || m < 0 || world < 1 || rank < 0 || rank >= world || !out || cap < 17) return -17;
    const HdmLayout L = hdm_layout(n, world, (m + world - 1) / world);
    const long mloc = hdm_rows_of_rank(m, world, rank);
    const HdmWorkPlan p = hdm_work_plan(L, mloc, false, 0, hdm_knobs_from_env());
    const int64_t v[17] = {L.n16, L.nblk, L.npb, L.npb_loc, L.Lr, L.R, L.astride, mloc, p.Bc, p.nsplit, p.nslab, p.shared_ts,
                           p.gram_queue_global, (int64_t) p.t_bytes, (int64_t) p.slab_bytes, (int64_t) p.exch_bytes, (int64_t) p.gm_bytes};
    memcpy(out, v, sizeof(v));
    return 17;
}
// the grouped build's plan (grouped_plan.h) for an operator described by arrays -- host only, no context, no device
int HMiGroupedPlanQuery(int nRow, int nCones, const int *dims, const int *kindOk, const int *rowBeg, const int *rows, int64_t *counts,
                        int *eligible, int *slotOf, int *jobs, int *mRow, int *mCol, int64_t *mPtr, int *mSlot, int *mIdx, int *vRow,
                        int64_t *vPtr, int *vSlot, int *vIdx) {
    if (nRow < 0 || nCones < 0 || !dims || !kindOk || !rowBeg || !counts || rowBeg[0] != 0) return -1;
    std::vector<HdmGroupedCone> cs((size_t) nCones);
    for (int k = 0; k < nCones; ++k) {
        if (rowBeg[k + 1] < rowBeg[k] || (rowBeg[k + 1] > rowBeg[k] && !rows)) return -1;
        for (int q = rowBeg[k]; q < rowBeg[k + 1]; ++q) if (rows[q] < 0 || rows[q] >= nRow) return -1;
        cs[(size_t) k].n = dims[k]; cs[(size_t) k].mloc = rowBeg[k + 1] - rowBeg[k];
        cs[(size_t) k].rows = rows ? rows + rowBeg[k] : nullptr; cs[(size_t) k].kind_ok = kindOk[k] != 0;
    }
    const HdmGroupedPlan p = hdm_grouped_plan(nRow, cs);
    int nel = 0;
    for (int k = 0; k < nCones; ++k) {
        const int e = hdm_grouped_eligible(cs[(size_t) k]) ? 1 : 0;
        nel += e;
        if (eligible) eligible[k] = e;
        if (slotOf) slotOf[k] = p.slot_of[(size_t) k];
    }
    const int64_t v[8] = {(int64_t) p.cones.size(), (int64_t) p.jobs.size(), (int64_t) p.m_row.size(), (int64_t) p.m_slot.size(),
                          (int64_t) p.v_row.size(), (int64_t) p.v_slot.size(), (int64_t) (p.x_doubles + p.g_doubles + p.v_doubles), nel};
    memcpy(counts, v, sizeof(v));
    if (jobs) for (size_t j = 0; j < p.jobs.size(); ++j) { jobs[4 * j] = p.jobs[j].slot; jobs[4 * j + 1] = p.jobs[j].q0; jobs[4 * j + 2] = p.jobs[j].q1; jobs[4 * j + 3] = p.jobs[j].first; }
    auto put = [](int *dst, const std::vector<int> &src) { if (dst && !src.empty()) memcpy(dst, src.data(), sizeof(int) * src.size()); };
    put(mRow, p.m_row); put(mCol, p.m_col); put(mSlot, p.m_slot); put(mIdx, p.m_idx); put(vRow, p.v_row); put(vSlot, p.v_slot); put(vIdx, p.v_idx);
    if (mPtr) for (size_t e = 0; e < p.m_ptr.size(); ++e) mPtr[e] = p.m_ptr[e];
    if (vPtr) for (size_t e = 0; e < p.v_ptr.size(); ++e) vPtr[e] = p.v_ptr[e];
    return 8;
}
int HMiConeGetWorkPlan(hdsdp_cone *cone, int64_t *out, int cap) {
    const MiCone *c = cone_data(cone);
    if (!c || !out || cap < 7) return -1;
    if (!c->work_ready) return 0;
    const int64_t v[7] = {c->Bc, c->nsplit, c->nslab, c->shared_ts, c->gram_queue_global, (int64_t) (sizeof(double) * c->T.count()),
                          (int64_t) (sizeof(double) * (size_t) c->R * c->R * c->nslab)};
    memcpy(out, v, sizeof(v));
    return 7;
}

// ---------------------------------------------------------------- single-process multi-device mode (group_impl.h)
int HMiSetDevicesEx(int nDevices, const int *deviceIds, int transport) {
    if (nDevices < 1 || !deviceIds || transport < -1 || transport > GRP_RCCL) return 1;
    g_group_env_done = true;     // an explicit call overrides HDSDP_MI355X_GPUS
    // -1: the environment's choice (HDSDP_MI355X_TRANSPORT), else the default -- group_setup reads it
    return group_setup(nDevices, deviceIds, transport);
}
int HMiSetDevices(int nDevices, const int *deviceIds) { return HMiSetDevicesEx(nDevices, deviceIds, -1); }
int HMiGetDeviceGroup(int *deviceIds, int maxIds, int *transport) {
    if (!g_group) { if (transport) *transport = -1; if (deviceIds && maxIds > 0 && g_main.init) deviceIds[0] = g_main.device; return g_main.init ? 1 : 0; }
    for (int r = 0; r < g_group->W && r < maxIds; ++r) if (deviceIds) deviceIds[r] = g_group->dev[r];
    if (transport) *transport = g_group->transport;
    return g_group->W;
}
void HMiSetShardMinDim(int nMin) { if (g_group) g_group->min_n = nMin; }
int HMiConeGetShardCount(hdsdp_cone *cone) {
    return (cone && cone->coneBuildSchur == gc_build_schur) ? ((MiConeGroup *) cone->coneData)->G->W : 1;
}
// the last sharded build's profile of shard `shard` (a plain cone is its own shard 0): see include/hdsdp_mi355x.h for the layout
int HMiConeGetBuildProfile(hdsdp_cone *cone, int shard, double *out, int cap) {
    MiCone *c = nullptr;
    if (cone->coneBuildSchur == gc_build_schur) {
        MiConeGroup *cg = (MiConeGroup *) cone->coneData;
        if (shard < 0 || shard >= (int) cg->shard.size()) return -1;
        c = cg->shard[shard];
    } else {
        if (shard != 0 || cone->coneBuildSchur != cone_build_schur) return -1;
        c = (MiCone *) cone->coneData;
    }
    const MiCone::BuildProfile &pf = c->prof;
    if (!pf.valid) return 0;
    const int need = 8 + 6 * pf.pieces;
    if (!out || cap < need) return -need;
    out[0] = pf.pieces; out[1] = pf.staged; out[2] = pf.invert; out[3] = pf.staged ? pf.step1 : pf.cong;
    out[4] = pf.reduce; out[5] = pf.allreduce_host; out[6] = pf.extract; out[7] = c->world;
    for (int k = 0; k < pf.pieces; ++k) {
        double *o = out + 8 + 6 * k;
        o[0] = pf.step2[k]; o[1] = pf.wait_gpu[k]; o[2] = pf.wait_host[k]; o[3] = pf.gram[k]; o[4] = pf.bytes[k]; o[5] = pf.flight[k];
    }
    return need;
}

void HMiConeGetGroupTraffic(hdsdp_cone *cone, int64_t *bytesAllToAll, int64_t *bytesAllReduce) {
    int64_t a = 0, b = 0;
    if (cone && cone->coneBuildSchur == gc_build_schur) { MiConeGroup *cg = (MiConeGroup *) cone->coneData; a = cg->bytes_a2a; b = cg->bytes_ar; }
    if (bytesAllToAll) *bytesAllToAll = a;
    if (bytesAllReduce) *bytesAllReduce = b;
}
// ---------------------------------------------------------------- fused small-block Phase-A pass (small.hip)
static int small_plan(MiCone *c) {
    MiCone::SmallPlan &sp = c->small;
    if (sp.state) return sp.state;
    sp.state = -1;
    if (c->path != PATH_R1 || c->world != 1 || c->synthetic || c->n > SMALL_P || c->mloc != c->m || c->m > SMALL_P) return -1;
    const int n = c->n, m = c->m;
    std::vector<int> fp(m + 1, 0), fi, dense_of(m, -1), dense_rows;
    std::vector<double> fv, sg(m, 0.0);
    for (int q = 0; q < m; ++q) {
        const MiCoeff &co = c->blk.rows[c->own[q]];
        if (co.type != MI_COEFF_SPR1 && co.type != MI_COEFF_DSR1) return -1;
        int nz = 0;
        for (int r = 0; r < n; ++r) nz += (co.factor[r] != 0.0);
        sg[q] = co.sign;
        if (nz > SMALL_SPMAX) {                       // dense factor: all n entries, in order
            if ((int) dense_rows.size() >= SMALL_NDENSE) return -1;
            dense_of[q] = (int) dense_rows.size();
            dense_rows.push_back(q);
            for (int r = 0; r < n; ++r) { fi.push_back(r); fv.push_back(co.factor[r]); }
        } else {
            for (int r = 0; r < n; ++r) if (co.factor[r] != 0.0) { fi.push_back(r); fv.push_back(co.factor[r]); }
        }
        fp[q + 1] = (int) fi.size();
    }
    dense_rows.resize(SMALL_NDENSE, 0);
    const size_t nf = std::max<size_t>(1, fi.size());
    if (sp.fp.alloc(m + 1) != hipSuccess || sp.fi.alloc(nf) != hipSuccess ||
        sp.fv.alloc(nf) != hipSuccess || sp.sgn.alloc(m) != hipSuccess ||
        sp.dense_of.alloc(m) != hipSuccess ||
        sp.dense_rows.alloc(SMALL_NDENSE) != hipSuccess ||
        sp.io.alloc(7 * (size_t) m + 16, hipHostMallocMapped) != hipSuccess)
        return -1;
    if (hdm_memcpy_h2d_sync(sp.fp.get(), fp.data(), sizeof(int) * (m + 1)) != hipSuccess ||
        (fi.size() && (hdm_memcpy_h2d_sync(sp.fi.get(), fi.data(), sizeof(int) * fi.size()) != hipSuccess ||
                       hdm_memcpy_h2d_sync(sp.fv.get(), fv.data(), sizeof(double) * fv.size()) != hipSuccess)) ||
        hdm_memcpy_h2d_sync(sp.sgn.get(), sg.data(), sizeof(double) * m) != hipSuccess ||
        hdm_memcpy_h2d_sync(sp.dense_of.get(), dense_of.data(), sizeof(int) * m) != hipSuccess ||
        hdm_memcpy_h2d_sync(sp.dense_rows.get(), dense_rows.data(), sizeof(int) * SMALL_NDENSE) != hipSuccess)
        return -1;
    sp.ndense = 0;
    for (int q = 0; q < m; ++q) sp.ndense += (dense_of[q] >= 0);
    sp.state = 1;
    return 1;
}

int HMiKKTPhaseAEligible(hdsdp_kkt *HKKT) {
    if (!HKKT || HKKT->nCones != 1 || priv_of(HKKT)->st.form() != HDM_KKT_DENSE) return 0;
    hdsdp_cone *hc = HKKT->cones[0];
    if (hc->coneBuildSchur != cone_build_schur) return 0;
    MiCone *c = (MiCone *) hc->coneData;
    return (c->m == HKKT->nRow && small_plan(c) == 1) ? 1 : 0;
}

hdsdp_retcode HMiKKTPhaseA(hdsdp_kkt *HKKT, double barHsdTau, double *rowDual, double *rhs, double *d1, double *d2, double *d3,
                           int *isInterior, double *logdet) {
    StatScope stat_(ST_BUILD_M, __func__);
    if (!HMiKKTPhaseAEligible(HKKT)) return HDSDP_RETCODE_FAILED;
    MiCone *c = (MiCone *) HKKT->cones[0]->coneData;
    MiCone::SmallPlan &sp = c->small;
    MiKKTPriv *pv = priv_of(HKKT);
    MiLin *ls = (MiLin *) c->dualFactor->chol, *lm = (MiLin *) HKKT->kktM->chol;
    const int m = c->m, n = c->n;
    HIP_RC(hipStreamSynchronize(g.stream));            // the mapped block is about to be rewritten
    double *yin = sp.io.get(), *bin = sp.io.get() + m, *out = sp.io.get() + 2 * (size_t) m;
    for (int i = 0; i < m; ++i) { yin[i] = rowDual ? rowDual[i] : 0.0; bin[i] = rhs ? rhs[i] : 0.0; }
    out[0] = -1.0;
    HdmSmallArgs a = {};
    a.n = n; a.m = m; a.C = c->Cfull.get(); a.ldc = c->n16;
    a.fp = sp.fp.get(); a.fi = sp.fi.get(); a.fv = sp.fv.get(); a.sgn = sp.sgn.get(); a.dense_of = sp.dense_of.get(); a.ndense = sp.ndense; a.dense_rows = sp.dense_rows.get();
    a.y = sp.io.dev(); a.b = sp.io.dev() + m; a.out = sp.io.dev() + 2 * (size_t) m;
    a.tau = barHsdTau; a.eye = cone_eye(c); a.Rd = c->Rd;
    a.Sout = c->S.get(); a.lds = c->n16;
    c->dual.S_overwritten();                           // (the pass writes S itself)
    a.LS = ls->ch.L.get(); a.WS = ls->ch.Dinv.get(); a.M = lm->Mdev.get(); a.ldm = lm->ch.npad; a.LM = lm->ch.L.get(); a.WM = lm->ch.Dinv.get();
    if (ls->ch.npad != SMALL_P || lm->ch.npad != SMALL_P) return HDSDP_RETCODE_FAILED;
    // (the operator's accumulators as HKKTBuildUp(KKT_TYPE_INFEASIBLE) leaves them, hdsdp_schur.c:141-165, :256-268: the
    // kernel itself zeroes what it does not fill of the 128 x 128 device matrix)
    // (the build starts an empty diagonal channel -- the stream is idle, the pinned channel is free to write)
    kkt_channel_start(HKKT, pv, KKT_TYPE_INFEASIBLE);
    RC(hdm_small_phase_a(a, g.stream));
    if (pv->st.mirror()) {
        HIP_RC(hipMemcpy2DAsync(HKKT->kktMatElem, sizeof(double) * m, lm->Mdev.get(), sizeof(double) * SMALL_P, sizeof(double) * m, m,
                                hipMemcpyDeviceToHost, g.stream));
        pv->bytes_d2h += (int64_t) sizeof(double) * m * m;
    }
    HIP_RC(hipStreamSynchronize(g.stream));
    const int infoS = (int) out[0], infoM = (int) out[1];
    ls->ch.factored = (infoS == 0); ls->ch.have_inv = false;
    c->dualFactor->nFactorizes += 1;
    if (isInterior) *isInterior = (infoS == 0);
    if (infoS != 0) return HDSDP_RETCODE_OK;           // "not positive definite" is a value, not an error
    if (logdet) *logdet = out[2];
    memset(HKKT->dASinvVec, 0, sizeof(double) * m); memset(HKKT->dASinvRdSinvVec, 0, sizeof(double) * m);
    for (int i = 0; i < m; ++i) { HKKT->dASinvVec[i] = out[4 + i]; HKKT->dASinvRdSinvVec[i] = out[4 + m + i]; }
    HKKT->dTraceSinv = (c->Rd != 0.0) ? out[3] : 0.0;
    pv->st.small_pass_done(lm->Mdev.get(), SMALL_P);
    lm->ch.factored = (infoM == 0); lm->ch.have_inv = false;
    HKKT->kktM->nFactorizes += 1;
    if (infoM != 0) {
        // the Schur matrix is not numerically positive definite: the multi-launch path's way out (pivoted solver) takes over
        fprintf(stderr, "[hdsdp_mi355x] HMiKKTPhaseA: Schur matrix is not positive definite (pivot %d); solving through HKKTFactorize\n", infoM);
        if (HKKTFactorize(HKKT) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
        if (d1 && HKKTSolve(HKKT, rhs, d1) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
        if (d2 && HKKTSolve(HKKT, HKKT->dASinvVec, d2) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
        if (d3 && HKKTSolve(HKKT, HKKT->dASinvRdSinvVec, d3) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
        return HDSDP_RETCODE_OK;
    }
    HKKT->kktM->nSolves += 3;
    if (d1) memcpy(d1, out + 4 + 2 * (size_t) m, sizeof(double) * m);
    if (d2) memcpy(d2, out + 4 + 3 * (size_t) m, sizeof(double) * m);
    if (d3) memcpy(d3, out + 4 + 4 * (size_t) m, sizeof(double) * m);
    const double *stamp = out + 4 + 5 * (size_t) m;
    for (int i = 0; i < 6; ++i) g.stage_ms[i] = (stamp[i + 1] - stamp[i]) * 1e-5;   // HMiGetStageTimes: 100 MHz ticks -> ms
    g.stage_ms[6] = (stamp[6] > stamp[0]) ? stamp[7] / ((stamp[6] - stamp[0]) * 10.0) : 0.0;   // shader clock during the pass, GHz
    return HDSDP_RETCODE_OK;
}

// host only (no device call): the reverse Cuthill-McKee order HKKTInit looks at for a sparse Schur pattern; lower-triangular CSC in,
// perm[old] = new out
int HMiRcmOrder(int m, const int *colBeg, const int *rowIdx, int *perm) {
    if (m <= 0 || !colBeg || !rowIdx || !perm) return 1;
    std::vector<int> beg(colBeg, colBeg + m + 1), idx(rowIdx, rowIdx + colBeg[m]);
    const std::vector<int> p = hdm_rcm_order(m, beg, idx);
    for (int i = 0; i < m; ++i) perm[i] = p[i];
    return 0;
}

// host only (no device call): the tile form's symbolic phase (HdmBsp::symbolic) on a lower-triangular CSC pattern.  perm[old] = new;
// stats[0..4] = block rows, tiles of the factor, levels, rows sent to the dense tail, update source pairs; blockPtr (nb + 1) and
// blockRow (ntiles) = the factor's block pattern by block column, lower with the diagonal first.  Any output may be NULL: a first
// call with blockPtr = blockRow = NULL sizes them through stats.  Returns what HdmBsp::init would for the pattern (1: no tile form).
int HMiBspSymbolic(int m, const int *colBeg, const int *rowIdx, double maxFraction, int *perm, int *stats, int *blockPtr, int *blockRow) {
    if (m <= 0 || !colBeg || !rowIdx) return 1;
    HdmBsp bs;
    HdmBspLists ls;
    const int rc = bs.symbolic(m, colBeg, rowIdx, maxFraction, ls);
    if (stats) { stats[0] = bs.nb; stats[1] = bs.ntiles; stats[2] = bs.nlevels; stats[3] = ls.tail_rows; stats[4] = (int) ls.src.size(); }
    if (rc) return rc;
    if (perm) for (int i = 0; i < m; ++i) perm[i] = bs.perm[i];
    if (blockPtr) for (int k = 0; k <= bs.nb; ++k) blockPtr[k] = bs.bptr[k];
    if (blockRow) for (int q = 0; q < bs.ntiles; ++q) blockRow[q] = bs.brow[q];
    return 0;
}

// how the operator's matrix will be factored: *permuted = 1 if the factor object holds P M P' (reverse Cuthill-McKee order of
// the sparse pattern), *fraction = blocks inside the pattern's block envelope / blocks of the dense lower triangle (1 = dense)
int HMiKKTTileInfo(hdsdp_kkt *HKKT, int *tiles, int64_t *denseTiles, int *levels, int64_t *bytes) {
    if (tiles) *tiles = 0;
    if (denseTiles) *denseTiles = 0;
    if (levels) *levels = 0;
    if (bytes) *bytes = 0;
    if (!HKKT || !HKKT->kktM) return 0;
    MiLin *l = (MiLin *) HKKT->kktM->chol;
    if (!l->bsp) return 0;
    if (tiles) *tiles = l->bsp->ntiles;
    if (denseTiles) *denseTiles = l->bsp->dense_tiles();
    if (levels) *levels = l->bsp->nlevels;
    if (bytes) *bytes = (int64_t) l->bsp->bytes();
    return 1;
}
int HMiKKTNegativePivots(hdsdp_kkt *HKKT) {
    if (!HKKT || !HKKT->kktM) return -1;
    MiLin *l = (MiLin *) HKKT->kktM->chol;
    return (l->bsp && l->bsp->factored) ? l->bsp->negative : -1;
}
int HMiBspSolve(int m, const int *colBeg, const int *rowIdx, const double *val, const double *b, double *x, int *info, int *stats,
                double *ms) {
    if (ensure_ctx()) return 1;
    HdmBsp bs;
    int rc = 1;
    HdmBuf<int> rows_d, cols_d;   // (declared after bs: freed before it, as ever)
    HdmBuf<double> vals_d;
    do {
        if (bs.init(m, colBeg, rowIdx, 1.0)) break;
        const long nnz = colBeg[m];
        std::vector<int> cols((size_t) nnz);
        for (int c = 0; c < m; ++c) for (int q = colBeg[c]; q < colBeg[c + 1]; ++q) cols[q] = c;
        if (rows_d.alloc(nnz) != hipSuccess || cols_d.alloc(nnz) != hipSuccess ||
            vals_d.alloc(nnz) != hipSuccess) break;
        if (hipMemcpy(rows_d.get(), rowIdx, sizeof(int) * nnz, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(cols_d.get(), cols.data(), sizeof(int) * nnz, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(vals_d.get(), val, sizeof(double) * nnz, hipMemcpyHostToDevice) != hipSuccess) break;
        hipLaunchKernelGGL(mi_csc_scatter_kernel, dim3((unsigned) ((nnz + 255) / 256)), dim3(256), 0, g.stream, bs.view_M(), rows_d.get(), cols_d.get(), nnz, vals_d.get());
        int inf = 0;
        const int reps = ms ? 3 : 1;
        float best = 1e30f;
        bool bad = false;
        for (int r = 0; r < reps && !bad; ++r) {
            if (bs.load_M(g.stream)) { bad = true; break; }
            (void) hipEventRecord(g.ev[6], g.stream);
            if (bs.factor(g.stream, &inf)) { bad = true; break; }
            (void) hipEventRecord(g.ev[7], g.stream);
            (void) hipEventSynchronize(g.ev[7]);
            float e = 0.f;
            (void) hipEventElapsedTime(&e, g.ev[6], g.ev[7]);
            best = std::min(best, e);
        }
        if (bad) break;
        if (info) *info = inf;
        if (ms) *ms = best;
        if (stats) { stats[0] = bs.nb; stats[1] = bs.ntiles; stats[2] = bs.nlevels; stats[3] = bs.negative; }
        if (inf == 0 && b && x && bs.solve_host(b, x, g.stream)) break;
        rc = 0;
    } while (0);
    return rc;
}
// the CSC values of a host matrix scattered into the accumulation store of a stand-alone tile object (what HMiBspSolve does)
static int bsp_probe_scatter(HdmBsp &bs, int m, const int *colBeg, const int *rowIdx, const double *val) {
    const long nnz = colBeg[m];
    std::vector<int> cols((size_t) nnz);
    for (int c = 0; c < m; ++c) for (int q = colBeg[c]; q < colBeg[c + 1]; ++q) cols[q] = c;
    HdmBuf<int> rows_d, cols_d;
    HdmBuf<double> vals_d;
    if (rows_d.alloc(nnz) != hipSuccess || cols_d.alloc(nnz) != hipSuccess || vals_d.alloc(nnz) != hipSuccess) return 1;
    if (hipMemcpy(rows_d.get(), rowIdx, sizeof(int) * nnz, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(cols_d.get(), cols.data(), sizeof(int) * nnz, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(vals_d.get(), val, sizeof(double) * nnz, hipMemcpyHostToDevice) != hipSuccess) return 1;
    hipLaunchKernelGGL(mi_csc_scatter_kernel, dim3((unsigned) ((nnz + 255) / 256)), dim3(256), 0, g.stream, bs.view_M(), rows_d.get(), cols_d.get(), nnz, vals_d.get());
    return (hipGetLastError() != hipSuccess || hipStreamSynchronize(g.stream) != hipSuccess) ? 1 : 0;   // (the buffers go with this scope)
}
// The tile form's residual kernel (refine.hip: HdmBspRefine::residual) on a host matrix: r = b - M x and |r|_2^2 with x, b and r in
// the driver's order.  Before the values are scattered, every padding row and column of the last block row and the whole trash tile
// are filled with NaN: a kernel that read any of them would return it.
int HMiTileResidualProbe(int m, const int *colBeg, const int *rowIdx, const double *val, const double *x, const double *b, double *r, double *norm2) {
    if (m < 1 || !colBeg || !rowIdx || !val || !x || !b || !r || !norm2 || ensure_ctx()) return 1;
    HdmBsp bs;
    HdmBspRefine t;
    if (bs.init(m, colBeg, rowIdx, 1.0) || bs.zero_M(g.stream) || hipStreamSynchronize(g.stream) != hipSuccess) return 1;
    const int first_pad = m - (bs.nb - 1) * 128;               // rows (and, in the diagonal tile, columns) of the last block from here on
    std::vector<double> img(16384);
    for (int k = 0; k < bs.nb; ++k)
        for (int q = bs.bptr[k]; q < bs.bptr[k + 1]; ++q) {
            if (bs.brow[q] != bs.nb - 1 || first_pad >= 128) continue;
            for (int c = 0; c < 128; ++c)
                for (int i = 0; i < 128; ++i) img[(size_t) i + 128 * (size_t) c] = (i >= first_pad || (k == bs.nb - 1 && c >= first_pad)) ? NAN : 0.0;
            if (hipMemcpy(bs.Mval.get() + ((size_t) q << 14), img.data(), sizeof(double) * 16384, hipMemcpyHostToDevice) != hipSuccess) return 1;
        }
    std::fill(img.begin(), img.end(), NAN);
    if (hipMemcpy(bs.Mval.get() + ((size_t) bs.ntiles << 14), img.data(), sizeof(double) * 16384, hipMemcpyHostToDevice) != hipSuccess) return 1;
    if (bsp_probe_scatter(bs, m, colBeg, rowIdx, val) || t.prepare(bs)) return 1;
    double *B = t.vec(0), *X = t.vec(1), *R = t.vec(4), *T = t.vec(5), *nrm = t.vec(6);
    if (hipMemsetAsync(B, 0, sizeof(double) * 2 * (size_t) t.len, g.stream) != hipSuccess ||
        hipMemcpyAsync(T, b, sizeof(double) * (size_t) m, hipMemcpyHostToDevice, g.stream) != hipSuccess ||
        hdm_refine_scatter(B, T, bs.perm_dev.get(), m, g.stream) ||
        hipMemcpyAsync(T, x, sizeof(double) * (size_t) m, hipMemcpyHostToDevice, g.stream) != hipSuccess ||
        hdm_refine_scatter(X, T, bs.perm_dev.get(), m, g.stream)) return 1;
    if (t.residual(bs.Mval.get(), X, B, R, nrm, g.stream) || hdm_refine_gather(T, R, bs.perm_dev.get(), m, 0, g.stream)) return 1;
    if (hipMemcpyAsync(r, T, sizeof(double) * (size_t) m, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
        hipMemcpyAsync(norm2, nrm, sizeof(double), hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
        hipStreamSynchronize(g.stream) != hipSuccess) return 1;
    return 0;
}
// The production refined solve of the tile form on a host matrix: scatter, load_M, factor, then lin_refine_column over the
// stand-alone object, its residual reading the accumulation store.  *info as HMiBspSolve; with a zero pivot nothing is solved.
// status .. tol as HMiLinsysGetRefine reports them; stats[0..3] = block rows, tiles stored, levels, negative pivots.
int HMiBspRefinedSolve(int m, const int *colBeg, const int *rowIdx, const double *val, const double *b, double *x, int maxSteps, double relTol,
                       double absTol, int *info, int *status, int *steps, double *resid0, double *resid, double *tol, int *stats) {
    if (m < 1 || !colBeg || !rowIdx || !val || !b || !x || ensure_ctx()) return 1;
    HdmBsp bs;
    HdmBspRefine t;
    int inf = 0;
    if (bs.init(m, colBeg, rowIdx, 1.0) || bsp_probe_scatter(bs, m, colBeg, rowIdx, val) || bs.load_M(g.stream) || bs.factor(g.stream, &inf)) return 1;
    if (info) *info = inf;
    if (stats) { stats[0] = bs.nb; stats[1] = bs.ntiles; stats[2] = bs.nlevels; stats[3] = bs.negative; }
    if (inf != 0) return 0;
    if (t.prepare(bs)) return 1;
    HdmRefineStats rf;
    LinRefineTiles form(bs, t, bs.Mval.get());
    if (lin_refine_column(form, m, maxSteps, relTol, absTol, b, x, rf) != HDSDP_RETCODE_OK) return 1;
    if (status) *status = rf.status;
    if (steps) *steps = rf.steps;
    if (resid0) *resid0 = rf.resid0;
    if (resid) *resid = rf.resid;
    if (tol) *tol = rf.tol;
    return 0;
}
// What the tile form's refined solve costs beside the unrefined one (tools/refine_tiles_timing.py): one factorisation, then the
// nVariants variants alternate solve by solve, warmup + reps rounds, host clock around each solve (every one ends in a stream
// synchronisation).  Variant v: caps[v] < 0 = HdmBsp::solve_host, the unrefined solve; otherwise the refined solve with that cap
// under relTols[v] / absTols[v].  ms[v * reps + r]; corrections[v] = correction solves over the timed rounds; status[v] and
// resid[2 v], resid[2 v + 1] (|r_0|, |r|) of the last one; stats as HMiBspSolve; *workBytes = what the refined solve allocated.
int HMiBspRefineTimingProbe(int m, const int *colBeg, const int *rowIdx, const double *val, const double *b, int nVariants, const int *caps,
                            const double *relTols, const double *absTols, int warmup, int reps, double *ms, int *corrections, int *status,
                            double *resid, int *stats, int64_t *workBytes) {
    if (m < 1 || !colBeg || !rowIdx || !val || !b || nVariants < 1 || !caps || !relTols || !absTols || warmup < 0 || reps < 1 || !ms || ensure_ctx())
        return 1;
    HdmBsp bs;
    HdmBspRefine t;
    int inf = 0;
    if (bs.init(m, colBeg, rowIdx, 1.0) || bsp_probe_scatter(bs, m, colBeg, rowIdx, val) || bs.load_M(g.stream) || bs.factor(g.stream, &inf)) return 1;
    if (stats) { stats[0] = bs.nb; stats[1] = bs.ntiles; stats[2] = bs.nlevels; stats[3] = bs.negative; }
    if (inf != 0 || t.prepare(bs)) return 1;
    if (workBytes) *workBytes = (int64_t) t.bytes();
    std::vector<double> x((size_t) m);
    std::vector<HdmRefineStats> rf((size_t) nVariants);
    if (corrections) std::fill(corrections, corrections + nVariants, 0);
    LinRefineTiles form(bs, t, bs.Mval.get());
    for (int r = -warmup; r < reps; ++r)
        for (int v = 0; v < nVariants; ++v) {
            const int64_t before = rf[(size_t) v].total_steps;
            const auto t0 = std::chrono::steady_clock::now();
            if (caps[v] < 0) { if (bs.solve_host(b, x.data(), g.stream)) return 1; }
            else if (lin_refine_column(form, m, caps[v], relTols[v], absTols[v], b, x.data(), rf[(size_t) v]) != HDSDP_RETCODE_OK) return 1;
            const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (r < 0) continue;
            ms[(size_t) v * reps + r] = dt;
            if (corrections) corrections[v] += (int) (rf[(size_t) v].total_steps - before);
        }
    for (int v = 0; v < nVariants; ++v) {
        if (status) status[v] = rf[(size_t) v].status;
        if (resid) { resid[2 * v] = rf[(size_t) v].resid0; resid[2 * v + 1] = rf[(size_t) v].resid; }
    }
    return 0;
}
void HMiKKTEnvelopeInfo(hdsdp_kkt *HKKT, int *permuted, double *fraction) {
    if (permuted) *permuted = 0;
    if (fraction) *fraction = 1.0;
    if (!HKKT || !HKKT->kktM) return;
    MiLin *l = (MiLin *) HKKT->kktM->chol;
    if (l->bsp) { if (permuted) *permuted = 1; if (fraction) *fraction = (double) l->bsp->ntiles / (double) l->bsp->dense_tiles(); return; }
    if (permuted) *permuted = l->perm.empty() ? 0 : 1;
    if (fraction && !l->ch.env_colh.empty()) {
        double in = 0.0, all = 0.0;
        for (int k = 0; k < l->ch.nblk; ++k) { in += l->ch.env_colh[k] - k + 1; all += l->ch.nblk - k; }
        *fraction = in / all;
    }
}

int HMiGetCallStats(double *seconds, int64_t *calls, int n) {
    for (int k = 0; k < n && k < ST_N; ++k) { if (seconds) seconds[k] = g_stat_sec[k]; if (calls) calls[k] = g_stat_calls[k]; }
    return ST_N;
}
const char *HMiCallStatName(int k) { return (k >= 0 && k < ST_N) ? g_stat_name[k] : ""; }
int HMiGetAssembleCounts(int64_t *counts, int n) {
    for (int k = 0; k < n && k < HDM_ASM_N; ++k) if (counts) counts[k] = g_asm_counts[k].load(std::memory_order_relaxed);
    return HDM_ASM_N;
}
void HMiResetCallStats(void) { for (int k = 0; k < ST_N; ++k) { g_stat_sec[k] = 0.0; g_stat_calls[k] = 0; } g_stat_nfn = 0; }
int HMiRcclSelfTest(int device) {
    if (ensure_ctx()) return 1;
    const int d = device < 0 ? g_main.device : device;
    return rccl_group_self_test(1, &d, 60000);
}
int HMiRcclGroupSelfTest(int nDevices, const int *deviceIds, int timeoutMs) {
    if (nDevices < 1 || !deviceIds) return 1;
    return rccl_group_self_test(nDevices, deviceIds, timeoutMs);
}
