// engine_kkt.h -- exported C ABI, first part: utilities, HFpLinsys* and HKKT* (dense and sparse Schur operator, RCM order, host mirror, row access)
// Implementation header of engine.hip: included exactly once, there, in this order (inside extern "C"); split out of a 3 300-line file in round 3, nothing else changed.
// The rules about the operator's matrix live in kkt_store.h: how it is stored (HdmKktForm), what state it is in (HdmKktState, one
// transition per writer), and how it reaches the factor (hdm_kkt_load_plan, whose comment is the table of all cases).  This file
// performs them: HKKTInit is a sequence of steps, HKKTFactorize gets the plan, stages, commits and loads.

const char *HMiVersion(void) { return "hdsdp-mi355x 0.1 (gfx950, fp64 MFMA)"; }

int HMiDeviceInit(int device) {
    if (g.init) return 0;
    if (device >= 0) {
        char buf[16];
        snprintf(buf, sizeof(buf), "%d", device);
        setenv("LOCAL_RANK", buf, 0);
    }
    return ensure_ctx();
}
int HMiDeviceSynchronize(void) {
    if (ensure_ctx()) return 1;
    HDM_HIP_CHECK(hipStreamSynchronize(g.stream));
    return 0;
}
void *HMiStream(void) { return ensure_ctx() ? nullptr : (void *) g.stream; }
void HMiSetKernelTiming(int on) { hdm_timing_enable(on); }
void HMiSetDebugBuffer(void *dev, int role) { hdm_set_debug_buffer((unsigned long long *) dev, role); }
int HMiGetKernelTiming(double *ms, double *flops, int64_t *launches) {
    long l[HDM_NROLES];
    if (hdm_timing_collect(ms, flops, l)) return 1;
    for (int r = 0; r < HDM_NROLES; ++r) launches[r] = l[r];
    return 0;
}
int HMiGetKernelTimingEx(double *ms, double *flops, double *issued, int64_t *launches) {
    long l[HDM_NROLES];
    if (hdm_timing_collect(ms, flops, l, issued)) return 1;
    for (int r = 0; r < HDM_NROLES; ++r) launches[r] = l[r];
    return 0;
}
void HMiGetStageTimes(double *ms, int n) {
    for (int i = 0; i < n && i < 8; ++i) ms[i] = g.stage_ms[i];
}

// ---------------------------------------------------------------- HFpLinsys*
// the eleven slots of the reference's linear-system vtable (hdsdp_linsolver.h): every object of the engine has the same ones
static void lin_fill_vtable(hdsdp_linsys_fp *h, int nCol, linsys_type Ltype) {
    h->nCol = nCol; h->LinType = Ltype;
    h->cholCreate = lin_create; h->cholSetParam = lin_setparam; h->cholSymbolic = lin_symbolic; h->cholNumeric = lin_numeric;
    h->cholPsdCheck = lin_psdcheck; h->cholFSolve = lin_fsolve; h->cholBSolve = lin_bsolve; h->cholSolve = lin_solve;
    h->cholGetDiag = lin_getdiag; h->cholInvert = lin_invert; h->cholDestroy = lin_destroy;
}
hdsdp_retcode HFpLinsysCreate(hdsdp_linsys_fp **pHLin, int nCol, linsys_type Ltype) {
    if (!pHLin) return HDSDP_RETCODE_FAILED;
    switch (Ltype) {
        case HDSDP_LINSYS_DENSE_DIRECT:
        case HDSDP_LINSYS_DENSE_ITERATIVE:  // Schur system: a direct blocked Cholesky in place of the reference's PCG to 1e-12
            break;                          // (hdsdp_linsolver.c:1446-1588); HMiLinsysSetRefine iterates on the true residual
        case HDSDP_LINSYS_SPARSE_DIRECT:    // sparse dual matrix: CSC in, dense factorisation on the device (see MiLin)
            break;
        default:
            fprintf(stderr, "[hdsdp_mi355x] HFpLinsysCreate: linsys_type %d is not on the accelerated path "
                            "(sparse indefinite / iterative backends stay with the CPU reference; DENSE_INDEFINITE is only reached by switching)\n", (int) Ltype);
            return HDSDP_RETCODE_FAILED;
    }
    hdsdp_linsys_fp *h = (hdsdp_linsys_fp *) calloc(1, sizeof(hdsdp_linsys_fp));
    if (!h) return HDSDP_RETCODE_MEMORY;
    lin_fill_vtable(h, nCol, Ltype);
    hdsdp_retcode rc = h->cholCreate(&h->chol, nCol);
    if (rc != HDSDP_RETCODE_OK) { free(h); return rc; }
    ((MiLin *) h->chol)->type = Ltype;
    ((MiLin *) h->chol)->csc_in = (Ltype == HDSDP_LINSYS_SPARSE_DIRECT);
    *pHLin = h;
    return HDSDP_RETCODE_OK;
}
void HFpLinsysSetParam(hdsdp_linsys_fp *HLin, double relTol, double absTol, int nThreads, int maxIter, int nRestartFreq) {
    (void) nThreads; (void) nRestartFreq;
    MiLin *l = (MiLin *) HLin->chol;
    // the refined solve's tolerance (refine_rule.h: hdm_refine_tol; values <= 0 take the reference's defaults); the direct solve
    // itself needs none, and maxIter is recorded only: the step cap is HMiLinsysSetRefine's
    l->relTol = relTol; l->absTol = absTol; l->maxIter = maxIter;
}
// the refined solve (refine_rule.h): 0 = off (the default), else the step cap, clamped to 8
int HMiLinsysSetRefine(hdsdp_linsys_fp *HLin, int maxSteps) {
    if (!HLin || !HLin->chol) return 1;
    MiLin *l = (MiLin *) HLin->chol;
    l->st->refine_set(maxSteps);
    if (l->st->refine() == 0) { l->rf.release(); l->rf.unrefined(HDM_REFINE_OFF); }
    return 0;
}
int HMiLinsysGetRefine(hdsdp_linsys_fp *HLin, int *status, int *steps, double *resid0, double *resid, double *tol, int64_t *solves,
                       int64_t *totalSteps) {
    if (!HLin || !HLin->chol) return -1;
    const MiLin *l = (const MiLin *) HLin->chol;
    if (status) *status = l->rf.status;
    if (steps) *steps = l->rf.steps;
    if (resid0) *resid0 = l->rf.resid0;
    if (resid) *resid = l->rf.resid;
    if (tol) *tol = l->rf.tol;
    if (solves) *solves = l->rf.solves;
    if (totalSteps) *totalSteps = l->rf.total_steps;
    return l->st->refine();
}
int64_t HMiLinsysRefineBytes(hdsdp_linsys_fp *HLin) { return (HLin && HLin->chol) ? ((const MiLin *) HLin->chol)->rf.bytes() : 0; }
int HMiKKTSetRefine(hdsdp_kkt *HKKT, int maxSteps) { return (HKKT && HKKT->kktM) ? HMiLinsysSetRefine(HKKT->kktM, maxSteps) : 1; }
// the tile form's own switch on top of the step cap (kkt_store.h): a tile operator is refined only with both on before HKKTFactorize
int HMiLinsysSetRefineTiles(hdsdp_linsys_fp *HLin, int on) {
    if (!HLin || !HLin->chol) return 1;
    MiLin *l = (MiLin *) HLin->chol;
    l->st->refine_tiles_set(on != 0);
    if (!on) l->rf.tiles.release();
    return 0;
}
int HMiLinsysGetRefineTiles(hdsdp_linsys_fp *HLin) { return (HLin && HLin->chol) ? (((const MiLin *) HLin->chol)->st->refine_tiles() ? 1 : 0) : -1; }
int HMiKKTSetRefineTiles(hdsdp_kkt *HKKT, int on) { return (HKKT && HKKT->kktM) ? HMiLinsysSetRefineTiles(HKKT->kktM, on) : 1; }
hdsdp_retcode HFpLinsysSymbolic(hdsdp_linsys_fp *HLin, int *colMatBeg, int *colMatIdx) {
    return HLin->cholSymbolic(HLin->chol, colMatBeg, colMatIdx);
}
hdsdp_retcode HFpLinsysNumeric(hdsdp_linsys_fp *HLin, int *colMatBeg, int *colMatIdx, double *colMatElem) {
    StatScope stat_(ST_LINSYS, __func__);
    // hdsdp_linsolver.c:2029-2044: a failed factorisation of the Schur system switches to the indefinite solver
    HLin->nFactorizes += 1;
    hdsdp_retcode rc = HLin->cholNumeric(HLin->chol, colMatBeg, colMatIdx, colMatElem);
    if (rc == HDSDP_RETCODE_FAILED && HLin->LinType == HDSDP_LINSYS_DENSE_ITERATIVE) {
        fprintf(stderr, "[hdsdp_mi355x] KKT system is almost indefinite. Switch to the pivoted (LDL-equivalent) solver.\n");
        rc = lin_switch_indefinite(HLin);
    }
    return rc;
}
hdsdp_retcode HFpLinsysSwitchToBackUp(hdsdp_linsys_fp *HLin) { (void) HLin; return HDSDP_RETCODE_OK; }
hdsdp_retcode HFpLinsysPsdCheck(hdsdp_linsys_fp *HLin, int *colMatBeg, int *colMatIdx, double *colMatElem, int *isPsd) {
    StatScope stat_(ST_LINSYS, __func__);
    HLin->nFactorizes += 1;
    return HLin->cholPsdCheck(HLin->chol, colMatBeg, colMatIdx, colMatElem, isPsd);
}
void HFpLinsysFSolve(hdsdp_linsys_fp *HLin, int nRhs, double *rhsVec, double *solVec) {
    StatScope stat_(ST_LINSYS, __func__);
    HLin->nSolves += 1;
    HLin->cholFSolve(HLin->chol, nRhs, rhsVec, solVec);
}
void HFpLinsysBSolve(hdsdp_linsys_fp *HLin, int nRhs, double *rhsVec, double *solVec) {
    StatScope stat_(ST_LINSYS, __func__);
    HLin->nSolves += 1;
    HLin->cholBSolve(HLin->chol, nRhs, rhsVec, solVec);
}
hdsdp_retcode HFpLinsysSolve(hdsdp_linsys_fp *HLin, int nRhs, double *rhsVec, double *solVec) {
    StatScope stat_(ST_LINSYS, __func__);
    // hdsdp_linsolver.c:2085-2110: NaN in the solution (or the right-hand side) counts as a failure, and a failed solve
    // of the Schur system switches to the indefinite solver and solves again
    hdsdp_retcode rc = HLin->cholSolve(HLin->chol, nRhs, rhsVec, solVec);
    if (solVec && solVec[0] != solVec[0]) rc = HDSDP_RETCODE_FAILED;
    if (rhsVec[0] != rhsVec[0]) rc = HDSDP_RETCODE_FAILED;
    if (rc != HDSDP_RETCODE_OK && HLin->LinType == HDSDP_LINSYS_DENSE_ITERATIVE) {
        fprintf(stderr, "[hdsdp_mi355x] KKT system is unstable. Switch to the pivoted (LDL-equivalent) solver.\n");
        if (lin_switch_indefinite(HLin) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
        return HFpLinsysSolve(HLin, nRhs, rhsVec, solVec);
    }
    HLin->nSolves += 1;
    return rc;
}
hdsdp_retcode HFpLinsysGetDiag(hdsdp_linsys_fp *HLin, double *diagElem) { return HLin->cholGetDiag(HLin->chol, diagElem); }
void HFpLinsysInvert(hdsdp_linsys_fp *HLin, double *dFullMatrix, double *dAuxiMatrix) {
    StatScope stat_(ST_LINSYS, __func__);
    HLin->cholInvert(HLin->chol, dFullMatrix, dAuxiMatrix);
}
void HFpLinsysClear(hdsdp_linsys_fp *HLin) {
    if (!HLin) return;
    if (HLin->cholDestroy) HLin->cholDestroy(&HLin->chol);
    memset(HLin, 0, sizeof(hdsdp_linsys_fp));
}
void HFpLinsysDestroy(hdsdp_linsys_fp **pHLin) {
    if (!pHLin || !*pHLin) return;
    HFpLinsysClear(*pHLin);
    free(*pHLin);
    *pHLin = nullptr;
}

// ---------------------------------------------------------------- HKKT*
hdsdp_retcode HKKTCreate(hdsdp_kkt **pHKKT) {
    if (!pHKKT) return HDSDP_RETCODE_FAILED;
    hdsdp_kkt *k = (hdsdp_kkt *) calloc(1, sizeof(hdsdp_kkt));
    if (!k) return HDSDP_RETCODE_MEMORY;
    *pHKKT = k;
    return HDSDP_RETCODE_OK;
}

// a linear-system object for a sparse Schur operator in TILE form: the same vtable, no dense factor behind it
static hdsdp_retcode linsys_create_tiles(hdsdp_linsys_fp **pHLin, int nCol, std::unique_ptr<HdmBsp> bsp) {
    hdsdp_linsys_fp *h = (hdsdp_linsys_fp *) calloc(1, sizeof(hdsdp_linsys_fp));
    if (!h) return HDSDP_RETCODE_MEMORY;
    lin_fill_vtable(h, nCol, HDSDP_LINSYS_SPARSE_DIRECT);
    MiLin *l = new MiLin();
    l->n = nCol; l->type = HDSDP_LINSYS_SPARSE_DIRECT; l->csc_in = true; l->bsp = std::move(bsp);
    h->chol = l;
    *pHLin = h;
    return HDSDP_RETCODE_OK;
}

// ---- HKKTInit's steps.  The rules they perform (sparse or dense, envelope and order, the five switches) are kkt_store.h's.
// An LP cone builds on the caller's device and stream into the operator's matrix; a device-group cone's shards build on worker
// threads and devices of their own (group_impl.h: grun), with no ordering against the caller's stream that the LP cone's
// accumulation could rely on.  The two are not combined in one operator.
static bool kkt_cones_combine(int nCones, hdsdp_cone **cones) {
    bool lp = false, grp = false;
    for (int i = 0; i < nCones; ++i) { lp = lp || cones[i]->coneBuildSchur == lp_build_schur; grp = grp || cones[i]->coneBuildSchur == gc_build_schur; }
    if (lp && grp) fprintf(stderr, "[hdsdp_mi355x] HKKTInit: an LP cone cannot share an operator with a device-group (sharded) cone\n");
    return !(lp && grp);
}

// the reference struct's host fields (hdsdp_schur.c:181-254)
static hdsdp_retcode kkt_init_host_fields(hdsdp_kkt *HKKT, int nRow, int nCones, hdsdp_cone **cones) {
    HKKT->nRow = nRow;
    HKKT->nCones = nCones;
    HKKT->cones = cones;
    int maxDim = 0;
    for (int i = 0; i < nCones; ++i) maxDim = std::max(maxDim, cones[i]->coneGetDim(cones[i]->coneData));
    HKKT->maxConeDim = maxDim;
    const size_t nn = (size_t) maxDim * maxDim;
    HKKT->invBuffer = (double *) calloc(nn, sizeof(double));
    HKKT->kktBuffer = (double *) calloc(nn, sizeof(double));
    HKKT->kktBuffer2 = (double *) calloc(nn, sizeof(double));
    HKKT->dASinvVec = (double *) calloc(nRow, sizeof(double));
    HKKT->dASinvCSinvVec = (double *) calloc(nRow, sizeof(double));
    HKKT->dASinvRdSinvVec = (double *) calloc(nRow, sizeof(double));
    HKKT->kktDiag = (double **) calloc(nRow, sizeof(double *));
    if (!HKKT->invBuffer || !HKKT->kktBuffer || !HKKT->kktBuffer2 || !HKKT->dASinvVec || !HKKT->dASinvCSinvVec ||
        !HKKT->dASinvRdSinvVec || !HKKT->kktDiag)
        return HDSDP_RETCODE_MEMORY;
    return HDSDP_RETCODE_OK;
}

struct KktPattern { std::vector<int> beg, idx, cols; };   // the aggregated pattern: lower-triangular CSC, plus each entry's column

// Dense Schur matrix (hdsdp_schur.c:11-44) or the aggregated-pattern CSC (:46-139), by the reference's own rule
// (kkt_store.h): the columns' patterns are collected from the cones (coneAddSymNz / coneGetKKTMap) unless a cone's share or
// the growing pattern says dense.  False: the operator is dense.
static bool kkt_collect_pattern(hdsdp_kkt *HKKT, const HdmKktSwitches &sw, KktPattern &pat) {
    const int nRow = HKKT->nRow, nCones = HKKT->nCones;
    hdsdp_cone **cones = HKKT->cones;
    if (!sw.sparse) return false;
    for (int i = 0; i < nCones; ++i)
        if (!cones[i]->coneGetSymNnz || !cones[i]->coneAddSymNz || !cones[i]->coneGetKKTMap ||
            !hdm_kkt_count_is_sparse(cones[i]->coneGetSymNnz(cones[i]->coneData), nRow)) return false;
    for (int i = 0; i < nCones; ++i)      // an engine cone may serve a second operator: its pattern walk starts over
        if (cones[i]->coneBuildSchur == cone_build_schur) ((MiCone *) cones[i]->coneData)->kkt_counted = 0;
    std::vector<int> col((size_t) nRow);
    pat.beg.assign((size_t) nRow + 1, 0);
    for (int iCol = 0; iCol < nRow; ++iCol) {
        std::fill(col.begin(), col.end(), 0);
        for (int i = 0; i < nCones; ++i) cones[i]->coneAddSymNz(cones[i]->coneData, iCol, col.data());
        for (int iRow = iCol; iRow < nRow; ++iRow)
            if (col[iRow]) { col[iRow] = (int) pat.idx.size(); pat.idx.push_back(iRow); pat.cols.push_back(iCol); }
        for (int i = 0; i < nCones; ++i) cones[i]->coneGetKKTMap(cones[i]->coneData, iCol, col.data());
        pat.beg[iCol + 1] = (int) pat.idx.size();
        if (!hdm_kkt_count_is_sparse((int64_t) pat.idx.size(), nRow)) return false;      // aggregation made it dense after all
    }
    return hdm_kkt_columns_are_sparse(nRow, pat.beg.data(), pat.idx.data());
}

// The block envelope of a sparse operator's dense device matrix, in the driver's order or -- where kkt_store.h's rule says it
// is cheaper -- in a reverse Cuthill-McKee order of the pattern.  The factor object then holds P M P' (MiLin::perm): the
// builders keep writing M at the driver's indices, the pattern's entries are scattered to their permuted places when the matrix
// is loaded for factorisation, and right-hand sides / solutions are permuted on the host.
static hdsdp_retcode kkt_init_envelope(MiKKTPriv *pv, MiLin *lm, const HdmKktSwitches &sw, const KktPattern &pat, int nRow) {
    if (!sw.envelope || lm->ch.nblk <= 1) return HDSDP_RETCODE_OK;
    const size_t nnz = pat.idx.size();
    const HdmKktEnvelope nat = hdm_kkt_envelope(pat.idx.data(), pat.cols.data(), nnz, lm->ch.nblk, nullptr);
    if (sw.rcm && hdm_kkt_rcm_eligible((int64_t) nnz, nRow)) {
        std::vector<int> perm = hdm_rcm_order(nRow, pat.beg, pat.idx);
        const HdmKktEnvelope rcm = hdm_kkt_envelope(pat.idx.data(), pat.cols.data(), nnz, lm->ch.nblk, perm.data());
        if (hdm_kkt_rcm_taken(rcm.cost, nat.cost)) {
            std::vector<int> prow(nnz), pcol(nnz);
            for (size_t q = 0; q < nnz; ++q) {
                int r = perm[pat.idx[q]], c = perm[pat.cols[q]];
                if (r < c) std::swap(r, c);
                prow[q] = r; pcol[q] = c;
            }
            if (pv->sp_prow.alloc(std::max<size_t>(1, nnz)) != hipSuccess ||
                pv->sp_pcol.alloc(std::max<size_t>(1, nnz)) != hipSuccess)
                return HDSDP_RETCODE_MEMORY;
            if (hdm_memcpy_h2d_sync(pv->sp_prow.get(), prow.data(), sizeof(int) * nnz) != hipSuccess ||
                hdm_memcpy_h2d_sync(pv->sp_pcol.get(), pcol.data(), sizeof(int) * nnz) != hipSuccess)
                return HDSDP_RETCODE_FAILED;
            lm->perm = std::move(perm);
            return lm->ch.set_envelope(rcm.first.data()) ? HDSDP_RETCODE_FAILED : HDSDP_RETCODE_OK;
        }
    }
    return lm->ch.set_envelope(nat.first.data()) ? HDSDP_RETCODE_FAILED : HDSDP_RETCODE_OK;
}

// The Schur system's tolerances: what the refined solve (refine_rule.h) iterates to.  The reference sets them on its dense
// (iterative) Schur system only; a sparse operator's refined solve is held to the same accuracy here.
static void kkt_set_accuracy(hdsdp_kkt *HKKT) {
    const int nRow = HKKT->nRow;
    double acc = 1e-12;  // KKT_ACCURACY (hdsdp.h:27); loosened for big systems exactly as hdsdp_schur.c:21-35
    int iters = -1;
    if (nRow > 20000) { acc *= 100.0; iters = 500; } else if (nRow > 15000) { acc *= 50.0; iters = 450; }
    else if (nRow > 5000) { acc *= 5.0; iters = 120; }
    HFpLinsysSetParam(HKKT->kktM, 5.0 * acc, acc, -1, iters, -1);
}

// Storage of a sparse operator: the host CSC, and on the device the TILE form (bsparse.h) when it pays -- the rows are reordered
// (dense rows last, reverse Cuthill-McKee for the rest), and matrix and factor exist only as the 128 x 128 tiles inside the block
// pattern of the Cholesky factor: O(tiles of L) memory, a level-scheduled left-looking factorisation.  Taken when those tiles
// are at most half of the dense lower triangle's; otherwise the dense device matrix factored on its block envelope.
static hdsdp_retcode kkt_init_sparse_storage(hdsdp_kkt *HKKT, MiKKTPriv *pv, const HdmKktSwitches &sw, const KktPattern &pat) {
    const int nRow = HKKT->nRow;
    const size_t nnz = pat.idx.size();
    HKKT->kktMatBeg = (int *) malloc(sizeof(int) * ((size_t) nRow + 1));
    HKKT->kktMatIdx = (int *) malloc(sizeof(int) * std::max<size_t>(1, nnz));
    if (!HKKT->kktMatBeg || !HKKT->kktMatIdx) return HDSDP_RETCODE_MEMORY;
    memcpy(HKKT->kktMatBeg, pat.beg.data(), sizeof(int) * ((size_t) nRow + 1));
    memcpy(HKKT->kktMatIdx, pat.idx.data(), sizeof(int) * nnz);
    // (kktMatElem is a field of the reference's own struct: it stays a raw pointer, freed in HKKTClear)
    if (hipHostMalloc((void **) &HKKT->kktMatElem, sizeof(double) * std::max<size_t>(1, nnz), hipHostMallocDefault) != hipSuccess)
        return HDSDP_RETCODE_MEMORY;
    memset(HKKT->kktMatElem, 0, sizeof(double) * nnz);
    for (int iCol = 0; iCol < nRow; ++iCol) HKKT->kktDiag[iCol] = &HKKT->kktMatElem[pat.beg[iCol]];
    std::unique_ptr<HdmBsp> bsp_own;
    if (sw.tiles && nRow > 2 * HDM_KKT_BLOCK) {
        bsp_own.reset(new HdmBsp());
        if (bsp_own->init(nRow, pat.beg.data(), pat.idx.data(), 0.5)) bsp_own.reset();
    }
    const HdmBsp *bsp = bsp_own.get();   // (for the report below; the operator's linear system owns it from here)
    hdsdp_retcode rc = bsp ? linsys_create_tiles(&HKKT->kktM, nRow, std::move(bsp_own)) : HFpLinsysCreate(&HKKT->kktM, nRow, HDSDP_LINSYS_SPARSE_DIRECT);
    if (rc != HDSDP_RETCODE_OK) return rc;
    rc = HFpLinsysSymbolic(HKKT->kktM, HKKT->kktMatBeg, HKKT->kktMatIdx);
    if (rc != HDSDP_RETCODE_OK) return rc;
    kkt_set_accuracy(HKKT);
    // the pattern as (row, column) pairs on the device
    pv->nnz = (long) nnz;
    if (pv->sp_rows.alloc(std::max<size_t>(1, nnz)) != hipSuccess ||
        pv->sp_cols.alloc(std::max<size_t>(1, nnz)) != hipSuccess ||
        pv->sp_vals.alloc(std::max<size_t>(1, nnz)) != hipSuccess)
        return HDSDP_RETCODE_MEMORY;
    if (hdm_memcpy_h2d_sync(pv->sp_rows.get(), pat.idx.data(), sizeof(int) * nnz) != hipSuccess ||
        hdm_memcpy_h2d_sync(pv->sp_cols.get(), pat.cols.data(), sizeof(int) * nnz) != hipSuccess)
        return HDSDP_RETCODE_FAILED;
    if (!bsp && (rc = kkt_init_envelope(pv, (MiLin *) HKKT->kktM->chol, sw, pat, nRow)) != HDSDP_RETCODE_OK) return rc;
    printf("    Using sparse Schur complement (%d nnzs)\n", HKKT->kktMatBeg[nRow]);
    if (bsp)
        fprintf(stderr, "[hdsdp_mi355x] sparse Schur operator in tile form: %d of %ld tiles (%.2f GiB instead of %.2f), %d levels\n", bsp->ntiles,
                bsp->dense_tiles(), (double) bsp->bytes() / (1 << 30), 2.0 * 8.0 * (double) bsp->nb * 128 * bsp->nb * 128 / (1 << 30), bsp->nlevels);
    return HDSDP_RETCODE_OK;
}

// Storage of a dense operator: the m x m host matrix and the Schur system's tolerances
static hdsdp_retcode kkt_init_dense_storage(hdsdp_kkt *HKKT) {
    const int nRow = HKKT->nRow;
    // pinned so the D2H/H2D of M after BuildUp / before Factorize runs at PCIe rate
    if (hipHostMalloc((void **) &HKKT->kktMatElem, sizeof(double) * (size_t) nRow * nRow, hipHostMallocDefault) != hipSuccess)
        return HDSDP_RETCODE_MEMORY;
    memset(HKKT->kktMatElem, 0, sizeof(double) * (size_t) nRow * nRow);
    hdsdp_retcode rc = HFpLinsysCreate(&HKKT->kktM, nRow, HDSDP_LINSYS_DENSE_ITERATIVE);
    if (rc != HDSDP_RETCODE_OK) return rc;
    kkt_set_accuracy(HKKT);
    for (int i = 0; i < nRow; ++i) HKKT->kktDiag[i] = &HKKT->kktMatElem[i + (size_t) i * nRow];
    return HDSDP_RETCODE_OK;
}

// What every form has on the device: outside the tile form M stays a dense m x m matrix -- the cones' builders write it at
// global (row, column) indices, the blocked Cholesky factors it densely; what the sparse form changes is the host side, where
// the driver, the CPU cones (through kktMapping / kktDiag) and HKKTRegularize see the nnz-long CSC, not m^2 doubles -- plus the
// accumulators, the diagonal channel, and the state the storage starts in.
static hdsdp_retcode kkt_init_device_common(hdsdp_kkt *HKKT, MiKKTPriv *pv) {
    const int nRow = HKKT->nRow, nCones = HKKT->nCones;
    hdsdp_cone **cones = HKKT->cones;
    MiLin *l = (MiLin *) HKKT->kktM->chol;
    if (!l->bsp) {
        const size_t mm = sizeof(double) * (size_t) l->ch.npad * l->ch.npad;
        if (l->Mdev.alloc(mm / sizeof(double)) != hipSuccess) return HDSDP_RETCODE_MEMORY;
        if (hdm_memset_sync(l->Mdev.get(), 0, mm) != hipSuccess) return HDSDP_RETCODE_FAILED;
    }
    if (pv->vecs.alloc(3 * (size_t) nRow + 4) != hipSuccess) return HDSDP_RETCODE_MEMORY;
    pv->n_engine = pv->n_foreign = 0;
    for (int i = 0; i < nCones; ++i) {
        if (cones[i]->coneBuildSchur == cone_build_schur || cones[i]->coneBuildSchur == gc_build_schur ||
            cones[i]->coneBuildSchur == lp_build_schur) pv->n_engine += 1;
        else pv->n_foreign += 1;
    }
    if (pv->chan.alloc((size_t) std::max(1, nRow)) != hipSuccess ||
        pv->chan_dev.alloc((size_t) nRow + 1) != hipSuccess)
        return HDSDP_RETCODE_MEMORY;
    memset(pv->chan.get(), 0, sizeof(double) * std::max(1, nRow));
    pv->bytes_d2h = pv->bytes_h2d = 0;
    l->st = &pv->st;
    pv->st.storage_decided(l->bsp ? HDM_KKT_TILES : HKKT->isKKTSparse ? HDM_KKT_CSC : HDM_KKT_DENSE, !l->perm.empty());
    return HDSDP_RETCODE_OK;
}

// HDSDP_MI355X_DEVICE_M=1: an unchanged driver keeps M on the device when it can.  Its host cones
// outside cones[] (the bound cone on y) write the diagonal only, and that goes through the channel.
static void kkt_apply_device_m(hdsdp_kkt *HKKT, MiKKTPriv *pv) {
    if (pv->n_engine > 0 && pv->n_foreign == 0) {
        HMiKKTSetHostMirror(HKKT, 0);
        fprintf(stderr, "[hdsdp_mi355x] HDSDP_MI355X_DEVICE_M=1: M stays on the device (m = %d, diagonal channel)\n", HKKT->nRow);
    }
    else if (pv->n_foreign > 0)
        fprintf(stderr, "[hdsdp_mi355x] HDSDP_MI355X_DEVICE_M=1: the host copy of M is kept: %d cone(s) of this operator accumulate on the host\n",
                pv->n_foreign);
    else fprintf(stderr, "[hdsdp_mi355x] HDSDP_MI355X_DEVICE_M=1: the host copy of M is kept: the operator has no engine cone\n");
}

// What else an unchanged driver can opt into through the environment, each by the setter a caller would use
static void kkt_apply_opt_ins(hdsdp_kkt *HKKT, MiKKTPriv *pv) {
    const int nCones = HKKT->nCones;
    if (hdm_env_on<ENV_GROUPED_BUILD>()) {
        const int k = grouped_set(HKKT, pv, 1);
        fprintf(stderr, "[hdsdp_mi355x] HDSDP_MI355X_GROUPED_BUILD=1: %d of %d cone(s) are built in one grouped pass\n", k, nCones);
    }
    // the three question sets (cone_set.h): environment switch, setter, what the members then do
    const struct { bool asked; const char *name; int (*set)(hdsdp_kkt *, int); const char *does; } sets[3] = {
        {hdm_env_on<ENV_GROUPED_CHECK>(), "CHECK", HMiKKTSetGroupedCheck, "a point question in one grouped launch"},
        {hdm_env_on<ENV_GROUPED_RATIO>(), "RATIO", HMiKKTSetGroupedRatio, "a ratio test in one grouped launch pair"},
        {hdm_env_on<ENV_GROUPED_STEP>(), "STEP", HMiKKTSetGroupedStep, "a step-and-check in one grouped launch"}};
    for (const auto &t : sets)
        if (t.asked) {
            const int k = t.set(HKKT, 1);
            fprintf(stderr, "[hdsdp_mi355x] HDSDP_MI355X_GROUPED_%s=1: %d of %d cone(s) answer %s\n", t.name, k, nCones, t.does);
        }
    // the ratio set's two opt-ins: each acts only while the grouped ratio test itself is on
    const struct { bool asked; const char *name; int (*set)(hdsdp_kkt *, int); const char *does; } opts[2] = {
        {hdm_env_on<ENV_GRATIO_CHECKER>(), "CHECKER", HMiKKTSetGroupedRatioChecker, "a ratio test on the checker buffer from the grouped launch too"},
        {hdm_env_on<ENV_GRATIO_REST>(), "REST", HMiKKTSetGroupedRatioRest, "with the safeguard's fresh-start test and cuts inside the grouped launch"}};
    for (const auto &t : opts)
        if (t.asked) {
            if (!pv->rat.on)
                fprintf(stderr, "[hdsdp_mi355x] HDSDP_MI355X_GRATIO_%s=1: nothing to do, the grouped ratio test is not on "
                                "(HDSDP_MI355X_GROUPED_RATIO=1 and at least two members)\n", t.name);
            else {
                const int k = t.set(HKKT, 1);
                fprintf(stderr, "[hdsdp_mi355x] HDSDP_MI355X_GRATIO_%s=1: %d of %d cone(s) answer %s\n", t.name, k, nCones, t.does);
            }
        }
    // HDSDP_MI355X_REFINE=k: Schur solves are refined with at most k steps (HMiKKTSetRefine)
    if (const int k = hdm_env_int<ENV_REFINE>().value_or(0); k > 0) {
        (void) HMiKKTSetRefine(HKKT, k);
        fprintf(stderr, "[hdsdp_mi355x] HDSDP_MI355X_REFINE=%d: Schur solves are refined, at most %d step(s)\n", k, pv->st.refine());
    }
    // HDSDP_MI355X_REFINE_TILES=1: ... and a tile-form operator's too (HMiKKTSetRefineTiles; it needs the step cap above as well)
    if (const int t = hdm_env_int<ENV_REFINE_TILES>().value_or(0); t > 0) {
        (void) HMiKKTSetRefineTiles(HKKT, 1);
        fprintf(stderr, "[hdsdp_mi355x] HDSDP_MI355X_REFINE_TILES=%d: the tile form of a sparse operator is refined too (step cap %d)\n", t, pv->st.refine());
    }
}

hdsdp_retcode HKKTInit(hdsdp_kkt *HKKT, int nRow, int nCones, hdsdp_cone **cones) {
    if (ensure_ctx() || !kkt_cones_combine(nCones, cones)) return HDSDP_RETCODE_FAILED;
    const HdmKktSwitches sw = hdm_kkt_switches();
    MiKKTPriv *pv = priv_of(HKKT);
    hdsdp_retcode rc = kkt_init_host_fields(HKKT, nRow, nCones, cones);
    if (rc != HDSDP_RETCODE_OK) return rc;
    KktPattern pat;
    HKKT->isKKTSparse = kkt_collect_pattern(HKKT, sw, pat) ? 1 : 0;
    rc = HKKT->isKKTSparse ? kkt_init_sparse_storage(HKKT, pv, sw, pat) : kkt_init_dense_storage(HKKT);
    if (rc != HDSDP_RETCODE_OK) return rc;
    rc = kkt_init_device_common(HKKT, pv);
    if (rc != HDSDP_RETCODE_OK) return rc;
    if (sw.device_m) kkt_apply_device_m(HKKT, pv);
    // eligibility for the grouped Schur build (engine_grouped.h) and membership of the three question sets (cone_set.h's rules:
    // the operator initialised last has a cone no ACTIVE set holds) are decided for every operator; the grouped pass and the
    // grouped launches are used when their switches are on
    grouped_init_plan(HKKT, pv);
    const auto engine_cone = [&](int i) { return own_cone_with_factor(HKKT->cones[i]); };
    pv->chk.populate(nCones, engine_cone);
    pv->rat.populate(nCones, engine_cone);
    pv->stp.populate(nCones, engine_cone);
    kkt_apply_opt_ins(HKKT, pv);
    HKKT->dPrimalX = nullptr;
    return HDSDP_RETCODE_OK;
}

// kktDiag[] -> the host matrix's diagonal (mirror on) or the diagonal channel (mirror off)
static void kkt_point_diag(hdsdp_kkt *HKKT, MiKKTPriv *pv) {
    if (!HKKT->kktDiag || !HKKT->kktMatElem || !pv->chan.get()) return;
    const int m = HKKT->nRow;
    for (int i = 0; i < m; ++i)
        HKKT->kktDiag[i] = !pv->st.mirror() ? &pv->chan.get()[i] :
                           HKKT->isKKTSparse ? &HKKT->kktMatElem[HKKT->kktMatBeg[i]] : &HKKT->kktMatElem[i + (size_t) i * m];
}

// one pass over diag(M) on the device (mi_diag_pass_kernel): fold = upload the channel and add it (once per build: the caller
// tells the state), add = add v; mn (optional) receives the minimum of the diagonal after the pass's additions
static hdsdp_retcode kkt_diag_pass(hdsdp_kkt *HKKT, MiKKTPriv *pv, bool fold, bool add, double v, double *mn) {
    const int m = HKKT->nRow;
    if (fold) {
        if (hipMemcpyAsync(pv->chan_dev.get(), pv->chan.get(), sizeof(double) * (size_t) m, hipMemcpyHostToDevice, g.stream) != hipSuccess)
            return HDSDP_RETCODE_FAILED;
        pv->bytes_h2d += (int64_t) sizeof(double) * m;
    }
    hipLaunchKernelGGL(mi_diag_pass_kernel, dim3(1), dim3(1024), 0, g.stream, kkt_view(HKKT), m, fold ? pv->chan_dev.get() : nullptr,
                       add ? 1 : 0, v, mn ? pv->chan_dev.get() + m : nullptr);
    if (hipGetLastError() != hipSuccess) return HDSDP_RETCODE_FAILED;
    if (mn && (hipMemcpyAsync(mn, pv->chan_dev.get() + m, sizeof(double), hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
               hipStreamSynchronize(g.stream) != hipSuccess))
        return HDSDP_RETCODE_FAILED;
    return HDSDP_RETCODE_OK;
}

static HdmMatView dense_view(double *base, long ld) { HdmMatView v; v.base = base; v.ld = ld; return v; }

// The value buffer is scattered into `view` at (rows[q], cols[q]); with `hostVals`, the host CSC's values go up into it first
// (nnz doubles).  Without, it holds them already.
static hdsdp_retcode kkt_csc_scatter(MiKKTPriv *pv, const double *hostVals, HdmMatView view, const int *rows, const int *cols) {
    if (pv->nnz <= 0) return HDSDP_RETCODE_OK;
    if (hostVals && hipMemcpyAsync(pv->sp_vals.get(), hostVals, sizeof(double) * (size_t) pv->nnz, hipMemcpyHostToDevice, g.stream) != hipSuccess)
        return HDSDP_RETCODE_FAILED;
    hipLaunchKernelGGL(mi_csc_scatter_kernel, dim3((unsigned) ((pv->nnz + 255) / 256)), dim3(256), 0, g.stream, view, rows, cols, pv->nnz,
                       pv->sp_vals.get());
    return HDSDP_RETCODE_OK;
}
// the pattern's entries of `view` into the value buffer (an engine cone only writes inside the pattern it declared)
static void kkt_csc_gather(MiKKTPriv *pv, HdmMatView view) {
    if (pv->nnz > 0)
        hipLaunchKernelGGL(mi_csc_gather_kernel, dim3((unsigned) ((pv->nnz + 255) / 256)), dim3(256), 0, g.stream, view, pv->sp_rows.get(),
                           pv->sp_cols.get(), pv->nnz, pv->sp_vals.get());
}

// a build starts: host cones add their diagonal terms into an empty channel (a corrector build touches neither M nor the channel)
static void kkt_channel_start(hdsdp_kkt *HKKT, MiKKTPriv *pv, int typeKKT) {
    if (typeKKT != KKT_TYPE_CORRECTOR) memset(pv->chan.get(), 0, sizeof(double) * (size_t) HKKT->nRow);
    pv->st.build_started(typeKKT == KKT_TYPE_CORRECTOR);
}

static hdsdp_retcode kkt_clean(hdsdp_kkt *HKKT, int typeKKT) {  // hdsdp_schur.c:141-165
    const int m = HKKT->nRow;
    MiKKTPriv *pv = priv_of(HKKT);
    memset(HKKT->dASinvVec, 0, sizeof(double) * m);
    memset(HKKT->dASinvRdSinvVec, 0, sizeof(double) * m);
    if (typeKKT == KKT_TYPE_HOMOGENEOUS) {
        memset(HKKT->dASinvCSinvVec, 0, sizeof(double) * m);
        HKKT->dCSinv = HKKT->dCSinvCSinv = HKKT->dCSinvRdSinv = 0.0;
    }
    HKKT->dTraceSinv = 0.0;
    if (hipMemsetAsync(pv->vecs.get(), 0, sizeof(double) * (3 * (size_t) m + 4), g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    if (typeKKT != KKT_TYPE_CORRECTOR) {
        MiLin *l = (MiLin *) HKKT->kktM->chol;
        if (l->bsp) { if (l->bsp->zero_M(g.stream)) return HDSDP_RETCODE_FAILED; }
        else if (hipMemsetAsync(l->Mdev.get(), 0, sizeof(double) * (size_t) l->ch.npad * l->ch.npad, g.stream) != hipSuccess)
            return HDSDP_RETCODE_FAILED;
        if (HKKT->isKKTSparse) memset(HKKT->kktMatElem, 0, sizeof(double) * (size_t) HKKT->kktMatBeg[m]);   // (CPU cones add into it)
        // (dense host matrix: CPU cones add into it, so it starts from zero -- but with engine cones only, kkt_pull's copy
        // of the whole m x m device matrix replaces every entry, and 8 m^2 bytes of host memset per call are saved: 4 ms at
        // m = 2000, twice per iteration of the reference's driver)
        else if (pv->st.mirror() && !(pv->n_foreign == 0 && pv->n_engine > 0)) memset(HKKT->kktMatElem, 0, sizeof(double) * (size_t) m * m);
    }
    kkt_channel_start(HKKT, pv, typeKKT);
    return HDSDP_RETCODE_OK;
}

static hdsdp_retcode kkt_pull(hdsdp_kkt *HKKT, int typeKKT) {
    // device accumulators -> the host fields the driver and the CPU cones read (def_hdsdp_schur.h:44-61)
    const int m = HKKT->nRow;
    MiKKTPriv *pv = priv_of(HKKT);
    std::vector<double> h(3 * (size_t) m + 4);
    if (hipMemcpyAsync(h.data(), pv->vecs.get(), sizeof(double) * h.size(), hipMemcpyDeviceToHost, g.stream) != hipSuccess)
        return HDSDP_RETCODE_FAILED;
    // M: every cone ACCUMULATES (hdsdp_schur.c:256-268).  The engine's cones did so on the device, foreign (CPU) cones
    // straight into kktMatElem: with only engine cones the device matrix simply replaces the (zeroed) host one, with
    // only foreign cones there is nothing to bring back, and in the mixed case the device part is added to the host part.
    bool add_M = false;
    size_t mcount = 0;     // entries of the host matrix that came back through Mtmp
    if (typeKKT != KKT_TYPE_CORRECTOR && pv->st.mirror() && pv->n_engine > 0) {
        long ld = 0;
        double *Mdev = kkt_Mdev(HKKT, &ld);
        double *dst = HKKT->kktMatElem;
        mcount = HKKT->isKKTSparse ? (size_t) pv->nnz : (size_t) m * m;
        pv->bytes_d2h += (int64_t) (sizeof(double) * mcount);
        if (pv->n_foreign > 0) {
            if (!pv->Mtmp && pv->Mtmp.alloc(std::max<size_t>(1, mcount)) != hipSuccess) return HDSDP_RETCODE_MEMORY;
            dst = pv->Mtmp.get();
            add_M = true;
        }
        if (HKKT->isKKTSparse) {
            kkt_csc_gather(pv, kkt_view(HKKT));
            if (pv->nnz > 0 && hipMemcpyAsync(dst, pv->sp_vals.get(), sizeof(double) * (size_t) pv->nnz, hipMemcpyDeviceToHost, g.stream) != hipSuccess)
                return HDSDP_RETCODE_FAILED;
        } else if (hipMemcpy2DAsync(dst, sizeof(double) * m, Mdev, sizeof(double) * ld, sizeof(double) * m, m,
                                    hipMemcpyDeviceToHost, g.stream) != hipSuccess)
            return HDSDP_RETCODE_FAILED;
    }
    if (hipStreamSynchronize(g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    if (add_M) {
        if (HKKT->isKKTSparse) for (size_t q = 0; q < mcount; ++q) HKKT->kktMatElem[q] += pv->Mtmp.get()[q];
        else
            for (int j = 0; j < m; ++j)                    // lower triangle, column-major
                for (int i = j; i < m; ++i) HKKT->kktMatElem[i + (size_t) j * m] += pv->Mtmp.get()[i + (size_t) j * m];
    }
    for (int i = 0; i < m; ++i) {
        HKKT->dASinvVec[i] += h[i];
        HKKT->dASinvRdSinvVec[i] += h[m + i];
        if (typeKKT == KKT_TYPE_HOMOGENEOUS) HKKT->dASinvCSinvVec[i] += h[2 * (size_t) m + i];
    }
    if (typeKKT != KKT_TYPE_CORRECTOR) HKKT->dTraceSinv += h[3 * (size_t) m];
    if (typeKKT == KKT_TYPE_HOMOGENEOUS) {
        HKKT->dCSinv += h[3 * (size_t) m + 1];
        HKKT->dCSinvCSinv += h[3 * (size_t) m + 2];
        HKKT->dCSinvRdSinv += h[3 * (size_t) m + 3];
    }
    pv->st.build_finished(typeKKT == KKT_TYPE_CORRECTOR);
    return HDSDP_RETCODE_OK;
}

// HKKTBuildUp and HKKTBuildUpFixed: clean, then the cones in order -- the grouped cones of the operator (engine_grouped.h; none
// unless the switch is on) all at once, where the first of them sits, every other cone through its own slot -- then the pull.
static hdsdp_retcode kkt_build_cones(hdsdp_kkt *HKKT, int typeKKT, bool fixed, int kktStrategy) {
    hdsdp_retcode rc = kkt_clean(HKKT, typeKKT);
    if (rc != HDSDP_RETCODE_OK) return rc;
    MiKKTPriv *pv = priv_of(HKKT);
    const bool grouped = pv->grp.used() && typeKKT != KKT_TYPE_PRIMAL;
    pv->grp.last_cones = pv->grp.last_jobs = pv->grp.last_launches = 0;
    bool grouped_done = false;
    for (int i = 0; i < HKKT->nCones; ++i) {
        hdsdp_cone *c = HKKT->cones[i];
        if (grouped && pv->grp.plan.slot_of[(size_t) i] >= 0) {
            if (grouped_done) continue;
            grouped_done = true;
            rc = grouped_build(HKKT, pv, typeKKT);
        }
        else if (fixed) rc = c->coneBuildSchurFixed(c->coneData, c->iCone, HKKT, typeKKT, kktStrategy);
        else rc = c->coneBuildSchur(c->coneData, c->iCone, HKKT, typeKKT);  // == HConeBuildSchurComplement
        if (!fixed && stat_trace()) {
            const hipError_t e = hipDeviceSynchronize();
            fprintf(stderr, "[hdsdp_mi355x trace]   build type %d, cone %d of %d -> rc %d, %s\n", typeKKT, i, HKKT->nCones, (int) rc,
                    e == hipSuccess ? "ok" : hipGetErrorName(e));
        }
        if (rc != HDSDP_RETCODE_OK) return rc;
    }
    return kkt_pull(HKKT, typeKKT);
}

hdsdp_retcode HKKTBuildUp(hdsdp_kkt *HKKT, int typeKKT) {
    StatScope stat_(typeKKT == KKT_TYPE_CORRECTOR ? ST_BUILD_CORR : ST_BUILD_M, __func__);
    return kkt_build_cones(HKKT, typeKKT, false, 0);
}

hdsdp_retcode HKKTBuildUpExtraCone(hdsdp_kkt *HKKT, hdsdp_cone *cone, int typeKKT) {
    StatScope stat_(typeKKT == KKT_TYPE_CORRECTOR ? ST_BUILD_CORR : ST_BUILD_M, __func__);
    // CPU cones (bound / LP, hdsdp_conic_bound.c:201-249) write straight into the host fields
    return cone->coneBuildSchur(cone->coneData, cone->iCone, HKKT, typeKKT);
}

hdsdp_retcode HKKTBuildUpFixed(hdsdp_kkt *HKKT, int typeKKT, int kktStrategy) {
    StatScope stat_(typeKKT == KKT_TYPE_CORRECTOR ? ST_BUILD_CORR : ST_BUILD_M, __func__);
    return kkt_build_cones(HKKT, typeKKT, true, kktStrategy);
}

void HKKTExport(hdsdp_kkt *HKKT, double *dKKTASinvVec, double *dKKTASinvRdSinvVec, double *dKKTASinvCSinvVec,
                double *dCSinvCSinv, double *dCSinv, double *dCSinvRdCSinv, double *dTraceSinv) {
    const size_t b = sizeof(double) * (size_t) HKKT->nRow;
    if (dKKTASinvVec) memcpy(dKKTASinvVec, HKKT->dASinvVec, b);
    if (dKKTASinvRdSinvVec) memcpy(dKKTASinvRdSinvVec, HKKT->dASinvRdSinvVec, b);
    if (dKKTASinvCSinvVec) memcpy(dKKTASinvCSinvVec, HKKT->dASinvCSinvVec, b);
    if (dCSinvCSinv) *dCSinvCSinv = HKKT->dCSinvCSinv;
    if (dCSinv) *dCSinv = HKKT->dCSinv;
    if (dCSinvRdCSinv) *dCSinvRdCSinv = HKKT->dCSinvRdSinv;
    if (dTraceSinv) *dTraceSinv = HKKT->dTraceSinv;
}

// the plan's staging step (kkt_store.h: HdmKktStage)
static hdsdp_retcode kkt_stage(hdsdp_kkt *HKKT, MiKKTPriv *pv, MiLin *l, HdmKktStage stage) {
    switch (stage) {
    case HDM_KKT_STAGE_NONE: break;
    case HDM_KKT_STAGE_FOLD: return kkt_diag_pass(HKKT, pv, true, false, 0.0, nullptr);
    case HDM_KKT_STAGE_CSC_TO_FACTOR:
        RC(l->bsp->zero_L(g.stream));
        return kkt_csc_scatter(pv, HKKT->kktMatElem, l->bsp->view_L(), pv->sp_rows.get(), pv->sp_cols.get());
    case HDM_KKT_STAGE_CSC_TO_M:
        if (hipMemsetAsync(l->Mdev.get(), 0, sizeof(double) * (size_t) l->ch.npad * l->ch.npad, g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
        return kkt_csc_scatter(pv, HKKT->kktMatElem, dense_view(l->Mdev.get(), l->ch.npad), pv->sp_rows.get(), pv->sp_cols.get());
    }
    return HDSDP_RETCODE_OK;
}
// the plan's load step (kkt_store.h: HdmKktLoad)
static hdsdp_retcode kkt_load(hdsdp_kkt *HKKT, MiKKTPriv *pv, MiLin *l, const HdmKktLoadPlan &plan) {
    switch (plan.load) {
    case HDM_KKT_LOAD_STAGED: case HDM_KKT_LOAD_PIVOTED: break;
    case HDM_KKT_LOAD_TILES: RC(l->bsp->load_M(g.stream)); break;
    case HDM_KKT_LOAD_HOST:
        RC(l->ch.load_host(HKKT->kktMatElem, HKKT->nRow, g.stream));
        RC(lin_refine_keep_image(l, l->ch.L.get(), l->ch.npad));
        break;
    case HDM_KKT_LOAD_DEVICE: RC(l->ch.load_device(l->Mdev.get(), l->ch.npad, g.stream)); break;
    case HDM_KKT_LOAD_PERMUTED:
        if (plan.gather) kkt_csc_gather(pv, dense_view(l->Mdev.get(), l->ch.npad));
        if (hipMemsetAsync(l->ch.L.get(), 0, sizeof(double) * (size_t) l->ch.npad * l->ch.npad, g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
        RC(kkt_csc_scatter(pv, nullptr, dense_view(l->ch.L.get(), l->ch.npad), pv->sp_prow.get(), pv->sp_pcol.get()));
        RC(l->ch.finish_load(g.stream));
        break;
    }
    return HDSDP_RETCODE_OK;
}

hdsdp_retcode HKKTFactorize(hdsdp_kkt *HKKT) {
    StatScope stat_(ST_FACTORIZE, __func__);
    // hdsdp_schur.c:328-336.  Where M comes from and how it reaches the factor is hdm_kkt_load_plan's rule (kkt_store.h, with
    // the table); staged, the state records the source, which the pivoted solver reads (lin_factor_indef).
    MiKKTPriv *pv = priv_of(HKKT);
    MiLin *l = (MiLin *) HKKT->kktM->chol;
    HKKT->kktM->nFactorizes += 1;
    const HdmKktLoadPlan plan = hdm_kkt_load_plan(pv->st);
    if (!plan.ok) return HDSDP_RETCODE_FAILED;
    if (kkt_stage(HKKT, pv, l, plan.stage) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
    pv->bytes_h2d += plan.matrix_bytes(HKKT->nRow, pv->nnz);
    pv->st.commit(plan, HKKT->kktMatElem, HKKT->nRow, l->Mdev.get(), l->ch.npad);
    if (plan.load == HDM_KKT_LOAD_PIVOTED) return lin_factor_indef(l);     // switched earlier: stays switched (hdsdp_linsolver.c:1838)
    // tile form, mirror on, refined: the scattered factor store is the only image of the factorised matrix on the device
    if (pv->st.refine_wants_tile_copy() && l->rf.tiles.keep_copy(*l->bsp, g.stream)) return HDSDP_RETCODE_MEMORY;
    if (kkt_load(HKKT, pv, l, plan) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
    // the tile form factors LDL' like the reference's sparse direct solver (linalg/hdsdp_linsolver.c:596-626 over external/qdldl.c):
    // an indefinite matrix factors and the solves go on with the signed factor; only a pivot that is exactly zero is a failure
    int info = 0, nneg = 0;
    if (l->bsp ? l->bsp->factor(g.stream, &info, &nneg) : l->ch.factor(g.stream, &info)) return HDSDP_RETCODE_FAILED;
    if (info == 0) return HDSDP_RETCODE_OK;
    if (plan.on_pivot == HDM_KKT_PIVOT_FAIL) {
        fprintf(stderr, "[hdsdp_mi355x] HKKTFactorize: sparse Schur matrix (tile form): zero pivot at row %d of the reordered matrix\n", info);
        return HDSDP_RETCODE_FAILED;
    }
    // hdsdp_linsolver.c:2034-2039: the Schur system falls back to the symmetric-indefinite solver
    fprintf(stderr, "[hdsdp_mi355x] HKKTFactorize: Schur matrix is not positive definite (pivot %d). "
                    "Switch to the pivoted (LDL-equivalent) solver.\n", info);
    return lin_switch_indefinite(HKKT->kktM);
}

hdsdp_retcode HKKTSolve(hdsdp_kkt *HKKT, double *dRhsVec, double *dLhsVec) {
    StatScope stat_(ST_SOLVE, __func__);
    return HFpLinsysSolve(HKKT->kktM, 1, dRhsVec, dLhsVec);
}

void HKKTRegularize(hdsdp_kkt *HKKT, double dKKTReg) {  // hdsdp_schur.c:348-373
    MiKKTPriv *pv = priv_of(HKKT);
    if (!pv->st.mirror()) {
        // device-resident M (HMiKKTSetHostMirror(.., 0)): the same rule on the device matrix's diagonal plus the channel.  The
        // first call after a build adds the channel in place; every call then adds its regularisation on top, so the entries
        // are ((M_ii + channel_i) + reg1) + reg2 ..., the host mirror's order.  No part of M crosses the bus.
        if (!pv->st.m_valid()) return;
        double mn = INFINITY;
        const bool fold = !pv->st.chan_folded();
        if (kkt_diag_pass(HKKT, pv, fold, false, 0.0, &mn) != HDSDP_RETCODE_OK) return;
        if (fold) pv->st.channel_folded();
        const double reg = std::min(dKKTReg * mn, 1e-05);
        if (reg < 1e-14) return;
        (void) kkt_diag_pass(HKKT, pv, false, true, reg, nullptr);
        return;
    }
    double mn = INFINITY;
    for (int i = 0; i < HKKT->nRow; ++i) mn = std::min(mn, *HKKT->kktDiag[i]);
    dKKTReg = std::min(dKKTReg * mn, 1e-05);
    if (dKKTReg < 1e-14) dKKTReg = 0.0;
    for (int i = 0; i < HKKT->nRow; ++i) *HKKT->kktDiag[i] += dKKTReg;
}

void HKKTRegisterPSDP(hdsdp_kkt *HKKT, double **dPrimalX) { HKKT->dPrimalX = dPrimalX; }

void HKKTClear(hdsdp_kkt *HKKT) {
    if (!HKKT) return;
    free(HKKT->dASinvVec); free(HKKT->dASinvCSinvVec); free(HKKT->dASinvRdSinvVec);
    free(HKKT->invBuffer); free(HKKT->kktBuffer); free(HKKT->kktBuffer2);
    free(HKKT->kktMatBeg); free(HKKT->kktMatIdx);
    if (HKKT->kktMatElem) (void) hipHostFree(HKKT->kktMatElem);
    free(HKKT->kktDiag);
    HFpLinsysDestroy(&HKKT->kktM);
    priv_drop(HKKT);
    memset(HKKT, 0, sizeof(hdsdp_kkt));
}

void HKKTDestroy(hdsdp_kkt **pHKKT) {
    if (!pHKKT || !*pHKKT) return;
    HKKTClear(*pHKKT);
    free(*pHKKT);
    *pHKKT = nullptr;
}

void HMiKKTSetHostMirror(hdsdp_kkt *HKKT, int mirrorM) {
    MiKKTPriv *pv = priv_of(HKKT);
    if (!mirrorM && pv->n_foreign > 0) {
        fprintf(stderr, "[hdsdp_mi355x] HMiKKTSetHostMirror(0) ignored: %d cone(s) of this operator accumulate on the host\n",
                pv->n_foreign);
        return;
    }
    pv->st.mirror_switched(mirrorM != 0);
    kkt_point_diag(HKKT, pv);
}
int HMiKKTSetGroupedBuild(hdsdp_kkt *HKKT, int on) { return grouped_set(HKKT, priv_of(HKKT), on); }
int HMiKKTGetGroupedBuild(hdsdp_kkt *HKKT, int *cones, int *jobs, int *launches) {
    const MiGrouped &gr = priv_of(HKKT)->grp;
    if (cones) *cones = gr.last_cones;
    if (jobs) *jobs = gr.last_jobs;
    if (launches) *launches = gr.last_launches;
    return gr.last_cones > 0 ? 1 : 0;
}
// The question sets (cone_set.h).  An all-cones call: every cone of cones[] in order, no early exit, each through its own slot
// (`ask`, which also keeps the call's per-cone array and its reduction) -- the members of an active set reach the grouped launch
// through the first of them that is asked.  The first failing retcode is returned.
extern "C++" {
template <class Ask> hdsdp_retcode kkt_all_cones(hdsdp_kkt *HKKT, Ask ask) {
    hdsdp_retcode first = HDSDP_RETCODE_OK;
    for (int i = 0; i < HKKT->nCones; ++i)
        if (const hdsdp_retcode rc = ask(i, HKKT->cones[i]); rc != HDSDP_RETCODE_OK && first == HDSDP_RETCODE_OK) first = rc;
    return first;
}
// A Get call: living members, the three launch counters, answers from the store, members left out of the last launch
template <class Set> int kkt_set_get(const Set &s, long *out) {
    if (out) s.report(out);
    return s.on ? 1 : 0;
}
}  // extern "C++"
int HMiKKTSetGroupedCheck(hdsdp_kkt *HKKT, int on) { return priv_of(HKKT)->chk.turn(on); }
int HMiKKTGetGroupedCheck(hdsdp_kkt *HKKT, long out[6]) { return kkt_set_get(priv_of(HKKT)->chk, out); }
hdsdp_retcode HMiKKTCheckIsInterior(hdsdp_kkt *HKKT, double tau, const double *y, int *flags, double *logdets, int *all) {
    if (!HKKT || ensure_ctx()) return HDSDP_RETCODE_FAILED;
    int every = 1;
    const hdsdp_retcode first = kkt_all_cones(HKKT, [&](int i, hdsdp_cone *hc) {
        int in = 0;
        double ld = NAN;
        hdsdp_retcode rc = hc->coneInteriorCheck(hc->coneData, tau, (double *) y, &in);
        if (rc == HDSDP_RETCODE_OK && in) {
            rc = hc->coneGetBarrier(hc->coneData, tau, (double *) y, 0, &ld);
            if (rc != HDSDP_RETCODE_OK) ld = NAN;
        } else in = 0;
        if (flags) flags[i] = in;
        if (logdets) logdets[i] = in ? ld : NAN;
        every &= in;
        return rc;
    });
    if (all) *all = every;
    return first;
}
int HMiKKTSetGroupedRatio(hdsdp_kkt *HKKT, int on) { return priv_of(HKKT)->rat.turn(on); }
int HMiKKTGetGroupedRatio(hdsdp_kkt *HKKT, long out[7]) {
    if (out) out[6] = priv_of(HKKT)->rat.fallbacks;
    return kkt_set_get(priv_of(HKKT)->rat, out);
}
// the ratio set's two opt-ins: each acts only while the set is on; the number of members when on afterwards
int HMiKKTSetGroupedRatioChecker(hdsdp_kkt *HKKT, int on) {
    MiRatioSet &rs = priv_of(HKKT)->rat;
    return rs.turn_checker(on) ? rs.count() : 0;
}
int HMiKKTSetGroupedRatioRest(hdsdp_kkt *HKKT, int on) {
    MiRatioSet &rs = priv_of(HKKT)->rat;
    return rs.turn_rest(on) ? rs.count() : 0;
}
int HMiKKTGetGroupedRatioDetail(hdsdp_kkt *HKKT, long out[6]) {
    const MiRatioSet &rs = priv_of(HKKT)->rat;
    if (out) {
        out[0] = rs.checker_on ? 1 : 0; out[1] = rs.rest_on ? 1 : 0;
        out[2] = rs.checker_launches; out[3] = rs.device_rests; out[4] = rs.device_cuts; out[5] = rs.fallbacks;
    }
    return rs.on ? 1 : 0;
}
hdsdp_retcode HMiKKTRatioTest(hdsdp_kkt *HKKT, double dTauStep, const double *dy, double dAdaRatio, int whichBuffer, double *steps,
                              double *minStep) {
    if (!HKKT || ensure_ctx()) return HDSDP_RETCODE_FAILED;
    double mn = INFINITY;
    const hdsdp_retcode first = kkt_all_cones(HKKT, [&](int i, hdsdp_cone *hc) {
        double step = NAN;
        const hdsdp_retcode rc = hc->coneRatioTest(hc->coneData, dTauStep, (double *) dy, dAdaRatio, whichBuffer, &step);
        if (rc != HDSDP_RETCODE_OK) step = NAN;
        else if (step < mn) mn = step;
        if (steps) steps[i] = step;
        return rc;
    });
    if (minStep) *minStep = mn;
    return first;
}
int HMiKKTSetGroupedStep(hdsdp_kkt *HKKT, int on) { return priv_of(HKKT)->stp.turn(on); }
int HMiKKTGetGroupedStep(hdsdp_kkt *HKKT, long out[6]) { return kkt_set_get(priv_of(HKKT)->stp, out); }
hdsdp_retcode HMiKKTAddStepToBufferAndCheck(hdsdp_kkt *HKKT, double dStep, int whichBuffer, int *flags, int *allInterior) {
    if (!HKKT || ensure_ctx()) return HDSDP_RETCODE_FAILED;
    int every = 1;
    const hdsdp_retcode first = kkt_all_cones(HKKT, [&](int i, hdsdp_cone *hc) {
        int in = 0;
        const hdsdp_retcode rc = hc->coneAxpyBufferAndCheck(hc->coneData, dStep, whichBuffer, &in);
        if (rc != HDSDP_RETCODE_OK) in = 0;
        if (flags) flags[i] = in;
        every &= in ? 1 : 0;
        return rc;
    });
    if (allInterior) *allInterior = every;
    return first;
}
int HMiKKTGetDiagTarget(hdsdp_kkt *HKKT) {
    MiKKTPriv *pv = priv_of(HKKT);
    if (!HKKT->kktDiag || !pv->chan.get()) return -1;
    return pv->st.mirror() ? 0 : 1;
}
void HMiKKTGetMatrixTraffic(hdsdp_kkt *HKKT, int64_t *bytesToHost, int64_t *bytesToDevice) {
    const MiKKTPriv *pv = priv_of(HKKT);
    if (bytesToHost) *bytesToHost = pv->bytes_d2h;
    if (bytesToDevice) *bytesToDevice = pv->bytes_h2d;
}
void HMiConeSetExchangePieces(hdsdp_cone *cone, hmi_alltoall_piece_fn start, hmi_alltoall_wait_fn wait, int npieces) {
    MiCone *c = cone_data(cone);
    if (!c) return;                   // (not an SDP cone of the engine: nothing to exchange)
    c->a2a_start = start; c->a2a_wait = wait; c->a2a_pieces = std::max(1, npieces);
}
void HMiConeBuildPrimalXSXDirection(hdsdp_cone *cone, double *dPrimalScalMatrix, double *dPrimalXSXBuffer, int iDualMat) {
    cone->coneBuildPrimalDirection(cone->coneData, nullptr, dPrimalScalMatrix, dPrimalXSXBuffer, iDualMat);
}
void HMiConeGetExchangeStats(hdsdp_cone *cone, int *pieces, int *stagedLaunches) {
    MiCone *c = cone_data(cone);
    if (!c) { if (pieces) *pieces = 0; if (stagedLaunches) *stagedLaunches = 0; return; }
    if (pieces) *pieces = c->last_pieces;
    if (stagedLaunches) *stagedLaunches = c->last_staged;
}
int HMiConeGetPrimalRoute(hdsdp_cone *cone, int *negativePivots, double *growth) {
    const MiCone *c = cone_data(cone);
    if (!c || c->primal_route < 0) return -1;
    if (negativePivots) *negativePivots = c->primal_q;
    if (growth) *growth = c->primal_growth;
    return c->primal_route;
}
int HMiConeGetPrimalProfile(hdsdp_cone *cone, double *ms, int64_t *columns) {
    const MiCone *c = cone_data(cone);
    if (!c || c->primal_route != 1) return 1;
    if (ms) for (int k = 0; k < 4; ++k) ms[k] = c->primal_ms[k];
    if (columns) *columns = (int64_t) c->primal_cols;
    return 0;
}
void HMiConeSetExchange(hdsdp_cone *cone, hmi_alltoall_fn a2a, hmi_allreduce_fn ar, void *ctx) {
    MiCone *c = cone_data(cone);
    if (!c) return;
    c->alltoall = a2a; c->allreduce = ar; c->xctx = ctx;
}
hdsdp_retcode HMiConeGetExchangeBuffers(hdsdp_cone *cone, void **sendBuf, void **recvBuf, int64_t *chunkCount) {
    MiCone *c = cone_data(cone);
    if (!c) return HDSDP_RETCODE_FAILED;
    if (chunkCount) *chunkCount = (int64_t) c->npb_loc * c->Lr * 16;
    if (sendBuf) *sendBuf = c->AhatLoc;
    if (recvBuf) *recvBuf = c->AhatAll;
    return HDSDP_RETCODE_OK;
}
hdsdp_retcode HMiConeSetExchangeBuffers(hdsdp_cone *cone, void *sendBuf, void *recvBuf) {
    MiCone *c = cone_data(cone);
    if (!c || c->work_ready || !sendBuf || !recvBuf) return HDSDP_RETCODE_FAILED;
    c->AhatLoc = (double *) sendBuf;
    c->AhatAll = (c->world == 1) ? c->AhatLoc : (double *) recvBuf;
    const size_t ahat = sizeof(double) * hdm_exchange_doubles(cone_layout(c));
    if (hipMemsetAsync(c->AhatLoc, 0, ahat, g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    if (c->AhatAll != c->AhatLoc && hipMemsetAsync(c->AhatAll, 0, ahat, g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    return HDSDP_RETCODE_OK;
}
void *HMiKKTDeviceMatrix(hdsdp_kkt *HKKT, int64_t *ld) {
    long l = 0;
    double *p = kkt_Mdev(HKKT, &l);
    if (ld) *ld = l;
    return p;
}
hdsdp_retcode HMiKKTGetRows(hdsdp_kkt *HKKT, int nRows, const int *rows, double *out) {
    // full symmetric rows of the device copy of M (lower triangle stored: dense matrix or tile store)
    MiKKTPriv *pv = priv_of(HKKT);
    const int m = HKKT->nRow;
    if (!pv->st.m_valid()) return HDSDP_RETCODE_FAILED;
    HdmBuf<double> tmp;
    HIP_RC(tmp.alloc((size_t) std::max(1, m)));
    hdsdp_retcode rc = HDSDP_RETCODE_OK;
    for (int r = 0; r < nRows && rc == HDSDP_RETCODE_OK; ++r) {
        if (rows[r] < 0 || rows[r] >= m) { rc = HDSDP_RETCODE_FAILED; break; }
        pv->bytes_d2h += (int64_t) sizeof(double) * m;
        hipLaunchKernelGGL(mi_get_row_kernel, dim3((m + 255) / 256), dim3(256), 0, g.stream, kkt_view(HKKT), rows[r], m, tmp.get());
        if (hipMemcpyAsync(out + (size_t) r * m, tmp.get(), sizeof(double) * (size_t) m, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
            hipStreamSynchronize(g.stream) != hipSuccess) rc = HDSDP_RETCODE_FAILED;
    }
    return rc;
}
