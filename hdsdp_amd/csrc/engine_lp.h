// engine_lp.h -- the LP cone (the diagonal block of an SDPA file): the reference's hdsdp_conic_lp.c slot for slot, with the
// Schur build M += A diag(d)^2 A^T on the device.
// Implementation header of engine.hip: included exactly once, there, inside the anonymous namespace after engine_build.h
// (its kernels are in lp_kernels.h, at global scope).
//
// What lives where.  The constraint data twice on the device: by constraint row (the reference's rowMatBeg layout: the Schur
// vectors A v) and by LP column (the dual update A^T y).  The host keeps the reference's CSC (feature detection, norms,
// A^T x) and the nCol-long dual buffers: every update is computed on the device from y, brought back, and finished on the host
// in the reference's order (hdsdp_conic_lp.c:46-83), so that the interior checks, the ratio test and the barrier decide
// exactly as the reference does.  The build's scalars (TraceSinv, CSinv, CSinvCSinv) are sums over nCol entries of d and are
// added to the operator's host fields in the reference's order; the vectors and M accumulate on the device.

// buffers (interface/hdsdp_conic.h:24-26) and norms (hdsdp_conic_sdp.c: ABS_NORM 1, FRO_NORM 2)
enum { LP_DUALVAR = 0, LP_DUALCHECK = 1, LP_DUALSTEP = 2, LP_ABS_NORM = 1 };

struct MiLPCone {
    int m = 0, n = 0;
    std::vector<int> rbeg, ridx;         // by constraint row: the reference's rowMatBeg / rowMatIdx / rowMatElem
    std::vector<double> rval;
    std::vector<int> cnt;                // entries per LP column
    std::vector<double> obj, dual, chk, step, dinv;
    double Rd = 0.0, perturb = 0.0;
    HdmBuf<int> d_rbeg, d_ridx, d_cbeg, d_cidx;
    HdmBuf<double> d_rval, d_cval, d_obj, d_y, d_out, d_d;
    HdmPinned<double> h_y, h_out, h_d;   // pinned staging
    // dense path: W = A[:, chunk] diag(d) in the Gram role's K-major blocked layout, kc LP columns per chunk
    int mpad = 0, kc = 0;
    HdmBuf<double> W;
    long wspan = 0;
    // sparse path: lower pairs (i, j) and their terms (k, A_ik A_jk)
    int64_t terms = 0;                   // sum over LP columns of nnz (nnz + 1) / 2
    long npair = 0;
    HdmBuf<int> p_row, p_col, t_col;
    HdmBuf<long> p_beg;
    HdmBuf<double> t_val;
    bool pairs_ready = false;
    int mode = 0, path = 0;              // mode: 0 auto, 1 dense, 2 sparse; path: what builds use (1 / 2)
    double cost_dense = 0.0, cost_sparse = 0.0;
};

constexpr double LP_PAIR_CAP = 1073741824.0;   // bytes a pair list may take on the device (1 GiB)
constexpr int LP_KC_MAX = 8192;

int64_t lp_sparse_bytes(const MiLPCone *c) {
    const double pairs = std::min<double>((double) c->terms, 0.5 * (double) c->m * (c->m + 1));
    return (int64_t) (12.0 * (double) c->terms + 16.0 * pairs);
}

// The path rule: modelled seconds of one build on either path.  Dense: the lower half of W W^T on the matrix
// pipe at 40 TFLOP/s (about half the fp64 MFMA peak, what the Gram role sustains at these shapes) plus the zeroing, scatter and
// read of W at 3 TB/s and a launch per chunk.  Sparse: the pair list read once at 3 TB/s.  The sparse path is taken when it is
// modelled faster and its list fits LP_PAIR_CAP.
void lp_plan(MiLPCone *c) {
    const double m = c->m, K = (double) hdm_roundup(c->n, 16);
    const long chunks = (c->n + c->kc - 1) / c->kc;
    c->cost_dense = m * m * K / 40e12 + 3.0 * 8.0 * c->mpad * K / 3e12 + 3.0 * chunks * 5e-6;
    const double sb = (double) lp_sparse_bytes(c);
    c->cost_sparse = (sb <= LP_PAIR_CAP) ? sb / 3e12 + 5e-6 : INFINITY;
}

int lp_build_pairs(MiLPCone *c) {
    if (c->pairs_ready) return 0;
    if ((double) lp_sparse_bytes(c) > LP_PAIR_CAP) return 1;
    // by LP column, ascending constraint (the by-row lists read column-wise)
    std::vector<int> cb((size_t) c->n + 1, 0);
    for (int j = 0; j < c->n; ++j) cb[j + 1] = cb[j] + c->cnt[j];
    std::vector<int> ci(c->rval.size()), pos(cb.begin(), cb.end() - 1);
    std::vector<double> cv(c->rval.size());
    for (int i = 0; i < c->m; ++i)
        for (int e = c->rbeg[i]; e < c->rbeg[i + 1]; ++e) { const int j = c->ridx[e]; ci[pos[j]] = i; cv[pos[j]++] = c->rval[e]; }
    struct Term { int64_t key; int k; double v; };
    std::vector<Term> t;
    t.reserve((size_t) c->terms);
    for (int k = 0; k < c->n; ++k)
        for (int a = cb[k]; a < cb[k + 1]; ++a)
            for (int b = cb[k]; b <= a; ++b) {
                int i = ci[a], j = ci[b];
                if (i < j) std::swap(i, j);
                t.push_back({(int64_t) i + (int64_t) j * c->m, k, cv[a] * cv[b]});
            }
    std::stable_sort(t.begin(), t.end(), [](const Term &x, const Term &y) { return x.key < y.key; });   // k stays ascending in a pair
    std::vector<int> prow, pcol, tcol(t.size());
    std::vector<long> pbeg;
    std::vector<double> tval(t.size());
    for (size_t q = 0; q < t.size(); ++q) {
        if (q == 0 || t[q].key != t[q - 1].key) {
            prow.push_back((int) (t[q].key % c->m)); pcol.push_back((int) (t[q].key / c->m)); pbeg.push_back((long) q);
        }
        tcol[q] = t[q].k; tval[q] = t[q].v;
    }
    pbeg.push_back((long) t.size());
    c->npair = (long) prow.size();
    const size_t np = std::max<size_t>(1, prow.size()), nt = std::max<size_t>(1, t.size());
    if (c->p_row.alloc(np) != hipSuccess || c->p_col.alloc(np) != hipSuccess ||
        c->p_beg.alloc(np + 1) != hipSuccess || c->t_col.alloc(nt) != hipSuccess ||
        c->t_val.alloc(nt) != hipSuccess)
        return 1;
    if ((c->npair && (hdm_memcpy_h2d_sync(c->p_row.get(), prow.data(), sizeof(int) * prow.size()) != hipSuccess ||
                      hdm_memcpy_h2d_sync(c->p_col.get(), pcol.data(), sizeof(int) * pcol.size()) != hipSuccess ||
                      hdm_memcpy_h2d_sync(c->t_col.get(), tcol.data(), sizeof(int) * tcol.size()) != hipSuccess ||
                      hdm_memcpy_h2d_sync(c->t_val.get(), tval.data(), sizeof(double) * tval.size()) != hipSuccess)) ||
        hdm_memcpy_h2d_sync(c->p_beg.get(), pbeg.data(), sizeof(long) * pbeg.size()) != hipSuccess)
        return 1;
    c->pairs_ready = true;
    return 0;
}

int lp_build_dense_buffer(MiLPCone *c) {
    if (c->W) return 0;
    c->wspan = hdm_lp_span(c->kc, c->mpad);
    if (c->W.alloc((size_t) c->wspan) != hipSuccess) return 1;
    return hdm_memset_sync(c->W.get(), 0, sizeof(double) * (size_t) c->wspan) != hipSuccess;
}

int lp_set_path(MiLPCone *c, int mode) {
    int path = mode;
    if (mode == 0) path = (c->cost_sparse < c->cost_dense) ? 2 : 1;
    if (path == 2 && lp_build_pairs(c)) return 1;
    if (path == 1 && lp_build_dense_buffer(c)) return 1;
    c->mode = mode;
    c->path = path;
    return 0;
}

// out = A^T (a y), length nCol, on the device (csp_Axpy's arithmetic), copied back into `out`
int lp_at_y(MiLPCone *c, double a, const double *y, double *out) {
    if (a == 0.0) { std::fill(out, out + c->n, 0.0); return 0; }     // (csp_Axpy returns at once, :23-25)
    memcpy(c->h_y.get(), y, sizeof(double) * c->m);
    if (hipMemcpyAsync(c->d_y.get(), c->h_y.get(), sizeof(double) * c->m, hipMemcpyHostToDevice, g.stream) != hipSuccess) return 1;
    hipLaunchKernelGGL(lp_col_axpy_kernel, dim3((c->n + 255) / 256), dim3(256), 0, g.stream, c->n, c->d_cbeg.get(), c->d_cidx.get(), c->d_cval.get(), a,
                       (const double *) c->d_y.get(), c->d_out.get());
    if (hipMemcpyAsync(c->h_out.get(), c->d_out.get(), sizeof(double) * c->n, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
        hipStreamSynchronize(g.stream) != hipSuccess) return 1;
    memcpy(out, c->h_out.get(), sizeof(double) * c->n);
    return 0;
}

double *lp_buffer(MiLPCone *c, int which) {
    return which == LP_DUALVAR ? c->dual.data() : which == LP_DUALCHECK ? c->chk.data() : c->step.data();
}

// LPConeIUpdateBuffer (:46-83)
void lp_update_buffer(MiLPCone *c, double dCCoef, double dACoefScal, const double *dACoef, double dEyeCoef, int which) {
    double *t = lp_buffer(c, which);
    if (lp_at_y(c, dACoefScal, dACoef, t)) {
        fprintf(stderr, "[hdsdp_mi355x] LP cone: dual update failed on the device\n");
        std::fill(t, t + c->n, NAN);
        return;
    }
    for (int j = 0; j < c->n; ++j) t[j] += dCCoef * c->obj[j];
    if (which != LP_DUALSTEP) dEyeCoef += c->perturb;
    if (dEyeCoef != 0.0)
        for (int j = 0; j < c->n; ++j) t[j] += dEyeCoef;
}
int lp_is_interior(const MiLPCone *c, const double *t) {
    for (int j = 0; j < c->n; ++j)
        if (t[j] <= 0.0) return 0;
    return 1;
}

// ---------------------------------------------------------------- slots
void lp_destroy_data(void **pcd) {
    MiLPCone *c = (MiLPCone *) *pcd;
    if (!c) return;
    delete c;
    *pcd = nullptr;
}
void lp_setstart(void *cd, double rResi) { ((MiLPCone *) cd)->Rd = rResi; }                          // :169-173
void lp_update(void *cd, double tau, double *y) {                                                   // :216-221
    MiLPCone *c = (MiLPCone *) cd;
    lp_update_buffer(c, tau, -1.0, y, -c->Rd, LP_DUALVAR);
}
hdsdp_retcode lp_ratio_test(void *cd, double dTauStep, double *dy, double dAdaRatio, int whichBuffer, double *maxStep) {   // :223-259
    MiLPCone *c = (MiLPCone *) cd;
    lp_update_buffer(c, dTauStep, -1.0, dy, dAdaRatio * c->Rd, LP_DUALSTEP);
    const double *t = (whichBuffer == LP_DUALVAR) ? c->dual.data() : c->chk.data();
    double s = 0.0;
    for (int j = 0; j < c->n; ++j) s = std::min(s, c->step[j] / t[j]);
    s = 1.0 / s;
    *maxStep = (s > 0.0) ? 100.0 : -s;     // no blocking component: 1 / 0 = +inf -> 100
    return HDSDP_RETCODE_OK;
}
int64_t lp_getsymnnz(void *cd) { const MiLPCone *c = (const MiLPCone *) cd; return (int64_t) c->m * c->m; }   // :135-136, :375-378
int lp_getdim(void *cd) { return ((MiLPCone *) cd)->n; }

hdsdp_retcode lp_build_schur(void *cd, int iCone, void *kktv, int typeKKT) {   // LPConeGetKKT, :266-348
    MiLPCone *c = (MiLPCone *) cd;
    hdsdp_kkt *kkt = (hdsdp_kkt *) kktv;
    MiKKTPriv *pv = priv_of(kkt);
    if (kkt->nRow != c->m) { fprintf(stderr, "[hdsdp_mi355x] LP cone of %d rows in an operator of %d\n", c->m, kkt->nRow); return HDSDP_RETCODE_FAILED; }
    if (typeKKT == KKT_TYPE_PRIMAL) {
        if (!kkt->dPrimalX || !kkt->dPrimalX[iCone]) return HDSDP_RETCODE_FAILED;
        memcpy(c->dinv.data(), kkt->dPrimalX[iCone], sizeof(double) * c->n);
    } else {
        for (int j = 0; j < c->n; ++j) c->dinv[j] = 1.0 / c->dual[j];
    }
    const double *d = c->dinv.data();
    // the scalars, in the reference's order, straight into the host fields (kkt_pull adds the device part after the builds)
    if (c->Rd != 0.0) for (int j = 0; j < c->n; ++j) kkt->dTraceSinv += d[j];
    if (typeKKT == KKT_TYPE_HOMOGENEOUS)
        for (int j = 0; j < c->n; ++j) {
            const double cs = c->obj[j] * d[j];
            kkt->dCSinv += cs;
            kkt->dCSinvCSinv += cs * cs;
        }
    HIP_RC(hipStreamSynchronize(g.stream));      // (h_d may still feed the previous build's copy)
    memcpy(c->h_d.get(), d, sizeof(double) * c->n);
    HIP_RC(hipMemcpyAsync(c->d_d.get(), c->h_d.get(), sizeof(double) * c->n, hipMemcpyHostToDevice, g.stream));
    if (c->m > 0)
        hipLaunchKernelGGL(lp_vecs_kernel, dim3(c->m), dim3(256), 0, g.stream, c->m, (const int *) c->d_rbeg.get(), (const int *) c->d_ridx.get(),
                           (const double *) c->d_rval.get(), (const double *) c->d_d.get(), (const double *) c->d_obj.get(), c->Rd,
                           typeKKT == KKT_TYPE_HOMOGENEOUS ? 1 : 0, pv->vecs.get());
    HIP_RC(hipGetLastError());
    if (typeKKT == KKT_TYPE_CORRECTOR) return HDSDP_RETCODE_OK;
    MiLin *l = (MiLin *) kkt->kktM->chol;
    if (kkt->isKKTSparse || l->bsp || !l->Mdev.get()) {
        fprintf(stderr, "[hdsdp_mi355x] LP cone: the Schur operator is not dense\n");   // (the reference asserts, :303-305)
        return HDSDP_RETCODE_FAILED;
    }
    const long ldm = l->ch.npad;
    if (c->path == 2) {
        if (c->npair > 0)
            hipLaunchKernelGGL(lp_pairs_kernel, dim3((unsigned) ((c->npair + 255) / 256)), dim3(256), 0, g.stream, c->npair,
                               (const int *) c->p_row.get(), (const int *) c->p_col.get(), (const long *) c->p_beg.get(), (const int *) c->t_col.get(),
                               (const double *) c->t_val.get(), (const double *) c->d_d.get(), l->Mdev.get(), ldm);
        HIP_RC(hipGetLastError());
        return HDSDP_RETCODE_OK;
    }
    // dense path: chunk by chunk, W = A[:, chunk] diag(d) and M(lower) += W W^T on the Gram role (K-major operands, STORE
    // epilogue with beta = 1).  The role's edge tiles compute whole 16-row sub-tiles only (its own launches have R rows, a
    // multiple of 16 in practice), so the product runs over m16 rows; rows m .. m16 - 1 of W are zero and add nothing to the
    // padding of M (npad, a multiple of 128, is at least m16)
    const int m16 = (int) hdm_roundup(c->m, 16);
    const long ldb = (long) c->mpad * 16;
    for (int c0 = 0; c0 < c->n; c0 += c->kc) {
        const int kv = std::min(c->kc, c->n - c0), kp = (int) hdm_roundup(kv, 16);
        HIP_RC(hipMemsetAsync(c->W.get(), 0, sizeof(double) * (size_t) (kp / 16) * ldb, g.stream));
        hipLaunchKernelGGL(lp_scatter_kernel, dim3((kv + 255) / 256), dim3(256), 0, g.stream, c0, kv, (const int *) c->d_cbeg.get(),
                           (const int *) c->d_cidx.get(), (const double *) c->d_cval.get(), (const double *) c->d_d.get(), ldb, c->W.get());
        HIP_RC(hipGetLastError());
        RC(hdm_launch_gemm(hdm_gram_lp(c->m, m16, c->mpad, c->kc, kv, kp, c->W.get(), l->Mdev.get(), ldm), g.stream));
    }
    return HDSDP_RETCODE_OK;
}
hdsdp_retcode lp_build_schur_fixed(void *cd, int iCone, void *kktv, int typeKKT, int strategy) {   // :366-370
    (void) strategy;
    return lp_build_schur(cd, iCone, kktv, typeKKT);
}
void lp_build_primal_dir(void *cd, void *kktv, double *X, double *XSX, int iDualMat) {   // :350-364
    (void) kktv;
    MiLPCone *c = (MiLPCone *) cd;
    const double *s = iDualMat ? c->dual.data() : c->step.data();
    for (int j = 0; j < c->n; ++j) XSX[j] = X[j] * X[j] * s[j];
}
hdsdp_retcode lp_interior(void *cd, double tau, double *y, int *isInterior) {   // :390-396
    MiLPCone *c = (MiLPCone *) cd;
    lp_update(c, tau, y);
    *isInterior = lp_is_interior(c, c->dual.data());
    return HDSDP_RETCODE_OK;
}
hdsdp_retcode lp_interior_expert(void *cd, double dCCoef, double dACoefScal, double *dACoef, double dEyeCoef, int whichBuffer,
                                 int *isInterior) {   // :398-410
    MiLPCone *c = (MiLPCone *) cd;
    lp_update_buffer(c, dCCoef, dACoefScal, dACoef, dEyeCoef, whichBuffer);
    *isInterior = lp_is_interior(c, whichBuffer == LP_DUALVAR ? c->dual.data() : c->chk.data());
    return HDSDP_RETCODE_OK;
}
hdsdp_retcode lp_barrier(void *cd, double tau, double *y, int whichBuffer, double *logdet) {   // :425-447
    MiLPCone *c = (MiLPCone *) cd;
    const double *t = (whichBuffer == LP_DUALVAR) ? c->dual.data() : c->chk.data();
    if (y) lp_update(c, tau, y);
    double s = 0.0;
    for (int j = 0; j < c->n; ++j) s += log(t[j]);
    *logdet = s;
    return HDSDP_RETCODE_OK;
}
hdsdp_retcode lp_axpy_check(void *cd, double dStep, int whichBuffer, int *isInterior) {   // :449-464
    MiLPCone *c = (MiLPCone *) cd;
    double *t = c->dual.data();
    if (whichBuffer != LP_DUALVAR) { t = c->chk.data(); c->chk = c->dual; }
    for (int j = 0; j < c->n; ++j) t[j] += dStep * c->step[j];
    *isInterior = lp_is_interior(c, t);
    return HDSDP_RETCODE_OK;
}
void lp_reduce_resi(void *cd, double v) { ((MiLPCone *) cd)->Rd = v; }        // :412-416
void lp_set_perturb(void *cd, double v) { ((MiLPCone *) cd)->perturb = v; }   // :418-423
void lp_precover(void *cd, double dBarrierMu, double *y, double *dy, double *X, double *aux) {   // LPConeGetPrimal, :466-487
    (void) aux;
    MiLPCone *c = (MiLPCone *) cd;
    lp_update_buffer(c, 1.0, -1.0, y, 0.0, LP_DUALCHECK);
    if (!lp_is_interior(c, c->chk.data())) {
        printf("Recovery step is infeasible\n");   // (the reference returns HDSDP_RETCODE_FAILED; the slot is void)
        return;
    }
    lp_update_buffer(c, 0.0, 1.0, dy, 0.0, LP_DUALSTEP);
    for (int j = 0; j < c->n; ++j) X[j] = dBarrierMu * (c->chk[j] + c->step[j]) / (c->chk[j] * c->chk[j]);
}
void lp_get_dual(void *cd, double *dConeDual, double *dummy) {   // :489-493
    (void) dummy;
    MiLPCone *c = (MiLPCone *) cd;
    memcpy(dConeDual, c->dual.data(), sizeof(double) * c->n);
}
void lp_a_times_x(void *cd, double *X, double *ATimesX) {   // csp_ATxpy, :507-513
    MiLPCone *c = (MiLPCone *) cd;
    for (int i = 0; i < c->m; ++i) {
        double a = 0.0;
        for (int e = c->rbeg[i]; e < c->rbeg[i + 1]; ++e) a += X[c->ridx[e]] * c->rval[e];
        ATimesX[i] += 1.0 * a;
    }
}
double lp_trace_cx(void *cd, double *X) {   // :495-505
    MiLPCone *c = (MiLPCone *) cd;
    double s = 0.0;
    for (int j = 0; j < c->n; ++j) s += c->obj[j] * X[j];
    return s;
}
double lp_x_dot_s(void *cd, double *X) {   // :361-364
    MiLPCone *c = (MiLPCone *) cd;
    double s = 0.0;
    for (int j = 0; j < c->n; ++j) s += c->dual[j] * X[j];
    return s;
}
double lp_coeff_norm(void *cd, int whichNorm) {   // :193-203, csp_sum_abs / csp_fro_norm (the "diagonal" entries, LP column ==
    MiLPCone *c = (MiLPCone *) cd;                //  constraint index, count half there too)
    double s = 0.0;
    for (int i = 0; i < c->m; ++i)
        for (int e = c->rbeg[i]; e < c->rbeg[i + 1]; ++e) {
            const double v = c->rval[e];
            if (whichNorm == LP_ABS_NORM) s += (c->ridx[e] == i) ? 0.5 * fabs(v) : fabs(v);
            else s += (c->ridx[e] == i) ? 0.5 * v * v : v * v;
        }
    return whichNorm == LP_ABS_NORM ? s : sqrt(s);
}
double lp_obj_norm(void *cd, int whichNorm) {   // :175-191
    MiLPCone *c = (MiLPCone *) cd;
    double s = 0.0;
    if (whichNorm == LP_ABS_NORM) for (int j = 0; j < c->n; ++j) s += fabs(c->obj[j]);
    else { for (int j = 0; j < c->n; ++j) s += c->obj[j] * c->obj[j]; s = sqrt(s); }
    return s;
}
void lp_scal(void *cd, double dScal) {   // :205-209: rscl, i.e. LAPACK drscl: x *= 1 / a
    MiLPCone *c = (MiLPCone *) cd;
    const double r = 1.0 / dScal;
    for (int j = 0; j < c->n; ++j) c->obj[j] *= r;
    if (hdm_memcpy_h2d_sync(c->d_obj.get(), c->obj.data(), sizeof(double) * c->n) != hipSuccess)
        fprintf(stderr, "[hdsdp_mi355x] LP cone: objective upload failed\n");
}
void lp_view(void *cd) {   // :560-565 (the reference prints its two counts the other way round)
    MiLPCone *c = (MiLPCone *) cd;
    printf("LP Cone of %d variables and %d constraints \n", c->m, c->n);
}
// LPConeGetStatsImpl (:567-667): implied bounds on y and free primal variables, on the host copy
void lp_getstat(void *cd, double *rowRHS, int intF[20], double dblF[20]) {
    (void) rowRHS;
    enum { F_NODINTERIOR = 3, F_IMPYBOUND = 6, D_IMPYBOUNDUP = 9, D_IMPYBOUNDLOW = 10 };
    MiLPCone *c = (MiLPCone *) cd;
    if (c->n % 2 != 0 || c->n < 100) return;
    std::vector<double> lo((size_t) c->m, 0.0), up((size_t) c->m, 0.0);
    const int half = c->n / 2;
    int implied = 1, hasUp = 0, hasLo = 0;
    double maxUp = 1.0, minLo = -1.0;
    for (int i = 0; i < c->m; ++i) {
        for (int e = c->rbeg[i]; e < c->rbeg[i + 1]; ++e) {
            if (c->rbeg[i + 1] - c->rbeg[i] > 2) { implied = 0; break; }
            const double v = c->rval[e];
            if (v > 0.0) {
                if (up[i]) { implied = 0; break; }
                hasUp = 1;
                up[i] = std::max(up[i], c->obj[c->ridx[e]] / v);
            } else {
                if (lo[i]) { implied = 0; break; }
                hasLo = 1;
                lo[i] = std::min(lo[i], c->obj[c->ridx[e]] / v);
            }
        }
        if (!implied) break;
    }
    if (implied) {
        intF[F_IMPYBOUND] = 1;
        if (hasUp) {
            for (int i = 0; i < c->m; ++i) maxUp = std::max(maxUp, up[i]);
            if (maxUp <= 0.0) maxUp = 1.0;
            dblF[D_IMPYBOUNDUP] = maxUp;
        }
        if (hasLo) {
            for (int i = 0; i < c->m; ++i) minLo = std::min(minLo, lo[i]);
            if (minLo >= 0.0) minLo = -1.0;
            dblF[D_IMPYBOUNDLOW] = minLo;
        }
    }
    for (int j = 0; j < half; ++j)
        if (c->obj[j] + c->obj[j + half] != 0.0) return;
    for (int i = 0; i < c->m; ++i) {
        const int nz = c->rbeg[i + 1] - c->rbeg[i], h = nz / 2;
        if (nz % 2 != 0) return;
        for (int r = 0; r < h; ++r)
            if (c->rval[c->rbeg[i] + r] + c->rval[c->rbeg[i] + r + h] != 0.0) return;
    }
    intF[F_NODINTERIOR] = 1;
}

// LPConeProcDataImpl (:101-160): CSC of nCol rows and nRow + 1 columns, column 0 = the objective
hdsdp_retcode lp_cone_create(hdsdp_cone **pCone, int iCone, int nRow, int nCol, const int *beg, const int *idx, const double *val) {
    if (!pCone || nRow < 1 || nCol < 1 || !beg || beg[0] != 0) return HDSDP_RETCODE_FAILED;
    for (int i = 0; i <= nRow; ++i)
        if (beg[i + 1] < beg[i]) return HDSDP_RETCODE_FAILED;
    for (int e = 0; e < beg[nRow + 1]; ++e)
        if (!idx || !val || idx[e] < 0 || idx[e] >= nCol) {
            fprintf(stderr, "[hdsdp_mi355x] HMiConeCreateLP: entry %d names LP column %d of %d\n", e, idx ? idx[e] : -1, nCol);
            return HDSDP_RETCODE_FAILED;
        }
    if (ensure_ctx()) return HDSDP_RETCODE_FAILED;
    MiLPCone *c = new MiLPCone();
    c->m = nRow; c->n = nCol;
    c->obj.assign((size_t) nCol, 0.0);
    for (int e = 0; e < beg[1]; ++e) c->obj[idx[e]] = val[e];
    const int o = beg[1], nnz = beg[nRow + 1] - o;
    c->rbeg.resize((size_t) nRow + 1);
    for (int i = 0; i <= nRow; ++i) c->rbeg[i] = beg[i + 1] - o;
    c->ridx.assign(idx + o, idx + o + nnz);
    c->rval.assign(val + o, val + o + nnz);
    c->dual.assign((size_t) nCol, 0.0); c->chk = c->dual; c->step = c->dual; c->dinv = c->dual;
    c->cnt.assign((size_t) nCol, 0);
    for (int e = 0; e < nnz; ++e) c->cnt[c->ridx[e]] += 1;
    for (int j = 0; j < nCol; ++j) c->terms += (int64_t) c->cnt[j] * (c->cnt[j] + 1) / 2;
    // by LP column, ascending constraint
    std::vector<int> cb((size_t) nCol + 1, 0), ci((size_t) std::max(1, nnz));
    std::vector<double> cv((size_t) std::max(1, nnz));
    for (int j = 0; j < nCol; ++j) cb[j + 1] = cb[j] + c->cnt[j];
    {
        std::vector<int> pos(cb.begin(), cb.end() - 1);
        for (int i = 0; i < nRow; ++i)
            for (int e = c->rbeg[i]; e < c->rbeg[i + 1]; ++e) { const int j = c->ridx[e]; ci[pos[j]] = i; cv[pos[j]++] = c->rval[e]; }
    }
    c->mpad = (int) hdm_roundup(nRow, 128);
    c->kc = (int) std::min<long>(hdm_roundup(nCol, 16), std::max<long>(16, ((1L << 25) / c->mpad) / 16 * 16));
    c->kc = std::min(c->kc, LP_KC_MAX);
    const size_t nz1 = (size_t) std::max(1, nnz);
    bool ok = c->d_rbeg.alloc(nRow + 1) == hipSuccess && c->d_ridx.alloc(nz1) == hipSuccess &&
              c->d_rval.alloc(nz1) == hipSuccess && c->d_cbeg.alloc(nCol + 1) == hipSuccess &&
              c->d_cidx.alloc(nz1) == hipSuccess && c->d_cval.alloc(nz1) == hipSuccess &&
              c->d_obj.alloc(nCol) == hipSuccess && c->d_y.alloc(nRow) == hipSuccess &&
              c->d_out.alloc(nCol) == hipSuccess && c->d_d.alloc(nCol) == hipSuccess &&
              c->h_y.alloc(nRow) == hipSuccess &&
              c->h_out.alloc(nCol) == hipSuccess &&
              c->h_d.alloc(nCol) == hipSuccess;
    ok = ok && hdm_memcpy_h2d_sync(c->d_rbeg.get(), c->rbeg.data(), sizeof(int) * (nRow + 1)) == hipSuccess &&
         hdm_memcpy_h2d_sync(c->d_cbeg.get(), cb.data(), sizeof(int) * (nCol + 1)) == hipSuccess &&
         hdm_memcpy_h2d_sync(c->d_obj.get(), c->obj.data(), sizeof(double) * nCol) == hipSuccess &&
         (nnz == 0 || (hdm_memcpy_h2d_sync(c->d_ridx.get(), c->ridx.data(), sizeof(int) * nnz) == hipSuccess &&
                       hdm_memcpy_h2d_sync(c->d_rval.get(), c->rval.data(), sizeof(double) * nnz) == hipSuccess &&
                       hdm_memcpy_h2d_sync(c->d_cidx.get(), ci.data(), sizeof(int) * nnz) == hipSuccess &&
                       hdm_memcpy_h2d_sync(c->d_cval.get(), cv.data(), sizeof(double) * nnz) == hipSuccess));
    lp_plan(c);
    ok = ok && lp_set_path(c, 0) == 0;
    if (!ok) {
        void *p = c;
        lp_destroy_data(&p);
        fprintf(stderr, "[hdsdp_mi355x] HMiConeCreateLP: device allocation or upload failed\n");
        return HDSDP_RETCODE_MEMORY;
    }
    hdsdp_cone *h = (hdsdp_cone *) calloc(1, sizeof(hdsdp_cone));
    h->iCone = iCone;
    h->cone = HDSDP_CONETYPE_LP;
    h->coneData = c;
    h->coneDestroyData = lp_destroy_data;
    h->coneSetStart = lp_setstart;
    h->coneUpdate = lp_update;
    h->coneRatioTest = lp_ratio_test;
    h->coneGetSymNnz = lp_getsymnnz;
    h->coneGetDim = lp_getdim;
    h->coneAddSymNz = nullptr;            // (the reference asserts: an LP cone makes the Schur matrix dense, :375-388)
    h->coneGetKKTMap = nullptr;
    h->coneBuildSchur = lp_build_schur;
    h->coneBuildSchurFixed = lp_build_schur_fixed;
    h->coneBuildPrimalDirection = lp_build_primal_dir;
    h->coneInteriorCheck = lp_interior;
    h->coneInteriorCheckExpert = lp_interior_expert;
    h->coneGetBarrier = lp_barrier;
    h->coneAxpyBufferAndCheck = lp_axpy_check;
    h->coneReduceResi = lp_reduce_resi;
    h->coneSetPerturb = lp_set_perturb;
    h->conePRecover = lp_precover;
    h->coneDRecover = lp_get_dual;
    h->coneATimesXpy = lp_a_times_x;
    h->coneTraceCX = lp_trace_cx;
    h->coneXDotS = lp_x_dot_s;
    h->coneGetCoeffNorm = lp_coeff_norm;
    h->coneGetObjNorm = lp_obj_norm;
    h->coneScal = lp_scal;
    h->coneView = lp_view;
    h->getstat = lp_getstat;
    *pCone = h;
    return HDSDP_RETCODE_OK;
}
