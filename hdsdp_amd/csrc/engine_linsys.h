// engine_linsys.h -- the linear-system objects behind HFpLinsys* (dense / CSC-in dual matrices, the Schur system with its pivoted way out)
// Implementation header of engine.hip: included exactly once, there, in this order (the pieces share the anonymous namespace
// and the engine's thread-local context `g`); split out of a 3 300-line file in round 3, nothing else changed.
// Whether a system is switched to the pivoted solver and where its last factorised matrix came from is HdmKktState's
// (kkt_store.h, with the table of how the Schur operator's matrix reaches the factor): lin_factor_indef reads the source from it.
// The refined solve (lin_solve_refined: refine_rule.h's loop on refine.hip's residual) asks the same state what its residual reads;
// lin_refine_column is that loop once, over what a storage form supplies (the dense forms, the tile form).
// =============================================================================================
// linear-system objects
// =============================================================================================
// the last refined solve and the running totals (HMiLinsysGetRefine)
struct HdmRefineStats {
    int status = HDM_REFINE_OFF, steps = 0;
    double resid0 = 0.0, resid = 0.0, tol = 0.0;
    int64_t solves = 0, total_steps = 0;
    void unrefined(HdmRefineStatus why) { status = why; steps = 0; resid0 = resid = tol = 0.0; }
};

struct MiLin {
    int n = 0;
    linsys_type type = HDSDP_LINSYS_DENSE_DIRECT;
    HdmChol ch;
    HdmBuf<double> work;     // npad x npad device scratch (Invert)
    double relTol = 0, absTol = 0;
    int maxIter = -1;
    // Schur systems: M lives here (device, ld = ch.npad) before factorisation
    HdmBuf<double> Mdev;
    // sparse Schur operator in tile form (bsparse.h): the matrix and its factor are 128 x 128 tiles inside the block pattern of
    // the Cholesky factor; no dense m x m array exists anywhere (ch stays uninitialised, Mdev null)
    std::unique_ptr<HdmBsp> bsp;
    // symmetric-indefinite fallback (HFpLinsysSwitchToIndefinite, hdsdp_linsolver.c:1827-1857): once switched (st->indef()),
    // every later factorisation goes through the pivoted solver, like the reference's replaced vtable
    std::unique_ptr<HdmLu> lu;
    // whether the solver is switched and where the last factorised matrix came from (kkt_store.h).  A Schur operator's linear
    // system shares the operator's state (HKKTInit points st at it); any other has its own: a dense host matrix.
    HdmKktState own, *st = &own;
    // sparse Schur operator: the factor object holds P M P' (perm[old] = new, a bandwidth-reducing order of the pattern);
    // right-hand sides go in permuted and solutions come back in the caller's order.  Empty = identity.
    std::vector<int> perm;
    std::vector<double> pbuf;
    // HDSDP_LINSYS_SPARSE_DIRECT (the reference's QDLDL backend for a sparse dual matrix, hdsdp_linsolver.c:509-809):
    // the matrix arrives as a lower-triangular CSC and is factored densely on the device.  Result-equivalent for every
    // caller: QDLDL's forward / backward solves carry the D^-1/2 scaling (:669-721), i.e. they ARE the Cholesky factor's,
    // GetDiag returns sqrt(D) (:746-756), Invert the full inverse (:758-772); a fill-reducing order only changes the
    // factor by an orthogonal similarity, which neither logdet nor the Lanczos spectrum sees.
    bool csc_in = false;
    std::vector<int> cscBeg, cscIdx;
    std::vector<double> dense;
    // the refined solve (refine_rule.h, refine.hip).  Whether it is on and what its residual reads is the
    // state's (kkt_store.h: hdm_kkt_refine_source); everything here is allocated at the first use and freed when it goes off.
    struct Refine : HdmRefineStats {
        HdmSymRes res;
        HdmBspRefine tiles;        // the tile form's part (refine.h): plan, slots, vectors, and the copy of the factor store
        HdmBuf<double> Mcopy;      // npad x npad: the loaded image of a host matrix, as the factorisation saw it
        HdmBuf<double> v;          // 5 npad + 8: right-hand side, iterate, previous iterate, unrefined solution, residual; |r|^2
        HdmBuf<int> perm;          // device copy of MiLin::perm
        std::vector<double> stage; // the returned iterate on its way to the caller
        void release() { res.part.reset(); res.npart.reset(); Mcopy.reset(); v.reset(); perm.reset(); stage.clear(); stage.shrink_to_fit(); tiles.release(); }
        int64_t bytes() const { return (int64_t) (res.bytes() + sizeof(double) * (Mcopy.count() + v.count()) + sizeof(int) * perm.count() + tiles.bytes()); }
    } rf;
};

hdsdp_retcode lin_create(void **pchol, int nCol) {
    if (ensure_ctx()) return HDSDP_RETCODE_FAILED;
    MiLin *l = new MiLin();
    l->n = nCol;
    if (l->ch.init(nCol)) { delete l; return HDSDP_RETCODE_MEMORY; }
    *pchol = l;
    return HDSDP_RETCODE_OK;
}
void lin_setparam(void *chol, void *param) { (void) chol; (void) param; }
hdsdp_retcode lin_symbolic(void *chol, int *colMatBeg, int *colMatIdx) {
    MiLin *l = (MiLin *) chol;
    if (l->csc_in && colMatBeg && colMatIdx) {   // keep the pattern: later calls may pass it again or not at all
        l->cscBeg.assign(colMatBeg, colMatBeg + l->n + 1);
        l->cscIdx.assign(colMatIdx, colMatIdx + colMatBeg[l->n]);
    }
    return HDSDP_RETCODE_OK;
}
// lower-triangular CSC -> dense n x n column-major (lower triangle valid), on the host: a format conversion of n^2 doubles
const double *lin_densify(MiLin *l, const int *colMatBeg, const int *colMatIdx, const double *colMatElem) {
    const int *beg = colMatBeg ? colMatBeg : (l->cscBeg.empty() ? nullptr : l->cscBeg.data());
    const int *idx = colMatIdx ? colMatIdx : (l->cscIdx.empty() ? nullptr : l->cscIdx.data());
    if (!beg || !idx || !colMatElem) return nullptr;
    const size_t n = (size_t) l->n;
    l->dense.assign(n * n, 0.0);
    for (size_t j = 0; j < n; ++j)
        for (int p = beg[j]; p < beg[j + 1]; ++p) {
            const size_t i = (size_t) idx[p];
            if (i >= j) l->dense[i + j * n] = colMatElem[p];
            else l->dense[j + i * n] = colMatElem[p];     // an upper entry, should a caller hand one over
        }
    return l->dense.data();
}

// the loaded image of a host matrix (n x n of `img`, on the device) is kept for the refined solve's residual: asked for by the
// state after the load and before the factorisation overwrites it
hdsdp_retcode lin_refine_keep_image(MiLin *l, const double *img, long ldimg) {
    if (!l->st->refine_wants_copy()) return HDSDP_RETCODE_OK;
    const size_t npad = (size_t) l->ch.npad;
    if (l->rf.Mcopy.reserve(npad * npad) != hipSuccess) return HDSDP_RETCODE_MEMORY;
    HIP_RC(hipMemcpy2DAsync(l->rf.Mcopy.get(), sizeof(double) * npad, img, sizeof(double) * (size_t) ldimg, sizeof(double) * (size_t) l->n,
                            (size_t) l->n, hipMemcpyDeviceToDevice, g.stream));
    return HDSDP_RETCODE_OK;
}
hdsdp_retcode lin_factor_host(MiLin *l, const double *A, int *info) {
    RC(l->ch.load_host(A, l->n, g.stream));
    RC(lin_refine_keep_image(l, l->ch.L.get(), l->ch.npad));
    RC(l->ch.factor(g.stream, info));
    return HDSDP_RETCODE_OK;
}
// lapackIndefiniteLinSolverNumeric (hdsdp_linsolver.c:1706-1727): copy + pivoted factorisation; a singular matrix fails
hdsdp_retcode lin_factor_indef(MiLin *l) {
    if (!l->lu) {
        l->lu.reset(new HdmLu());
        if (l->lu->init(l->n)) { l->lu.reset(); return HDSDP_RETCODE_MEMORY; }
    }
    if (l->st->src_dev()) RC(l->lu->load_device_lower(l->st->src_dev(), l->st->src_ld(), g.stream));
    else if (l->st->src_host()) {
        RC(l->lu->load_host_lower(l->st->src_host(), l->st->src_ld(), g.stream));
        RC(lin_refine_keep_image(l, l->lu->A.get(), l->lu->npad));
    }
    else return HDSDP_RETCODE_FAILED;
    int info = 0;
    RC(l->lu->factor(g.stream, &info));
    return info == 0 ? HDSDP_RETCODE_OK : HDSDP_RETCODE_FAILED;
}
// linalg/hdsdp_linsolver.c:1082-1110 (copy + dpotrf; info != 0 is a failure here)
hdsdp_retcode lin_numeric(void *chol, int *colMatBeg, int *colMatIdx, double *colMatElem) {
    MiLin *l = (MiLin *) chol;
    if (l->bsp) return HDSDP_RETCODE_FAILED;      // (a tile-form Schur operator is factored by HKKTFactorize, nothing else owns one)
    if (l->csc_in) {
        colMatElem = const_cast<double *>(lin_densify(l, colMatBeg, colMatIdx, colMatElem));
        if (!colMatElem) return HDSDP_RETCODE_FAILED;
    }
    l->st->host_matrix_given(colMatElem, l->n);
    if (l->st->indef()) return lin_factor_indef(l);
    int info = 0;
    if (lin_factor_host(l, colMatElem, &info) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
    return info == 0 ? HDSDP_RETCODE_OK : HDSDP_RETCODE_FAILED;
}
// HFpLinsysSwitchToIndefinite (hdsdp_linsolver.c:1827-1857): only the Schur system (DENSE_ITERATIVE) has this way out;
// the matrix is re-read from where the failed factorisation took it
hdsdp_retcode lin_switch_indefinite(hdsdp_linsys_fp *HLin) {
    MiLin *l = (MiLin *) HLin->chol;
    if (l->bsp) return HDSDP_RETCODE_OK;      // the tile form's factorisation is an LDL' already (bsparse.h): nothing to switch to
    HLin->LinType = HDSDP_LINSYS_DENSE_INDEFINITE;
    l->st->switched_to_pivoted();
    return lin_factor_indef(l);
}
// linalg/hdsdp_linsolver.c:1112-1144 (info > 0 => "not PSD" is a value, not an error)
hdsdp_retcode lin_psdcheck(void *chol, int *colMatBeg, int *colMatIdx, double *colMatElem, int *isPsd) {
    MiLin *l = (MiLin *) chol;
    if (l->bsp) return HDSDP_RETCODE_FAILED;
    if (l->csc_in) {
        colMatElem = const_cast<double *>(lin_densify(l, colMatBeg, colMatIdx, colMatElem));
        if (!colMatElem) return HDSDP_RETCODE_FAILED;
    }
    if (l->st->indef()) return HDSDP_RETCODE_FAILED;   // :1729-1739, no PSD check on the pivoted factor
    int info = 0;
    if (lin_factor_host(l, colMatElem, &info) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
    *isPsd = (info == 0) ? 1 : 0;
    return HDSDP_RETCODE_OK;
}
// :1146-1196 dtrsm with L / L^T ; solVec == NULL => in place
void lin_fsolve(void *chol, int nRhs, double *rhs, double *sol) {
    MiLin *l = (MiLin *) chol;
    if (l->st->indef() || l->bsp) return;                        // :1741-1759, no half solves with the pivoted factor
    // the slot returns void (hdsdp_linsolver.h:22): a device failure can only be reported, and poisons the output so that
    // the caller's next NaN check (e.g. HFpLinsysSolve, :2085-2110) sees it
    if (l->ch.solve_host(rhs, sol ? sol : rhs, nRhs, 1, g.stream)) {
        fprintf(stderr, "[hdsdp_mi355x] forward substitution failed on the device\n");
        (sol ? sol : rhs)[0] = NAN;
    }
}
void lin_bsolve(void *chol, int nRhs, double *rhs, double *sol) {
    MiLin *l = (MiLin *) chol;
    if (l->st->indef() || l->bsp) return;
    if (l->ch.solve_host(rhs, sol ? sol : rhs, nRhs, 2, g.stream)) {
        fprintf(stderr, "[hdsdp_mi355x] backward substitution failed on the device\n");
        (sol ? sol : rhs)[0] = NAN;
    }
}
// ---- the refined solve: refine_rule.h's loop on the device ----
// d = M^-1 v through the factor's own substitution path (HdmChol::solve_device, or the pivoted solver's once switched), from and
// to vectors in the driver's order: x <- d, or x <- x + d.  A permuted factor's right-hand side and solution are permuted here.
static hdsdp_retcode lin_refine_apply(MiLin *l, const HdmRefineSource &src, const double *v, double *x, bool add) {
    const int n = l->n;
    if (src.pivoted) {
        HdmLu &lu = *l->lu;
        double *b = lu.vec.get(), *d = lu.vec.get() + 2L * lu.npad;
        RC(hdm_refine_scatter(b, v, nullptr, n, g.stream));
        RC(lu.solve_device(b, d, 1, lu.npad, g.stream));
        RC(hdm_refine_gather(x, d, nullptr, n, add ? 1 : 0, g.stream));
        return HDSDP_RETCODE_OK;
    }
    HdmChol &c = l->ch;
    double *b = c.vec.get(), *d = c.vec.get() + 2L * c.npad;
    const int *perm = src.permute ? l->rf.perm.get() : nullptr;
    HIP_RC(hipMemsetAsync(c.vec.get(), 0, sizeof(double) * 4L * c.npad, g.stream));
    RC(hdm_refine_scatter(b, v, perm, n, g.stream));
    RC(c.solve_device(b, d, 1, c.npad, 0, g.stream));
    RC(hdm_refine_gather(x, d, perm, n, add ? 1 : 0, g.stream));
    return HDSDP_RETCODE_OK;
}
// One right-hand side of a refined solve, over what a storage form supplies (`Form`):
//   B, X, XP, X0, R, nrm   device vectors of `len` entries each (right-hand side, iterate, previous iterate, unrefined solution,
//                          residual) and one double, in whatever order and padding the form's factor works in
//   load(rhs)              the caller's right-hand side -> B          store(pick, out)   an iterate -> the caller's vector
//   apply(v, x, add)       x <- M^-1 v, or x <- x + M^-1 v, through the factor's own substitution path
//   residual()             R <- B - M X in twice the working precision, nrm <- |R|^2
//   gave_up()              the substitution before the last residual has to be thrown away (asked after a synchronisation);
//                          attempts: 2 where that can happen -- the whole solve then starts again from B -- else 1
// The caller's vectors are read once, at the start, and written once, at the end: in-place solves are safe.
template <class Form>
static hdsdp_retcode lin_refine_column(Form &f, int n, int cap, double relTol, double absTol, const double *rhs, double *out, HdmRefineStats &rf) {
    double bnorm2 = 0.0;
    for (int i = 0; i < n; ++i) bnorm2 += rhs[i] * rhs[i];
    const double tol = hdm_refine_tol(relTol, absTol, std::sqrt(bnorm2));
    RC(f.load(rhs));
    for (int attempt = 0; attempt < f.attempts; ++attempt) {
        HdmRefineLoop loop(cap, tol);
        bool gave_up = false;
        double norm2 = 0.0;
        // the residual of X and its squared norm on the host
        auto residual = [&]() -> hdsdp_retcode {
            RC(f.residual());
            HIP_RC(hipMemcpyAsync(&norm2, f.nrm, sizeof(double), hipMemcpyDeviceToHost, g.stream));
            HIP_RC(hipStreamSynchronize(g.stream));
            gave_up = f.gave_up();
            return HDSDP_RETCODE_OK;
        };
        RC(f.apply(f.B, f.X, false));
        RC(residual());
        bool more = !gave_up && loop.first(norm2);
        while (more) {
            HIP_RC(hipMemcpyAsync(f.XP, f.X, sizeof(double) * (size_t) f.len, hipMemcpyDeviceToDevice, g.stream));
            if (loop.solves == 0) HIP_RC(hipMemcpyAsync(f.X0, f.X, sizeof(double) * (size_t) f.len, hipMemcpyDeviceToDevice, g.stream));
            RC(f.apply(f.R, f.X, true));
            RC(residual());
            more = !gave_up && loop.next(norm2);
        }
        if (gave_up) continue;      // (flow_gave_up switched the object to per-block launches: the second attempt cannot give up)
        const double *pick = loop.keep == HDM_REFINE_KEEP_CURRENT ? f.X : loop.keep == HDM_REFINE_KEEP_PREVIOUS ? f.XP : loop.solves > 0 ? f.X0 : f.X;
        RC(f.store(pick, out));
        rf.status = loop.status; rf.steps = loop.steps; rf.resid0 = loop.resid0; rf.resid = loop.resid; rf.tol = tol;
        rf.solves += 1; rf.total_steps += loop.solves;
        return HDSDP_RETCODE_OK;
    }
    return HDSDP_RETCODE_FAILED;
}
// the dense forms: vectors in the driver's order, the residual of a dense lower triangle (HdmSymRes), corrections through
// lin_refine_apply; after a give-up of the single-launch substitution the whole solve starts again from the right-hand side
struct LinRefineDense {
    MiLin *l;
    const HdmRefineSource &src;
    const double *M;
    long ldm, len;
    double *B, *X, *XP, *X0, *R, *nrm;
    int attempts = 2;
    LinRefineDense(MiLin *l_, const HdmRefineSource &s, const double *M_, long ld) : l(l_), src(s), M(M_), ldm(ld), len(l_->n) {
        const long npad = l->ch.npad;
        B = l->rf.v.get(); X = B + npad; XP = B + 2 * npad; X0 = B + 3 * npad; R = B + 4 * npad; nrm = B + 5 * npad;
    }
    hdsdp_retcode load(const double *rhs) {
        HIP_RC(hipMemcpyAsync(B, rhs, sizeof(double) * (size_t) l->n, hipMemcpyHostToDevice, g.stream));
        return HDSDP_RETCODE_OK;
    }
    hdsdp_retcode apply(const double *v, double *x, bool add) { return lin_refine_apply(l, src, v, x, add); }
    hdsdp_retcode residual() { RC(l->rf.res.run(M, ldm, l->n, X, B, R, nrm, g.stream)); return HDSDP_RETCODE_OK; }
    bool gave_up() { return !src.pivoted && l->ch.flow_gave_up(); }
    hdsdp_retcode store(const double *pick, double *out) {
        std::vector<double> &stage = l->rf.stage;
        stage.resize((size_t) l->n);
        HIP_RC(hipMemcpyAsync(stage.data(), pick, sizeof(double) * (size_t) l->n, hipMemcpyDeviceToHost, g.stream));
        HIP_RC(hipStreamSynchronize(g.stream));
        memcpy(out, stage.data(), sizeof(double) * (size_t) l->n);
        return HDSDP_RETCODE_OK;
    }
};
// the tile form: every vector in the tile store's order (HdmBsp::perm_dev applied once on the way in and once on the way out,
// padded to nb * 128), the residual of the tile store `mat`, corrections through HdmBsp::solve_device.  The level loops have no
// give-up path.  Shared by the operator's linear system and HMiBspRefinedSolve.
struct LinRefineTiles {
    HdmBsp &bs;
    HdmBspRefine &t;
    const double *mat;      // the tile store the residual reads
    long len;
    double *B, *X, *XP, *X0, *R, *T, *nrm;
    int attempts = 1;
    LinRefineTiles(HdmBsp &bs_, HdmBspRefine &t_, const double *store_) : bs(bs_), t(t_), mat(store_), len(t_.len) {
        B = t.vec(0); X = t.vec(1); XP = t.vec(2); X0 = t.vec(3); R = t.vec(4); T = t.vec(5); nrm = t.vec(6);
    }
    hdsdp_retcode load(const double *rhs) {
        HIP_RC(hipMemsetAsync(B, 0, sizeof(double) * (size_t) len, g.stream));
        HIP_RC(hipMemcpyAsync(T, rhs, sizeof(double) * (size_t) bs.m, hipMemcpyHostToDevice, g.stream));
        RC(hdm_refine_scatter(B, T, bs.perm_dev.get(), bs.m, g.stream));
        return HDSDP_RETCODE_OK;
    }
    hdsdp_retcode apply(const double *v, double *x, bool add) { RC(t.apply(bs, v, x, add, g.stream)); return HDSDP_RETCODE_OK; }
    hdsdp_retcode residual() { RC(t.residual(mat, X, B, R, nrm, g.stream)); return HDSDP_RETCODE_OK; }
    bool gave_up() { return false; }
    hdsdp_retcode store(const double *pick, double *out) {
        RC(hdm_refine_gather(T, pick, bs.perm_dev.get(), bs.m, 0, g.stream));
        t.stage.resize((size_t) bs.m);
        HIP_RC(hipMemcpyAsync(t.stage.data(), T, sizeof(double) * (size_t) bs.m, hipMemcpyDeviceToHost, g.stream));
        HIP_RC(hipStreamSynchronize(g.stream));
        memcpy(out, t.stage.data(), sizeof(double) * (size_t) bs.m);
        return HDSDP_RETCODE_OK;
    }
};
// nRhs columns one after another; false in *refined: the state has no matrix for the residual and the solve runs as it always did
static hdsdp_retcode lin_solve_refined(MiLin *l, int nRhs, double *rhs, double *sol, bool *refined) {
    *refined = false;
    if (l->st->refine() == 0) { l->rf.unrefined(HDM_REFINE_OFF); return HDSDP_RETCODE_OK; }
    const HdmRefineSource src = hdm_kkt_refine_source(*l->st);
    if (l->bsp) {
        const bool tiles = src.matrix == HDM_REFINE_MAT_TILES_M || src.matrix == HDM_REFINE_MAT_TILES_COPY;
        const double *store = src.matrix == HDM_REFINE_MAT_TILES_M ? l->bsp->Mval.get() : l->rf.tiles.copy.get();
        if (!tiles || !l->bsp->factored || !store) {
            l->rf.unrefined(src.matrix == HDM_REFINE_MAT_NONE ? src.why_none : HDM_REFINE_NO_MATRIX);
            return HDSDP_RETCODE_OK;
        }
        if (l->rf.tiles.prepare(*l->bsp)) return HDSDP_RETCODE_MEMORY;
        *refined = true;
        LinRefineTiles form(*l->bsp, l->rf.tiles, store);
        for (int r = 0; r < nRhs; ++r)
            RC(lin_refine_column(form, l->n, l->st->refine(), l->relTol, l->absTol, rhs + (size_t) r * l->n, (sol ? sol : rhs) + (size_t) r * l->n, l->rf));
        return HDSDP_RETCODE_OK;
    }
    const bool factored = src.pivoted ? (l->lu && l->lu->factored) : l->ch.factored;
    if (src.matrix == HDM_REFINE_MAT_NONE || !factored) {
        l->rf.unrefined(src.matrix == HDM_REFINE_MAT_NONE ? src.why_none : HDM_REFINE_NO_MATRIX);
        return HDSDP_RETCODE_OK;
    }
    const double *M = src.matrix == HDM_REFINE_MAT_COPY ? l->rf.Mcopy.get() : l->st->src_dev();
    const long ldm = src.matrix == HDM_REFINE_MAT_COPY ? (long) l->ch.npad : l->st->src_ld();
    if (!M) { l->rf.unrefined(HDM_REFINE_NO_MATRIX); return HDSDP_RETCODE_OK; }
    MiLin::Refine &rf = l->rf;
    if (rf.v.reserve(5 * (size_t) l->ch.npad + 8) != hipSuccess || rf.res.reserve(l->n)) return HDSDP_RETCODE_MEMORY;
    if (src.permute && !rf.perm) {
        if (rf.perm.alloc((size_t) l->n) != hipSuccess) return HDSDP_RETCODE_MEMORY;
        HIP_RC(hdm_memcpy_h2d_sync(rf.perm.get(), l->perm.data(), sizeof(int) * (size_t) l->n));
    }
    *refined = true;
    LinRefineDense form(l, src, M, ldm);
    for (int r = 0; r < nRhs; ++r)
        RC(lin_refine_column(form, l->n, l->st->refine(), l->relTol, l->absTol, rhs + (size_t) r * l->n, (sol ? sol : rhs) + (size_t) r * l->n, rf));
    return HDSDP_RETCODE_OK;
}

// :1198-1225 dpotrs
hdsdp_retcode lin_solve(void *chol, int nRhs, double *rhs, double *sol) {
    MiLin *l = (MiLin *) chol;
    bool refined = false;
    RC(lin_solve_refined(l, nRhs, rhs, sol, &refined));
    if (refined) return HDSDP_RETCODE_OK;
    if (l->st->indef()) {                              // :1761-1780 dsytrs
        if (!l->lu || !l->lu->factored) return HDSDP_RETCODE_FAILED;
        RC(l->lu->solve_host(rhs, sol ? sol : rhs, nRhs, g.stream));
        return HDSDP_RETCODE_OK;
    }
    if (l->bsp) {
        for (int r = 0; r < nRhs; ++r)
            RC(l->bsp->solve_host(rhs + (size_t) r * l->n, (sol ? sol : rhs) + (size_t) r * l->n, g.stream));
        return HDSDP_RETCODE_OK;
    }
    if (!l->ch.factored) return HDSDP_RETCODE_FAILED;
    if (!l->perm.empty()) {
        const int n = l->n;
        double *out = sol ? sol : rhs;
        l->pbuf.resize((size_t) n * nRhs);
        for (int r = 0; r < nRhs; ++r)
            for (int i = 0; i < n; ++i) l->pbuf[(size_t) r * n + l->perm[i]] = rhs[(size_t) r * n + i];
        RC(l->ch.solve_host(l->pbuf.data(), l->pbuf.data(), nRhs, 0, g.stream));
        for (int r = 0; r < nRhs; ++r)
            for (int i = 0; i < n; ++i) out[(size_t) r * n + i] = l->pbuf[(size_t) r * n + l->perm[i]];
        return HDSDP_RETCODE_OK;
    }
    RC(l->ch.solve_host(rhs, sol ? sol : rhs, nRhs, 0, g.stream));
    return HDSDP_RETCODE_OK;
}
// :1227-1236
hdsdp_retcode lin_getdiag(void *chol, double *diag) {
    MiLin *l = (MiLin *) chol;
    if (l->st->indef() || l->bsp) return HDSDP_RETCODE_FAILED;   // :1782-1788
    RC(l->ch.get_diag(diag, g.stream));
    return HDSDP_RETCODE_OK;
}
// :1238-1260 dpotri + HUtilMatSymmetrize: full symmetric inverse into dFullMatrix (n x n)
void lin_invert(void *chol, double *dFull, double *) {
    MiLin *l = (MiLin *) chol;
    if (l->st->indef() || l->bsp) return;              // :1790-1797
    HdmChol &c = l->ch;
    if (l->work.reserve((size_t) c.npad * c.npad) != hipSuccess) return;
    if (c.inverse_full(l->work.get(), c.npad, g.stream)) return;
    (void) hipMemcpy2DAsync(dFull, sizeof(double) * c.n, l->work.get(), sizeof(double) * c.npad, sizeof(double) * c.n, c.n,
                            hipMemcpyDeviceToHost, g.stream);
    (void) hipStreamSynchronize(g.stream);
}
void lin_destroy(void **pchol) {
    if (!pchol || !*pchol) return;
    delete (MiLin *) *pchol;
    *pchol = nullptr;
}
