// engine_create.h -- cone construction: choice of the device path and of the rows' form (the rows themselves: engine_rows.h), the objective, the synthetic family
// Implementation header of engine.hip: included exactly once, there, in this order (the pieces share the anonymous namespace
// and the engine's thread-local context `g`); split out of a 3 300-line file in round 3, nothing else changed.
int grp_sum_launch(const double *const *ptrs, int W, long lo, long cnt, double *out, hipStream_t s) {
    MiGrpPtrs pl = {};
    for (int q = 0; q < W && q < 16; ++q) pl.p[q] = ptrs[q];
    hipLaunchKernelGGL(mi_grp_sum_kernel, dim3((unsigned) ((cnt + 255) / 256)), dim3(256), 0, s, pl, W, lo, cnt, out);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
// ---------------------------------------------------------------- cone construction
// A cone under construction is owned: whichever way a make_* function leaves before it has handed the cone over, everything the
// cone holds goes back through the teardown of a finished cone (engine_build_small.h: cone_destroy_data).
struct ConeDeleter { void operator()(MiCone *c) const { void *p = c; cone_destroy_data(&p); } };
using ConeOwner = std::unique_ptr<MiCone, ConeDeleter>;

static int upload_objective(MiCone *c) {   // full symmetric (it feeds the S assembly), through a packed image
    const long P = (long) c->n * (c->n + 1) / 2;
    const long nn = (long) c->n16 * c->n16;
    HdmBuf<double> stage_dev;
    HdmPinned<double> stage_host;
    HDM_HIP_CHECK(stage_dev.alloc((size_t) P));
    HDM_HIP_CHECK(stage_host.alloc((size_t) P));
    memset(stage_host.get(), 0, sizeof(double) * (size_t) P);
    for (size_t e = 0; e < c->blk.obj.idx.size(); ++e) stage_host.get()[c->blk.obj.idx[e]] = c->blk.obj.val[e];
    HDM_HIP_CHECK(hipMemcpyAsync(stage_dev.get(), stage_host.get(), sizeof(double) * (size_t) P, hipMemcpyHostToDevice, g.stream));
    if (hdm_unpack_sym(stage_dev.get(), P, c->Cfull.get(), nn, c->n, c->n16, 1, g.stream)) return 1;
    HDM_HIP_CHECK(hipStreamSynchronize(g.stream));
    return 0;
}

// Resident or streamed constraint rows?  The rule is row_store_rule.h's (hdm_rows_stream); the device's figures are read here.
// (Only the congruence + Gram path asks: the other paths' rows are always resident.)
static bool cone_wants_streaming(const MiCone *c) {
    const HdmRowFacts f = cone_row_facts(c);
    return hdm_rows_stream(f, f.gemm_path ? device_facts() : HdmDeviceFacts(), hdm_env_int<ENV_STREAM_A>());
}

// device path a block takes by itself: the rank-one fast path iff every non-zero constraint is rank one (the reference's
// all-M2 plans), the sparse gather path iff all rows are short triplet lists, else congruence + Gram; sharded blocks
// (world > 1) always take the latter
static int natural_path(const MiBlockData &blk, int nRow, int nCol, int world) {
    int nz = 0, r1 = 0;
    for (int i = 0; i < nRow; ++i) {
        int t = blk.rows[i].type;
        if (t != MI_COEFF_ZERO) nz++;
        if (t == MI_COEFF_SPR1 || t == MI_COEFF_DSR1) r1++;
    }
    int path = (nz > 0 && r1 == nz && world == 1) ? PATH_R1 : PATH_GEMM;
    if (path == PATH_GEMM && world == 1 && nz > 0) {
        // sparse gather path: only triplet-class rows, and the pair products are far cheaper than m congruences
        bool all_sparse = true;
        double tot = 0.0;
        for (int i = 0; i < nRow; ++i) {
            int t = blk.rows[i].type;
            if (t == MI_COEFF_DENSE || t == MI_COEFF_DSR1) all_sparse = false;
            tot += (double) blk.rows[i].stored;
        }
        if (all_sparse && tot * tot < 0.05 * (double) nRow * nCol * (double) nCol * nCol) path = PATH_SPARSE;
    }
    return path;
}

// Direct rows (direct_rows.h): decided here, once, before the rows are uploaded -- the rule and the partition are the header's;
// what stays here is the switch, the new local order (own, rows_own and the first mloc entries of rows_seg: everything uploaded
// after this call follows it) and the device copies of the term table and of the rank-one rows' factors.
// HDSDP_MI355X_DIRECT_ROWS: unset = the rule; 0 = off; k > 0 = on whatever the size, kmax = k.
static_assert(HDM_DR_ZERO == MI_COEFF_ZERO && HDM_DR_SPARSE == MI_COEFF_SPARSE && HDM_DR_DENSE == MI_COEFF_DENSE &&
              HDM_DR_SPR1 == MI_COEFF_SPR1 && HDM_DR_DSR1 == MI_COEFF_DSR1 && HDM_DR_PATH_GEMM == PATH_GEMM,
              "direct_rows.h restates the classes of coeff.h and the path numbers");
static int cone_plan_direct_rows(MiCone *c, int natural, bool force_gemm, bool force_path, bool streamed) {
    const HdmEnvInt e = hdm_env_int<ENV_DIRECT_ROWS>();
    const int sw = e.set ? std::max(0, (int) e.value) : -1;
    const HdmDirectRule rule = hdm_direct_rule(c->world, c->synthetic, streamed, natural, force_gemm, force_path, c->n, c->n16, sw);
    if (!rule.on || c->mloc == 0 || (int) c->blk.rows.size() != c->m) return 0;
    std::vector<int> type((size_t) c->m);
    std::vector<long> stored((size_t) c->m);
    for (int i = 0; i < c->m; ++i) { type[i] = c->blk.rows[i].type; stored[i] = (long) c->blk.rows[i].idx.size(); }
    const HdmDirectPlan p = hdm_direct_partition(type, stored, rule);
    if (p.nDirect == 0 || (int) p.order.size() != c->mloc) return 0;
    c->own = p.order;
    c->dr_n = p.nDirect; c->dr_r1 = p.nRankOne; c->dr_kmax = rule.kmax;
    HDM_HIP_CHECK(hdm_memcpy_h2d_sync(c->rows_seg.get(), c->own.data(), sizeof(int) * (size_t) c->mloc));
    HDM_HIP_CHECK(hdm_memcpy_h2d_sync(c->rows_own.get(), c->own.data(), sizeof(int) * (size_t) c->mloc));
    std::vector<HdmDirectTerm> terms;
    std::vector<long> ptr(1, 0L);
    terms.reserve((size_t) p.nterms);
    c->dr_r1_16 = (int) hdm_roundup(std::max(1, p.nRankOne), 16);
    std::vector<double> fac((size_t) c->n16 * c->dr_r1_16, 0.0);   // K-major, zero-padded to n16
    int slot = 0;
    for (int q = p.nCongruence; q < c->mloc; ++q) {
        const MiCoeff &co = c->blk.rows[c->own[q]];
        const bool r1 = hdm_direct_is_r1(co.type);
        hdm_direct_terms(co.type, c->n, co.idx, co.val, co.sign, slot, terms);
        if (r1) {
            for (int r = 0; r < c->n; ++r) fac[(size_t) slot * c->n16 + r] = co.factor[r];
            slot += 1;
        }
        ptr.push_back((long) terms.size());
    }
    c->dr_max_lcol = -1;
    for (const HdmDirectTerm &t : terms) {
        if ((t.x < 0) != (t.y < 0) || t.x >= c->n || t.y >= c->n || -1 - t.x >= slot || -1 - t.y >= slot) {
            fprintf(stderr, "[hdsdp_mi355x] direct rows: a term names a vector outside the block\n");
            return 1;
        }
        c->dr_max_lcol = std::max(c->dr_max_lcol, std::max(t.x, t.y));
    }
    HDM_HIP_CHECK(c->dr_terms.alloc(std::max<size_t>(1, terms.size())));
    HDM_HIP_CHECK(c->dr_ptr.alloc(ptr.size()));
    HDM_HIP_CHECK(c->dr_fac.alloc(fac.size()));
    HDM_HIP_CHECK(c->dr_U.alloc(fac.size()));
    HDM_HIP_CHECK(hdm_memcpy_h2d_sync(c->dr_terms.get(), terms.data(), sizeof(HdmDirectTerm) * terms.size()));
    HDM_HIP_CHECK(hdm_memcpy_h2d_sync(c->dr_ptr.get(), ptr.data(), sizeof(long) * ptr.size()));
    HDM_HIP_CHECK(hdm_memcpy_h2d_sync(c->dr_fac.get(), fac.data(), sizeof(double) * fac.size()));
    HDM_HIP_CHECK(hdm_memset_sync(c->dr_U.get(), 0, sizeof(double) * fac.size()));
    return 0;
}

// the device data of one SDP block for rank `rank` of `world` on the calling thread's context, from the block's presolved
// host data.  A shard of a sharded block (world > 1) copies the entries of its own rows only (the others keep class, counts
// and trace): W shards of one block together hold one more copy of the data, not W.  With `take` the source is moved from.
static hdsdp_retcode make_sdp_cone_from_block(MiCone **out, MiBlockData &src, bool take, int rank, int world) {
    if (ensure_ctx()) return HDSDP_RETCODE_FAILED;
    const int nRow = src.m, nCol = src.n;
    ConeOwner owner(new MiCone());
    MiCone *c = owner.get();
    c->n = nCol; c->m = nRow; c->rank = rank; c->world = world;
    if (world > 1) hdm_gemm_reserve_cus(8);   // the exchange's collectives run beside the persistent GEMM launches
    if (take) c->blk = std::move(src);
    else if (world == 1) c->blk = src;
    else {
        c->blk.n = src.n; c->blk.m = src.m; c->blk.perm = src.perm; c->blk.strategy = src.strategy; c->blk.stored = src.stored;
        for (int t = 0; t < 5; ++t) c->blk.counts[t] = src.counts[t];
        c->blk.obj = src.obj;
        c->blk.rows.resize((size_t) nRow);
        for (int i = 0; i < nRow; ++i) {
            if (i % world == rank) { c->blk.rows[i] = src.rows[i]; continue; }
            MiCoeff &d = c->blk.rows[i];
            const MiCoeff &o = src.rows[i];
            d.type = o.type; d.nnz = o.nnz; d.rank = o.rank; d.stored = o.stored; d.trace = o.trace; d.sign = o.sign; d.factor_nnz = o.factor_nnz;
            d.is_eye = o.is_eye; d.eye_val = o.eye_val; d.unit_col = o.unit_col;
        }
    }
    if (cone_alloc_common(c)) return HDSDP_RETCODE_MEMORY;
    c->trA.assign((size_t) nRow, 0.0);
    for (int i = 0; i < nRow; ++i) c->trA[i] = c->blk.rows[i].trace;
    const int natural = natural_path(c->blk, nRow, nCol, world);
    c->path = natural;
    const bool force = hdm_env_on<ENV_FORCE_GEMM>();
    if (force) c->path = PATH_GEMM;
    const HdmEnvInt forcesp = hdm_env_int<ENV_FORCE_PATH>();
    if (forcesp.set && world == 1) c->path = (int) forcesp.value;
    if (c->mloc == 0) c->path = PATH_GEMM;   // no constraint touches this block: only the objective's scalars remain
    {
        CreateTimer t_(1);
        // (rows too many to stay resident beside the work buffers -- congruence + Gram path only -- live in the compressed copy)
        const bool stream = cone_wants_streaming(c);
        if (cone_plan_direct_rows(c, natural, force, forcesp.set, stream)) return HDSDP_RETCODE_MEMORY;
        if (stream ? c->rows.ingest_expanded(cone_row_shape(c), c->blk) : c->rows.upload_resident(cone_row_shape(c), c->blk)) return HDSDP_RETCODE_MEMORY;   // the dense forms also feed the S assembly
        if (upload_objective(c)) return HDSDP_RETCODE_MEMORY;
    }
    if (c->path == PATH_R1) {
        c->mloc16 = (int) hdm_roundup(std::max(1, c->mloc), 16);
        const size_t av = sizeof(double) * (size_t) c->n16 * c->mloc16;
        std::vector<double> hA((size_t) c->n16 * c->mloc16, 0.0), hs(c->mloc16, 0.0);
        for (int q = 0; q < c->mloc; ++q) {
            const MiCoeff &co = c->blk.rows[c->own[q]];
            if (co.type == MI_COEFF_ZERO) continue;
            for (int r = 0; r < nCol; ++r) hA[(size_t) q * c->n16 + r] = co.factor[r];
            hs[q] = co.sign;
        }
        if (c->Avec.alloc(av / sizeof(double)) != hipSuccess || c->U.alloc(av / sizeof(double)) != hipSuccess ||
            c->V.alloc(av / sizeof(double)) != hipSuccess || c->W.alloc(std::max(av, sizeof(double) * (size_t) c->n16 * c->n16) / sizeof(double)) != hipSuccess ||
            c->sgn.alloc(c->mloc16) != hipSuccess ||
            c->Gr1.alloc((size_t) c->mloc16 * c->mloc16) != hipSuccess ||
            c->Ct.alloc((size_t) c->n16 * c->n16) != hipSuccess ||
            c->Xinv.alloc((size_t) c->n16 * c->n16) != hipSuccess)
            return HDSDP_RETCODE_MEMORY;
        if (hdm_memcpy_h2d_sync(c->Avec.get(), hA.data(), av) != hipSuccess ||
            hdm_memcpy_h2d_sync(c->sgn.get(), hs.data(), sizeof(double) * c->mloc16) != hipSuccess)
            return HDSDP_RETCODE_FAILED;
    }
    if (c->path == PATH_SPARSE) {
        std::vector<int> rp(c->mloc + 1, 0), ti, tj;
        std::vector<double> tv;
        for (int q = 0; q < c->mloc; ++q) {
            const MiCoeff &co = c->blk.rows[c->own[q]];
            for (size_t e = 0; e < co.idx.size(); ++e) {
                long pk = co.idx[e];
                int col = 0; long start = 0;
                while (pk >= start + (nCol - col)) { start += nCol - col; ++col; }
                ti.push_back(col + (int) (pk - start)); tj.push_back(col); tv.push_back(co.val[e]);
            }
            rp[q + 1] = (int) ti.size();
        }
        const size_t nt = std::max<size_t>(1, ti.size());
        const size_t nn2 = sizeof(double) * (size_t) hdm_roundup(nCol, 128) * hdm_roundup(nCol, 128);
        if (c->sp_rp.alloc(rp.size()) != hipSuccess ||
            c->sp_ti.alloc(nt) != hipSuccess ||
            c->sp_tj.alloc(nt) != hipSuccess ||
            c->sp_tv.alloc(nt) != hipSuccess ||
            c->Xinv.alloc(nn2 / sizeof(double)) != hipSuccess || c->Yinv.alloc(nn2 / sizeof(double)) != hipSuccess ||
            c->W.alloc(nn2 / sizeof(double)) != hipSuccess || c->Ct.alloc(nn2 / sizeof(double)) != hipSuccess)
            return HDSDP_RETCODE_MEMORY;
        if (hdm_memcpy_h2d_sync(c->sp_rp.get(), rp.data(), sizeof(int) * rp.size()) != hipSuccess ||
            (ti.size() && (hdm_memcpy_h2d_sync(c->sp_ti.get(), ti.data(), sizeof(int) * ti.size()) != hipSuccess ||
                           hdm_memcpy_h2d_sync(c->sp_tj.get(), tj.data(), sizeof(int) * tj.size()) != hipSuccess ||
                           hdm_memcpy_h2d_sync(c->sp_tv.get(), tv.data(), sizeof(double) * tv.size()) != hipSuccess)))
            return HDSDP_RETCODE_FAILED;
    }
    if (hipStreamSynchronize(g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    // On the congruence + Gram path everything downstream reads the device copy (A_L forms, the sweep copy): the host copy of
    // the entries -- 19 GB at n = m = 2000, 40 %-filled -- goes back now.  The rank-one and gather paths keep theirs (small,
    // and their host-side norms and plans read them).
    if (c->path == PATH_GEMM) { for (MiCoeff &co : c->blk.rows) co.release(); c->blk.obj.release(); }
    {
        CreateTimer t_(2);
        if (cone_make_sweep_copy(c)) return HDSDP_RETCODE_FAILED;
    }
    *out = owner.release();
    return HDSDP_RETCODE_OK;
}

static hdsdp_retcode make_synth_cone(MiCone **out, int nCol, int nRow, int rank, int world) {
    if (ensure_ctx()) return HDSDP_RETCODE_FAILED;
    ConeOwner owner(new MiCone());
    MiCone *c = owner.get();
    c->n = nCol; c->m = nRow; c->rank = rank; c->world = world; c->synthetic = true; c->path = PATH_GEMM;
    if (world > 1) hdm_gemm_reserve_cus(8);
    if (cone_alloc_common(c)) return HDSDP_RETCODE_MEMORY;
    if (const hdsdp_retcode rc = c->rows.generate(cone_row_shape(c), cone_wants_streaming(c)); rc != HDSDP_RETCODE_OK) return rc;
    if (hdm_synth_obj(c->Cfull.get(), c->n, c->n16, c->m, g.stream)) return HDSDP_RETCODE_FAILED;
    // b_i = tr(A_i): diagonal draws only (host, m*n splitmix evaluations)
    c->trA.assign((size_t) nRow, 0.0);
    const uint64_t P = (uint64_t) nCol * (nCol + 1) / 2, gam = 0x9E3779B97F4A7C15ULL;
    for (int i = 0; i < nRow; ++i) {
        double tr = 0.0;
        uint64_t k = 0;
        for (int j = 0; j < nCol; ++j) {
            uint64_t z = gam + (2 * ((uint64_t) i * P + k) + 1) * gam;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
            z = z ^ (z >> 31);
            tr += 2.0 * ((double) (z >> 11) / 9007199254740992.0) - 1.0;
            k += nCol - j;
        }
        c->trA[i] = tr;
    }
    if (hipStreamSynchronize(g.stream) != hipSuccess) return HDSDP_RETCODE_FAILED;
    if (cone_make_sweep_copy(c)) return HDSDP_RETCODE_FAILED;
    *out = owner.release();
    return HDSDP_RETCODE_OK;
}
