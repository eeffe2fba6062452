// engine_build.h -- the GPU Schur builders: congruence + Gram (all build types, the exchange of a sharded build, KKT_TYPE_PRIMAL), corrector components
// Implementation header of engine.hip: included exactly once, there, in this order (the pieces share the anonymous namespace
// and the engine's thread-local context `g`); split out of a 3 300-line file in round 3, nothing else changed.
// --- the GPU Schur builder ---------------------------------------------------------------------
// phase 0: both steps; 1: step 1 only; 2: step 2 only (count <= Bc, T still holds step 1's output), optionally only the
// output tiles of the tile columns in `colmask` -- the multi-GPU build runs step 2 by packed-index range so that the
// finished ranges can leave for the other ranks while the rest is still being computed
// `src_rows`: skyline matrices the buffer behind Asrc holds (its span for the launcher's check is hdm_afull_span of them)
int congruence_rows(MiCone *c, HdmChol &ch, const double *Asrc, long src_rows, int count, long row0, int phase = 0,
                    unsigned long long colmask = 0) {
    // rows row0 .. row0+count-1 of AhatLoc  <-  blocked( Linv * A * Linv^T ): step 1 into T, step 2 from there (gemm_calls.h)
    const HdmLayout L = cone_layout(c);
    for (int b0 = 0; b0 < count; b0 += c->Bc) {
        const int nb = std::min(c->Bc, count - b0);
        if (phase != 2 && c->shared_ts && hdm_zero_diag_upper(c->T.get(), (long) c->n16 * c->n16, c->n16, nb, g.stream)) return 1;
        if (phase != 2 && hdm_launch_gemm(hdm_cong_step1(L, c->n, ch.Linv.get(), ch.npad, Asrc, src_rows, b0, nb, c->T.get()), g.stream)) return 1;
        if (phase == 1) continue;
        if (hdm_launch_gemm(hdm_cong_step2(L, c->n, c->Bc, ch.Linv.get(), ch.npad, c->T.get(), nb, c->AhatLoc, row0 + b0, colmask), g.stream)) return 1;
    }
    return 0;
}

// Gram partial sums of the K splits [z0, z0 + nz): slabs slab0.. <- (or +=, `accumulate`) Ahat * Ahat^T over their share of this
// rank's p-range.  slab0 < 0: slab z0 (one slab per split)
int gram_splits(MiCone *c, int z0, int nz, int slab0 = -1, bool accumulate = false) {
    double *slab = c->slabs + (long) (slab0 < 0 ? z0 : slab0) * c->R * c->R;
    return hdm_launch_gemm(hdm_gram_splits(cone_layout(c), c->n, c->m, c->nsplit, z0, nz, c->AhatAll, slab, accumulate, c->gram_queue_global), g.stream);
}

// the K splits [z0, z0 + nz) in groups of nslab, launch after launch on the engine stream, every group accumulating into the slabs
// the one before left (`fresh`: the first group of a build overwrites them).  Fixed order: bitwise reproducible.
// The first group of a build is its largest (a range's groups are nslab, nslab, ..., remainder; the pieces of an exchange are equal
// ranges), so it initialises every slab a later group adds to; slabs_used = its size is what the reduction sums.
int gram_range(MiCone *c, int z0, int nz, bool fresh) {
    for (int z = z0; z < z0 + nz; z += c->nslab) {
        const int k = std::min(c->nslab, z0 + nz - z);
        if (fresh) c->slabs_used = k;
        else if (k > c->slabs_used) { fprintf(stderr, "[hdsdp_mi355x] Gram groups out of order\n"); return 1; }
        if (gram_splits(c, z, k, 0, !fresh)) return 1;
        fresh = false;
    }
    return 0;
}
int gram_reduce(MiCone *c) {
    return hdm_slab_reduce(c->slabs, c->R * c->R, c->slabs_used, c->Gm.get(), c->R * c->R, c->R, g.stream);
}
int gram_all(MiCone *c) {
    // Gm(lower) = sum over this rank's p-range of Ahat * Ahat^T, rows in segment order (more splits than slabs:
    // work_plan.h says why)
    if (gram_range(c, 0, c->nsplit, true)) return 1;
    return gram_reduce(c);
}

// world > 1: the all-to-all that re-shards Ahat from "by constraint" to "by packed-index range", and the Gram product.
// With the piecewise hooks registered the exchange runs in pieces along the packed index and the Gram splits of a piece
// start as soon as it has arrived, while the later pieces are still on the links.
// number of pieces of the piecewise exchange (whole groups of Gram K splits)
int exchange_pieces(const MiCone *c) {
    int P = (c->a2a_start && c->a2a_wait) ? c->a2a_pieces : 1;
    if (const HdmEnvInt e = hdm_env_int<ENV_A2A_PIECES>(); e.set) P = std::max(1, (int) e.value);
    if (!(c->a2a_start && c->a2a_wait)) P = 1;
    while (P > 1 && (c->nsplit % P)) --P;
    return P;
}
// p-blocks [lo, hi) of every destination's chunk that piece k of P carries
void piece_range(const MiCone *c, int k, int P, long *lo, long *hi) { hdm_piece_range(cone_layout(c), c->nsplit, k, P, lo, hi); }
// Tile columns of congruence step 2 whose output piece k needs.  P-block q belongs to the 16 x 16 sub-block q / 16 of the
// blocked lower triangle, sub-blocks are numbered column by column (gemm_geom.h: hdm_blk_col_of), and tile
// column tn produces the sub-block columns 8 tn .. 8 tn + 7: a range of p-blocks is a range of tile columns.
unsigned long long piece_tile_cols(const MiCone *c, int k, int P) {
    long lo, hi;
    piece_range(c, k, P, &lo, &hi);
    auto col_of = [&](long sub) { return hdm_blk_col_of(sub, c->nblk); };
    unsigned long long mask = 0;
    for (int d = 0; d < c->world; ++d) {
        const long g0 = (long) d * c->npb_loc + lo, g1 = std::min<long>(c->npb, (long) d * c->npb_loc + hi);
        if (g0 >= g1) continue;
        for (int tn = col_of(g0 / 16) / 8; tn <= col_of((g1 - 1) / 16) / 8; ++tn) mask |= 1ULL << tn;
    }
    return mask;
}

static inline double host_now() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static inline int prof_record(hipEvent_t &ev, hipStream_t s) {
    if (!ev && hipEventCreate(&ev) != hipSuccess) return 1;
    return hipEventRecord(ev, s) != hipSuccess;
}

// `staged`: congruence step 2 was launched piece by piece and c->piece_ev[k] marks the point where piece k's p-blocks
// are final, so piece k can leave while the later tile columns are still being computed; otherwise the whole stream
// is drained first.
hdsdp_retcode exchange_and_gram(MiCone *c, bool staged = false) {
    if (!c->alltoall && !(c->a2a_start && c->a2a_wait)) {
        fprintf(stderr, "[hdsdp_mi355x] world > 1 but no exchange hook registered\n");
        return HDSDP_RETCODE_FAILED;
    }
    if (!staged) HIP_RC(hipStreamSynchronize(g.stream));
    const int P = exchange_pieces(c);
    const double sent_share = (double) (c->world - 1) * 8.0;   // bytes this shard sends per double of a piece
    if (P <= 1) {
        if (staged) HIP_RC(hipStreamSynchronize(g.stream));
        const double t0 = host_now();
        if (c->alltoall) { if (c->alltoall(c->xctx)) return HDSDP_RETCODE_FAILED; }
        else {
            if (c->a2a_start(c->xctx, 0, (int64_t) c->npb_loc * c->Lr * 16, 0) || c->a2a_wait(c->xctx, 0)) return HDSDP_RETCODE_FAILED;
        }
        c->prof.wait_host[0] = c->prof.flight[0] = (host_now() - t0) * 1e3;
        c->prof.bytes[0] = sent_share * (double) c->npb_loc * c->Lr * 16;
        if (prof_record(c->pe_ga[0], g.stream) || gram_range(c, 0, c->nsplit, true) || prof_record(c->pe_gb[0], g.stream)) return HDSDP_RETCODE_FAILED;
        return gram_reduce(c) ? HDSDP_RETCODE_FAILED : HDSDP_RETCODE_OK;
    }
    const int zper = c->nsplit / P;
    for (int k = 0; k < P; ++k) {
        long lo, hi;
        piece_range(c, k, P, &lo, &hi);
        const int64_t off = (int64_t) lo * c->Lr * 16, end = (int64_t) hi * c->Lr * 16;   // doubles inside a chunk
        if (staged) HIP_RC(hipEventSynchronize(c->piece_ev[k]));
        c->pt_start[k] = host_now();
        c->prof.bytes[k] = sent_share * (double) (end - off);
        if (c->a2a_start(c->xctx, off, end - off, k)) {
            if (k == 0 && c->alltoall) {
                // the piecewise flavour is not available in this process group: one blocking exchange from now on
                fprintf(stderr, "[hdsdp_mi355x] piecewise all-to-all failed to start; using the blocking exchange\n");
                c->a2a_pieces = 1; c->a2a_start = nullptr; c->a2a_wait = nullptr;
                HIP_RC(hipStreamSynchronize(g.stream));
                if (c->alltoall(c->xctx)) return HDSDP_RETCODE_FAILED;
                return gram_all(c) ? HDSDP_RETCODE_FAILED : HDSDP_RETCODE_OK;
            }
            return HDSDP_RETCODE_FAILED;
        }
    }
    for (int k = 0; k < P; ++k) {
        const double t0 = host_now();
        if (c->a2a_wait(c->xctx, k)) return HDSDP_RETCODE_FAILED;
        const double t1 = host_now();
        c->prof.wait_host[k] = (t1 - t0) * 1e3;
        c->prof.flight[k] = (t1 - c->pt_start[k]) * 1e3;
        // (piece after piece into the same slabs: they are launched in order on one stream)
        if (prof_record(c->pe_ga[k], g.stream) || gram_range(c, k * zper, zper, k == 0) || prof_record(c->pe_gb[k], g.stream))
            return HDSDP_RETCODE_FAILED;
    }
    return gram_reduce(c) ? HDSDP_RETCODE_FAILED : HDSDP_RETCODE_OK;
}

// KKT_TYPE_PRIMAL, route 1 (build_primal): X = W^T diag(sigma) W with sigma = +-1, the transformed rows are At_i = W A_i W^T, and
//   M_ij = tr(A_i X A_j X) = sum_{k,l} sigma_k sigma_l At_i(k, l) At_j(k, l),
// the Gram product of the packed rows with the weight sigma_k sigma_l on packed column (k, l).  The plain Gram product G has run
// with weight +1 everywhere; the columns of weight -1 (one index in the negative set, the other not) or those of weight +1,
// whichever are fewer, are gathered into a compact operand and their own Gram product G- / G+ is added with alpha -2 / +2:
//   signed G = G - 2 G-  =  2 G+ - G.
// Chunks of at most 2 GiB of gathered operand; the Gram role's kernel on the chunk (split-K into the slabs, which are free after
// the plain product's reduction), then Gm = (+-1) Gm + sum of the slabs.  Sharded: this rank's partial Gm over its own K range
// (all rows of it are here after the exchange), before the all-reduce.  Fixed order throughout: bitwise reproducible.
static constexpr long PSIG_GATHER_BYTES = 2L << 30;
int signed_correction(MiCone *c) {
    c->primal_cols = 0;
    std::vector<double> sg((size_t) c->n16);
    HIP_RC(hipMemcpyAsync(sg.data(), c->gram_sig, sizeof(double) * (size_t) c->n16, hipMemcpyDeviceToHost, g.stream));
    HIP_RC(hipStreamSynchronize(g.stream));
    // p-block q holds matrix column pb.col; its packed columns q 16 + r are the rows pb.bi 16 + r (gemm_geom.h: hdm_pblock_decode)
    const long pb0 = (long) c->rank * c->npb_loc, pb1 = std::min(c->npb, pb0 + c->npb_loc);
    std::vector<int> neg, pos;
    for (long q = pb0; q < pb1; ++q) {
        const HdmPBlock pb = hdm_pblock_decode(q, c->nblk);
        const long col = pb.col;
        if (col >= c->n) continue;
        for (int r = 0; r < 16; ++r) {
            const long row = (long) pb.bi * 16 + r;
            if (row >= c->n) break;
            ((sg[row] * sg[col] < 0.0) ? neg : pos).push_back((int) (q * 16 + r));
        }
    }
    const bool use_neg = neg.size() <= pos.size();
    const std::vector<int> &cols = use_neg ? neg : pos;
    const double alpha = use_neg ? -2.0 : 2.0, beta0 = use_neg ? 1.0 : -1.0;
    const long ncols = (long) cols.size(), R = c->R;
    c->primal_cols = ncols;
    if (ncols == 0) {
        if (use_neg) return 0;                                        // no column of weight -1 here: G is already signed
        hipLaunchKernelGGL(mi_psig_combine_kernel, dim3((unsigned) ((R * R + 255) / 256)), dim3(256), 0, g.stream, c->Gm.get(),
                           (const double *) c->slabs, R * R, 0, R, -1.0);
        HIP_RC(hipGetLastError());
        return 0;
    }
    HIP_RC(c->pcols.reserve((size_t) ncols));
    HIP_RC(hipMemcpyAsync(c->pcols.get(), cols.data(), sizeof(int) * (size_t) ncols, hipMemcpyHostToDevice, g.stream));
    HIP_RC(hipStreamSynchronize(g.stream));      // (pageable source going out of scope)
    const long RT = (R + HDM_TILE - 1) / HDM_TILE, tiles = RT * (RT + 1) / 2;
    const long ncols16 = hdm_roundup(ncols, 16);
    const long kc = std::min(ncols16, std::max(16L, (PSIG_GATHER_BYTES / (8 * R)) & ~15L));   // columns per chunk
    // the Gram role's tile loads carry no row mask: up to RT * 128 rows of the last k block are read
    const long need = R * kc + RT * HDM_TILE * 16 + HDM_OPERAND_PAD_DOUBLES;
    if (c->pgat.count() < (size_t) need) {
        HIP_RC(c->pgat.alloc((size_t) need));
        HIP_RC(hipMemsetAsync(c->pgat.get(), 0, sizeof(double) * (size_t) need, g.stream));
    }
    // split-K over the slabs: enough (split, tile) jobs to fill the chip, at least 8 k blocks per split
    int nz = (int) std::max(1L, std::min<long>({(long) c->nslab, (1024 + tiles - 1) / tiles, std::max(1L, kc / 16 / 8)}));
    const long seg_stride = c->npb_loc * c->Lr * 16;
    std::vector<hipEvent_t> ev;
    auto mark = [&]() { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return 1; ev.push_back(e);
                        return hipEventRecord(e, g.stream) != hipSuccess ? 1 : 0; };
    int rc = 0;
    for (long j0 = 0; j0 < ncols && !rc; j0 += kc) {
        const long nc = std::min(kc, ncols - j0), nc16 = hdm_roundup(nc, 16);
        const long tot = R * nc16;
        rc |= mark();
        hipLaunchKernelGGL(mi_psig_gather_kernel, dim3((unsigned) std::min<long>((tot + 255) / 256, 16384)), dim3(256), 0, g.stream,
                           (const double *) c->AhatAll, seg_stride, c->Lr, R, (const int *) (c->pcols.get() + j0), nc, nc16, pb0, c->pgat.get());
        if (hipGetLastError() != hipSuccess) rc = 1;
        rc |= mark();
        if (!rc && hdm_launch_gemm(hdm_gram_gathered(R, nc, nc16, nz, alpha, j0 != 0, c->pgat.get(), (long) c->pgat.count(), c->slabs,
                                                     c->gram_queue_global), g.stream)) rc = 1;
    }
    rc |= mark();
    if (!rc) {
        hipLaunchKernelGGL(mi_psig_combine_kernel, dim3((unsigned) ((R * R + 255) / 256)), dim3(256), 0, g.stream, c->Gm.get(),
                           (const double *) c->slabs, R * R, nz, R, beta0);
        if (hipGetLastError() != hipSuccess) rc = 1;
    }
    rc |= mark();
    if (hipEventSynchronize(ev.back()) != hipSuccess) rc = 1;
    double gat = 0.0, gem = 0.0, cmb = 0.0;
    float t = 0.f;
    for (size_t k = 0; !rc && k + 1 < ev.size(); ++k) {
        if (hipEventElapsedTime(&t, ev[k], ev[k + 1]) != hipSuccess) { rc = 1; break; }
        if (k + 2 == ev.size()) cmb += t; else if (k % 2 == 0) gat += t; else gem += t;
    }
    for (hipEvent_t e : ev) (void) hipEventDestroy(e);
    c->primal_ms[1] = gat; c->primal_ms[2] = gem; c->primal_ms[3] = cmb;
    return rc;
}

hdsdp_retcode build_gemm_path(MiCone *c, hdsdp_kkt *kkt, MiKKTPriv *pv, int typeKKT, HdmChol *chOverride = nullptr);
double *kkt_Mdev(hdsdp_kkt *kkt, long *ld);
HdmMatView kkt_view(hdsdp_kkt *kkt);
hdsdp_retcode build_r1_path(MiCone *c, hdsdp_kkt *kkt, MiKKTPriv *pv, int typeKKT);
hdsdp_retcode build_sparse_path(MiCone *c, hdsdp_kkt *kkt, MiKKTPriv *pv, int typeKKT);

// KKT_TYPE_PRIMAL (hdsdp_conic_sdp.c:1745-1753; driver hdsdp_psdp.c:156,203,420): the builder runs on the registered
// primal matrix X in place of S^-1.  S^-1 = Linv^T Linv enters every path only through the lower-triangular Linv, so
// X is brought to the same form: factor the index-reversed matrix J X J = F F^T on the device, then W = J F^T J is
// lower triangular with W^T W = X and takes Linv's place in the GEMM path (all strategies give the same numbers, and
// the reference itself re-routes M2 columns for this type, :1782-1788).  X must be positive definite, which a
// primal interior point is; an indefinite X is reported like a failed dpotrf.
// KKT_TYPE_PRIMAL with a registered matrix that is NOT positive definite (the primal refinement does hand such iterates
// over, hdsdp_psdp.c:203,420; the reference's trace formulas do not care): no triangular factor exists, so the product is
// formed the way the reference's M3 column does it, one owned row at a time:  B_i = X A_i X  (three plain MFMA GEMMs on
// the A_L form: X A = X A_L + X A_L^T),  then  M_ij = <A_j, B_i>  for all j in one pass over the resident constraint data.
// 4 n^3 + m n^2 flops per row instead of the congruence path's n^3 + m n^2 / 2: a fallback, used only on this condition.
hdsdp_retcode build_primal_general(MiCone *c, hdsdp_kkt *kkt, MiKKTPriv *pv, const double *X) {
    if (c->world > 1) {
        fprintf(stderr, "[hdsdp_mi355x] KKT_TYPE_PRIMAL: an indefinite primal matrix is not supported on a sharded block\n");
        return HDSDP_RETCODE_FAILED;
    }
    const int n = c->n, m = kkt->nRow;
    long ldx = 0, ldm = 0;
    RC(cone_upload_X(c, X, &ldx));
    const size_t np2 = sizeof(double) * (size_t) ldx * ldx;
    HIP_RC(c->Pr1.reserve(np2 / sizeof(double)));
    HIP_RC(c->Pr2.reserve(np2 / sizeof(double)));
    (void) ldm;
    const HdmMatView Mview = kkt_view(kkt);
    HdmBuf<double> row, ALsq;   // freed on every way out
    HIP_RC(row.alloc((size_t) m));
    HIP_RC(ALsq.alloc((size_t) c->n16 * c->n16, hdm_operand_pad(c->n16)));
    const int n16 = c->n16;
    const HdmOperand Xm = hdm_mmajor(c->Xup.get(), ldx), Xk = hdm_kmajor(c->Xup.get(), ldx);
    // vectors: ASinv_i = <A_i, X>, ASinvRdSinv_i = Rd <A_i, X^2>   (Pr2 <- X X^T)
    hdsdp_retcode rc = HDSDP_RETCODE_OK;
    if (hdm_launch_gemm(hdm_gemm_product(c->Pr2.get(), ldx, n16, n16, n16, 1.0, Xm, Xm), g.stream) ||
        cone_sym_dot2(c, c->Xup.get(), c->Pr2.get(), ldx, pv->vecs.get(), pv->vecs.get() + m, 2.0, 2.0 * c->Rd))
        rc = HDSDP_RETCODE_FAILED;
    for (int qi = 0; qi < c->mloc && rc == HDSDP_RETCODE_OK; ++qi) {
        // this fallback multiplies with A_L as a generic operand in both orientations: unpack the row's skyline storage
        // into a square scratch matrix first
        const double *Arow = c->rows.rows(qi, 1);
        if (!Arow || hdm_sky_to_square(Arow, ALsq.get(), c->n16, g.stream)) { rc = HDSDP_RETCODE_FAILED; break; }
        const double *AL = ALsq.get();
        // Pr1 = X A_L            (B operand element (j, k) = A_L(k, j): K-major)
        if (hdm_launch_gemm(hdm_gemm_product(c->Pr1.get(), ldx, n16, n16, n16, 1.0, Xm, hdm_kmajor(AL, n16)), g.stream)) { rc = HDSDP_RETCODE_FAILED; break; }
        // Pr1 += X A_L^T         (B operand element (j, k) = A_L(j, k): M-major)
        if (hdm_launch_gemm(hdm_gemm_product(c->Pr1.get(), ldx, n16, n16, n16, 1.0, Xm, hdm_mmajor(AL, n16), 1.0), g.stream)) { rc = HDSDP_RETCODE_FAILED; break; }
        // Pr2 = Pr1 X            (B operand element (j, k) = X(k, j): K-major)
        if (hdm_launch_gemm(hdm_gemm_product(c->Pr2.get(), ldx, n16, n16, n16, 1.0, hdm_mmajor(c->Pr1.get(), ldx), Xk), g.stream)) { rc = HDSDP_RETCODE_FAILED; break; }
        if (hipMemsetAsync(row.get(), 0, sizeof(double) * (size_t) m, g.stream) != hipSuccess ||
            cone_sym_dot2(c, c->Pr2.get(), nullptr, ldx, row.get(), row.get(), 2.0, 0.0)) { rc = HDSDP_RETCODE_FAILED; break; }
        hipLaunchKernelGGL(mi_put_row_kernel, dim3((m + 255) / 256), dim3(256), 0, g.stream, Mview, c->own[qi], row.get(), m);
    }
    if (hipStreamSynchronize(g.stream) != hipSuccess) rc = HDSDP_RETCODE_FAILED;
    if (rc != HDSDP_RETCODE_OK) return rc;
    if (c->Rd != 0.0) {                      // dTraceSinv += tr X (hdsdp_conic_sdp.c:1767-1769)
        double tr = 0.0;
        for (int i = 0; i < n; ++i) tr += X[(size_t) i * (n + 1)];
        kkt->dTraceSinv += tr;
    }
    return HDSDP_RETCODE_OK;
}

// Route 1 of KKT_TYPE_PRIMAL: the signed factor of an X that is not positive definite, and its acceptance test.  J X J = F S F^T
// without pivoting (HdmChol::factor_signed), W = J F^T J (lower triangular, in Linv's place as on route 0), sigma = J S J, so
// X = W^T diag(sigma) W.  An LDL' without pivoting can grow without bound, and M's rounding error scales with |W|^4 where the
// positive definite route's scales with |X|^2; so the factor is only used when, measured on the device,
//   residual = |W^T diag(sigma) W - X|_F / |X|_F <= PSIG_MAX_RESIDUAL   and   growth = |W|_F^2 / |X|_F <= PSIG_MAX_GROWTH sqrt(n)
// ("KKT_TYPE_PRIMAL with an indefinite X", says why these two).  For a positive definite X the growth is
// tr X / |X|_F <= sqrt(n).  Returns 0 and *ok; `why` names the failed check.
static constexpr double PSIG_MAX_RESIDUAL = 1e-11;
static constexpr double PSIG_MAX_GROWTH = 8.0;
int primal_signed_factor(MiCone *c, HdmChol &ch, const double *Xr, const double *X, bool *ok, const char **why) {
    *ok = false; *why = "zero pivot";
    const double t0 = host_now();
    int info = 0, nneg = 0;
    if (ch.load_host(Xr, c->n, g.stream)) return 1;
    HIP_RC(hipStreamSynchronize(g.stream));
    if (ch.factor_signed(g.stream, &info, &nneg)) return 1;
    c->primal_q = nneg;
    c->primal_growth = 0.0; c->primal_resid = 0.0;
    if (info != 0) return 0;                           // an exactly zero (or non-finite) pivot: no factor of this form exists
    if (ch.set_reverse_inverse(g.stream)) return 1;
    const long np = ch.npad;
    HIP_RC(c->psig.reserve((size_t) np));
    if (ch.reverse_signs(c->psig.get(), g.stream)) return 1;
    long ldx = 0;
    if (cone_upload_X(c, X, &ldx)) return 1;
    if (ldx != np) { fprintf(stderr, "[hdsdp_mi355x] KKT_TYPE_PRIMAL: factor and primal matrix disagree on their padding\n"); return 1; }
    const size_t np2 = sizeof(double) * (size_t) np * np;
    HIP_RC(c->Pr1.reserve(np2 / sizeof(double)));
    HIP_RC(c->Pr2.reserve(np2 / sizeof(double)));
    HIP_RC(c->pchk.reserve(3 * MI_PSIG_BLOCKS + 8));
    // Pr1 = diag(sigma) W,  Pr2 = W^T Pr1   (A operand element (i, k) = W(k, i), B operand element (j, k) = Pr1(k, j): both K-major)
    hipLaunchKernelGGL(mi_psig_rowscale_kernel, dim3((unsigned) ((np * np + 255) / 256)), dim3(256), 0, g.stream,
                       (const double *) ch.Linv.get(), (const double *) c->psig.get(), c->Pr1.get(), np, (int) np);
    HIP_RC(hipGetLastError());
    RC(hdm_launch_gemm(hdm_gemm_product(c->Pr2.get(), np, c->n16, c->n16, c->n16, 1.0, hdm_kmajor(ch.Linv.get(), np), hdm_kmajor(c->Pr1.get(), np)), g.stream));
    hipLaunchKernelGGL(mi_psig_norms_kernel, dim3(MI_PSIG_BLOCKS), dim3(256), 0, g.stream, (const double *) c->Pr2.get(), (const double *) c->Xup.get(),
                       (const double *) ch.Linv.get(), np, c->n, c->pchk.get());
    hipLaunchKernelGGL(mi_psig_norms_final_kernel, dim3(1), dim3(64), 0, g.stream, (const double *) c->pchk.get(), MI_PSIG_BLOCKS,
                       c->pchk.get() + 3 * MI_PSIG_BLOCKS);
    HIP_RC(hipGetLastError());
    double nr[3] = {0, 0, 0};
    HIP_RC(hipMemcpyAsync(nr, c->pchk.get() + 3 * MI_PSIG_BLOCKS, sizeof(nr), hipMemcpyDeviceToHost, g.stream));
    HIP_RC(hipStreamSynchronize(g.stream));
    const double xf = std::sqrt(nr[1]);
    c->primal_resid = xf > 0.0 ? std::sqrt(nr[0]) / xf : INFINITY;
    c->primal_growth = xf > 0.0 ? nr[2] / xf : INFINITY;
    c->primal_ms[0] = (host_now() - t0) * 1e3;
    if (!(c->primal_resid <= PSIG_MAX_RESIDUAL)) { *why = "reconstruction residual"; return 0; }
    if (!(c->primal_growth <= PSIG_MAX_GROWTH * std::sqrt((double) c->n))) { *why = "growth"; return 0; }
    *ok = true; *why = "";
    return 0;
}

static bool primal_signed_enabled() { return hdm_env_on<ENV_PRIMAL_SIGNED>(); }

// Every shard of a sharded block factors the same replicated X with the same kernels, so all of them must come to the same
// decision (a shard that went on alone would wait for the others in the exchange).  Checked, not assumed: the sums of
// (accepted, q) over the ranks must be world times this rank's.
int primal_shards_agree(MiCone *c, bool ok, bool *agree) {
    *agree = true;
    if (c->world <= 1) return 0;
    if (!c->allreduce) return 1;
    HIP_RC(c->pchk.reserve(3 * MI_PSIG_BLOCKS + 8));
    double *w = c->pchk.get() + 3 * MI_PSIG_BLOCKS + 4;
    const double mine[2] = {ok ? 1.0 : 0.0, (double) c->primal_q};
    HIP_RC(hipMemcpyAsync(w, mine, sizeof(mine), hipMemcpyHostToDevice, g.stream));
    HIP_RC(hipStreamSynchronize(g.stream));
    if (c->allreduce(c->xctx, w, 2)) return 1;
    double sum[2] = {0, 0};
    HIP_RC(hipMemcpyAsync(sum, w, sizeof(sum), hipMemcpyDeviceToHost, g.stream));
    HIP_RC(hipStreamSynchronize(g.stream));
    *agree = sum[0] == c->world * mine[0] && sum[1] == c->world * mine[1];
    return 0;
}

// KKT_TYPE_PRIMAL routing: 0 = X positive definite, the Cholesky factor (unchanged); 1 = the signed factor passed its acceptance
// test: the congruence + Gram path with the signed Gram correction; 2 = neither: the row-by-row fallback on one device, a refusal
// on a sharded block.  HDSDP_MI355X_PRIMAL_SIGNED=0: route 1 is never tried (0 or 2, as before it existed).
hdsdp_retcode build_primal(MiCone *c, int iCone, hdsdp_kkt *kkt, MiKKTPriv *pv) {
    if (!kkt->dPrimalX || !kkt->dPrimalX[iCone]) return HDSDP_RETCODE_FAILED;   // :1747-1750
    const double *X = kkt->dPrimalX[iCone];
    const int n = c->n;
    if (!c->primal) {
        c->primal.reset(new HdmChol());
        if (c->primal->init(n)) return HDSDP_RETCODE_MEMORY;
    }
    std::vector<double> Xr((size_t) n * n);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) Xr[(size_t) i + (size_t) j * n] = X[(size_t) (n - 1 - i) + (size_t) (n - 1 - j) * n];
    HdmChol &ch = *c->primal;
    int info = 0;
    if (ch.load_host(Xr.data(), n, g.stream)) return HDSDP_RETCODE_FAILED;
    HIP_RC(hipStreamSynchronize(g.stream));   // Xr is pageable host memory going out of scope
    if (ch.factor(g.stream, &info)) return HDSDP_RETCODE_FAILED;
    if (info == 0) {
        c->primal_route = 0; c->primal_q = 0; c->primal_growth = 0.0;
        if (ch.set_reverse_inverse(g.stream)) return HDSDP_RETCODE_FAILED;
        return build_gemm_path(c, kkt, pv, KKT_TYPE_PRIMAL, &ch);
    }
    if (!primal_signed_enabled()) {               // X is not positive definite: no factor to lean on
        c->primal_route = 2; c->primal_q = 0; c->primal_growth = 0.0;
        return build_primal_general(c, kkt, pv, X);
    }
    bool ok = false, agree = true;
    const char *why = "";
    if (primal_signed_factor(c, ch, Xr.data(), X, &ok, &why)) return HDSDP_RETCODE_FAILED;
    if (primal_shards_agree(c, ok, &agree)) return HDSDP_RETCODE_FAILED;
    if (!agree) {
        fprintf(stderr, "[hdsdp_mi355x] KKT_TYPE_PRIMAL: the shards of a block disagree about the signed factor of the same X\n");
        return HDSDP_RETCODE_FAILED;
    }
    if (!ok) {
        c->primal_route = 2;
        if (c->world > 1) {
            fprintf(stderr, "[hdsdp_mi355x] KKT_TYPE_PRIMAL: an indefinite primal matrix is not supported on a sharded block unless its "
                            "signed factor passes; it failed the %s check (negative pivots %d, growth %.3g, residual %.3g)\n",
                    why, c->primal_q, c->primal_growth, c->primal_resid);
            return HDSDP_RETCODE_FAILED;
        }
        return build_primal_general(c, kkt, pv, X);
    }
    c->primal_route = 1;
    c->gram_sig = c->psig.get();
    hdsdp_retcode rc = build_gemm_path(c, kkt, pv, KKT_TYPE_PRIMAL, &ch);
    c->gram_sig = nullptr;
    // the "S row" back to I for every other build (it is written once, at allocation: cone_alloc_gemm_work)
    if (c->rank == 0 && c->work_ready && hdm_blocked_eye(c->AhatLoc, c->Lr, c->mloc + 1, c->nblk, c->n, g.stream)) rc = HDSDP_RETCODE_FAILED;
    return rc;
}

hdsdp_retcode cone_build_schur(void *cd, int iCone, void *kktv, int typeKKT) {
    (void) iCone;
    MiCone *c = (MiCone *) cd;
    hdsdp_kkt *kkt = (hdsdp_kkt *) kktv;
    MiKKTPriv *pv = priv_of(kkt);
    if (typeKKT == KKT_TYPE_PRIMAL) return build_primal(c, iCone, kkt, pv);
    MiLin *l = (MiLin *) c->dualFactor->chol;
    if (!l->ch.factored) {
        fprintf(stderr, "[hdsdp_mi355x] BuildSchur: the dual matrix has no valid Cholesky factor\n");
        return HDSDP_RETCODE_FAILED;
    }
    if (c->path == PATH_R1) return build_r1_path(c, kkt, pv, typeKKT);
    if (c->path == PATH_SPARSE) return build_sparse_path(c, kkt, pv, typeKKT);
    return build_gemm_path(c, kkt, pv, typeKKT);
}
hdsdp_retcode cone_build_schur_fixed(void *cd, int iCone, void *kktv, int typeKKT, int strategy) {
    (void) strategy;  // all strategies are the same numbers (reference invariant, hdsdp_utils.c:536-707)
    return cone_build_schur(cd, iCone, kktv, typeKKT);
}

// where the builders put M: the dense device matrix, or the tile store of a sparse operator in tile form
HdmMatView kkt_view(hdsdp_kkt *kkt) {
    MiLin *l = (MiLin *) kkt->kktM->chol;
    if (l->bsp) return l->bsp->view_M();
    HdmMatView v;
    v.base = l->Mdev.get(); v.ld = l->ch.npad;
    return v;
}
double *kkt_Mdev(hdsdp_kkt *kkt, long *ld) {
    MiLin *l = (MiLin *) kkt->kktM->chol;
    if (ld) *ld = l->ch.npad;
    return l->Mdev.get();
}

hdsdp_retcode corrector_components(MiCone *c, HdmChol &ch, MiKKTPriv *pv, int m) {
    // ASinv_i = <A_i, S^-1>, ASinvRdSinv_i = Rd <A_i, S^-2>   (hdsdp_conic_sdp.c:1035-1056)
    const size_t nn = sizeof(double) * (size_t) ch.npad * ch.npad;
    if (c->Xinv.reserve(nn / sizeof(double)) != hipSuccess) return HDSDP_RETCODE_MEMORY;
    if (c->Yinv.reserve(nn / sizeof(double)) != hipSuccess) return HDSDP_RETCODE_MEMORY;
    RC(ch.inverse_full(c->Xinv.get(), ch.npad, g.stream));
    const double *Y = nullptr;
    if (c->Rd != 0.0) {
        const HdmOperand X = hdm_mmajor(c->Xinv.get(), ch.npad);   // Y = X * X^T = S^-2
        RC(hdm_launch_gemm(hdm_gemm_product(c->Yinv.get(), ch.npad, c->n16, c->n16, c->n16, 1.0, X, X), g.stream));
        Y = c->Yinv.get();
    }
    // A is stored in A_L form: <A, X> = 2 <A_L, X>
    if (c->world == 1) {
        RC(cone_sym_dot2(c, c->Xinv.get(), Y, ch.npad, pv->vecs.get(), pv->vecs.get() + m, 2.0, 2.0 * c->Rd));
        return HDSDP_RETCODE_OK;
    }
    // Sharded block: pv->vecs is the accumulator of the whole operator (every engine cone adds into it), so the sum
    // over the ranks runs on this cone's own contribution only and is added afterwards; reducing pv->vecs itself would
    // multiply what the cones before this one have put there by the number of ranks.
    HIP_RC(c->corr.reserve(2 * (size_t) m));
    HIP_RC(hipMemsetAsync(c->corr.get(), 0, sizeof(double) * 2 * (size_t) m, g.stream));
    RC(cone_sym_dot2(c, c->Xinv.get(), Y, ch.npad, c->corr.get(), c->corr.get() + m, 2.0, 2.0 * c->Rd));
    HIP_RC(hipStreamSynchronize(g.stream));
    if (!c->allreduce || c->allreduce(c->xctx, c->corr.get(), (int64_t) 2 * m)) return HDSDP_RETCODE_FAILED;
    if (c->kkt_owner) RC(hdm_axpy_mat(pv->vecs.get(), pv->vecs.get(), c->corr.get(), 1.0, 2L * m, g.stream));
    HIP_RC(hipStreamSynchronize(g.stream));
    return HDSDP_RETCODE_OK;
}

// The direct rows of the cone (direct_rows.h): local rows [mloc - dr_n, mloc) of the transformed-row buffer from their terms.
// U = Linv [a_j] for the rank-one ones is the call build_r1_path makes: the generic role, whose every tile runs the masked loop
// (DESIGN section 4 records what an unmasked generic tile once did).  With a factor override `ch` is the primal factor object.
hdsdp_retcode direct_rows_build(MiCone *c, HdmChol &ch) {
    if (c->dr_r1 > 0) {
        RC(hdm_launch_gemm(hdm_gemm_product(c->dr_U.get(), c->n16, c->n16, c->dr_r1_16, c->n16, 1.0, hdm_mmajor(ch.Linv.get(), ch.npad),
                                            hdm_kmajor(c->dr_fac.get(), c->n16), 0.0, hdm_klimit(HDM_KLIM_BY_M)), g.stream));
    }
    HdmDirectArgs a = {};
    a.dst = c->AhatLoc; a.row_stride = c->Lr; a.row0 = c->mloc - c->dr_n; a.nrows = c->dr_n; a.nblk = c->nblk; a.n = c->n;
    a.terms = c->dr_terms.get(); a.row_ptr = c->dr_ptr.get();
    a.Linv = ch.Linv.get(); a.ldl = ch.npad; a.U = c->dr_U.get(); a.ldu = c->n16;
    a.dst_span = (long) hdm_exchange_doubles(cone_layout(c)); a.linv_span = hdm_linv_span(ch.npad); a.u_span = (long) c->dr_U.count();
    a.max_lcol = c->dr_max_lcol; a.nu = c->dr_r1;
    return hdm_direct_rows(a, g.stream) ? HDSDP_RETCODE_FAILED : HDSDP_RETCODE_OK;
}

hdsdp_retcode build_gemm_path(MiCone *c, hdsdp_kkt *kkt, MiKKTPriv *pv, int typeKKT, HdmChol *chOverride) {
    MiLin *l = (MiLin *) c->dualFactor->chol;
    HdmChol &ch = chOverride ? *chOverride : l->ch;
    const int m = kkt->nRow;
    if (typeKKT == KKT_TYPE_CORRECTOR) return corrector_components(c, ch, pv, m);
    if (!c->work_ready) {
        if (cone_alloc_gemm_work(c)) return HDSDP_RETCODE_MEMORY;
        c->work_ready = true;
    }
    if (c->gram_sig && c->rank == 0) {   // route 1 of KKT_TYPE_PRIMAL: the "S row" carries diag(sigma) (build_primal restores I)
        hipLaunchKernelGGL(mi_psig_srow_kernel, dim3(c->nblk), dim3(256), 0, g.stream, c->AhatLoc, (long) c->Lr, (long) c->mloc + 1,
                           c->nblk, c->n, c->gram_sig);
        HIP_RC(hipGetLastError());
    }
    HIP_RC(hipEventRecord(g.ev[0], g.stream));
    RC(ch.invert_factor(g.stream));
    HIP_RC(hipEventRecord(g.ev[1], g.stream));
    const long afull_rows = std::max(1, c->mloc);   // matrices behind the resident storage (engine_rows.h: its allocation)
    // Multi-GPU: run step 2 of the owned rows by packed-index range, in the order of the exchange pieces, so that a piece
    // crosses the links while the later ranges are still being computed (at two ranks the all-to-all moves 8 GB per
    // rank over a single link, more than the Gram product alone can hide).  Needs the piecewise exchange hooks, all
    // owned rows in one launch group and at most 64 tile columns.  HDSDP_MI355X_STAGED_A2A=0: drain, then exchange.
    const int NT = hdm_ntiles(c->n16);
    int P = (c->world > 1) ? exchange_pieces(c) : 1;
    bool staged = c->world > 1 && P > 1 && P <= 64 && c->mloc <= c->Bc && hdm_colmask_honoured(NT) && hdm_env_on<ENV_STAGED_A2A>();
    c->last_pieces = P; c->last_staged = 0;
    const double *Ares = c->rows.resident();
    if (c->rows.streamed()) {
        // constraint data not resident: a batch is regenerated, transformed, and its buffer reused (stream order keeps the
        // generator of batch k + 1 behind step 1 of batch k, the only reader)
        staged = false;
        for (int q0 = 0, B = c->rows.batch(); q0 < c->mloc; q0 += B) {
            const int nb = std::min(B, c->mloc - q0);
            const double *A = c->rows.rows(q0, nb);
            if (!A) return HDSDP_RETCODE_FAILED;
            RC(congruence_rows(c, ch, A, B, nb, q0));
        }
    } else if (!staged) RC(congruence_rows(c, ch, Ares, afull_rows, c->mloc - c->dr_n, 0));
    if (c->dr_n > 0) RC(direct_rows_build(c, ch));   // (one device, resident rows: never staged, never streamed)
    if (c->rank == 0) {
        // "I row": A = I => T = Linv, At = Linv Linv^T.  Reuse step 2 with T := Linv.
        RC(hdm_launch_gemm(hdm_cong_irow(cone_layout(c), ch.Linv.get(), ch.npad, c->AhatLoc, c->mloc), g.stream));
        if (typeKKT == KKT_TYPE_HOMOGENEOUS) {
            if (!c->CL.get()) {
                HIP_RC(c->CL.alloc((size_t) c->astride, hdm_operand_pad(c->n16)));
                HIP_RC(hipMemsetAsync(c->CL.get(), 0, sizeof(double) * (size_t) c->astride, g.stream));
                RC(hdm_lower_half(c->Cfull.get(), c->CL.get(), c->n, c->n16, g.stream));
            }
            RC(congruence_rows(c, ch, c->CL.get(), 1, 1, c->mloc + 2));
        }
    }
    if (staged) {
        RC(congruence_rows(c, ch, Ares, afull_rows, c->mloc, 0, 1));
        if (prof_record(c->pe_s1, g.stream)) return HDSDP_RETCODE_FAILED;
        const unsigned long long all = (NT >= 64) ? ~0ULL : ((1ULL << NT) - 1);
        unsigned long long done = 0;
        for (int k = 0; k < P; ++k) {
            unsigned long long mk = (k == P - 1 ? all : piece_tile_cols(c, k, P)) & all & ~done;
            if (mk) { RC(congruence_rows(c, ch, Ares, afull_rows, c->mloc, 0, 2, mk)); c->last_staged += 1; }
            done |= mk;
            if (!c->piece_ev[k]) HIP_RC(hipEventCreateWithFlags(&c->piece_ev[k], hipEventDisableTiming));
            HIP_RC(hipEventRecord(c->piece_ev[k], g.stream));
            if (prof_record(c->pe_s2[k], g.stream)) return HDSDP_RETCODE_FAILED;
        }
    }
    HIP_RC(hipEventRecord(g.ev[2], g.stream));
    c->prof.valid = false;
    if (c->world > 1) { RC(exchange_and_gram(c, staged)); }
    else { RC(gram_all(c)); }
    if (c->gram_sig) RC(signed_correction(c));   // this rank's partial, before the all-reduce
    HIP_RC(hipEventRecord(g.ev[3], g.stream));
    if (c->world > 1) {
        HIP_RC(hipStreamSynchronize(g.stream));
        const double t0 = host_now();
        if (!c->allreduce || c->allreduce(c->xctx, c->Gm.get(), (int64_t) c->R * c->R)) return HDSDP_RETCODE_FAILED;
        c->prof.allreduce_host = (host_now() - t0) * 1e3;
    }
    const int hsd = (typeKKT == KKT_TYPE_HOMOGENEOUS);
    const long pI = (c->world == 1) ? c->mloc : (c->m + c->world - 1) / c->world;  // rows owned by rank 0 = position of the "I row"
    if (c->kkt_owner)
        RC(hdm_extract(c->Gm.get(), c->R, c->R, pI, c->rows_seg.get(), kkt_view(kkt), pv->vecs.get(), pv->vecs.get() + m, pv->vecs.get() + 2 * m,
                       pv->vecs.get() + 3 * m, c->Rd, hsd, g.stream));
    HIP_RC(hipEventRecord(g.ev[4], g.stream));
    HIP_RC(hipEventSynchronize(g.ev[4]));
    float ms = 0;
    for (int i = 0; i < 4; ++i) {
        (void) hipEventElapsedTime(&ms, g.ev[i], g.ev[i + 1]);
        g.stage_ms[i] = ms;
    }
    if (c->world > 1) {
        // the sharded build's profile: every event above has completed (ev[4] is the last on the stream)
        auto el = [](hipEvent_t a, hipEvent_t b) { float t = 0.f; return (a && b && hipEventElapsedTime(&t, a, b) == hipSuccess) ? (double) t : 0.0; };
        MiCone::BuildProfile &pf = c->prof;
        const int Pp = std::max(1, std::min(c->last_pieces, MiCone::BuildProfile::MAXP));
        pf.pieces = Pp; pf.staged = staged ? 1 : 0;
        pf.invert = g.stage_ms[0]; pf.cong = g.stage_ms[1]; pf.extract = g.stage_ms[3];
        pf.step1 = staged ? el(g.ev[1], c->pe_s1) : 0.0;
        for (int k = 0; k < Pp; ++k) {
            pf.step2[k] = staged ? el(k == 0 ? c->pe_s1 : c->pe_s2[k - 1], c->pe_s2[k]) : 0.0;
            pf.wait_gpu[k] = el(k == 0 ? g.ev[2] : c->pe_gb[k - 1], c->pe_ga[k]);
            pf.gram[k] = el(c->pe_ga[k], c->pe_gb[k]);
        }
        pf.reduce = el(c->pe_gb[Pp - 1], g.ev[3]);
        pf.valid = true;
    }
    return HDSDP_RETCODE_OK;
}
