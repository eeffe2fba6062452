// engine_rows.h -- MiRows: the one owner of an SDP block's constraint rows on the device
// Implementation header of engine.hip: included exactly once, there, before engine_cone.h (the pieces share the anonymous
// namespace and the engine's thread-local context `g`).
// The rows -- the A_L forms the congruence, the S / dS sweeps, the norms and A X read -- live in one of three forms
// (row_store_rule.h: HdmRowForm; the rule that chooses among them is there too).  Everything that depends on the form is in this
// file: the storage, the three ways a store is filled, rows() for whoever reads the dense form, and the sweep copy.

// what the store knows of its cone (MiCone is its owner; `own` points at the cone's vector, which outlives the store's use of it)
struct MiRowShape {
    int n = 0, n16 = 0, mloc = 0, world = 1;
    long astride = 0;                       // elements per stored row (skyline storage of the A_L form, gemm_geom.h)
    const std::vector<int> *own = nullptr;  // global indices of the owned rows, in local order
};

// Rows of a presolved block -> A_L forms in skyline storage on the device.  The entries travel as they are -- (packed index,
// value), 12 bytes each -- and are scattered on the device into a zeroed target (hdm_scatter_low): host threads copy a group
// of rows into one of two pinned staging buffers while the other one crosses PCIe.  (Up to round 4 the host densified every row
// into a packed image first -- a 16 MB memset and an 800 K-entry scatter per row on one core, one synchronisation per 16 rows:
// most of the 14 s the reference's driver spent in its pre-solver at n = m = 2000.)
struct RowUploader {
    struct Stage { HdmPinned<int> hi; HdmBuf<int> di; HdmPinned<double> hv; HdmBuf<double> dv; HdmPinned<long> hb; HdmBuf<long> db; hipEvent_t ev = nullptr; bool used = false; } st[2];
    const MiRowShape &sh;
    const MiBlockData &blk;
    long cap = 0;
    static constexpr int rowcap = 1024;
    int which = 0;
    RowUploader(const MiRowShape &sh_, const MiBlockData &blk_) : sh(sh_), blk(blk_) {}
    const MiCoeff &row(int q) const { return blk.rows[(*sh.own)[q]]; }
    int init() {
        long maxrow = 1, total = 0;
        for (int q = 0; q < sh.mloc; ++q) {
            const long k = (long) row(q).idx.size();
            maxrow = std::max(maxrow, k);
            total += k;
        }
        // entries per staging buffer: 192 MiB worth, or one row if that is more -- and never more than the block holds (a problem
        // of many small blocks creates many cones: each would otherwise pin 384 MiB of host memory for a few KB of entries)
        cap = std::max(maxrow, std::min((long) ((192L << 20) / 12), std::max(1L, total)));
        for (auto &b : st) {
            if (b.hi.alloc((size_t) cap) != hipSuccess ||
                b.hv.alloc((size_t) cap) != hipSuccess ||
                b.hb.alloc(rowcap + 1) != hipSuccess ||
                b.di.alloc((size_t) cap) != hipSuccess || b.dv.alloc((size_t) cap) != hipSuccess ||
                b.db.alloc(rowcap + 1) != hipSuccess || hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess)
                return 1;
        }
        return 0;
    }
    // owned rows q0 .. q0 + count - 1 into the ZEROED storage at dst (stride astride), queued on the engine stream
    int rows(int q0, int count, double *dst) {
        for (int r0 = q0; r0 < q0 + count;) {
            Stage &b = st[which];
            which ^= 1;
            if (b.used && hipEventSynchronize(b.ev) != hipSuccess) return 1;   // its previous group has left the buffer
            int nc = 0;
            long tot = 0, mx = 0;
            long *hb = b.hb.get();
            hb[0] = 0;
            while (r0 + nc < q0 + count && nc < rowcap) {
                const long k = (long) row(r0 + nc).idx.size();
                if (nc > 0 && tot + k > cap) break;
                tot += k; mx = std::max(mx, k); nc += 1;
                hb[nc] = tot;
            }
            std::atomic<int> next{0};
            mi_parallel(tot >= (1L << 20) ? 0 : 1, [&](int) {
                for (int q = next.fetch_add(1); q < nc; q = next.fetch_add(1)) {
                    const MiCoeff &co = row(r0 + q);
                    if (co.idx.empty()) continue;
                    memcpy(b.hi.get() + hb[q], co.idx.data(), sizeof(int) * co.idx.size());
                    memcpy(b.hv.get() + hb[q], co.val.data(), sizeof(double) * co.val.size());
                }
            });
            if (tot > 0) {
                if (hipMemcpyAsync(b.di.get(), b.hi.get(), sizeof(int) * (size_t) tot, hipMemcpyHostToDevice, g.stream) != hipSuccess ||
                    hipMemcpyAsync(b.dv.get(), b.hv.get(), sizeof(double) * (size_t) tot, hipMemcpyHostToDevice, g.stream) != hipSuccess ||
                    hipMemcpyAsync(b.db.get(), hb, sizeof(long) * (size_t) (nc + 1), hipMemcpyHostToDevice, g.stream) != hipSuccess ||
                    hdm_scatter_low(b.di.get(), b.dv.get(), b.db.get(), mx, dst + (long) (r0 - q0) * sh.astride, sh.astride, sh.n, sh.n16, nc, g.stream))
                    return 1;
            }
            if (hipEventRecord(b.ev, g.stream) != hipSuccess) return 1;
            b.used = true;
            r0 += nc;
        }
        return 0;
    }
    ~RowUploader() {   // (the stages' buffers go after this body: once their last copies have left them)
        for (auto &b : st) {
            if (b.ev) (void) hipEventSynchronize(b.ev);
            if (b.ev) (void) hipEventDestroy(b.ev);
        }
    }
};

class MiRows {
    MiRowShape sh;
    HdmRowForm form_ = HDM_ROWS_RESIDENT;
    HdmBuf<double> Afull;      // RESIDENT: mloc x astride constraint matrices in A_L form: strict lower + half diagonal
    HdmBuf<double> Abatch;     // streamed: the buffer a batch of Bs matrices is regenerated / expanded into
    int Bs = 0;
    HdmZs zs;                  // zero-suppressed copy for the S / dS sweeps (schur.h); EXPANDED: the only image of the data
    bool zs_in_use = false;    // the sweeps read the copy (it may exist and be switched off: HMiConeUseSweepCopy)

    size_t resident_count() const { return (size_t) sh.astride * std::max(1, sh.mloc); }   // (also the span role launches vouch for)
    int alloc_batch() {
        Bs = (int) hdm_rows_batch(sh.mloc, hdm_knobs_from_env().bc_max);
        if (Abatch.alloc((size_t) sh.astride * Bs, hdm_operand_pad(sh.n16)) != hipSuccess) {
            fprintf(stderr, "[hdsdp_mi355x] cannot allocate %.1f GiB for a batch of constraint matrices\n", (double) sh.astride * Bs * 8 / (1 << 30));
            return 1;
        }
        return hdm_memset_sync(Abatch.get(), 0, sizeof(double) * (size_t) sh.astride * Bs) != hipSuccess;
    }

public:
    HdmRowForm form() const { return form_; }
    bool streamed() const { return form_ != HDM_ROWS_RESIDENT; }
    // the resident storage (owned row q at q * astride), or nullptr: what reads all rows in place asks for this
    const double *resident() const { return Afull.get(); }
    // The A_L forms of the owned rows q0 .. q0 + count - 1 on the device (stride astride): the resident storage, or -- streamed --
    // the batch buffer after regenerating / expanding them into it (count <= batch(); valid until the next call; ordered on the
    // engine stream behind whatever still reads the previous batch).
    const double *rows(int q0, int count) {
        if (!streamed()) return Afull.get() ? Afull.get() + (long) q0 * sh.astride : nullptr;
        if (!Abatch.get() || count > Bs || q0 < 0 || q0 + count > sh.mloc) return nullptr;
        if (form_ == HDM_ROWS_EXPANDED) return hdm_zs_expand(zs, q0, count, Abatch.get(), sh.astride, g.stream) ? nullptr : Abatch.get();
        const std::vector<int> &own = *sh.own;
        if (sh.world == 1) {                       // owned rows are consecutive in the global numbering
            if (hdm_synth_fill_low(Abatch.get(), sh.astride, sh.n, sh.n16, own[q0], count, g.stream)) return nullptr;
        } else {
            for (int q = 0; q < count; ++q)
                if (hdm_synth_fill_low(Abatch.get() + (long) q * sh.astride, sh.astride, sh.n, sh.n16, own[q0 + q], 1, g.stream)) return nullptr;
        }
        return Abatch.get();
    }
    int batch() const { return streamed() ? std::max(1, Bs) : std::max(1, sh.mloc); }   // (one batch = everything when the data is resident)
    bool has_rows() const { return streamed() ? Abatch.get() != nullptr : Afull.get() != nullptr; }

    // ---- the sweep copy ----
    bool sweep_copy_in_use() const { return zs_in_use; }
    const HdmZs &sweep_copy() const { return zs; }
    void use_sweep_copy(bool on) { zs_in_use = on && zs.val; }
    // the copy from the store's own rows, unless there is one already, and in use if it came out (more than max_fill of the stored
    // positions non-zero, or no memory: no copy, and the sweeps read the dense form).  Nonzero: a device error.
    int make_sweep_copy(double max_fill) {
        if (!zs.val && has_rows() && sh.mloc > 0 &&
            hdm_zs_build_from([&](int q0, int nb) { return rows(q0, nb); }, batch(), sh.astride, sh.mloc, sh.astride, max_fill, &zs, g.stream))
            return 1;
        use_sweep_copy(true);
        return 0;
    }
    // the copy gives its memory back (row_store_rule.h: hdm_sweep_copy_yields) -- never where the rows live in it
    void yield_sweep_copy() {
        if (form_ == HDM_ROWS_EXPANDED) return;
        hdm_zs_free(&zs);
        zs_in_use = false;
    }

    // ---- construction: one of the three, once ----
    // every owned row of a presolved block resident as an A_L form in skyline storage
    int upload_resident(const MiRowShape &shape, const MiBlockData &blk) {
        sh = shape; form_ = HDM_ROWS_RESIDENT;
        HDM_HIP_CHECK(Afull.alloc(resident_count(), hdm_operand_pad(sh.n16)));
        HDM_HIP_CHECK(hdm_memset_sync(Afull.get(), 0, sizeof(double) * resident_count()));
        RowUploader up(sh, blk);
        return (up.init() || up.rows(0, sh.mloc, Afull.get()) || hipStreamSynchronize(g.stream) != hipSuccess) ? 1 : 0;
    }
    // INGESTED rows that are too many to stay resident (round 5): batch after batch they are scattered into the batch buffer and
    // compressed into the zero-suppressed copy (two passes: counts, then values -- every batch crosses PCIe twice), which from
    // then on is the ONLY image of the constraint data: the sweeps read it as they always do, and whoever needs the dense A_L
    // forms (the congruence, norms, A X) has a batch expanded from it (rows -> hdm_zs_expand) -- what the counter-based generator
    // does for the synthetic family.  n = 2000, m = 8000 at 40 % fill: 57 GB instead of 136.
    int ingest_expanded(const MiRowShape &shape, const MiBlockData &blk) {
        sh = shape;
        if (alloc_batch()) return 1;
        {
            RowUploader up(sh, blk);
            if (up.init()) return 1;
            bool bad = false;
            auto source = [&](int q0, int nb) -> const double * {
                if (hipMemsetAsync(Abatch.get(), 0, sizeof(double) * (size_t) sh.astride * nb, g.stream) != hipSuccess || up.rows(q0, nb, Abatch.get())) { bad = true; return nullptr; }
                return Abatch.get();
            };
            if (hdm_zs_build_from(source, Bs, sh.astride, sh.mloc, sh.astride, 1.0, &zs, g.stream) || bad) return 1;
            if (hipStreamSynchronize(g.stream) != hipSuccess) return 1;
        }
        if (!zs.val) {
            fprintf(stderr, "[hdsdp_mi355x] block n = %d, m = %d: no room for the compressed copy its streamed rows live in\n", sh.n, sh.mloc);
            return 1;
        }
        form_ = HDM_ROWS_EXPANDED;
        zs_in_use = true;
        fprintf(stderr, "[hdsdp_mi355x] block n = %d, m = %d: %.1f GiB of constraint data are kept as a %.1f GiB zero-suppressed copy and expanded %d matrices at a time, not resident\n",
                sh.n, sh.mloc, (double) sh.astride * sh.mloc * 8 / (1 << 30),
                (8.0 * (double) zs.nnz + 192.0 * (double) zs.nchunk * sh.mloc) / (1 << 30), Bs);
        return 0;
    }
    // the synthetic family: every owned row generated into resident storage, or nothing kept -- BASELINE configs[4] on
    // one device is 136 GB of A_L forms beside 130 GB of transformed rows -- and every reader walks them batch by batch through rows()
    hdsdp_retcode generate(const MiRowShape &shape, bool stream) {
        sh = shape; form_ = stream ? HDM_ROWS_GENERATED : HDM_ROWS_RESIDENT;
        if (stream) {
            if (alloc_batch()) return HDSDP_RETCODE_MEMORY;
            fprintf(stderr, "[hdsdp_mi355x] block n = %d, m = %d: %.1f GiB of constraint data are streamed (regenerated %d matrices at a time), not resident\n",
                    sh.n, sh.mloc, (double) sh.astride * sh.mloc * 8 / (1 << 30), Bs);
            return HDSDP_RETCODE_OK;
        }
        if (Afull.alloc(resident_count(), hdm_operand_pad(sh.n16)) != hipSuccess) {
            fprintf(stderr, "[hdsdp_mi355x] cannot allocate %.1f GiB for the constraint matrices\n", (double) sh.astride * sh.mloc * 8 / (1 << 30));
            return HDSDP_RETCODE_MEMORY;
        }
        if (hdm_memset_sync(Afull.get(), 0, sizeof(double) * resident_count()) != hipSuccess) return HDSDP_RETCODE_FAILED;
        for (int q = 0; q < sh.mloc; ++q)  // owned rows are strided in the global numbering
            if (hdm_synth_fill_low(Afull.get() + (long) q * sh.astride, sh.astride, sh.n, sh.n16, (*sh.own)[q], 1, g.stream)) return HDSDP_RETCODE_FAILED;
        return HDSDP_RETCODE_OK;
    }
};
