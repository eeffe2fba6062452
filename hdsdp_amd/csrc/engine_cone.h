// engine_cone.h -- the MI355X SDP cone: device state (MiCone), the operator's private state (MiKKTPriv) and the cone slots -- S assembly, interior checks, barrier, ratio test, norms, A X, primal recovery
// Implementation header of engine.hip: included exactly once, there, in this order (the pieces share the anonymous namespace
// and the engine's thread-local context `g`); split out of a 3 300-line file in round 3, nothing else changed.
// =============================================================================================
// MI355X SDP cone
// =============================================================================================
enum { PATH_GEMM = 0, PATH_R1 = 1, PATH_SPARSE = 2 };

struct MiKKTPriv;

struct MiCone {
    int n = 0, m = 0;          // block dimension, global number of constraints
    int rank = 0, world = 1;   // row sharding: constraint i is owned by rank i % world
    int mloc = 0;              // constraints owned here
    int n16 = 0;               // n rounded up to 16 (MFMA sub-tile)
    int nblk = 0;              // n16 / 16
    long npb = 0;              // p-blocks of the blocked congruence layout: nblk(nblk+1)/2 * 16
    long npb_loc = 0;          // p-blocks per rank (K range of the local Gram part)
    int Lr = 0;                // rows per segment of the Gram operand (local rows + 3 augmented, padded)
    int path = PATH_GEMM;
    bool synthetic = false;
    MiBlockData blk;           // presolve results (empty rows for synthetic)
    std::vector<int> own;      // global indices of the owned constraints, in local order: ascending, unless the cone has direct rows
    // Direct rows (direct_rows.h): local rows [mloc - dr_n, mloc) are written into the transformed-row buffer from their
    // terms, without the congruence; the local order is then congruence rows (ascending), direct rows (ascending).
    std::vector<int> own_asc;  // `own` ascending, for the pattern protocol (the same vector's order for a cone without direct rows)
    int dr_n = 0, dr_r1 = 0, dr_kmax = 0;   // direct rows, the rank-one ones among them, the kmax in force (0: the form is off)
    int dr_max_lcol = -1;      // largest column of the factor inverse a term names
    HdmBuf<HdmDirectTerm> dr_terms;   // the term table, row d's terms at [dr_ptr[d], dr_ptr[d + 1])
    HdmBuf<long> dr_ptr;
    HdmBuf<double> dr_fac, dr_U;      // n16 x dr_r1_16: the rank-one direct rows' factors (K-major, zero-padded), and L^-1 times them
    int dr_r1_16 = 0;
    // device data
    MiRows rows;               // the constraint rows: resident, generated per batch or expanded per batch, and the sweep copy (engine_rows.h)
    HdmBuf<double> Cfull;      // n16 x n16 objective, full symmetric
    HdmBuf<double> CL;         // objective in A_L form (GEMM path, HSD builds)
    HdmBuf<double> Avec;       // n16 x mloc16 rank-one factors (R1 path)
    HdmBuf<double> sgn;        // mloc signs (R1 path)
    int mloc16 = 0;
    long astride = 0;          // elements per stored constraint matrix (skyline storage of the A_L form, gemm_geom.h)
    HdmBuf<int> sp_rp, sp_ti, sp_tj;   // sparse path: triplets of the owned rows
    HdmBuf<double> sp_tv;
    HdmBuf<int> rows_seg;      // world*Lr: segment-ordered Gram row -> global constraint (-1 pad, -2.. aug)
    HdmBuf<int> rows_own;      // mloc: owned row -> global constraint
    HdmBuf<double> S, Scheck;  // n x n (ld n16) dual matrix buffers
    HdmBuf<double> ydev;
    HdmPinned<double> yhost;   // pinned staging of the owned multipliers (the upload is asynchronous)
    HdmPinned<double> chk;     // mapped pinned block of the single-launch small-block check: y[mloc], then info, log det
    HdmBuf<double> corr;       // sharded corrector build: this cone's 2m dot products before they join the operator's
    hdsdp_linsys_fp *dualFactor = nullptr;
    std::unique_ptr<HdmChol> primal;   // KKT_TYPE_PRIMAL: factor object of the registered primal matrix (lazy)
    // KKT_TYPE_PRIMAL with an indefinite X, route 1 (engine_build.h: build_primal): X = W^T diag(sigma) W from the signed factor
    HdmBuf<double> psig;              // sigma on the device (npad, +1 in the padding)
    const double *gram_sig = nullptr; // not owned (psig): set for the duration of a route-1 build: the Gram product takes the signed weights
    HdmBuf<int> pcols;                // packed columns of the correction's sign (this rank's K range)
    HdmBuf<double> pgat;              // the gathered operand (one chunk)
    HdmBuf<double> pchk;              // acceptance check: 3 * MI_PSIG_BLOCKS partial sums + 3 totals; then the shards' agreement words
    int primal_route = -1, primal_q = 0;          // HMiConeGetPrimalRoute: the last KKT_TYPE_PRIMAL build
    double primal_growth = 0.0, primal_resid = 0.0;
    double primal_ms[4] = {0, 0, 0, 0};           // route 1: signed factor + check, gather, correction GEMMs, combine (ms)
    long primal_cols = 0;                         // route 1: columns of the correction on this rank (0: none needed)
    std::unique_ptr<HdmLanczos> lanczos;   // ratio test state (lazy); dS lives in `dS`
    // the ratio test's safeguard (cone_ratio_test): a factor object and a buffer for S + step dS, and a Lanczos object that
    // always starts fresh (lazy, only made when a step has failed the check)
    std::unique_ptr<HdmChol> safe;
    HdmBuf<double> Ssafe;
    std::unique_ptr<HdmLanczos> lanczos_fresh;
    double nrm[4] = {0, 0, 0, 0}; bool norms_ready = false;   // data norms (rows abs / Frobenius, objective abs / Frobenius)
    double objScal = 1.0;           // product of the coneScal factors applied to C
    std::unique_ptr<HdmChol> checker;   // second factor object (primal recovery works on S without the residual term)
    HdmBuf<double> dS;
    HdmBuf<double> Xup;             // uploaded primal matrix of the cone utilities
    HdmBuf<double> Pr1, Pr2;        // primal recovery scratch (npad x npad each; Xinv / Yinv are sized per builder path)
    double Rd = 0.0, perturb = 0.0;
    std::vector<double> trA;   // host: tr(A_i) of all m constraints (b of the synthetic family)
    // work space
    int Bc = 8;                // constraints per congruence batch
    HdmBuf<double> T;          // Bc x n16 x n16
    HdmBuf<double> ahat_loc_own, ahat_all_own;   // what AhatLoc / AhatAll point at, unless the caller supplied them (HMiConeSetExchangeBuffers: torch-owned, for RCCL; these two then stay empty)
    double *AhatLoc = nullptr; // [world*npb_loc][Lr][16] congruence output of the owned rows
    double *AhatAll = nullptr; // [world][npb_loc][Lr][16] after the transpose (== AhatLoc when world == 1: not owned)
    HdmBuf<double> slabs_own;  // the Gram slabs where they have a buffer of their own (!shared_ts)
    double *slabs = nullptr;   // nslab x R x R; not owned: slabs_own or, with shared_ts, T
    HdmBuf<double> Gm;         // R x R augmented Gram (lower valid)
    int nsplit = 1;            // K splits of the Gram product
    int nslab = 1;             // slabs they are summed into; more splits than slabs run in groups that accumulate (engine_build.h: gram_range)
    int slabs_used = 0;        // slabs the current build's groups have written
    bool gram_queue_global = false;   // the Gram launch's workgroups draw (split, tile) jobs from ONE queue in split order
    long R = 0;                // world * Lr
    // R1 work
    HdmBuf<double> U, V, Gr1, Ct, W, Xinv, Yinv;
    // exchange hooks (world > 1)
    hmi_alltoall_fn alltoall = nullptr;
    hmi_alltoall_piece_fn a2a_start = nullptr;   // piecewise exchange overlapped with the Gram product (optional)
    hmi_alltoall_wait_fn a2a_wait = nullptr;
    int a2a_pieces = 1;
    hipEvent_t piece_ev[64] = {};                // staged exchange: congruence step 2 finished the p-blocks of piece k
    int last_pieces = 1, last_staged = 0;        // HMiConeGetExchangeStats
    // Where the last sharded Schur build of this shard spent its time (HMiConeGetBuildProfile; bench.py prints min / max over
    // the ranks): device times between HIP events on the engine stream, host times around the two blocking hooks.
    struct BuildProfile {
        static constexpr int MAXP = 64;
        bool valid = false;
        int pieces = 1, staged = 0;
        double invert = 0, step1 = 0, cong = 0, reduce = 0, allreduce_host = 0, extract = 0;
        double step2[MAXP] = {};       // step 2 of the tile columns piece k needs (staged builds)
        double wait_gpu[MAXP] = {};    // engine stream idle before piece k's Gram splits: the piece had not arrived
        double wait_host[MAXP] = {};   // host time inside the wait hook for piece k
        double gram[MAXP] = {};        // Gram splits of piece k
        double bytes[MAXP] = {};       // bytes this shard sent for piece k
        double flight[MAXP] = {};      // host time from handing piece k to the transport until its wait returned
    } prof;
    hipEvent_t pe_s1 = nullptr, pe_s2[BuildProfile::MAXP] = {}, pe_ga[BuildProfile::MAXP] = {}, pe_gb[BuildProfile::MAXP] = {};
    double pt_start[BuildProfile::MAXP] = {};    // host clock (s) at a2a_start of piece k
    hmi_allreduce_fn allreduce = nullptr;
    void *xctx = nullptr;
    bool work_ready = false;
    bool shared_ts = false;    // T and the Gram slabs are one buffer (one GPU): T's diagonal-tile uppers are re-zeroed per batch
    // single-process multi-device mode: the shards of one block share ONE Schur operator (the caller's); only shard 0
    // writes into it, the others stop after the all-reduce
    bool kkt_owner = true;
    int kkt_counted = 0;       // progress of the aggregated-pattern queries (cone_add_sym_nz)
    // Where the dual matrix, the step matrix and the dual factor stand (dual_state.h): the points S and dS were assembled at,
    // from which cone_assemble answers a request on the line through them without a sweep.  Every writer of S, dS or the
    // dual factor object names what it did through one of this object's transitions.
    HdmDualState dual;
    // the check set (engine_check_set.h), the ratio set (engine_ratio_set.h) and the step set (engine_step_set.h) this cone is a
    // member of, and its place there: cone_set.h's links, assigned and cleared by its rules alone
    HdmConeLink<MiCone> in_check, in_ratio, in_step;
    // fused single-launch Phase-A pass of a small rank-one block (small.hip): factors as a CSR, built on first use
    struct SmallPlan {
        int state = 0;         // 0 = not looked at, 1 = ready, -1 = not eligible
        HdmBuf<int> fp, fi, dense_of, dense_rows;
        HdmBuf<double> fv, sgn;
        int ndense = 0;
        HdmPinned<double> io;  // mapped pinned block: y[m], b[m] in; 4 + 5 m doubles out
    } small;
};

// The grouped Schur build of an operator (grouped_plan.h: rule and plan; engine_grouped.h performs it).
// Decided at HKKTInit: which cones are eligible (`desc`, `n_eligible`).  The job and contributor lists (`plan`: empty unless at
// least two cones are eligible), their device copies and the staging buffers are made when the switch is first turned on, so an
// operator that never uses the pass pays for none of them.
struct MiGrouped {
    bool on = false;                 // HMiKKTSetGroupedBuild / HDSDP_MI355X_GROUPED_BUILD
    std::vector<HdmGroupedCone> desc;   // the operator's cones as the rule sees them (rows: the cones' own vectors, not owned)
    int n_eligible = 0;
    bool planned = false;
    HdmGroupedPlan plan;
    bool dev_ready = false;
    int max_n16 = 0;
    HdmPinned<HdmGroupedConeDev> cones_host;   // refreshed per build (Rd moves), uploaded from here
    HdmBuf<HdmGroupedConeDev> cones_dev;
    HdmBuf<HdmGroupedJob> jobs;
    HdmBuf<int> m_row, m_col, m_slot, m_idx, v_row, v_slot, v_idx;
    HdmBuf<long> m_ptr, v_ptr;
    HdmBuf<double> X, G, V;          // staging: S^-1 per cone, packed local Gram matrices, local vectors + scalars
    int last_cones = 0, last_jobs = 0, last_launches = 0;   // the last build (HMiKKTGetGroupedBuild)
    bool used() const { return on && plan.used(); }
};

// The three question sets of an operator: a question put to one small SDP cone is answered for ALL members in one launch, the
// first time one of them is asked something its stored answer does not serve.  Members, lifetimes and counters are cone_set.h's,
// and so is what a set does with its members (HdmQuestionSet: populate at HKKTInit, the switch, the launch, the answer); each
// struct here is a kind's own state and declares the hooks (cone_set.h lists them) its engine_*_set.h defines.  The switch makes
// everything a launch needs, so that a launch allocates nothing.  DESIGN.md section 25.
// a hook's "could not be made": the HIP error that says so is cleared
const char *set_lacks(const char *what) { (void) hipGetLastError(); return what; }

// The check set (engine_check_set.h): "interior at (tau, y)?" and "log det S at (tau, y)" on the dual buffer,
// by one launch of hdm_grouped_check_kernel.  Members: small_check_rule.h (the cones whose own one-launch check would run).  The
// stored answer is the dual state itself; left out of a launch: who already stood at the point.
// HMiKKTSetGroupedCheck / HDSDP_MI355X_GROUPED_CHECK.
struct MiCheckQ { double tau; const double *y; };
struct MiCheckSet : HdmQuestionSet<MiCone, MiCheckSet> {
    static constexpr const char *NO_MEMORY = "[hdsdp_mi355x] grouped interior check: no pinned memory for %s; the per-cone checks stay\n";
    HdmPinned<HdmSmallCheckArgs> table;    // mapped pinned, one entry per member: the launch's arguments, launched members first
    MiCheckSet() : HdmQuestionSet<MiCone, MiCheckSet>(&MiCone::in_check) {}
    void free_launch() { table.reset(); }
    bool eligible(const MiCone *c) const;
    void empty();
    const char *prepare(size_t k, MiCone *c), *alloc_tables();
    HdmSetSort sort(size_t k, MiCone *c, const MiCheckQ &q);
    bool serves(size_t k, MiCone *c, const MiCheckQ &q);
    void fill(int place, size_t k, MiCone *c, const MiCheckQ &q), commit(int place, size_t k, MiCone *c, const MiCheckQ &q);
    int fire(int nl, const MiCheckQ &q);
};
// The ratio set (engine_ratio_set.h): "how far along (dTauStep, dy)?" on the dual buffer, by one pair of
// launches.  Members: small_ratio_rule.h.  HMiKKTSetGroupedRatio / HDSDP_MI355X_GROUPED_RATIO.
// Two opt-ins of its own, each only while the set is on, both off again whenever the set is switched, released or populated
// (DESIGN.md section 26): the set also answers BUFFER_DUALCHECK (HMiKKTSetGroupedRatioChecker / HDSDP_MI355X_GRATIO_CHECKER),
// and the rest of the safeguard -- fresh-start test and cuts -- runs in the launch (HMiKKTSetGroupedRatioRest / ..._GRATIO_REST).
struct MiRatioQ { double dTauStep; const double *dy; double dAdaRatio; int whichBuffer; };
struct MiRatioSet : HdmQuestionSet<MiCone, MiRatioSet> {
    static constexpr const char *NO_MEMORY = "[hdsdp_mi355x] grouped ratio test: no memory for %s; the per-cone tests stay\n";
    std::vector<HdmRatioSlot> slots;       // one per member: the answer of the last launch it was in (small_ratio_rule.h)
    std::vector<long> yoff;                // one per member: where its multipliers start in `ybuf`; ytot: where the next would
    long ytot = 0;
    HdmPinned<HdmGroupedRatioArgs> table;  // mapped pinned, one entry per member: the launch's arguments, launched members first
    HdmPinned<double> ybuf;                // mapped pinned: the members' gathered multipliers
    // safeguard fallbacks since HKKTInit (members whose step left the cone and took the host's fresh-start test and cuts)
    long fallbacks = 0;
    bool checker_on = false, rest_on = false;      // the two opt-ins
    HdmPinned<HdmGroupedRestArgs> rest_table;      // rest_on: mapped pinned, indexed like `table`
    HdmPinned<double> rest_words;                  // rest_on: mapped pinned, HDM_GROUPED_REST_WORDS per member, by slot
    // since HKKTInit: launches that asked the checker, members given the rest on the device, cuts made there
    long checker_launches = 0, device_rests = 0, device_cuts = 0;
    MiRatioSet() : HdmQuestionSet<MiCone, MiRatioSet>(&MiCone::in_ratio) {}
    void free_launch() { table.reset(); ybuf.reset(); rest_table.reset(); rest_words.reset(); checker_on = rest_on = false; }
    void reset_counters() { HdmConeSet<MiCone>::reset_counters(); fallbacks = checker_launches = device_rests = device_cuts = 0; }
    int turn_checker(int on_), turn_rest(int on_);   // the opt-ins' switches: 1 if on afterwards
    bool eligible(const MiCone *c) const;
    void empty();
    const char *prepare(size_t k, MiCone *c), *alloc_tables();
    HdmSetSort sort(size_t k, MiCone *c, const MiRatioQ &q);
    bool serves(size_t k, MiCone *c, const MiRatioQ &q);
    void fill(int place, size_t k, MiCone *c, const MiRatioQ &q), commit(int place, size_t k, MiCone *c, const MiRatioQ &q);
    int fire(int nl, const MiRatioQ &q);
};
// The step set (engine_step_set.h): "is S + dStep dS still inside?" on the checker buffer, by one launch of
// hdm_grouped_step_check_kernel.  Members: small_step_rule.h.  HMiKKTSetGroupedStep / HDSDP_MI355X_GROUPED_STEP.
struct MiStepSet : HdmQuestionSet<MiCone, MiStepSet> {
    static constexpr const char *NO_MEMORY = "[hdsdp_mi355x] grouped step-and-check: no memory for %s; the per-cone checks stay\n";
    std::vector<HdmStepSlot> slots;        // one per member: the answer of the last launch it was in (small_step_rule.h)
    // one per member: the switch made its step buffer (zeros: no step matrix yet), when its dS counter stood at ds_at_on
    std::vector<char> made_dS;
    std::vector<unsigned long> ds_at_on;
    HdmPinned<HdmGroupedStepArgs> table;   // mapped pinned, one entry per member: the launch's arguments, launched members first
    HdmPinned<int> words;                  // mapped pinned, one word per member: the sweep's info, -1 until the launch has reported
    MiStepSet() : HdmQuestionSet<MiCone, MiStepSet>(&MiCone::in_step) {}
    void free_launch() { table.reset(); words.reset(); }
    bool eligible(const MiCone *c) const;
    void empty();
    const char *prepare(size_t k, MiCone *c), *alloc_tables();
    HdmSetSort sort(size_t k, MiCone *c, const double &q);
    bool serves(size_t k, MiCone *c, const double &q);
    void fill(int place, size_t k, MiCone *c, const double &q), commit(int place, size_t k, MiCone *c, const double &q);
    int fire(int nl, const double &q);
};
// the set a cone is a member of through `link`, as its own kind (a link is assigned by sets of its kind's type only)
template <class Set> Set *set_of(const HdmConeLink<MiCone> &link) { return static_cast<Set *>(link.set); }

struct MiKKTPriv {
    MiGrouped grp;
    MiCheckSet chk;
    MiRatioSet rat;
    MiStepSet stp;
    // how M is stored, what state it is in and where the last factorised matrix came from (kkt_store.h); the operator's linear
    // system (MiLin::st) points here
    HdmKktState st;
    HdmBuf<double> vecs;      // device: ASinv[m], ASinvRdSinv[m], ASinvCSinv[m], scal[4]
    HdmBuf<double> rhs;
    // cones of HKKT->cones[] whose coneBuildSchur is this engine's (they accumulate on the device) and the others (the
    // reference's CPU cones: they accumulate into the host fields, hdsdp_conic_*.c)
    int n_engine = 0, n_foreign = 0;
    HdmPinned<double> Mtmp;   // pinned m x m staging buffer for the mixed case (device part added to the host part)
    // sparse Schur operator (isKKTSparse, hdsdp_schur.c:46-139): the host matrix is the aggregated CSC pattern; its
    // entries as (row, column) pairs on the device, plus a staging vector of nnz values
    long nnz = 0;
    HdmBuf<int> sp_rows, sp_cols;
    HdmBuf<int> sp_prow, sp_pcol;   // the same entries in the factor object's (permuted, lower) coordinates, if it is permuted
    HdmBuf<double> sp_vals;
    // diagonal channel (host mirror off, engine_kkt.h): kktDiag[i] -> chan[i], pinned; host cones add their diagonal terms
    // there, and the first HKKTRegularize / HKKTFactorize after a build adds it (8 m bytes up) to the device matrix's diagonal
    HdmPinned<double> chan;
    HdmBuf<double> chan_dev;      // device: m doubles + 1 (the minimum the regulariser reads)
    int64_t bytes_d2h = 0, bytes_h2d = 0;   // M and the channel moved since HKKTInit (HMiKKTGetMatrixTraffic)
};

// the kkt private state hangs off kktM->chol's MiLin (Mdev) plus a side struct keyed by the kkt pointer
std::vector<std::pair<hdsdp_kkt *, MiKKTPriv *>> g_priv;
MiKKTPriv *priv_of(hdsdp_kkt *k) {
    for (auto &p : g_priv)
        if (p.first == k) return p.second;
    MiKKTPriv *n = new MiKKTPriv();
    g_priv.push_back({k, n});
    return n;
}
void priv_drop(hdsdp_kkt *k) {
    for (size_t i = 0; i < g_priv.size(); ++i)
        if (g_priv[i].first == k) {
            delete g_priv[i].second;
            g_priv.erase(g_priv.begin() + i);
            return;
        }
}

// single-process multi-device mode (group_impl.h): a group cone's slots fan out to one MiCone per device
hdsdp_retcode gc_build_schur(void *cd, int iCone, void *kktv, int typeKKT);
MiCone *cone_data(hdsdp_cone *cone);   // the block's device data; for a group cone that of shard 0
int group_configure_from_env();
bool group_wants_block(const MiBlockData &blk);
bool group_wants_synthetic(int nRow, int nCol);
hdsdp_retcode group_create_cone(hdsdp_cone **pCone, int iCone, int nRow, int nCol, MiBlockData *blk, bool synthetic);

// the factor object of the cone's dual matrix
HdmChol *dual_chol(const MiCone *c) { return &((MiLin *) c->dualFactor->chol)->ch; }
// the point (tau, eye, y): the owned multipliers gathered through own[] into a buffer of the caller's (mloc doubles; no y_host:
// zeros), which the point then names; *any: one of them is non-zero
HdmDualPoint cone_point(const MiCone *c, double tau, double eye, const double *y_host, double *yo, bool *any = nullptr) {
    bool a = false;
    for (int q = 0; q < c->mloc; ++q) { yo[q] = y_host ? y_host[c->own[q]] : 0.0; a |= (yo[q] != 0.0); }
    if (any) *any = a;
    return HdmDualPoint{tau, eye, yo, c->mloc};
}

// The cone's lazy state, each piece made if absent where a path first needs it (the ratio set's switch makes a member's step matrix
// and Lanczos object, so that a launch allocates nothing): a factor or Lanczos object of the block's dimension, which is not kept
// if its buffers could not be made; and the step matrix, zeros, so that the padding reads as 0.
template <class T> hdsdp_retcode cone_make(std::unique_ptr<T> &p, int n) {
    if (!p) { p.reset(new T()); if (p->init(n)) { p.reset(); return HDSDP_RETCODE_MEMORY; } }
    return HDSDP_RETCODE_OK;
}
hipError_t cone_make_dS(MiCone *c) {
    if (c->dS.get()) return hipSuccess;
    const size_t n2 = (size_t) c->n16 * c->n16;
    if (const hipError_t e = c->dS.alloc(n2); e != hipSuccess) return e;
    return hdm_memset_sync(c->dS.get(), 0, sizeof(double) * n2);
}

HdmLayout cone_layout(const MiCone *c) { return {c->world, c->n16, c->nblk, c->npb, c->npb_loc, c->Lr, c->R, c->astride}; }
// the block and the device as row_store_rule.h sees them
HdmRowFacts cone_row_facts(const MiCone *c) { return hdm_row_facts(cone_layout(c), c->n, c->m, c->mloc, c->synthetic, c->path == PATH_GEMM); }
MiRowShape cone_row_shape(const MiCone *c) { return {c->n, c->n16, c->mloc, c->world, c->astride, &c->own}; }
HdmDeviceFacts device_facts() {
    HdmDeviceFacts d;
    d.known = hipMemGetInfo(&d.free_bytes, &d.total_bytes) == hipSuccess;
    (void) hipGetLastError();
    return d;
}

int cone_alloc_common(MiCone *c) {
    c->own.clear();
    // One GPU: constraints that are zero on this block (most of them in a many-block problem; the reference's
    // "sparse SDP cone", hdsdp_conic_sdp.c:1814-1886, loops over the non-zero ones only) are left out of the device
    // data altogether: no congruence, no Gram rows, nothing written to their rows of M.  Sharded blocks keep the plain
    // cyclic deal (row i on rank i % world) that the exchange layout is built on.
    const bool compact = (c->world == 1 && !c->synthetic && (int) c->blk.rows.size() == c->m);
    for (int i = c->rank; i < c->m; i += c->world)
        if (!compact || c->blk.rows[i].type != MI_COEFF_ZERO) c->own.push_back(i);
    c->mloc = (int) c->own.size();
    c->own_asc = c->own;
    const HdmLayout L = hdm_layout(c->n, c->world, compact ? c->mloc : (c->m + c->world - 1) / c->world);   // work_plan.h
    c->n16 = L.n16; c->nblk = L.nblk; c->npb = L.npb; c->npb_loc = L.npb_loc; c->Lr = L.Lr; c->R = L.R; c->astride = L.astride;
    const size_t n2 = (size_t) c->n16 * c->n16, nn = sizeof(double) * n2;
    HDM_HIP_CHECK(c->S.alloc(n2));
    HDM_HIP_CHECK(c->Scheck.alloc(n2));
    HDM_HIP_CHECK(c->Cfull.alloc(n2));
    HDM_HIP_CHECK(hdm_memset_sync(c->Cfull.get(), 0, nn));
    HDM_HIP_CHECK(c->ydev.alloc((size_t) std::max(1, c->m)));
    std::vector<int> rs((size_t) c->R, -1);
    for (int gq = 0; gq < c->world; ++gq) {
        int cnt = 0;
        if (compact) { for (int i : c->own) rs[cnt++] = i; }
        else for (int i = gq; i < c->m; i += c->world) rs[(size_t) gq * c->Lr + cnt++] = i;
        if (gq == 0) { rs[cnt] = -2; rs[cnt + 1] = -3; rs[cnt + 2] = -4; }  // I, S, C rows
    }
    HDM_HIP_CHECK(c->rows_seg.alloc((size_t) c->R));
    HDM_HIP_CHECK(hdm_memcpy_h2d_sync(c->rows_seg.get(), rs.data(), sizeof(int) * (size_t) c->R));
    HDM_HIP_CHECK(c->rows_own.alloc((size_t) std::max(1, c->mloc)));
    HDM_HIP_CHECK(hdm_memcpy_h2d_sync(c->rows_own.get(), c->own.data(), sizeof(int) * (size_t) c->mloc));
    if (HFpLinsysCreate(&c->dualFactor, c->n, HDSDP_LINSYS_DENSE_DIRECT) != HDSDP_RETCODE_OK) return 1;
    return 0;
}

// The work space of the congruence + Gram path: the plan is work_plan.h's (hdm_work_plan: batch size, K splits, slabs, which
// buffers are shared -- and why), what stays here is what depends on the device: every allocation degrades quietly when memory
// is short, through the plan's own helpers, so that what the cone holds is always a plan the rule could have made.
int cone_alloc_gemm_work(MiCone *c) {
    const HdmLayout L = cone_layout(c);
    const size_t n2 = (size_t) c->n16 * c->n16, tpad = hdm_operand_pad(c->n16);
    if (hdm_sweep_copy_yields(c->rows.form(), c->rows.sweep_copy_in_use(), cone_row_facts(c), device_facts())) c->rows.yield_sweep_copy();
    const HdmKnobs knobs = hdm_knobs_from_env();
    HdmWorkPlan p = hdm_work_plan(L, c->mloc, c->rows.streamed(), c->rows.batch(), knobs);
    // the intermediates: if the allocation fails the batch is halved (and the slab count planned again for that batch)
    while (c->T.alloc(n2 * (size_t) p.Bc, tpad) != hipSuccess) {
        (void) hipGetLastError();
        if (p.Bc <= 8) { fprintf(stderr, "[hdsdp_mi355x] out of device memory for the congruence intermediates\n"); return 1; }
        p = hdm_work_plan(L, c->mloc, c->rows.streamed(), c->rows.batch(), knobs, p.Bc / 2);
    }
    c->Bc = (int) p.Bc;
    HDM_HIP_CHECK(hdm_memset_sync(c->T.get(), 0, p.t_bytes));  // step 1 writes lower tiles only; the rest must read as 0
    if (!c->AhatLoc) {
        const size_t ahat = hdm_exchange_doubles(L);
        HDM_HIP_CHECK(c->ahat_loc_own.alloc(ahat + HDM_OPERAND_PAD_DOUBLES));
        c->AhatLoc = c->ahat_loc_own.get();
        HDM_HIP_CHECK(hdm_memset_sync(c->AhatLoc, 0, sizeof(double) * ahat));
        if (c->world == 1) c->AhatAll = c->AhatLoc;
        else {
            HDM_HIP_CHECK(c->ahat_all_own.alloc(ahat + HDM_OPERAND_PAD_DOUBLES));
            c->AhatAll = c->ahat_all_own.get();
            HDM_HIP_CHECK(hdm_memset_sync(c->AhatAll, 0, sizeof(double) * ahat));
        }
    }
    // the slabs: in T where the two share a buffer (grown to the slabs' size if that is the larger), else in a buffer of their
    // own; halved until they fit
    if (p.shared_ts) {
        while (p.slab_bytes > p.t_bytes + tpad && c->T.alloc(p.slab_bytes / sizeof(double), tpad) != hipSuccess) {
            (void) hipGetLastError();
            if (c->T.alloc(n2 * (size_t) p.Bc, tpad) != hipSuccess) { (void) hipGetLastError(); return 1; }
            if (!hdm_plan_halve_slabs(p, L)) { fprintf(stderr, "[hdsdp_mi355x] out of device memory for the Gram slabs\n"); return 1; }
        }
        c->slabs = c->T.get();
    } else {
        while (c->slabs_own.alloc(p.slab_bytes / sizeof(double)) != hipSuccess) {
            (void) hipGetLastError();
            if (!hdm_plan_halve_slabs(p, L)) { fprintf(stderr, "[hdsdp_mi355x] out of device memory for the Gram slabs\n"); return 1; }
        }
        c->slabs = c->slabs_own.get();
    }
    c->shared_ts = p.shared_ts;
    c->nslab = (int) p.nslab;
    c->nsplit = (int) p.nsplit;
    c->gram_queue_global = p.gram_queue_global;
    HDM_HIP_CHECK(c->Gm.alloc((size_t) c->R * c->R));
    // the "S row" (At = I) never changes
    if (c->rank == 0) {
        if (hdm_blocked_eye(c->AhatLoc, c->Lr, c->mloc + 1, c->nblk, c->n, g.stream)) return 1;
    }
    return 0;
}

// --- vtable slots ---------------------------------------------------------------------------
void cone_setstart(void *cd, double rResi) { ((MiCone *) cd)->Rd = rResi; }  // hdsdp_conic_sdp.c:1546-1550
int cone_getdim(void *cd) { return ((MiCone *) cd)->n; }
// rows of M this block contributes to: all m for a dense block (:1404-1405), the k rows on which the block has data for
// a block most constraints are zero on (the reference's sparse SDP cone, :1479-1480) -- what HKKTInit weighs against
// 0.3 m^2 when it chooses between the dense Schur matrix and the aggregated-pattern CSC
int cone_kkt_rows(const MiCone *c) {
    const bool compact = (c->world == 1 && !c->synthetic && (int) c->blk.rows.size() == c->m);
    // the reference makes a block a sparse SDP cone iff at most 0.3 m of the constraints have data on it
    // (HUserDataChooseCone, hdsdp_user_data.c:82-86; HDSDP_SPARSE_CONE_THRESHOLD); its dense cone claims all of M
    return (compact && (double) c->mloc <= 0.3 * (double) c->m) ? c->mloc : c->m;
}
int64_t cone_getsymnnz(void *cd) { MiCone *c = (MiCone *) cd; const int64_t k = cone_kkt_rows(c); return k * k; }
// the two pattern queries of HKKTAllocSparseKKT (hdsdp_schur.c:46-139), with the protocol of the reference's sparse SDP
// cone (sdpSparseConeAddSymNnzImpl / sdpSparseConeGetSymMapping, hdsdp_conic_sdp.c:2086-2170): columns are visited in
// order; in the column of its next row the block marks that row and all its later ones (the rows in ascending order: own_asc --
// a cone with direct rows keeps `own` in another).  The positions handed back in
// the second call are not kept: the engine's builders write a dense device matrix at global (row, column) indices and
// the operator gathers the pattern's entries from it.
void cone_add_sym_nz(void *cd, int iCol, int *schurMatCol) {
    MiCone *c = (MiCone *) cd;
    if (c->kkt_counted >= c->mloc || c->own_asc[c->kkt_counted] != iCol) return;
    for (int e = c->kkt_counted; e < c->mloc; ++e) schurMatCol[c->own_asc[e]] = 1;
}
void cone_get_kkt_map(void *cd, int iCol, int *schurMatCol) {
    (void) schurMatCol;
    MiCone *c = (MiCone *) cd;
    if (c->kkt_counted < c->mloc && c->own_asc[c->kkt_counted] == iCol) c->kkt_counted += 1;
}

// The sweep copy at creation, when the block's rows have arrived: by the rule (row_store_rule.h: hdm_sweep_copy_rule).  A block
// whose rows live in the copy has it already.
int cone_make_sweep_copy(MiCone *c) {
    const HdmEnvInt zs_env = hdm_env_int<ENV_ZS>();
    if (c->rows.form() == HDM_ROWS_EXPANDED) return 0;
    const HdmSweepCopyRule r = hdm_sweep_copy_rule(cone_row_facts(c), c->rows.has_rows(), zs_env);
    return r.build ? c->rows.make_sweep_copy(r.max_fill) : 0;
}

// the identity coefficient of the dual matrix: the residual and the perturbation   hdsdp_conic_sdp.c:383-385
double cone_eye(const MiCone *c) { return -c->Rd + c->perturb; }
double *cone_dual_buffer(MiCone *c, HdmDualTarget which) {
    return which == HDM_DUAL_S ? c->S.get() : which == HDM_DUAL_SCHECK ? c->Scheck.get() : c->dS.get();
}

// target <- T(p) by a sweep over the owned constraint matrices (p.y: the cone's pinned staging buffer, `any` of them non-zero)
// Sharded: every rank sums its own rows (rank 0 also adds tau*C and the identity term), then all-reduce.
int cone_sweep(MiCone *c, const HdmDualPoint &p, bool any, double *target) {
    HDM_HIP_CHECK(hipMemcpyAsync(c->ydev.get(), p.y, sizeof(double) * c->mloc, hipMemcpyHostToDevice, g.stream));
    const double lead = (c->rank == 0) ? 1.0 : 0.0, ctau = lead * p.tau, ceye = lead * p.eye;
    // The sweep reads the zero-suppressed copy of the constraint data where one is in use (cone_make_sweep_copy: made at creation).
    MiRows &rows = c->rows;
    if (any && rows.sweep_copy_in_use()) {
        if (hdm_sym_combine_zs(rows.sweep_copy(), c->ydev.get(), c->Cfull.get(), ctau, ceye, target, c->n, c->n16, c->n16, g.stream)) return 1;
    } else if (!rows.streamed() || !any) {
        if (hdm_sym_combine(rows.resident(), c->astride, any ? c->mloc : 0, c->ydev.get(), c->Cfull.get(), ctau, ceye, target, c->n,
                            c->n16, c->n16, g.stream)) return 1;
    } else {
        // streamed data without a sweep copy: batch after batch, the later ones on top of what the earlier ones left in the
        // target (tau' = 1, no identity term; each element is read and rewritten by the one thread that owns it)
        for (int q0 = 0, B = rows.batch(); q0 < c->mloc; q0 += B) {
            const int nb = std::min(B, c->mloc - q0);
            const double *A = rows.rows(q0, nb);
            if (!A) return 1;
            if (hdm_sym_combine(A, c->astride, nb, c->ydev.get() + q0, q0 == 0 ? c->Cfull.get() : target, q0 == 0 ? ctau : 1.0,
                                q0 == 0 ? ceye : 0.0, target, c->n, c->n16, c->n16, g.stream)) return 1;
        }
    }
    if (c->world > 1) {
        HDM_HIP_CHECK(hipStreamSynchronize(g.stream));
        if (!c->allreduce || c->allreduce(c->xctx, target, (int64_t) c->n16 * c->n16)) return 1;
    }
    return 0;
}

// S (or the checker buffer, or dS) <- tau*C - sum y_i A_i - Rd*I (+ perturb)   hdsdp_conic_sdp.c:343-402, :1616-1633
// The entry of every dual-matrix request.  What the buffers already hold decides how it is answered -- nothing, a copy,
// S + alpha dS (+ delta I), or the sweep: the rule is hdm_dual_plan's (dual_state.h), this performs it and commits it.
int cone_assemble(MiCone *c, double tau, const double *y_host, HdmDualTarget which, const double *eye_override = nullptr) {
    // the upload of a sweep is asynchronous: the source is a pinned buffer of the cone, and the previous upload from it has
    // been consumed by the time it is rewritten (every caller synchronises on the factorisation that follows)
    if (!c->yhost) HDM_HIP_CHECK(c->yhost.alloc((size_t) std::max(1, c->mloc)));
    HDM_HIP_CHECK(hipStreamSynchronize(g.stream));
    bool any = false;
    const HdmDualPoint p = cone_point(c, tau, eye_override ? *eye_override : cone_eye(c), y_host, c->yhost.get(), &any);
    const HdmDualPlan plan = hdm_dual_plan(c->dual, p, which, hdm_dual_mode(c->mloc, c->n), c->world);
    g_asm_counts[plan.counter].fetch_add(1, std::memory_order_relaxed);
    if (plan.line_missed && hdm_dual_debug()) hdm_dual_print_miss(stderr, c->dual, p, which, plan);
    double *target = cone_dual_buffer(c, which);
    const long cnt = (long) c->n16 * c->n16;
    switch (plan.action) {
    case HDM_DUAL_NONE: break;
    case HDM_DUAL_COPY_FROM_S:
        HDM_HIP_CHECK(hipMemcpyAsync(target, c->S.get(), sizeof(double) * (size_t) cnt, hipMemcpyDeviceToDevice, g.stream));
        break;
    case HDM_DUAL_AXPY: if (hdm_axpy_mat(target, c->S.get(), c->dS.get(), plan.alpha, cnt, g.stream)) return 1; break;
    case HDM_DUAL_AXPY_EYE: if (hdm_axpy_mat_eye(target, c->S.get(), c->dS.get(), plan.alpha, plan.delta, c->n16, c->n, g.stream)) return 1; break;
    case HDM_DUAL_SWEEP: if (cone_sweep(c, p, any, target)) return 1; break;
    }
    c->dual.commit(plan, p, which);
    return 0;
}

// <A_i, X> (and <A_i, Y>) over the owned constraints: from the zero-suppressed copy when the cone has one, else from the dense storage
int cone_sym_dot2(MiCone *c, const double *X, const double *Y, long ldx, double *outx, double *outy, double sx, double sy) {
    if (c->rows.sweep_copy_in_use())
        return hdm_sym_dot2_zs(c->rows.sweep_copy(), c->n16, c->n16, X, Y, ldx, outx, outy, c->rows_own.get(), sx, sy, g.stream);
    for (int q0 = 0, B = c->rows.batch(); q0 < c->mloc; q0 += B) {     // (one batch = everything when the data is resident)
        const int nb = std::min(B, c->mloc - q0);
        const double *A = c->rows.rows(q0, nb);
        if (!A || hdm_sym_dot2(A, c->astride, c->n16, c->n16, nb, X, Y, ldx, outx, outy, c->rows_own.get() + q0, sx, sy, g.stream)) return 1;
    }
    return 0;
}

hdsdp_retcode cone_factor_S(MiCone *c, int *isPsd);
hdsdp_retcode cone_factor_check(MiCone *c, int *isPsd);
hdsdp_retcode cone_checker(MiCone *c, HdmChol **out);

// Interior check of a SMALL block (n <= 128, at most 1 MB of resident constraint data) in ONE launch and one synchronisation:
// assembly, Cholesky with the triangular inverse, pivot information and log det S (small.hip: hdm_small_check_kernel).  The
// same point asked for again -- the reference's line search asks "interior?" and then for the barrier at the point it has just
// checked -- is answered from what the factor object holds, with no device work at all.
// Returns 0 when it has answered (*isPsd set), 1 when the block is not eligible (the caller takes the call-by-call route).
// The pieces are shared with the grouped form (engine_check_set.h), which puts every member of an operator's check set at the
// asked point in one launch: the rule, the point (gathered into the cone's own mapped block), the launch's arguments, and
// what a report word means for the factor object and the dual state.
bool small_check_switch() { return hdm_env_on<ENV_SMALL_CHECK>(); }
// the cone as small_check_rule.h sees it; `ch`: the factor object the launch would write (nullptr: the block's own part only)
HdmSmallCheckCone small_check_desc(const MiCone *c, const HdmChol *ch) {
    HdmSmallCheckCone d;
    d.on = small_check_switch(); d.world = c->world; d.resident = c->rows.resident() != nullptr; d.n16 = c->n16; d.mloc = c->mloc;
    if (ch) { d.fac_npad = ch->npad; d.fac_nblk = ch->nblk; }
    return d;
}
// the cone's mapped block (y[mloc], then info and log det), made on first use
int small_check_block(MiCone *c) {
    if (c->chk) return 0;
    if (c->chk.alloc((size_t) (c->mloc + 4), hipHostMallocMapped) != hipSuccess) { (void) hipGetLastError(); return 1; }
    return 0;
}
// the point (tau, eye, y gathered through own[] into the cone's block)
HdmDualPoint small_check_point(MiCone *c, double tau, const double *y_host, double eye) { return cone_point(c, tau, eye, y_host, c->chk.get()); }
// the launch's arguments for the point in the cone's block; the report word is set to -1 ("nothing reported")
HdmSmallCheckArgs small_check_args(MiCone *c, HdmChol *ch, const HdmDualPoint &p, int whichBuffer) {
    HdmSmallCheckArgs a = {};
    a.n = c->n; a.n16 = c->n16; a.m = c->mloc; a.A = c->rows.resident(); a.astride = c->astride; a.C = c->Cfull.get();
    a.y = c->chk.dev(); a.tau = p.tau; a.eye = p.eye;
    a.Sout = (whichBuffer == 0) ? c->S.get() : c->Scheck.get();
    a.L = ch->L.get(); a.W = ch->Dinv.get(); a.out = c->chk.dev() + c->mloc;
    c->chk.get()[c->mloc] = -1.0;
    return a;
}
// after the synchronisation: the report word into the factor object and the dual state.  Returns info, or -1 when the
// launch has not reported for this cone (nothing is committed then: a dual buffer stays S_overwritten).
int small_check_commit(MiCone *c, HdmChol *ch, const HdmDualPoint &p, int whichBuffer) {
    const double *yo = c->chk.get();
    const int info = (int) yo[c->mloc];
    if (info < 0) return -1;
    ch->factored = (info == 0); ch->have_inv = false;
    ch->logdet_ok = (info == 0); ch->logdet_val = yo[c->mloc + 1];
    if (whichBuffer == 0) {
        c->dualFactor->nFactorizes += 1;
        c->dual.S_assembled_at(p);
        c->dual.S_factored(info == 0);
    }
    return info;
}
int cone_small_check(MiCone *c, double tau, const double *y_host, const double *eye_override, int whichBuffer, int *isPsd, hdsdp_retcode *rc) {
    *rc = HDSDP_RETCODE_OK;
    if (!hdm_small_check_block_ok(small_check_desc(c, nullptr))) return 1;
    HdmChol *ch = dual_chol(c);
    if (whichBuffer != 0) { if (cone_checker(c, &ch) != HDSDP_RETCODE_OK) return 1; }
    if (!hdm_small_check_factor_ok(ch->npad, ch->nblk)) return 1;
    if (small_check_block(c)) return 1;
    const bool grouped = whichBuffer == 0 && !eye_override && c->in_check.active();
    HdmDualPoint p = small_check_point(c, tau, y_host, eye_override ? *eye_override : cone_eye(c));
    // (the grouped case is HdmQuestionSet::answer written out: the first test below also serves a cone outside any set, sets *isPsd,
    // and must keep its place before the launch's arguments are made)
    if (whichBuffer == 0 && c->dual.S_factored_at(p, isPsd)) {               // S = T(p) and its factor are in place
        if (grouped) set_of<MiCheckSet>(c->in_check)->from_store += 1;
        return 0;
    }
    if (grouped) {
        // every member of the set is put at this point in one launch; this cone then answers from its state.  A member the
        // launch has not reported for stays S_overwritten, and the call for that member fails.
        if (set_of<MiCheckSet>(c->in_check)->launch(MiCheckQ{tau, y_host}) || !c->dual.S_factored_at(p, isPsd)) *rc = HDSDP_RETCODE_FAILED;
        return 0;
    }
    const HdmSmallCheckArgs a = small_check_args(c, ch, p, whichBuffer);
    if (whichBuffer == 0) c->dual.S_overwritten();   // the launch writes S: what it holds is known again when the launch has reported
    else c->dual.checker_written();                  // ... or the checker buffer and the checker factor object
    if (hdm_small_check(a, g.stream) || hipStreamSynchronize(g.stream) != hipSuccess) { *rc = HDSDP_RETCODE_FAILED; return 0; }
    const int info = small_check_commit(c, ch, p, whichBuffer);
    if (info < 0) { *rc = HDSDP_RETCODE_FAILED; return 0; }
    if (isPsd) *isPsd = (info == 0);
    return 0;
}

void cone_update(void *cd, double tau, double *y) {
    StatScope stat_(ST_ASSEMBLE_FACTOR, __func__);
    ((MiCone *) cd)->dual.factor_stale();     // S moves, its factor does not follow
    cone_assemble((MiCone *) cd, tau, y, HDM_DUAL_S);
}

hdsdp_retcode cone_factor_S(MiCone *c, int *isPsd) {
    HdmChol *ch = dual_chol(c);
    c->dual.factor_stale();
    RC(ch->load_device(c->S.get(), c->n16, g.stream));
    int info = 0;
    RC(ch->factor(g.stream, &info));
    c->dualFactor->nFactorizes += 1;
    if (isPsd) *isPsd = (info == 0);
    return HDSDP_RETCODE_OK;
}

// the second factor object ("dualChecker" of the reference, def_hdsdp_conic.h): trial points of the line search and the
// primal recovery are factored here so that the factor of the current S stays valid
hdsdp_retcode cone_checker(MiCone *c, HdmChol **out) {
    if (const hdsdp_retcode rc = cone_make(c->checker, c->n); rc != HDSDP_RETCODE_OK) return rc;
    *out = c->checker.get();
    return HDSDP_RETCODE_OK;
}

hdsdp_retcode cone_factor_check(MiCone *c, int *isPsd) {
    HdmChol *ch = nullptr;
    RC(cone_checker(c, &ch));
    int info = 0;
    c->dual.checker_written();
    if (ch->load_device(c->Scheck.get(), c->n16, g.stream) || ch->factor(g.stream, &info)) return HDSDP_RETCODE_FAILED;
    if (isPsd) *isPsd = (info == 0);
    return HDSDP_RETCODE_OK;
}

// sdpDenseConeInteriorCheckExpert (hdsdp_conic_sdp.c:2192-2207): B = dCCoef*C + dACoefScal*sum_i dACoef_i A_i + dEyeCoef*I
// (+ the perturbation unless the target is the step buffer, :383-385) into the chosen buffer, then the PSD check
hdsdp_retcode cone_interior_expert(void *cd, double dCCoef, double dACoefScal, double *dACoef, double dEyeCoef,
                                   int whichBuffer, int *isInterior) {
    StatScope stat_(ST_ASSEMBLE_FACTOR, __func__);
    MiCone *c = (MiCone *) cd;
    std::vector<double> ys(std::max(1, c->m), 0.0);
    for (int i = 0; i < c->m; ++i) ys[i] = -dACoefScal * (dACoef ? dACoef[i] : 0.0);   // cone_assemble subtracts
    const double eye = dEyeCoef + c->perturb;
    {
        hdsdp_retcode rcs;
        if (cone_small_check(c, dCCoef, ys.data(), &eye, whichBuffer, isInterior, &rcs) == 0) return rcs;
    }
    if (cone_assemble(c, dCCoef, ys.data(), whichBuffer == 0 ? HDM_DUAL_S : HDM_DUAL_SCHECK, &eye)) return HDSDP_RETCODE_FAILED;
    HIP_RC(hipStreamSynchronize(g.stream));   // ys is read by an asynchronous copy
    return (whichBuffer == 0) ? cone_factor_S(c, isInterior) : cone_factor_check(c, isInterior);
}

// engine_step_set.h: c is a member of an active set and is asked dStep on the checker buffer.  Returns true when the set has
// answered (*rc, *isInterior), false when c's own path must run
bool step_set_answer(MiCone *c, double dStep, int *isInterior, hdsdp_retcode *rc);

// sdpDenseConeAddStepToBufferAndCheck (hdsdp_conic_sdp.c:2333-2361): S + dStep*dS with the dS of the last ratio test;
// BUFFER_DUALVAR updates S in place, BUFFER_DUALCHECK leaves S alone and factors the trial point in the checker
hdsdp_retcode cone_axpy_check(void *cd, double dStep, int whichBuffer, int *isInterior) {
    StatScope stat_(ST_ASSEMBLE_FACTOR, __func__);
    MiCone *c = (MiCone *) cd;
    if (whichBuffer != 0 && c->in_step.active()) {               // (the dual buffer stays per cone: S itself moves there)
        hdsdp_retcode rcs;
        if (step_set_answer(c, dStep, isInterior, &rcs)) return rcs;
    }
    if (!c->dS.get()) return HDSDP_RETCODE_FAILED;
    const long cnt = (long) c->n16 * c->n16;
    double *target = (whichBuffer == 0) ? c->S.get() : c->Scheck.get();
    if (whichBuffer == 0) c->dual.S_overwritten();   // S moves without a point being named: the next request assembles it
    else c->dual.checker_written();                  // the checker buffer is written here, its factor object in cone_factor_check
    RC(hdm_axpy_mat(target, c->S.get(), c->dS.get(), dStep, cnt, g.stream));
    return (whichBuffer == 0) ? cone_factor_S(c, isInterior) : cone_factor_check(c, isInterior);
}

// engine_ratio_set.h: a member's stored ratio-test answer is dropped (the identity coefficients are part of no dual-state
// transition, and an answer is served only while nothing at all has changed under it); nothing else happens
void ratio_set_drop_answer(MiCone *c);
// c is a member of an active set and is asked (dTauStep, dy, dAdaRatio) on the dual buffer, or on the checker buffer of a set that
// answers it.  Returns true when the set has answered (*rc, *maxStep), false when c's own path must run
bool ratio_set_answer(MiCone *c, double dTauStep, const double *dy, double dAdaRatio, int whichBuffer, double *maxStep, hdsdp_retcode *rc);

void cone_reduce_resi(void *cd, double resiReduction) { ((MiCone *) cd)->Rd = resiReduction; ratio_set_drop_answer((MiCone *) cd); }   // :2224-2228
void cone_set_perturb(void *cd, double dDualPerturb) { ((MiCone *) cd)->perturb = dDualPerturb; ratio_set_drop_answer((MiCone *) cd); }  // :2236-2241

// hdsdp_conic_sdp.c:2172-2180
hdsdp_retcode cone_interior(void *cd, double tau, double *y, int *isInterior) {
    StatScope stat_(ST_ASSEMBLE_FACTOR, __func__);
    MiCone *c = (MiCone *) cd;
    {
        hdsdp_retcode rcs;
        if (cone_small_check(c, tau, y, nullptr, 0, isInterior, &rcs) == 0) return rcs;
    }
    RC(cone_assemble(c, tau, y, HDM_DUAL_S));
    return cone_factor_S(c, isInterior);
}

// hdsdp_conic_sdp.c:2252-2291
hdsdp_retcode cone_barrier(void *cd, double tau, double *y, int whichBuffer, double *logdet) {
    StatScope stat_(ST_ASSEMBLE_FACTOR, __func__);
    MiCone *c = (MiCone *) cd;
    if (y) {   // only with BUFFER_DUALVAR (the reference asserts it)
        int psd = 0;
        hdsdp_retcode rcs;
        if (cone_small_check(c, tau, y, nullptr, 0, &psd, &rcs) == 0) { if (rcs != HDSDP_RETCODE_OK || !psd) return HDSDP_RETCODE_FAILED; }
        else {
            RC(cone_assemble(c, tau, y, HDM_DUAL_S));
            if (cone_factor_S(c, &psd) != HDSDP_RETCODE_OK || !psd) return HDSDP_RETCODE_FAILED;
        }
    }
    {   // a factor that came from the single-launch check brought its log det along
        const HdmChol *fq = (whichBuffer == 0) ? dual_chol(c) : c->checker.get();
        if (fq && fq->factored && fq->logdet_ok) { *logdet = fq->logdet_val; return HDSDP_RETCODE_OK; }
    }
    std::vector<double> d(c->n);
    if (whichBuffer == 0) {
        if (HFpLinsysGetDiag(c->dualFactor, d.data()) != HDSDP_RETCODE_OK) return HDSDP_RETCODE_FAILED;
    } else {
        if (!c->checker || !c->checker->factored || c->checker->get_diag(d.data(), g.stream)) return HDSDP_RETCODE_FAILED;
    }
    double s = 0.0;
    for (int i = 0; i < c->n; ++i) s += log(d[i]);
    *logdet = 2.0 * s;
    return HDSDP_RETCODE_OK;
}

// The reference's Lanczos estimate accepts the first Ritz value whose residual bound is small; it certifies that an eigenvalue
// lies near it, not that it is the largest.  A warm start (the previous test's Ritz image + 1e-3 x a fixed vector) can hold
// almost nothing of the new operator's top eigenvector, and the test then stops at a lower eigenvalue: a step past alpha*
// (n = 15, DESIGN.md: 0.678 for alpha* = 0.614, the reference's own recurrence gives the same number).  So a finite step is
// checked: S + (1 - 1e-3) step dS is factored in a scratch object.  If that succeeds the reference's number stands unchanged; if not, a
// Lanczos test from the fresh start vector is run (its own object: the warm-start state stays the reference's), the smaller
// step taken, and it is cut by 10 % until the factorisation succeeds.
// The check: is S + (1 - 1e-3) step dS inside the cone?  Factored in the scratch object (made on first use).
// (checked at (1 - 1e-3) step: the reference's own acceptance tolerance (gamma < 1e-3).  A step that is alpha* to
// rounding -- a rank-one dS, dS = -S -- or within that tolerance of it stands as the reference computed it, and
// the driver's trajectory with it; what is caught is a test that stopped at the wrong eigenvalue)
hdsdp_retcode ratio_inside(MiCone *c, int whichBuffer, double step, bool *ok) {
    if (const hdsdp_retcode rc = cone_make(c->safe, c->n); rc != HDSDP_RETCODE_OK) return rc;
    HIP_RC(c->Ssafe.reserve((size_t) c->n16 * c->n16));
    const double *Sb = (whichBuffer == 0) ? c->S.get() : c->Scheck.get();
    int info = 0;
    if (hdm_axpy_mat(c->Ssafe.get(), Sb, c->dS.get(), (1.0 - 1e-3) * step, (long) c->n16 * c->n16, g.stream) ||
        c->safe->load_device(c->Ssafe.get(), c->n16, g.stream) || c->safe->factor(g.stream, &info)) return HDSDP_RETCODE_FAILED;
    *ok = (info == 0);
    return HDSDP_RETCODE_OK;
}
// The rest, once a step has failed the check: the fresh-start test and the 10 % cuts.  The grouped form (engine_ratio_set.h) makes
// the check itself, in its second launch, and comes here for the members whose step failed it.
hdsdp_retcode ratio_safeguard_rest(MiCone *c, HdmChol *fac, int whichBuffer, double *maxStep) {
    if (const hdsdp_retcode rc = cone_make(c->lanczos_fresh, c->n); rc != HDSDP_RETCODE_OK) return rc;
    c->lanczos_fresh->nComputed = 0;
    double step = *maxStep, fresh = INFINITY;
    int steps = 0;
    bool ok = false;
    if (c->lanczos_fresh->solve(fac->Linv.get(), fac->npad, c->dS.get(), c->n16, g.stream, &fresh, &steps) == 0 && fresh < step) step = fresh;
    for (int it = 0; it < 64; ++it) {
        RC(ratio_inside(c, whichBuffer, step, &ok));
        if (ok) break;
        step *= 0.9;
    }
    const bool dbg = hdm_env_int<ENV_RATIO_DEBUG>().value_or(0) != 0;
    if (dbg) fprintf(stderr, "[hdsdp_mi355x ratio] n %d: step %.6e left the cone, safeguarded to %.6e (fresh start %.6e)\n", c->n,
                     *maxStep, step, fresh);
    *maxStep = ok ? step : 0.0;
    return HDSDP_RETCODE_OK;
}
hdsdp_retcode ratio_safeguard(MiCone *c, HdmChol *fac, int whichBuffer, double *maxStep) {
    // (a step of 1e6 or more stands for "unbounded": S + step dS is then rounding noise times the step, and no caller takes it)
    if (!(*maxStep > 0.0) || !(*maxStep < 1e6)) return HDSDP_RETCODE_OK;
    bool ok = false;
    if (const hdsdp_retcode rc = ratio_inside(c, whichBuffer, *maxStep, &ok); rc != HDSDP_RETCODE_OK) return rc;
    if (ok) return HDSDP_RETCODE_OK;
    return ratio_safeguard_rest(c, fac, whichBuffer, maxStep);
}

// sdpDenseConeRatioTestImpl (hdsdp_conic_sdp.c:1640-1686): dS = dTauStep*C - sum dy_i A_i + dAdaRatio*Rd*I, then the
// largest alpha with S + alpha dS >= 0 by Lanczos on L^-1 (-dS) L^-T (lanczos.hip).  L is the factor of the chosen
// buffer: the current S (BUFFER_DUALVAR) or the trial point factored last in the checker (BUFFER_DUALCHECK).
hdsdp_retcode cone_ratio_test(void *cd, double dTauStep, double *dy, double dAdaRatio, int whichBuffer, double *maxStep) {
    StatScope stat_(ST_RATIO, __func__);
    MiCone *c = (MiCone *) cd;
    HdmChol *fac = (whichBuffer == 0) ? dual_chol(c) : c->checker.get();   // LTarget, :1661-1665
    if (!fac || !fac->factored) return HDSDP_RETCODE_FAILED;
    // (the checker buffer stays per cone unless the set's opt-in for it is on: DESIGN.md section 26)
    if (c->in_ratio.active() && (whichBuffer == 0 || set_of<MiRatioSet>(c->in_ratio)->checker_on)) {
        hdsdp_retcode rcs;
        if (ratio_set_answer(c, dTauStep, dy, dAdaRatio, whichBuffer, maxStep, &rcs)) return rcs;
    }
    HIP_RC(cone_make_dS(c));
    const double eye = dAdaRatio * c->Rd;
    if (cone_assemble(c, dTauStep, dy, HDM_DUAL_DS, &eye)) return HDSDP_RETCODE_FAILED;
    if (c->n == 1) {   // :1668-1675
        double s0 = 0.0, d0 = 0.0;
        HIP_RC(hipMemcpyAsync(&d0, c->dS.get(), sizeof(double), hipMemcpyDeviceToHost, g.stream));
        HIP_RC(hipMemcpyAsync(&s0, (whichBuffer == 0) ? c->S.get() : c->Scheck.get(), sizeof(double), hipMemcpyDeviceToHost, g.stream));
        HIP_RC(hipStreamSynchronize(g.stream));
        // (the reference tests d0 > 0, which turns d0 == 0 -- a zero step matrix -- into -s0 / 0 = -inf: a step of minus
        // infinity for a direction that can be followed without limit)
        *maxStep = (d0 >= 0.0) ? INFINITY : (-s0 / d0);
        return HDSDP_RETCODE_OK;
    }
    RC(hdm_mirror_lower(c->dS.get(), c->n16, c->n, g.stream));
    if (fac->invert_factor(g.stream)) return HDSDP_RETCODE_FAILED;
    if (const hdsdp_retcode rc = cone_make(c->lanczos, c->n); rc != HDSDP_RETCODE_OK) return rc;
    int steps = 0;
    const bool dbg = hdm_env_int<ENV_RATIO_DEBUG>().value_or(0) != 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (c->lanczos->solve(fac->Linv.get(), fac->npad, c->dS.get(), c->n16, g.stream, maxStep, &steps)) return HDSDP_RETCODE_FAILED;
    if (dbg) fprintf(stderr, "[hdsdp_mi355x ratio] n %d: %d Lanczos steps, step %.6e, solve %.1f us\n", c->n, steps, *maxStep,
                     1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return ratio_safeguard(c, fac, whichBuffer, maxStep);
}

// The cone's `getstat` slot: the reference's feature detection (sdpDenseConeFeatureDetectImpl / sdpSparseConeFeatureDetectImpl,
// interface/hdsdp_conic_sdp.c:2651-2758; read once by the driver, interface/hdsdp.c:163-168) answered from the engine's own
// presolve, so that a driver whose SDP blocks live here needs no CPU cone beside them (second variant).
// Same decisions: class counts with the objective's class included (:1368-1381); "no primal interior" for a rank-one row whose
// right-hand side is below 1e-3 of its Frobenius norm (|sign| for a normalised factor); an implied trace bound from a row that
// is a multiple of the identity with b / multiple > 0 -- whose VALUE the reference then resets to 0 (:2714), kept as a
// behaviour -- or from unit-column rows e_i e_i' covering every column (their b summed); "very dense" from 0.7 m DENSE rows.
// A block most constraints are zero on (the reference's sparse SDP cone) reports the counts only (:2747-2758).
void cone_getstat(void *cd, double *rowRHS, int intF[20], double dblF[20]) {
    MiCone *c = (MiCone *) cd;
    enum { F_NOPINT = 2, F_VERYDENSE = 4, F_IMPTRACE = 5, F_NZERO = 15, F_NSP = 16, F_NDS = 17, F_NSPR1 = 18, F_NDSR1 = 19, D_IMPTRACEX = 11 };
    int stats[5] = {0, 0, 0, 0, 0};
    if (c->synthetic) stats[MI_COEFF_DENSE] = c->m + 1;
    else {
        for (int t = 0; t < 5; ++t) stats[t] = c->blk.counts[t];
        // the objective is counted with the class it had BEFORE the rank-one detection (:1373 counts it when the data is
        // processed, the presolve re-counts rows only, :1502-1504): theta1's all-ones objective stays "dense" in the features
        const double P = 0.5 * (double) c->n * (c->n + 1);
        stats[c->blk.obj.stored == 0 ? MI_COEFF_ZERO : ((double) c->blk.obj.stored > 0.3 * P ? MI_COEFF_DENSE : MI_COEFF_SPARSE)] += 1;
    }
    intF[F_NZERO] = stats[MI_COEFF_ZERO]; intF[F_NDS] = stats[MI_COEFF_DENSE]; intF[F_NSP] = stats[MI_COEFF_SPARSE];
    intF[F_NSPR1] = stats[MI_COEFF_SPR1]; intF[F_NDSR1] = stats[MI_COEFF_DSR1];
    const bool compact = (c->world == 1 && !c->synthetic && (int) c->blk.rows.size() == c->m);
    if (compact && (double) c->mloc <= 0.3 * (double) c->m) return;          // the reference's sparse SDP cone: counts only
    if (!c->synthetic && rowRHS) {
        bool nopint = false, imptrace = false;
        for (int i = 0; i < c->m; ++i) {
            const MiCoeff &a = c->blk.rows[i];
            if (a.rank == 1 && (a.type == MI_COEFF_SPR1 || a.type == MI_COEFF_DSR1) && fabs(rowRHS[i]) < 1e-3 * fabs(a.sign)) nopint = true;
        }
        if (nopint) intF[F_NOPINT] = 1;
        for (int i = 0; i < c->m && !imptrace; ++i) {
            const MiCoeff &a = c->blk.rows[i];
            if (a.is_eye && rowRHS[i] / a.eye_val > 0.0) imptrace = true;
        }
        double implied = 0.0;                                                // (reset whether or not an identity row was found)
        std::vector<int> seen((size_t) std::max(c->m, c->n), 0);
        if (!imptrace)
            for (int i = 0; i < c->m; ++i) {
                const MiCoeff &a = c->blk.rows[i];
                const int at = a.unit_col;
                if (at < 0 || seen[at]) continue;
                seen[at] = 1;
                implied += rowRHS[i];
            }
        int covered = 0;
        for (int i = 0; i < c->m; ++i) covered += seen[i];
        if (covered == c->n) imptrace = true;
        if (imptrace) { intF[F_IMPTRACE] = 1; dblF[D_IMPTRACEX] = implied; }
    }
    if ((double) stats[MI_COEFF_DENSE] >= 0.7 * (double) c->m) intF[F_VERYDENSE] = 1;
}
void cone_view(void *cd) {
    const MiCone *c = (const MiCone *) cd;
    printf("- MI355X engine cone of %d x %d and %d rows (device path %d).\n", c->n, c->n, c->m, c->path);
}

// ---- the remaining cone utilities of the reference's vtable (hdsdp_conic.c:137-153) ------------------------------------
// norms of the data: |A|_abs = sum |a_ij|, |A|_F over the full symmetric matrices (hdsdp_sdpdata.c:208-309 computes the same
// numbers per storage class); the synthetic family has no host copy, its norms come from one pass over the device data

static void coeff_norms(const MiCoeff &a, int n, double *abs_, double *fro2) {
    // raw lower-triangular entries (packed index): diagonal once, off-diagonal twice
    double sa = 0.0, sf = 0.0;
    long colstart = 0;
    int col = 0;
    for (size_t k = 0; k < a.idx.size(); ++k) {
        const long pidx = a.idx[k];
        while (col < n && pidx >= colstart + (n - col)) { colstart += n - col; ++col; }
        const bool diag = (pidx == colstart);
        const double v = a.val[k];
        sa += diag ? fabs(v) : 2.0 * fabs(v);
        sf += diag ? v * v : 2.0 * v * v;
    }
    *abs_ = sa; *fro2 = sf;
}

int cone_data_norms(MiCone *c, double *rows_abs, double *rows_fro, double *obj_abs, double *obj_fro) {
    if (c->norms_ready) {
        *rows_abs = c->nrm[0]; *rows_fro = c->nrm[1]; *obj_abs = c->nrm[2]; *obj_fro = c->nrm[3];
        return 0;
    }
    double ra = 0.0, rf2 = 0.0, oa = 0.0, of2 = 0.0;
    // (a block on the congruence + Gram path has its data resident in A_L form: one HBM-bound pass over it instead of a host
    // loop over the CSC entries, which took 1.0 s of the driver's presolve at n = m = 2000)
    const bool on_device = c->synthetic || (c->path == PATH_GEMM && c->rows.has_rows());   // (resident rows, or batches regenerated / expanded)
    if (!on_device) {
        for (int i = 0; i < c->m; ++i) { double a_, f_; coeff_norms(c->blk.rows[i], c->n, &a_, &f_); ra += a_; rf2 += f_; }
        coeff_norms(c->blk.obj, c->n, &oa, &of2);
        oa *= c->objScal; of2 *= c->objScal * c->objScal;
    } else {
        HdmBuf<double> tmp;
        HDM_HIP_CHECK(tmp.alloc(4));
        HDM_HIP_CHECK(hipMemsetAsync(tmp.get(), 0, sizeof(double) * 4, g.stream));
        for (int q0 = 0, B = c->rows.batch(); q0 < c->mloc; q0 += B) {
            const int nb = std::min(B, c->mloc - q0);
            const double *A = c->rows.rows(q0, nb);
            if (!A) return 1;
            hipLaunchKernelGGL(mi_low_norms_kernel, dim3(nb), dim3(256), 0, g.stream, A, c->astride, c->n, (long) c->n16, nb, 1, tmp.get());
        }
        hipLaunchKernelGGL(mi_low_norms_kernel, dim3(1), dim3(256), 0, g.stream, c->Cfull.get(), 0L, c->n, (long) c->n16, 1, 0, tmp.get() + 2);
        double h[4];
        HDM_HIP_CHECK(hipMemcpyAsync(h, tmp.get(), sizeof(h), hipMemcpyDeviceToHost, g.stream));
        HDM_HIP_CHECK(hipStreamSynchronize(g.stream));
        tmp.reset();   // (before the all-reduce, as ever)
        ra = h[0]; rf2 = h[1]; oa = h[2]; of2 = h[3];
        if (c->world > 1 && c->allreduce) {   // rows are sharded: sum the two row totals over the ranks
            HdmBuf<double> dv;
            HDM_HIP_CHECK(dv.alloc(2));
            double two[2] = {ra, rf2};
            HDM_HIP_CHECK(hipMemcpy(dv.get(), two, sizeof(two), hipMemcpyHostToDevice));
            if (c->allreduce(c->xctx, dv.get(), 2)) return 1;
            HDM_HIP_CHECK(hipMemcpy(two, dv.get(), sizeof(two), hipMemcpyDeviceToHost));
            ra = two[0]; rf2 = two[1];
        }
    }
    c->nrm[0] = ra; c->nrm[1] = sqrt(rf2); c->nrm[2] = oa; c->nrm[3] = sqrt(of2);
    c->norms_ready = true;
    return cone_data_norms(c, rows_abs, rows_fro, obj_abs, obj_fro);
}

double cone_coeff_norm(void *cd, int whichNorm) {
    StatScope stat_(ST_PRIMAL_UTIL, __func__);   // sdpDenseConeGetCoeffNorm, hdsdp_conic_sdp.c:1568-1586 (ABS_NORM 1, FRO_NORM 2)
    double v[4];
    if (cone_data_norms((MiCone *) cd, v, v + 1, v + 2, v + 3)) return NAN;
    return whichNorm == 1 ? v[0] : v[1];
}
double cone_obj_norm(void *cd, int whichNorm) {
    StatScope stat_(ST_PRIMAL_UTIL, __func__);     // sdpDenseConeGetObjNorm, :1558-1561
    double v[4];
    if (cone_data_norms((MiCone *) cd, v, v + 1, v + 2, v + 3)) return NAN;
    return whichNorm == 1 ? v[2] : v[3];
}
void cone_scal(void *cd, double dScal) {
    StatScope stat_(ST_PRIMAL_UTIL, __func__);             // sdpDenseConeScal, :1604-1614: the objective is scaled, nothing else
    MiCone *c = (MiCone *) cd;
    const long cnt = (long) c->n16 * c->n16;
    hipLaunchKernelGGL(mi_scale_kernel, dim3((unsigned) ((cnt + 255) / 256)), dim3(256), 0, g.stream, c->Cfull.get(), cnt, dScal);
    if (c->CL.get()) hipLaunchKernelGGL(mi_scale_kernel, dim3((unsigned) ((c->astride + 255) / 256)), dim3(256), 0, g.stream, c->CL.get(), c->astride, dScal);
    c->objScal *= dScal;
    c->norms_ready = false;
    c->dual.data_changed();          // S and dS were assembled with the old objective: no short-cut from them (cone_assemble)
    (void) hipStreamSynchronize(g.stream);
}

// X (host, n x n column-major, symmetric) -> the device scratch matrix Xup (ld = npad of the dual factor)
static int cone_upload_X(MiCone *c, const double *X, long *ldx) {
    const long ld = dual_chol(c)->npad;
    const size_t np2 = sizeof(double) * (size_t) ld * ld;
    HDM_HIP_CHECK(c->Xup.reserve(np2 / sizeof(double)));   // (Xinv / Yinv belong to the builders, sized per path)
    HDM_HIP_CHECK(hipMemsetAsync(c->Xup.get(), 0, np2, g.stream));
    HDM_HIP_CHECK(hipMemcpy2DAsync(c->Xup.get(), sizeof(double) * ld, X, sizeof(double) * c->n, sizeof(double) * c->n, c->n,
                                   hipMemcpyHostToDevice, g.stream));
    *ldx = ld;
    return 0;
}

// sdpDenseConeBuildPrimalXSXDirection (hdsdp_conic_sdp.c:2021-2040 -> fds_trimultiply, dense_opts.c:102-132), the cone's
// coneBuildPrimalDirection slot used by the primal refinement (hdsdp_psdp.c:236,295):  XSX += X^T D X  (full symmetric
// n x n, host), D = the dual matrix (iDualMat != 0) or the dual step dS of the last ratio test, both resident.  Two
// plain MFMA GEMMs on the device; only X goes up and the n x n product comes back.
void cone_build_primal_dir(void *cd, void *kktv, double *X, double *XSX, int iDualMat) {
    StatScope stat_(ST_PRIMAL_UTIL, __func__);
    (void) kktv;
    MiCone *c = (MiCone *) cd;
    const int n = c->n;
    long ldx = 0;
    const double *D = iDualMat ? c->S.get() : c->dS.get();
    if (!D) { fprintf(stderr, "[hdsdp_mi355x] primal direction: no dual step has been formed yet\n"); return; }
    if (cone_upload_X(c, X, &ldx)) return;
    const size_t np2 = sizeof(double) * (size_t) ldx * ldx;
    if (c->Pr1.reserve(np2 / sizeof(double)) != hipSuccess) return;
    if (c->Pr2.reserve(np2 / sizeof(double)) != hipSuccess) return;
    // Pr1 <- D as a full symmetric matrix (the resident copy has its lower triangle valid), zero padded
    if (hipMemsetAsync(c->Pr1.get(), 0, np2, g.stream) != hipSuccess) return;
    if (hipMemcpy2DAsync(c->Pr1.get(), sizeof(double) * ldx, D, sizeof(double) * c->n16, sizeof(double) * n, n,
                         hipMemcpyDeviceToDevice, g.stream) != hipSuccess) return;
    if (hdm_mirror_lower(c->Pr1.get(), ldx, n, g.stream)) return;
    const int n16 = c->n16;
    const HdmOperand Xt = hdm_kmajor(c->Xup.get(), ldx);
    // T = D X   (B operand element (j, k) = X(k, j): K-major)
    if (hdm_launch_gemm(hdm_gemm_product(c->Pr2.get(), ldx, n16, n16, n16, 1.0, hdm_mmajor(c->Pr1.get(), ldx), Xt), g.stream)) return;
    // P = X^T T   (A operand element (i, k) = X(k, i): K-major; B operand element (j, k) = T(k, j): K-major)
    if (hdm_launch_gemm(hdm_gemm_product(c->Pr1.get(), ldx, n16, n16, n16, 1.0, Xt, hdm_kmajor(c->Pr2.get(), ldx)), g.stream)) return;
    std::vector<double> h((size_t) n * n);
    if (hipMemcpy2DAsync(h.data(), sizeof(double) * n, c->Pr1.get(), sizeof(double) * ldx, sizeof(double) * n, n,
                         hipMemcpyDeviceToHost, g.stream) != hipSuccess) return;
    if (hipStreamSynchronize(g.stream) != hipSuccess) return;
    for (size_t e = 0; e < h.size(); ++e) XSX[e] += h[e];
}

void cone_a_times_x(void *cd, double *X, double *ATimesX) {
    StatScope stat_(ST_PRIMAL_UTIL, __func__);   // sdpDenseConeATimesX, :2470-2477: y_i += <A_i, X>
    MiCone *c = (MiCone *) cd;
    long ldx = 0;
    HdmBuf<double> out_own;   // per call, as ever: freed on return
    if (cone_upload_X(c, X, &ldx)) return;
    if (out_own.alloc(2 * (size_t) c->m) != hipSuccess) return;
    double *out = out_own.get();
    (void) hipMemsetAsync(out, 0, sizeof(double) * 2 * (size_t) c->m, g.stream);
    // A is stored in A_L form: <A, X> = 2 <A_L, X> for symmetric X
    if (cone_sym_dot2(c, c->Xup.get(), nullptr, ldx, out, out + c->m, 2.0, 0.0) == 0) {
        if (c->world > 1 && c->allreduce) { (void) hipStreamSynchronize(g.stream); (void) c->allreduce(c->xctx, out, c->m); }
        std::vector<double> h(c->m);
        if (hipMemcpyAsync(h.data(), out, sizeof(double) * c->m, hipMemcpyDeviceToHost, g.stream) == hipSuccess &&
            hipStreamSynchronize(g.stream) == hipSuccess)
            for (int i = 0; i < c->m; ++i) ATimesX[i] += h[i];
    }
}

static double cone_dot_with(MiCone *c, const double *dev, long ldd, int lower_valid, double *X) {
    long ldx = 0;
    HdmBuf<double> out_own;   // per call, as ever: freed on return
    double h = NAN;
    if (cone_upload_X(c, X, &ldx)) return NAN;
    if (out_own.alloc(1) != hipSuccess) return NAN;
    double *out = out_own.get();
    (void) hipMemsetAsync(out, 0, sizeof(double), g.stream);
    if (lower_valid) hipLaunchKernelGGL(mi_lower_dot_kernel, dim3(1), dim3(256), 0, g.stream, dev, ldd, c->Xup.get(), ldx, c->n, out);
    else hipLaunchKernelGGL(mi_mat_dot_kernel, dim3(1), dim3(256), 0, g.stream, dev, ldd, c->Xup.get(), ldx, c->n, 0, 1.0, out);
    if (hipMemcpyAsync(&h, out, sizeof(double), hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
        hipStreamSynchronize(g.stream) != hipSuccess) h = NAN;
    return h;
}
double cone_trace_cx(void *cd, double *X) {
    StatScope stat_(ST_PRIMAL_UTIL, __func__);   // sdpDenseConeTraceCX, :2520-2523
    MiCone *c = (MiCone *) cd;
    return cone_dot_with(c, c->Cfull.get(), c->n16, 0, X);
}
double cone_x_dot_s(void *cd, double *X) {
    StatScope stat_(ST_PRIMAL_UTIL, __func__);    // sdpDenseConeXDotS, :2549-2560 (S is lower-valid: fds_dot_fds, dense_opts.c:134-156)
    MiCone *c = (MiCone *) cd;
    return cone_dot_with(c, c->S.get(), c->n16, 1, X);
}
void cone_get_dual(void *cd, double *dConeDual, double *dummy) {
    StatScope stat_(ST_PRIMAL_UTIL, __func__);   // sdpDenseConeGetDual, :2494-2506: S, symmetrised
    (void) dummy;
    MiCone *c = (MiCone *) cd;
    const int n = c->n;
    if (hipMemcpy2DAsync(dConeDual, sizeof(double) * n, c->S.get(), sizeof(double) * c->n16, sizeof(double) * n, n,
                         hipMemcpyDeviceToHost, g.stream) != hipSuccess || hipStreamSynchronize(g.stream) != hipSuccess) return;
    for (int j = 0; j < n; ++j)
        for (int i = j + 1; i < n; ++i) dConeDual[(size_t) j + (size_t) i * n] = dConeDual[(size_t) i + (size_t) j * n];
}

// sdpDenseConeGetPrimal (hdsdp_conic_sdp.c:2393-2446), the cone's conePRecover slot:
//     X = mu * L^-T ( sym( L^-1 dS L^-T ) + I ) L^-1,   S = C - sum y_i A_i = L L^T (no residual term),  dS = sum dy_i A_i.
// The reference does four triangular solves with n right-hand sides on the checker factor; here S is factored into a
// second resident factor object, inverted once, and the four products are plain MFMA GEMMs with the explicit Linv.
// Like the reference, an S that is not positive definite prints a message and leaves the output untouched.
void cone_precover(void *cd, double dBarrierMu, double *y, double *dy, double *X, double *aux) {
    StatScope stat_(ST_PRIMAL_UTIL, __func__);
    (void) aux;
    MiCone *c = (MiCone *) cd;
    const double zero = 0.0;
    const int n = c->n;
    auto fail = [](const char *what) { fprintf(stderr, "[hdsdp_mi355x] primal recovery: %s\n", what); };
    if (cone_assemble(c, 1.0, y, HDM_DUAL_SCHECK, &zero)) return fail("S assembly failed");
    HdmChol *chp = nullptr;
    if (cone_checker(c, &chp) != HDSDP_RETCODE_OK) return fail("out of memory");
    HdmChol &ch = *chp;
    int info = 0;
    c->dual.checker_written();
    if (ch.load_device(c->Scheck.get(), c->n16, g.stream) || ch.factor(g.stream, &info)) return fail("factorisation failed");
    if (info != 0) {
        if (stat_trace()) fprintf(stderr, "[hdsdp_mi355x trace]     primal recovery: factorisation stopped at pivot %d\n", info);
        printf("Recovery step is infeasible\n");
        return;
    }
    if (cone_make_dS(c) != hipSuccess) return fail("out of memory");
    std::vector<double> ndy(c->m);
    for (int i = 0; i < c->m; ++i) ndy[i] = -dy[i];           // cone_assemble subtracts: dS = + sum dy_i A_i
    if (cone_assemble(c, 0.0, ndy.data(), HDM_DUAL_DS, &zero)) return fail("dS assembly failed");
    if (hipStreamSynchronize(g.stream) != hipSuccess) return fail("stream");   // ndy is read by an async copy
    if (hdm_mirror_lower(c->dS.get(), c->n16, n, g.stream)) return fail("mirror");
    if (ch.invert_factor(g.stream)) return fail("triangular inverse failed");
    const size_t np2 = sizeof(double) * (size_t) ch.npad * ch.npad;
    if (c->Pr1.reserve(np2 / sizeof(double)) != hipSuccess) return fail("out of memory");
    if (c->Pr2.reserve(np2 / sizeof(double)) != hipSuccess) return fail("out of memory");
    const int n16 = c->n16;
    const long np = ch.npad;
    const HdmOperand W = hdm_mmajor(ch.Linv.get(), np), Wt = hdm_kmajor(ch.Linv.get(), np);
    // T1 = W dS          (W = Linv)
    if (hdm_launch_gemm(hdm_gemm_product(c->Pr1.get(), np, n16, n16, n16, 1.0, W, hdm_mmajor(c->dS.get(), n16)), g.stream)) return fail("gemm");
    // Z = T1 W^T
    if (hdm_launch_gemm(hdm_gemm_product(c->Pr2.get(), np, n16, n16, n16, 1.0, hdm_mmajor(c->Pr1.get(), np), W), g.stream)) return fail("gemm");
    if (hdm_sym_scale(c->Pr2.get(), ch.npad, c->n16, 1.0, 1.0, g.stream)) return fail("sym");
    // T2 = W^T Z
    if (hdm_launch_gemm(hdm_gemm_product(c->Pr1.get(), np, n16, n16, n16, 1.0, Wt, hdm_mmajor(c->Pr2.get(), np)), g.stream)) return fail("gemm");
    // X = T2 W
    if (hdm_launch_gemm(hdm_gemm_product(c->Pr2.get(), np, n16, n16, n16, 1.0, hdm_mmajor(c->Pr1.get(), np), Wt), g.stream)) return fail("gemm");
    if (hdm_sym_scale(c->Pr2.get(), ch.npad, n, 0.0, dBarrierMu, g.stream)) return fail("sym");
    if (hipMemcpy2DAsync(X, sizeof(double) * n, c->Pr2.get(), sizeof(double) * ch.npad, sizeof(double) * n, n,
                         hipMemcpyDeviceToHost, g.stream) != hipSuccess) return fail("copy");
    (void) hipStreamSynchronize(g.stream);
}
