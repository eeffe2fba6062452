// kkt_store.h -- how the Schur operator's matrix M is stored, what state it is in, and how it reaches the factor.
// HKKTInit decides the storage once (sparse or dense host matrix, tile store or dense device matrix, block envelope, order);
// from then on every writer of M names what it did through one of HdmKktState's transitions, and HKKTFactorize asks
// hdm_kkt_load_plan what to do, performs it and commits it.  What is left of the factorised matrix afterwards -- what the residual
// of a refined solve may read -- is hdm_kkt_refine_source's answer, from the same state (the table is at the end of this file).
// Pure host arithmetic: no HIP call, no engine state.  The engine performs these rules (engine_kkt.h, engine_linsys.h, and
// HMiKKTPhaseA in engine_api.h); tests/test_kkt_store_cpu.py compiles this header alone.
#pragma once
#include "env_switches.h"
#include "refine_rule.h"
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

// ---- the five switches ----------------------------------------------------------------------
// HDSDP_MI355X_SPARSE_KKT=0  the operator's host matrix is always dense
// HDSDP_MI355X_KKT_TILES=0   a sparse operator never takes the tile form
// HDSDP_MI355X_KKT_ENVELOPE=0  the dense device matrix of a sparse operator is factored in full, in the driver's order
// HDSDP_MI355X_KKT_RCM=0     no reverse Cuthill-McKee order is looked for
// HDSDP_MI355X_DEVICE_M=1    HKKTInit turns the host mirror off where it can
// (when each is read: env_switches.h)
struct HdmKktSwitches { bool sparse, tiles, envelope, rcm, device_m; };
static inline HdmKktSwitches hdm_kkt_switches() {
    return {hdm_env_on<ENV_SPARSE_KKT>(), hdm_env_on<ENV_KKT_TILES>(), hdm_env_on<ENV_KKT_ENVELOPE>(), hdm_env_on<ENV_KKT_RCM>(),
            hdm_env_int<ENV_DEVICE_M>().value_or(0) == 1};
}

// ---- sparse or dense ------------------------------------------------------------------------
// The reference's rule (hdsdp_schur.c:229-238, :104-108; HDSDP_SPARSE_SCHUR_THRESHOLD, hdsdp.h:29): a cone whose share of M
// reaches 0.3 m^2 entries makes the matrix dense at once, and so does the aggregated pattern when it grows that far.
constexpr double HDM_KKT_SPARSE_THRESHOLD = 0.3;
static inline int64_t hdm_kkt_dense_count(int m) { return (int64_t) (HDM_KKT_SPARSE_THRESHOLD * (double) m * (double) m); }
// `count`: a cone's symmetric nnz, or the size of the pattern collected so far
static inline bool hdm_kkt_count_is_sparse(int64_t count, int m) { return count < hdm_kkt_dense_count(m); }
// A constraint no cone has data for leaves an empty column: the reference stops there ("KKT solver detects an empty column",
// :116-121); the engine keeps such an operator usable on the dense matrix, where the row stays zero until a CPU cone or the
// regularisation fills it.  So does a column whose first index is not the diagonal (kktDiag points at the first entry).
static inline bool hdm_kkt_columns_are_sparse(int m, const int *beg, const int *idx) {
    for (int c = 0; c < m; ++c)
        if (beg[c] == beg[c + 1] || idx[beg[c]] != c) return false;
    return true;
}

// ---- block envelope and order ---------------------------------------------------------------
// The blocked Cholesky of the (dense, mostly zero) device matrix of a sparse operator stops each block column where the
// pattern's block envelope ends, and the substitutions skip the blocks outside (HdmChol::set_envelope).  The factor fills inside
// its row envelope only, so nothing is approximated.
constexpr int HDM_KKT_BLOCK = 128;
// A reverse Cuthill-McKee order is looked for where it can pay: patterns up to 5e7 entries (its adjacency lists take 8 bytes per
// entry on the host) that do not already fill most of the triangle; it is taken when it cuts the factorisation's cost by a fifth.
constexpr int64_t HDM_KKT_RCM_MAX_NNZ = 50000000;
constexpr double HDM_KKT_RCM_MAX_FILL = 0.15;
constexpr double HDM_KKT_RCM_GAIN = 0.8;
static inline bool hdm_kkt_rcm_eligible(int64_t nnz, int m) {
    return nnz <= HDM_KKT_RCM_MAX_NNZ && (double) nnz < HDM_KKT_RCM_MAX_FILL * (double) m * m;
}
static inline bool hdm_kkt_rcm_taken(double cost_rcm, double cost_nat) { return cost_rcm < HDM_KKT_RCM_GAIN * cost_nat; }

struct HdmKktEnvelope {
    double cost = 0.0;          // of the factorisation, in block products
    std::vector<int> first;     // per block row: the first block column inside the envelope
};
// The envelope of the pattern (rows[q], cols[q]), q < nnz, over nb block rows; under perm (perm[old] = new) if given, each
// entry taken back into the lower triangle.
static inline HdmKktEnvelope hdm_kkt_envelope(const int *rows, const int *cols, size_t nnz, int nb, const int *perm) {
    HdmKktEnvelope e;
    e.first.resize(nb);
    for (int b = 0; b < nb; ++b) e.first[b] = b;
    for (size_t q = 0; q < nnz; ++q) {
        int r = rows[q], c = cols[q];
        if (perm) { r = perm[r]; c = perm[c]; if (r < c) std::swap(r, c); }
        const int br = r / HDM_KKT_BLOCK, bc = c / HDM_KKT_BLOCK;
        if (bc < e.first[br]) e.first[br] = bc;
    }
    std::vector<int> colh(nb);  // per block column: the last block row that reaches it
    for (int k = 0; k < nb; ++k) colh[k] = k;
    for (int b = 0; b < nb; ++b) for (int k = e.first[b]; k <= b; ++k) colh[k] = std::max(colh[k], b);
    for (int k = 0; k < nb; ++k) { const double h = colh[k] - k; e.cost += 1.0 + h + 0.5 * h * (h + 1.0); }
    return e;
}

// ---- state ----------------------------------------------------------------------------------
enum HdmKktForm {
    HDM_KKT_DENSE = 0,   // dense host matrix (and a dense device matrix)
    HDM_KKT_CSC,         // host CSC over a dense device matrix
    HDM_KKT_TILES        // host CSC over a tile store (bsparse.h)
};

enum HdmKktStage {       // what HKKTFactorize does to M before the factor object sees it
    HDM_KKT_STAGE_NONE = 0,
    HDM_KKT_STAGE_FOLD,            // upload the diagonal channel and add it to the device matrix's diagonal
    HDM_KKT_STAGE_CSC_TO_FACTOR,   // zero the tile factor store; upload the nnz host values; scatter them into it at (rows, cols)
    HDM_KKT_STAGE_CSC_TO_M         // zero the device matrix; upload the nnz host values; scatter them into it at (rows, cols)
};
enum HdmKktSource { HDM_KKT_SRC_NONE = 0, HDM_KKT_SRC_HOST_M, HDM_KKT_SRC_DEVICE_M };
// tile form, refined (cap and tile switch on at HKKTFactorize): which tile store held the matrix the factor was made from
enum HdmKktTileSource { HDM_KKT_TILE_SRC_NONE = 0, HDM_KKT_TILE_SRC_M_STORE, HDM_KKT_TILE_SRC_COPY };
enum HdmKktLoad {
    HDM_KKT_LOAD_STAGED = 0,   // (done by staging)
    HDM_KKT_LOAD_TILES,        // HdmBsp::load_M: the accumulation store is copied into the factor store
    HDM_KKT_LOAD_HOST,         // HdmChol::load_host from the host matrix
    HDM_KKT_LOAD_DEVICE,       // HdmChol::load_device from the device matrix
    HDM_KKT_LOAD_PERMUTED,     // zero the factor image, scatter the pattern's values at (prow, pcol), HdmChol::finish_load
    HDM_KKT_LOAD_PIVOTED       // the pivoted factorisation from the recorded source, in place of load and Cholesky
};
enum HdmKktOnPivot { HDM_KKT_PIVOT_FAIL = 0, HDM_KKT_PIVOT_SWITCH };

struct HdmKktLoadPlan {
    bool ok = false;                            // a requirement that is not met: FAILED before any device call, no step
    HdmKktStage stage = HDM_KKT_STAGE_NONE;
    HdmKktSource source = HDM_KKT_SRC_NONE;     // recorded by commit, read by the pivoted solver
    HdmKktLoad load = HDM_KKT_LOAD_STAGED;
    bool gather = false;                        // LOAD_PERMUTED: first gather the pattern's values from the device matrix
    HdmKktOnPivot on_pivot = HDM_KKT_PIVOT_FAIL;
    // bytes of M that HKKTFactorize sends up: the host CSC's values, or the dense mirror (load_host, or the pivoted solver's load)
    int64_t matrix_bytes(int64_t m, int64_t nnz) const {
        if (stage == HDM_KKT_STAGE_CSC_TO_FACTOR || stage == HDM_KKT_STAGE_CSC_TO_M) return 8 * nnz;
        return source == HDM_KKT_SRC_HOST_M ? 8 * m * m : 0;
    }
    // ... and of the channel, counted where it is uploaded
    int64_t channel_bytes(int64_t m) const { return stage == HDM_KKT_STAGE_FOLD ? 8 * m : 0; }
};

class HdmKktState {
    HdmKktForm form_ = HDM_KKT_DENSE;
    bool mirror_ = true;          // the host matrix is authoritative: refreshed after a build, uploaded before a factorisation
    bool permuted_ = false;       // CSC: the factor object holds P M P'
    bool indef_ = false;          // switched to the pivoted solver: stays switched (hdsdp_linsolver.c:1838)
    bool m_valid_ = false;        // the device matrix holds the result of the last build
    bool chan_folded_ = false;    // the diagonal channel of the current build is in the device matrix already
    // not owned: where the last factorised matrix came from (lower triangle valid)
    const double *srcHost = nullptr, *srcDev = nullptr;
    long srcLd = 0;
    // the refined solve (refine_rule.h): the step cap (0 = off) and what is left of the matrix the factor was made from
    int refine_ = 0;
    HdmKktSource fact_src_ = HDM_KKT_SRC_NONE;   // where the factorised matrix came from
    bool fact_copy_ = false;                     // host source: refinement was on then, so a device copy of the loaded image exists
    bool fact_dev_intact_ = false;               // device source: no build has overwritten the device matrix since
    // the tile form's refined solve has a switch of its own on top of the cap (HMiLinsysSetRefineTiles)
    bool refine_tiles_ = false;
    HdmKktTileSource fact_tile_ = HDM_KKT_TILE_SRC_NONE;   // accumulation store in place (with fact_dev_intact_), or a copy of the factor store
    friend HdmKktLoadPlan hdm_kkt_load_plan(const HdmKktState &);
    friend struct HdmRefineSource hdm_kkt_refine_source(const HdmKktState &);
    void factorised_from(HdmKktSource src) {
        fact_src_ = src; fact_copy_ = (src == HDM_KKT_SRC_HOST_M && refine_ > 0); fact_dev_intact_ = (src == HDM_KKT_SRC_DEVICE_M);
        fact_tile_ = HDM_KKT_TILE_SRC_NONE;
    }
    // tile form: load_M copied the accumulation store (it stays as it is), or staging scattered the host CSC into the factor store
    void tiles_factorised_from(HdmKktLoad load) {
        if (form_ != HDM_KKT_TILES || refine_ == 0 || !refine_tiles_) return;
        fact_tile_ = load == HDM_KKT_LOAD_TILES ? HDM_KKT_TILE_SRC_M_STORE : HDM_KKT_TILE_SRC_COPY;
        fact_dev_intact_ = (fact_tile_ == HDM_KKT_TILE_SRC_M_STORE);
    }

public:
    HdmKktForm form() const { return form_; }
    bool mirror() const { return mirror_; }       bool permuted() const { return permuted_; }   bool indef() const { return indef_; }
    bool m_valid() const { return m_valid_; }     bool chan_folded() const { return chan_folded_; }
    const double *src_host() const { return srcHost; }   const double *src_dev() const { return srcDev; }   long src_ld() const { return srcLd; }
    int refine() const { return refine_; }
    // the loaded image of a host matrix is to be copied on the device before it is factorised (asked after commit / host_matrix_given)
    bool refine_wants_copy() const { return fact_src_ == HDM_KKT_SRC_HOST_M && fact_copy_; }
    bool refine_tiles() const { return refine_tiles_; }
    // tile form with the mirror on: the scattered factor store is to be copied before HdmBsp::factor overwrites it (asked after commit)
    bool refine_wants_tile_copy() const { return fact_tile_ == HDM_KKT_TILE_SRC_COPY; }

    // Transitions, named for what happened.
    // HKKTInit decided the storage: a fresh device matrix and factor object.  The mirror keeps what it was told.
    void storage_decided(HdmKktForm form, bool permuted) {
        form_ = form; permuted_ = permuted; indef_ = false; m_valid_ = chan_folded_ = false;
        srcHost = srcDev = nullptr; srcLd = 0;
        factorised_from(HDM_KKT_SRC_NONE);
    }
    // a build of type t started: it zeroes M and the channel, unless it is a corrector build, which touches neither
    void build_started(bool corrector) { if (!corrector) { chan_folded_ = false; fact_dev_intact_ = false; } }
    // a build of type t finished: the device matrix holds its result (a corrector build leaves what was there)
    void build_finished(bool corrector) { if (!corrector) m_valid_ = true; }
    // the channel was uploaded and added to the device matrix's diagonal (HKKTRegularize, or staging)
    void channel_folded() { chan_folded_ = true; }
    // the host CSC was scattered into the zeroed device matrix, which is thereby the matrix to be factored
    void csc_scattered() { m_valid_ = true; }
    // the fused small pass (HMiKKTPhaseA) wrote M and its factor in one launch
    void small_pass_done(const double *Mdev, long ld) {
        m_valid_ = true; srcHost = nullptr; srcDev = Mdev; srcLd = ld;
        factorised_from(HDM_KKT_SRC_DEVICE_M);
    }
    // the mirror was switched (HMiKKTSetHostMirror): kkt_point_diag and the plan read it, nothing else changes
    void mirror_switched(bool on) { mirror_ = on; }
    // the solver was switched to the pivoted one (lin_switch_indefinite)
    void switched_to_pivoted() { indef_ = true; }
    // a host matrix was handed over for factorisation (HFpLinsysNumeric on a linear system that is no operator's)
    void host_matrix_given(const double *A, long ld) { srcHost = A; srcDev = nullptr; srcLd = ld; factorised_from(HDM_KKT_SRC_HOST_M); }
    // refinement was switched (HMiLinsysSetRefine): 0 = off, else the step cap.  What was factorised before keeps what it has.
    void refine_set(int maxSteps) {
        refine_ = hdm_refine_clamp(maxSteps);
        if (refine_ == 0) { fact_copy_ = false; drop_tile_copy(); }   // (off: the copies are freed)
    }
    // the tile form's own switch (HMiLinsysSetRefineTiles).  Off: the copy of the factor store is freed
    void refine_tiles_set(bool on) { refine_tiles_ = on; if (!on) drop_tile_copy(); }

    // staging of `plan` is done: record what it made of M and where the factorisation takes it from
    void commit(const HdmKktLoadPlan &plan, const double *Mhost, long ldHost, const double *Mdev, long ldDev) {
        if (plan.stage == HDM_KKT_STAGE_FOLD) channel_folded();
        if (plan.stage == HDM_KKT_STAGE_CSC_TO_M) csc_scattered();
        if (plan.source == HDM_KKT_SRC_HOST_M) { srcHost = Mhost; srcDev = nullptr; srcLd = ldHost; }
        if (plan.source == HDM_KKT_SRC_DEVICE_M) { srcHost = nullptr; srcDev = Mdev; srcLd = ldDev; }
        factorised_from(plan.source);
        tiles_factorised_from(plan.load);
    }

private:
    void drop_tile_copy() { if (fact_tile_ == HDM_KKT_TILE_SRC_COPY) fact_tile_ = HDM_KKT_TILE_SRC_NONE; }
};

// ---- the load rule --------------------------------------------------------------------------
// Where M comes from and how it reaches the factor.  With the host mirror on, the host matrix is authoritative (the driver and
// the CPU cones may have touched it through kktDiag / kktMatElem); otherwise the device matrix is, plus the diagonal channel,
// which is added in place so that the Cholesky, the permuted load and the pivoted solver all see the same matrix.
// HKKTFactorize performs stage, commits (the pivoted solver reads the recorded source from the state), then loads and factors.
//
//  form  | mirror | requires | staging                                           | source   | load into factor | on pivot failure
//  ------+--------+----------+---------------------------------------------------+----------+------------------+-----------------
//  TILES | on     | --       | zero factor store; upload nnz values; scatter     | --       | (staged)         | fail, message
//        |        |          | into factor store at (rows, cols)                 |          |                  | names the row
//  TILES | off    | M valid  | fold channel if not folded                        | --       | load_M           | fail
//  CSC   | on     | --       | zero device M; upload nnz values; scatter into    | device M | see below        | switch to pivoted
//        |        |          | device M; M becomes valid                         |          |                  |
//  CSC   | off    | M valid  | fold channel if not folded                        | device M | see below        | switch to pivoted
//  DENSE | on     | --       | none                                              | host M,  | load_host        | switch to pivoted
//        |        |          |                                                   | ld = m   |                  |
//  DENSE | off    | M valid  | fold channel if not folded                        | device M | load_device      | switch to pivoted
//
// CSC, not permuted: load_device from device M.  CSC, permuted: with the mirror off, gather the pattern's entries from device M
// into the value buffer (with it on, staging left them there); zero the factor image; scatter at (prow, pcol); finish_load.
// DENSE and CSC once switched to the pivoted solver: load and Cholesky are replaced by the pivoted factorisation from the
// recorded source; staging still runs.  (The tile form's factorisation is an LDL' already: it never switches.)
// Bytes sent up: 8 nnz for an uploaded CSC, 8 m^2 for the dense mirror, 8 m for a folded channel.
inline HdmKktLoadPlan hdm_kkt_load_plan(const HdmKktState &st) {
    HdmKktLoadPlan p;
    if (!st.mirror_ && !st.m_valid_) return p;
    p.ok = true;
    const bool tiles = st.form_ == HDM_KKT_TILES;
    if (!st.mirror_) p.stage = st.chan_folded_ ? HDM_KKT_STAGE_NONE : HDM_KKT_STAGE_FOLD;
    else p.stage = tiles ? HDM_KKT_STAGE_CSC_TO_FACTOR : st.form_ == HDM_KKT_CSC ? HDM_KKT_STAGE_CSC_TO_M : HDM_KKT_STAGE_NONE;
    if (tiles) {
        p.load = st.mirror_ ? HDM_KKT_LOAD_STAGED : HDM_KKT_LOAD_TILES;
        return p;
    }
    p.source = (st.mirror_ && st.form_ == HDM_KKT_DENSE) ? HDM_KKT_SRC_HOST_M : HDM_KKT_SRC_DEVICE_M;
    p.on_pivot = st.indef_ ? HDM_KKT_PIVOT_FAIL : HDM_KKT_PIVOT_SWITCH;   // (already switched: nothing left to switch to)
    if (st.indef_) p.load = HDM_KKT_LOAD_PIVOTED;
    else if (p.source == HDM_KKT_SRC_HOST_M) p.load = HDM_KKT_LOAD_HOST;
    else if (st.form_ == HDM_KKT_CSC && st.permuted_) { p.load = HDM_KKT_LOAD_PERMUTED; p.gather = !st.mirror_; }
    else p.load = HDM_KKT_LOAD_DEVICE;
    return p;
}

// ---- the refined solve's matrix -------------------------------------------------------------
// What the residual b - M x of a refined solve (refine_rule.h) reads, from the state alone:
//
//  factorised source            | the residual reads                                | valid
//  -----------------------------+---------------------------------------------------+-------------------------------------------
//  device M (mirror off, or a   | that matrix in place: channel folded, CSC         | until the next build that is no corrector
//  CSC scattered into it)       | scattered, regularised -- what the factor saw     | build starts (it zeroes M): then NO_MATRIX
//  host M (dense with the       | a device copy of the loaded image, taken after    | until the next factorisation; exists only if
//  mirror on, HFpLinsysNumeric) | the load and before the factorisation             | refinement was on then: else NO_MATRIX
//  nothing factorised yet       | --                                                | NO_MATRIX
//  tile form, its switch off   | --                                                | NOT_AVAILABLE
//  tile form, mirror off        | the accumulation store HdmBsp::Mval in place:     | until the next build that is no corrector
//  (cap and switch on at        | channel folded, regularised -- what load_M copied | build starts (it zeroes the store): then
//  HKKTFactorize)               |                                                   | NO_MATRIX
//  tile form, mirror on         | a device copy of the factor store (ntiles tiles), | until the next factorisation; exists only if
//  (cap and switch on then)     | taken after the scatter and before the            | cap and switch were on then: else NO_MATRIX;
//                               | factorisation overwrites it                       | freed when either goes off
//
// The tile form is refined only when the step cap AND its own switch (HMiLinsysSetRefineTiles / HDSDP_MI355X_REFINE_TILES) are on:
// with the cap alone the answer stays NOT_AVAILABLE and nothing is recorded or allocated.  Its loop runs in the tile store's own
// (permuted, padded) order, so nothing is permuted per step.
// Permuted CSC: the factor holds P M P', the residual's matrix is in the driver's order: right-hand sides and corrections are
// permuted on the device (permute).  Once switched to the pivoted solver the factor is of the recorded source in the driver's
// order: corrections are the pivoted solver's (pivoted), nothing is permuted.
enum HdmRefineMatrix { HDM_REFINE_MAT_NONE = 0, HDM_REFINE_MAT_DEVICE_M, HDM_REFINE_MAT_COPY, HDM_REFINE_MAT_TILES_M, HDM_REFINE_MAT_TILES_COPY };
struct HdmRefineSource {
    HdmRefineMatrix matrix = HDM_REFINE_MAT_NONE;
    HdmRefineStatus why_none = HDM_REFINE_OFF;     // matrix == NONE: the status of the (unrefined) solve
    bool permute = false, pivoted = false;
};
inline HdmRefineSource hdm_kkt_refine_source(const HdmKktState &st) {
    HdmRefineSource r;
    if (st.refine_ == 0) return r;
    if (st.form_ == HDM_KKT_TILES) {
        if (!st.refine_tiles_) { r.why_none = HDM_REFINE_NOT_AVAILABLE; return r; }
        r.why_none = HDM_REFINE_NO_MATRIX;
        if (st.fact_tile_ == HDM_KKT_TILE_SRC_M_STORE && st.fact_dev_intact_) r.matrix = HDM_REFINE_MAT_TILES_M;
        else if (st.fact_tile_ == HDM_KKT_TILE_SRC_COPY) r.matrix = HDM_REFINE_MAT_TILES_COPY;
        else return r;
        r.why_none = HDM_REFINE_OFF;
        return r;
    }
    r.why_none = HDM_REFINE_NO_MATRIX;
    if (st.fact_src_ == HDM_KKT_SRC_DEVICE_M && st.fact_dev_intact_) r.matrix = HDM_REFINE_MAT_DEVICE_M;
    else if (st.fact_src_ == HDM_KKT_SRC_HOST_M && st.fact_copy_) r.matrix = HDM_REFINE_MAT_COPY;
    else return r;
    r.why_none = HDM_REFINE_OFF;
    r.pivoted = st.indef_;
    r.permute = st.permuted_ && !st.indef_;
    return r;
}
