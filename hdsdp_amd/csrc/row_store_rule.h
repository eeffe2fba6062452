// row_store_rule.h -- where the constraint rows of an SDP block live on the device, as one rule: resident or streamed, how many
// rows a streamed batch holds, whether the zero-suppressed sweep copy is made, and when that copy gives way to the work buffers.
// Pure host arithmetic: no HIP call, no allocation, no engine state -- the caller reads the device's memory figures
// (hipMemGetInfo) into HdmDeviceFacts, the store (engine_rows.h: MiRows) performs what the rule says.  DESIGN.md section 21.
// tests/test_row_store_rule_cpu.py compiles this header alone.
#pragma once
#include "env_switches.h"
#include "work_plan.h"
#include "dual_state.h"
#include <algorithm>
#include <cstddef>

// ---- the forms --------------------------------------------------------------------------------
//   RESIDENT   the A_L forms of all owned rows stay in device memory (with or without a sweep copy beside them)
//   GENERATED  synthetic family, streamed: nothing is kept, a batch is regenerated where the dense form is read (counter-based
//              generator: any range of matrices, any number of times, bit-identical); a sweep copy where it pays and fits
//   EXPANDED   ingested rows, streamed: the zero-suppressed copy is the ONLY image of the data, a batch is expanded from it.
//              The copy is therefore never freed and never yielded; switching it off only sends the sweeps through batches.
enum HdmRowForm { HDM_ROWS_RESIDENT = 0, HDM_ROWS_GENERATED, HDM_ROWS_EXPANDED };

// ---- constants --------------------------------------------------------------------------------
constexpr double HDM_ROWS_GIB = (double) (1L << 30);
// a generous bound of what a build's intermediates and Gram slabs take beside the rows (work_plan.h: 32 GiB of intermediates,
// one buffer with the slabs on one device, up to 8 GiB of slabs of their own on a shard)
constexpr double HDM_ROWS_WORK_CAP_BYTES = 41.0 * HDM_ROWS_GIB;
// slack beside the Schur matrix, its factor and its inverse blocks: at n = 2000, m = 8000 the resident form comes to 285 of the
// 287 GiB a fresh MI355X shows -- it has run, but nothing else may be on the device then
constexpr double HDM_ROWS_SCHUR_SLACK_BYTES = 16.0 * HDM_ROWS_GIB;
// a shard compares against this share of the device's capacity (what a fresh device shows as free)
constexpr double HDM_ROWS_CAPACITY_SHARE = 0.97;
// the congruence intermediates a sweep copy must leave room for: HdmKnobs::tcap_gib's default
constexpr double HDM_ROWS_T_CAP_BYTES = 32.0 * HDM_ROWS_GIB;
// a sweep copy made by the cost rule is dropped when over this share of the stored positions is non-zero
constexpr double HDM_SWEEP_COPY_MAX_FILL = 0.6;

// ---- the facts --------------------------------------------------------------------------------
struct HdmRowFacts {
    int n = 0, n16 = 0;        // block dimension, rounded up to 16
    long m = 0, mloc = 0;      // constraints of the problem, rows owned here
    int world = 1;             // ranks the rows are dealt over
    long astride = 0, R = 0;   // elements per stored row, rows of the segment-ordered Gram matrix (work_plan.h: HdmLayout)
    size_t exch_bytes = 0;     // hdm_exchange_bytes of the layout
    bool synthetic = false;
    bool gemm_path = true;     // the block is on the congruence + Gram path (the only one whose rows may be streamed)
};
static inline HdmRowFacts hdm_row_facts(const HdmLayout &L, int n, long m, long mloc, bool synthetic, bool gemm_path) {
    HdmRowFacts f;
    f.n = n; f.n16 = L.n16; f.m = m; f.mloc = mloc; f.world = L.world; f.astride = L.astride; f.R = L.R;
    f.exch_bytes = hdm_exchange_bytes(L); f.synthetic = synthetic; f.gemm_path = gemm_path;
    return f;
}
struct HdmDeviceFacts {
    bool known = false;        // the two figures could be read
    size_t free_bytes = 0, total_bytes = 0;
};

// ---- resident or streamed ---------------------------------------------------------------------
// Resident needs the skyline storage of all owned rows NEXT TO what a build takes -- the transformed rows, intermediates / Gram
// slabs, the Schur matrix with its factor and some slack; if the device does not have that, the rows are made per batch instead.
// One device: against what is FREE now (whatever else lives on the device counts).  A shard of a sharded block (process per GPU
// or device group): against the device's CAPACITY, so that every rank of a job on identical devices takes the same decision --
// streaming changes the launch staging, and ranks that disagreed would run differently labelled, differently timed steps (equal
// results); a resident allocation that then fails is an error with a message.
// HDSDP_MI355X_STREAM_A=1 forces streaming (tests run small blocks both ways), 0 forbids it.
static inline double hdm_rows_resident_need(const HdmRowFacts &f) {
    const double rows = (double) std::max(1L, f.mloc);
    const double afull = 8.0 * (double) f.astride * rows;
    const double ahat = (double) f.exch_bytes;
    const double work = std::min(HDM_ROWS_WORK_CAP_BYTES, std::max(8.0 * (double) f.n16 * f.n16 * std::min(rows, 1024.0),
                                                                   8.0 * (double) f.R * f.R * 8.0));
    const double schur = 3.0 * 8.0 * (double) f.m * f.m + HDM_ROWS_SCHUR_SLACK_BYTES;
    return afull + ahat + work + schur;
}
static inline bool hdm_rows_stream(const HdmRowFacts &f, const HdmDeviceFacts &d, HdmEnvInt stream_a) {
    if (!f.gemm_path) return false;
    bool stream = false;
    if (d.known)
        stream = hdm_rows_resident_need(f) > (f.world > 1 ? HDM_ROWS_CAPACITY_SHARE * (double) d.total_bytes : (double) d.free_bytes);
    if (stream_a.set) stream = (int) stream_a.value != 0;
    return stream && f.mloc > 0;
}
// rows of a streamed batch = what one congruence launch takes: HDM_BC clamped to at least 1 here, launches evened out as the
// plan's are (work_plan.h: HdmKnobs::bc_max says which clamp the plan applies)
static inline long hdm_rows_batch(long mloc, long bc_max) { return hdm_even_out(mloc, std::max(1L, bc_max)); }

// ---- the sweep copy ---------------------------------------------------------------------------
// The zero-suppressed copy of the constraint data (schur.h: HdmZs) that the S / dS sweeps and the corrector's dot products read:
// made once, when the block's data has arrived (cone creation -- format preparation like the unpacking into A_L form; the two
// passes and the 14 GB allocation take 0.3-0.8 s at n = m = 2000, which does not belong into the first line search), for blocks
// whose sweep costs something (dual_state.h: hdm_sweep_costs, 16 MiB of constraint data or more) unless over 60 % of the stored
// positions are non-zero or the memory is not there (then the sweeps read the dense storage).
// HDSDP_MI355X_ZS=0: never; 2 or more: any size, any fill.
struct HdmSweepCopyRule { bool build; double max_fill; };
static inline HdmSweepCopyRule hdm_sweep_copy_rule(const HdmRowFacts &f, bool has_rows, HdmEnvInt zs_env) {
    const int env = zs_env.value_or(1);
    const double max_fill = env >= 2 ? 1.0 : HDM_SWEEP_COPY_MAX_FILL;
    if (!has_rows || f.mloc <= 0 || !env || !(env >= 2 || hdm_sweep_costs(f.mloc, f.n))) return {false, max_fill};
    return {true, max_fill};
}
// The copy is made at creation, before the work buffers of the first build: it must never be the reason they come out smaller.
// If what is free does not cover a generous bound of what the builders take, the copy goes (the sweeps then read the dense
// storage) -- except where it is the only image of the data.
static inline bool hdm_sweep_copy_yields(HdmRowForm form, bool copy_in_use, const HdmRowFacts &f, const HdmDeviceFacts &d) {
    if (form == HDM_ROWS_EXPANDED || !copy_in_use || !d.known) return false;
    const double rows = (double) std::max(1L, f.mloc);
    const double nn = 8.0 * (double) f.n16 * f.n16;
    const double want = std::min(HDM_ROWS_T_CAP_BYTES, nn * rows) + (double) f.exch_bytes + HDM_ROWS_WORK_CAP_BYTES;
    return (double) d.free_bytes < want;
}
