// work_plan.h -- how much work space a dense block's Schur build on the congruence + Gram path takes: the block's layout, the
// environment knobs, and the plan (constraints per congruence launch, K splits and slabs of the Gram product, buffer sizes).
// Pure host arithmetic on integers and doubles: no HIP call, no allocation, no engine state, no I/O -- the engine allocates
// what this header says (engine_cone.h: cone_alloc_common, cone_alloc_gemm_work; row_store_rule.h: hdm_rows_batch for a streamed block's batch buffer), and
// HMiWorkPlanQuery hands the same numbers to callers without a device (hdsdp_amd/dist.py: ShardPlan.hbm_bytes).
#pragma once
#include "env_switches.h"
#include "gemm_geom.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdlib>

// ---- layout ---------------------------------------------------------------------------------
struct HdmLayout {
    int world;       // ranks the constraint rows are dealt over (row i on rank i % world)
    int n16, nblk;   // n rounded up to 16 (MFMA sub-tile), n16 / 16
    long npb;        // p-blocks of the blocked congruence layout: nblk (nblk + 1) / 2 * 16
    long npb_loc;    // p-blocks per rank (K range of the local Gram part)
    int Lr;          // rows per segment of the Gram operand (local rows + 3 augmented, padded)
    long R;          // world * Lr: rows of the segment-ordered Gram matrix
    long astride;    // elements per constraint matrix in skyline storage (gemm_geom.h)
};
// `maxloc`: the most rows any rank owns -- ceil(m / world), or on one device the rows that are not zero on the block (the
// caller's choice: cone_alloc_common)
static inline HdmLayout hdm_layout(int n, int world, int maxloc) {
    HdmLayout L;
    L.world = world;
    L.n16 = (int) hdm_roundup(n, 16);
    L.nblk = L.n16 / 16;
    L.npb = (long) L.nblk * (L.nblk + 1) / 2 * 16;
    L.npb_loc = (L.npb + world - 1) / world;
    L.Lr = (world == 1) ? (int) hdm_roundup(maxloc + 3, 8) : (int) hdm_roundup(maxloc + 3, HDM_TILE);
    L.R = (long) world * L.Lr;
    L.astride = hdm_sky_size(L.n16);
    return L;
}
static inline long hdm_rows_of_rank(int m, int world, int rank) { return rank < m ? (m - rank + world - 1) / world : 0; }
// The exchange buffers: [world * npb_loc][Lr][16] doubles of congruence output each (HDM_OPERAND_PAD_DOUBLES of slack behind
// it not counted); one device reads the Gram operand where the congruence wrote it, a sharded block has a send and a receive side.
static inline size_t hdm_exchange_doubles(const HdmLayout &L) { return (size_t) L.world * L.npb_loc * L.Lr * 16; }
static inline size_t hdm_exchange_bytes(const HdmLayout &L) { return sizeof(double) * hdm_exchange_doubles(L) * (L.world == 1 ? 1 : 2); }

// ---- operand slack and spans ------------------------------------------------------------------
// Slack (bytes) appended to every device buffer that the role 1-3 GEMM kernels read as an operand: their staging loads
// carry no row mask (gemm_tile.h, SStager::load_nomask), so the last tile of the last matrix in a buffer may read up
// to 127 rows past its end.  `ld` = elements between consecutive rows (K-major) or 1 (M-major).
static inline size_t hdm_operand_pad(long ld) { return (size_t) 128 * (size_t) (ld < 16 ? 16 : ld) * 8 + 4096; }
#define HDM_OPERAND_PAD_DOUBLES 8192   /* the same slack for the [p-block][row][16] congruence output, in doubles */
// Elements readable from the start of each operand buffer of the Schur build, slack included -- what a role launch vouches for
// (gemm_calls.h), never more than the allocation: the intermediates T of `Bc` matrices, the factor inverse (npad x npad), a
// buffer of `rows` skyline matrices (the resident rows, a regenerated batch, CL), an exchange buffer, the LP cone's dense buffer.
static inline long hdm_t_span(const HdmLayout &L, long Bc) { return (long) L.n16 * L.n16 * Bc + (long) (hdm_operand_pad(L.n16) / sizeof(double)); }
static inline long hdm_linv_span(long npad) { return npad * npad; }
static inline long hdm_afull_span(const HdmLayout &L, long rows) { return L.astride * rows + (long) (hdm_operand_pad(L.n16) / sizeof(double)); }
static inline long hdm_exchange_span(const HdmLayout &L) { return (long) hdm_exchange_doubles(L) + HDM_OPERAND_PAD_DOUBLES; }
// the LP cone's dense buffer W: [kc / 16][mpad][16] doubles (engine_lp.h: lp_build_dense_buffer)
static inline long hdm_lp_span(int kc, int mpad) { return (long) (kc / 16) * mpad * 16 + HDM_OPERAND_PAD_DOUBLES; }

// ---- knobs ----------------------------------------------------------------------------------
// The A/B and test switches of the plan (include/hdsdp_mi355x.h lists them), as the environment states them at the call
// (env_switches.h: NOW).
struct HdmKnobs {
    long tcap_gib = 32;             // HDM_TCAP_GIB: GiB of congruence intermediates
    // HDM_BC, as written (not clamped here).  The plan takes min(memory bound, bc_max) and clamps THAT to at least 1
    // (hdm_work_plan); the batch of regenerated rows clamps bc_max itself to at least 1 before it evens the launches out
    // (row_store_rule.h: hdm_rows_batch).  Both come to 1 row per launch for HDM_BC <= 0.
    long bc_max = 1024;
    long gram_kstages = 0;          // HDM_GRAM_KSTAGES: stages per Gram job at any size (>= 1); 0 = by size.  One device only.
    bool nsplit_set = false;        // HDM_NSPLIT: the slab count, within [1, kblocks / 16]
    long nsplit = 0;
    bool share_t_slabs = true;      // HDM_SHARE_T_SLABS=0: intermediates and slabs in two buffers on one device too
    bool gram_queue_global = true;  // HDM_GRAM_QUEUE=0: one job queue per XCD over the splits x, x + 8, ...
};
static inline HdmKnobs hdm_knobs_from_env() {
    HdmKnobs k;
    if (const HdmEnvInt e = hdm_env_int<ENV_TCAP_GIB>(); e.set) k.tcap_gib = e.value;
    if (const HdmEnvInt e = hdm_env_int<ENV_BC>(); e.set) k.bc_max = e.value;
    if (const HdmEnvInt e = hdm_env_int<ENV_GRAM_KSTAGES>(); e.set) k.gram_kstages = std::max(1L, e.value);
    if (const HdmEnvInt e = hdm_env_int<ENV_NSPLIT>(); e.set) { k.nsplit_set = true; k.nsplit = e.value; }
    k.share_t_slabs = hdm_env_on<ENV_SHARE_T_SLABS>();
    k.gram_queue_global = hdm_env_on<ENV_GRAM_QUEUE>();
    return k;
}

// ---- plan -----------------------------------------------------------------------------------
struct HdmWorkPlan {
    long Bc;                 // constraints per congruence launch, launches evened out
    long nsplit, nslab;      // K splits of the Gram product; slabs they are summed into (nslab <= nsplit: the splits run in
                             // groups of nslab, group after group accumulating -- engine_build.h: gram_range)
    long rule_splits;        // the split count the K-length rule asks for whatever the slabs (0: short K range, splits = slabs)
    bool shared_ts;          // T and the slabs are ONE buffer of the larger size
    bool gram_queue_global;
    size_t t_bytes, slab_bytes, exch_bytes, gm_bytes;   // payloads (operand slack not counted): Bc n16^2, nslab R^2, both exchange sides, R^2 doubles
};

// `rows` in launches of at most `bmax`, all of the same size up to one row: 2000 rows at 1024 -> 2 x 1000, a rank's 250 -> one
// launch (rows, bmax >= 1)
static inline long hdm_even_out(long rows, long bmax) {
    const long launches = (rows + bmax - 1) / bmax;
    return (rows + launches - 1) / launches;
}

// Stages (16 k) per (split, tile) job of the Gram product, the smaller of two bounds (at least 96 -- prologue + epilogue under
// 4 % -- at most 2048):
//  * the split's operand panel (R rows) fills the memory-side cache: 2^28 B / (128 B x R);
//  * what a job costs beside its K loop.  Per job about two stage times of prologue + epilogue (a share 2 / kst of its time),
//    and at the end of the launch the 512 workgroups run dry over about half a job (a share 256 kst / (tiles x kblocks) of the
//    launch): least at kst = sqrt(tiles x kblocks / 128) -- 365 stages at n = m = 2000 (346 splits), the floor of 96 at
//    n = m = 1000 (336 splits, the count of rounds 2-4), beyond the cache bound at m = 8000.
static inline long hdm_gram_kstages(const HdmLayout &L, long tiles) {
    long kst = (long) ((double) (1L << 28) / (128.0 * (double) L.R));
    kst = std::min(kst, (long) std::sqrt((double) tiles * (double) L.npb_loc / 128.0));
    return std::max(96L, std::min(kst, 2048L));
}

static inline void hdm_plan_set_slabs(HdmWorkPlan &p, const HdmLayout &L, long ns) {
    p.nslab = ns;
    p.nsplit = std::max(p.rule_splits, ns);
    p.slab_bytes = sizeof(double) * (size_t) L.R * L.R * (size_t) ns;
}
// the slabs are the one allocation that is a tuning choice: when it fails, half as many (a multiple of 8, at least 8; the
// split count stays where the K-length rule put it).  false: nothing left to halve
static inline bool hdm_plan_halve_slabs(HdmWorkPlan &p, const HdmLayout &L) {
    if (p.nslab <= 8) return false;
    hdm_plan_set_slabs(p, L, std::max(8L, (p.nslab / 2) & ~7L));
    return true;
}

// `mloc` rows owned; `streamed`: the rows are regenerated in batches of `Bs` (one congruence launch per batch); `bc_cap`: a
// further bound on the batch (half the last one, after an allocation of T has failed: the slab count follows the batch).
static inline HdmWorkPlan hdm_work_plan(const HdmLayout &L, long mloc, bool streamed, long Bs, const HdmKnobs &k, long bc_cap = LONG_MAX) {
    HdmWorkPlan p;
    const double nn = sizeof(double) * (double) L.n16 * L.n16;
    // batch size: as many constraints per launch as 32 GiB of intermediates allow, at most 1024 (each launch pays a
    // dispatch ramp and a tail: measured step time 400.9 / 396.8 / 393.2 / 393.2 ms at 256 / 512 / 1000 / 2000 per launch on
    // one box).  The kernel's XCD-local decode pads a batch to a multiple of 8 itself.
    long bcmax = k.bc_max;
    if (streamed) bcmax = std::min(bcmax, Bs);
    const long bc = std::max(1L, std::min({(long) (((double) k.tcap_gib * (1L << 30)) / nn), bcmax, bc_cap}));
    p.Bc = hdm_even_out(std::max(1L, mloc), bc);
    p.t_bytes = sizeof(double) * (size_t) L.n16 * L.n16 * (size_t) p.Bc;
    p.exch_bytes = hdm_exchange_bytes(L);
    p.gm_bytes = sizeof(double) * (size_t) L.R * L.R;
    // Gram split-K.  The product over the packed index (K = 8 n(n+1) p-blocks of 16) is cut into K splits; a job is (split, tile),
    // a persistent workgroup draws jobs from ONE queue in split order (HdmGemmArgs.queue_global), partial sums go to slabs that
    // are reduced in fixed order.  What sets the split length (round 5, profiles/r05_a_8000_*, r05_b_*, r05_c_*): the Gram
    // kernel is matrix-pipe bound at whatever clock the board's power limit leaves, and what costs power beside the MFMAs is
    // HBM traffic.  A tile re-reads its two operand panels from the fabric for every job (L2 holds a few stages of them), so the
    // fabric sees 13-60 x the algorithmic bytes -- which is harmless as long as they are served by the 256 MiB memory-side cache,
    // i.e. as long as the operand bytes all workgroups of the chip are working on fit there.  With one queue in split order that
    // is the panel of ONE split (+ the next one's beginning): R rows x k_chunk x 8 B.  At n = 2000, m = 8000 the former form (80
    // splits of 25 000 k, one per XCD in flight) had 8 x 1.6 GB in use: 7.6 TB of HBM reads per Gram product, 99.7 % MFMA busy at
    // 2.11 GHz, 68 TFLOP/s; with 256 stages (4096 k, 262 MB) per job 2.37 GHz and 75.5 TFLOP/s (1698 vs 1877 ms, same box;
    // 192 / 384 / 512 stages: +0.7 / +2.4 / +5.7 %).  More splits than slabs: the splits run in groups of nslab, launch after
    // launch, group g accumulating into the slabs of group g - 1 (gram_all); 16 slabs cost 0.4 % against 80.
    // Short K ranges (small problems): among the multiples of 8 pick the split count whose last scheduling round is fullest.
    const long RT = (L.R + HDM_TILE - 1) / HDM_TILE;
    const long tiles = RT * (RT + 1) / 2;
    const long kblocks = L.npb_loc;
    const double slab_bytes = sizeof(double) * (double) L.R * L.R;
    const long slab_cap = std::max(1L, (long) ((4LL << 30) / slab_bytes));  // <= 4 GiB of slabs
    const long kcap = std::max(1L, kblocks / 64);
    long ns = 1;
    double best = -1.0;
    for (long cand = 1; cand <= 64 && cand <= slab_cap && cand <= kcap; ++cand) {
        if (cand > 8 && cand % 8) continue;
        const double rounds = (double) (tiles * cand) / 512.0;
        double eff = rounds / std::ceil(rounds);
        if (rounds < 2.0) eff *= 0.5 + 0.25 * rounds;  // too few workgroups to hide the tail
        if (cand < 8 && kcap >= 8 && slab_cap >= 8) eff *= 0.5;
        if (eff > best + 1e-9) { best = eff; ns = cand; }
    }
    // long K ranges: >= 96 k blocks (of 16) per job, and at least 128 such jobs' worth of K
    p.rule_splits = 0;
    const bool long_k = kblocks / 96 >= 128;
    if (L.world == 1 && (long_k || k.gram_kstages)) {
        const long kst = k.gram_kstages ? k.gram_kstages : hdm_gram_kstages(L, tiles);
        p.rule_splits = std::max(8L, (kblocks + kst - 1) / kst);
        // slabs: what fits the buffer the intermediates have anyway (one device: the two share it), at least 8 GiB worth, at least 8
        const long cap8 = std::max(8L, (long) (std::max((double) (8LL << 30), nn * (double) p.Bc) / slab_bytes));
        ns = std::max(ns, std::min(p.rule_splits, cap8));
    } else if (long_k) {
        // sharded block: the exchange pieces are whole groups of splits whose launches overlap the transfers
        // (engine_build.h), so the split count is a multiple of 8 (at most 1024), of the length the one-device rule gives
        // (HDM_GRAM_KSTAGES is not honoured here).  The slabs themselves are at most 8 GiB: a piece's splits run in groups of
        // them, piece after piece accumulating (gram_range)
        const long kst = hdm_gram_kstages(L, tiles);
        const long big = std::min(1024L, ((kblocks + kst - 1) / kst + 7) & ~7L);
        if (big > ns) {
            p.rule_splits = big;
            ns = std::max(ns, std::min(big, std::max(8L, (long) ((8LL << 30) / slab_bytes))));
        }
    }
    if (k.nsplit_set) ns = std::max(1L, std::min(k.nsplit, kblocks / 16));   // A/B knob: the slab count
    hdm_plan_set_slabs(p, L, ns);
    // One GPU: the congruence intermediates T are dead by the time the Gram product writes its split-K slabs, so the two
    // share ONE buffer (the larger of the two sizes: 33 GB instead of 32 + 33 GB at n = m = 2000).  The only thing step 2
    // reads of T that step 1 does not write is the strict upper triangle of T's diagonal tiles: with the buffer shared
    // it is re-zeroed before every batch (hdm_zero_diag_upper, 1 GB of stores per 1000 matrices) instead of once at
    // allocation.  Sharded builds keep them apart: there the Gram splits of the early exchange pieces run while step 2
    // still reads T for the later ones.
    p.shared_ts = (L.world == 1) && k.share_t_slabs;
    p.gram_queue_global = k.gram_queue_global;
    return p;
}
