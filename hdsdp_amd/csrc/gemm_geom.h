// gemm_geom.h -- the geometry of the fp64 MFMA GEMM family, stated once for the kernels (gemm_tile.h), their launcher
// (gemm_f64.hip) and the engine (engine_build.h): which tiles a launch runs and in what order, a tile's K range and class, the
// MFMAs its stage sequence executes, how far its unmasked loads reach, the two work shares of congruence step 2, and the 16 x 16
// blocked layout of the congruence output.
// Pure arithmetic on integers: no HIP header, no allocation, no state.  Under hipcc every function is __host__ __device__;
// tests/test_gemm_geom_cpu.py compiles this header alone with the host compiler.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

// (always inlined in device code: the kernels' register budget leaves no room for a call, and a tile's class must fold with
// the kernel's compile-time role)
#if defined(__HIPCC__)
#define HDM_HD __host__ __device__ __attribute__((always_inline))
#else
#define HDM_HD
#endif

#define HDM_TILE 128          // workgroup tile edge of the fp64 MFMA GEMM family
#define HDM_BK 16             // k-depth of one LDS stage
#define HDM_SUB 16            // MFMA sub-tile edge (v_mfma_f64_16x16x4_f64)

static inline long hdm_roundup(long x, long q) { return (x + q - 1) / q * q; }

enum HdmKLimit { HDM_KLIM_NONE = 0, HDM_KLIM_BY_M = 1, HDM_KLIM_BY_N = 2, HDM_KLIM_BAND = 3 };  // BAND: k in [tn*128, (tm+1)*128)
enum HdmEpilogue {
    HDM_EPI_STORE = 0,    // C = alpha*acc + beta*C, column-major
    HDM_EPI_BLOCKED = 1,  // congruence output: 16x16-blocked lower triangle, sqrt(2) off-diagonal blocks
    HDM_EPI_SLAB = 2      // split-K partial sums into slab[blockIdx.z]
};
// kernel roles: a distinct kernel symbol per role so that rocprofv3 --stats separates the hot-path
// launches (congruence step 1/2, Gram) from the small Cholesky/TRTRI helper GEMMs
// HDM_ROLE_CONG2D is internal to the launcher: a role-2 launch is issued as two kernels, the full diagonal tiles (computed
// as P + P^T from one product, gemm_tile.h) and everything else; callers never ask for it
enum HdmRole { HDM_ROLE_GENERIC = 0, HDM_ROLE_CONG1 = 1, HDM_ROLE_CONG2 = 2, HDM_ROLE_GRAM = 3, HDM_ROLE_CONG2D = 4, HDM_NROLES = 5 };

// "Skyline" storage of a matrix in A_L form (strict lower triangle + half the diagonal; the constraint matrices and the
// objective as the congruence reads them): only the 128-column panels from their diagonal block downwards are stored --
// panel t holds rows 128 t .. n-1 of columns 128 t .. 128 t + 127 as a plain column-major (n - 128 t) x 128 matrix, the
// panels follow each other.  53 % of the square at n = 2000 (34 GB instead of 64 GB for 2000 matrices); inside a panel
// every column is contiguous and 128-byte aligned (n is a multiple of 16), so tile loads stay full lines, and the one
// GEMM operand that reads A_L (congruence step 1, B side: rows = columns of panel tn, k = rows from the panel's top)
// sees panel tn as an ordinary K-major matrix with leading dimension n - 128 tn.  The strict upper triangle of each
// panel's top block is stored and stays zero.
HDM_HD inline long hdm_sky_panel(int t, int n) { return 128L * ((long) t * n - 64L * t * (t - 1)); }   // start of panel t
HDM_HD inline long hdm_sky_off(int i, int j, int n) {   // element (i, j), i >= 128 * (j / 128)
    const int t = j >> 7;
    return hdm_sky_panel(t, n) + (long) (j & 127) * (n - 128 * t) + (i - 128 * t);
}
HDM_HD inline long hdm_sky_size(int n) {                // elements of one matrix
    const int t = (n + 127) / 128 - 1;
    const long w = n - 128L * t;
    return hdm_sky_panel(t, n) + w * w;
}

// ---- the launch, as far as geometry goes ------------------------------------------------------
struct HdmTileGeom {
    int M, N, K;
    int klimit;                  // HdmKLimit
    int lower_only;
    unsigned long long colmask;  // as the caller wrote it (hdm_colmask_effective says what it means)
    int role;                    // HdmRole
    int slab;                    // split-K launch (HDM_EPI_SLAB): batch entry z is K split z
    int batch;
    long k_base, k_chunk;
    int npass;                   // products accumulated into one tile (2: the SYR2K form)
};
struct HdmTile { int tm, tn; };
struct HdmKRange { long kbeg, kend; };

HDM_HD constexpr int hdm_ntiles(int x) { return (x + HDM_TILE - 1) / HDM_TILE; }
// 16-row sub-tiles of tile row tm that hold rows of the matrix (8 or more: a full tile)
HDM_HD constexpr int hdm_valid_subrows(int M, int tm) { return (M - tm * HDM_TILE + 15) >> 4; }
// the cell-dealt short tiles exist for 4..7 sub-tile rows: fewer run as 4 (zeros from the stager, masked by the epilogue)
HDM_HD constexpr int hdm_cell_rows(int rv) { return rv < 4 ? 4 : rv; }
// a tile-column mask has 64 bits: a launch with more tile columns runs them all
HDM_HD constexpr bool hdm_colmask_honoured(int NT) { return NT <= 64; }
HDM_HD constexpr unsigned long long hdm_colmask_effective(unsigned long long mask, int NT) { return hdm_colmask_honoured(NT) ? mask : 0ULL; }

HDM_HD constexpr bool hdm_tile_selected(const HdmTileGeom &g, int tm, int tn) {
    const unsigned long long mask = hdm_colmask_effective(g.colmask, hdm_ntiles(g.N));
    return !((g.lower_only || g.klimit == HDM_KLIM_BAND) && tm < tn) && !(mask && !((mask >> tn) & 1ULL));
}
// a diagonal tile with all 128 rows: the tiles congruence step 2 runs as P + P^T in a launch of their own
HDM_HD constexpr bool hdm_full_diag(int M, int tm, int tn) { return tm == tn && hdm_valid_subrows(M, tm) >= 8; }
// subset 0: every selected tile; 1: the full diagonal tiles; 2: all the others
HDM_HD constexpr bool hdm_tile_in_subset(const HdmTileGeom &g, int tm, int tn, int subset) {
    return hdm_tile_selected(g, tm, tn) && (!subset || (subset == 1) == hdm_full_diag(g.M, tm, tn));
}
// K blocks a tile runs, up to the split-K cut: what the launch order sorts by
HDM_HD constexpr long hdm_tile_weight(int klimit, int tm, int tn) {
    return klimit == HDM_KLIM_BY_M ? tm + 1 : klimit == HDM_KLIM_BY_N ? tn + 1 : klimit == HDM_KLIM_BAND ? tm - tn + 1 : 1;
}
// The tiles of a launch in launch order: heaviest first, tiles of equal weight in row-major order.
// (A Z-order curve over (tm, tn), meant to let neighbours in the list share a column panel as well as a row panel in L2, RAISED
// the Gram kernel's fabric traffic from 391 to 425 GB per launch and changed no time -- same box, round 2)
inline std::vector<HdmTile> hdm_tile_list(const HdmTileGeom &g, int subset) {
    std::vector<std::pair<long, HdmTile>> v;
    for (int tm = 0; tm < hdm_ntiles(g.M); ++tm)
        for (int tn = 0; tn < hdm_ntiles(g.N); ++tn)
            if (hdm_tile_in_subset(g, tm, tn, subset)) v.push_back({hdm_tile_weight(g.klimit, tm, tn), HdmTile{tm, tn}});
    std::stable_sort(v.begin(), v.end(), [](const auto &x, const auto &y) { return x.first > y.first; });
    std::vector<HdmTile> h(v.size());
    for (size_t i = 0; i < v.size(); ++i) h[i] = v[i].second;
    return h;
}

HDM_HD constexpr long hdm_min(long a, long b) { return a < b ? a : b; }
// k range of tile (tm, tn) for batch entry z: the triangular operand's cut, then the split-K cut
HDM_HD constexpr HdmKRange hdm_tile_krange(int K, int klimit, bool slab, long k_base, long k_chunk, int tm, int tn, int z) {
    long kbeg = 0, kend = K;
    if (klimit == HDM_KLIM_BY_M) kend = hdm_min((long) K, (long) (tm + 1) * HDM_TILE);
    if (klimit == HDM_KLIM_BY_N) kend = hdm_min((long) K, (long) (tn + 1) * HDM_TILE);
    if (klimit == HDM_KLIM_BAND) { kbeg = (long) tn * HDM_TILE; kend = hdm_min((long) K, (long) (tm + 1) * HDM_TILE); }
    if (slab) {
        kbeg = k_base + (long) z * k_chunk;
        kend = hdm_min(kend, kbeg + k_chunk);
    }
    return {kbeg, kend};
}
HDM_HD constexpr HdmKRange hdm_tile_krange(const HdmTileGeom &g, int tm, int tn, int z) {
    return hdm_tile_krange(g.K, g.klimit, g.slab != 0, g.k_base, g.k_chunk, tm, tn, z);
}
// stages (16 k) of that range, all products
HDM_HD constexpr long hdm_tile_stages(const HdmTileGeom &g, int tm, int tn, int z) {
    const HdmKRange r = hdm_tile_krange(g, tm, tn, z);
    const long nst = r.kend / HDM_BK - r.kbeg / HDM_BK;
    return (nst < 0 ? 0 : nst) * g.npass;
}

// ---- a tile's class ---------------------------------------------------------------------------
// Roles 1-3 (generic launches run every tile through their masked loop, class MAIN).  hdm_tile_class asks the two predicates in
// the kernel's order.  (The kernel keeps the two predicates, its K range and hdm_cell_rows -- as an if-chain -- written out,
// each beside a pointer to here: through these functions the compiler gives the big kernels other code.)
enum HdmTileKind {
    HDM_CLS_DIAG_FULL,    // diagonal tile of a lower-only product, 36 cells dealt 9 per wave
    HDM_CLS_DIAG_SHORT,   // the last diagonal tile with RV < 8 sub-tile rows: RV (RV + 1) / 2 cells
    HDM_CLS_EDGE,         // bottom-edge tile below the diagonal: 8 RV cells
    HDM_CLS_SYMDIAG,      // step 2's full diagonal tile as P + P^T (role HDM_ROLE_CONG2D): one product over all 64 cells
    HDM_CLS_MAIN          // 2 x 2 wave quadrants, 16 accumulators per wave
};
struct HdmTileClass { HdmTileKind kind; int rv, RV; };   // valid sub-tile rows, and the compile-time count the cell paths run
HDM_HD constexpr bool hdm_tile_is_cell_diag(int role, int lower_only, int tm, int tn) {
    return role != HDM_ROLE_CONG2D && lower_only && tm == tn;
}
HDM_HD constexpr bool hdm_tile_is_edge(int role, int M, int N, int tm, int tn) {
    return role != HDM_ROLE_CONG2D && tm != tn && tm * HDM_TILE + HDM_TILE > M && tn * HDM_TILE + HDM_TILE <= N;
}
HDM_HD constexpr HdmTileClass hdm_tile_class(const HdmTileGeom &g, int tm, int tn) {
    const int rv = hdm_valid_subrows(g.M, tm) < 8 ? hdm_valid_subrows(g.M, tm) : 8;
    if (g.role == HDM_ROLE_GENERIC) return {HDM_CLS_MAIN, rv, 8};
    if (hdm_tile_is_cell_diag(g.role, g.lower_only, tm, tn))
        return hdm_full_diag(g.M, tm, tn) ? HdmTileClass{HDM_CLS_DIAG_FULL, rv, 8} : HdmTileClass{HDM_CLS_DIAG_SHORT, rv, hdm_cell_rows(rv)};
    if (hdm_tile_is_edge(g.role, g.M, g.N, tm, tn)) return {HDM_CLS_EDGE, rv, hdm_cell_rows(rv)};
    return {g.role == HDM_ROLE_CONG2D ? HDM_CLS_SYMDIAG : HDM_CLS_MAIN, rv, 8};
}

// ---- the MFMAs a tile executes ----------------------------------------------------------------
// A stage is 16 k = 4 k-steps; in a main tile each of the 4 waves owns 4 x 4 sub-tiles (row sub-tiles 2 i + wm, column
// sub-tiles 2 j + wn) and runs the live range j in [jlo, jhi], i in [ilo, 3] of them: one MFMA per pair and k-step.  Stages
// run in pairs (the LDS buffer index is a compile-time constant), and a K block of 128 is 4 pairs.
struct HdmLive { int jlo, jhi, ilo; };
constexpr int HDM_KBLOCK_PAIRS = HDM_TILE / HDM_BK / 2;
constexpr HdmLive HDM_LIVE_FULL = {0, 3, 0};
// In the congruence kernels the K block on an operand's diagonal is half zeros: in stage s of it whole 16-row sub-tiles of the
// operand are structurally zero, and a stage pair runs what is live in its first stage (pair p: s = 2 p, a wave's sub-tile p):
//   step 2, last block, B side lower triangular (both products): column sub-tiles < s are dead
constexpr HdmLive HDM_LIVE_CONG2_LAST[HDM_KBLOCK_PAIRS] = {{0, 3, 0}, {1, 3, 0}, {2, 3, 0}, {3, 3, 0}};
//   step 2's P + P^T tiles, last block, both operands on their diagonal: row and column sub-tiles < s are dead
constexpr HdmLive HDM_LIVE_CONG2D_LAST[HDM_KBLOCK_PAIRS] = {{0, 3, 0}, {1, 3, 1}, {2, 3, 2}, {3, 3, 3}};
//   step 1, first block, A_L on the B side (k >= column): column sub-tiles > s are dead
constexpr HdmLive HDM_LIVE_CONG1_FIRST[HDM_KBLOCK_PAIRS] = {{0, 0, 0}, {0, 1, 0}, {0, 2, 0}, {0, 3, 0}};
//   step 1, last block, Linv on the A side (k <= row): row sub-tiles < s are dead
constexpr HdmLive HDM_LIVE_CONG1_LAST[HDM_KBLOCK_PAIRS] = {{0, 3, 0}, {0, 3, 1}, {0, 3, 2}, {0, 3, 3}};

HDM_HD constexpr int hdm_live_per_kstep(HdmLive l) { return (l.jhi - l.jlo + 1) * (4 - l.ilo); }        // MFMAs of one wave
HDM_HD constexpr long hdm_pair_mfmas(HdmLive l) { return 2L * 4 * 4 * hdm_live_per_kstep(l); }          // 2 stages x 4 k-steps x 4 waves
constexpr long HDM_KBLOCK_MFMAS = HDM_KBLOCK_PAIRS * hdm_pair_mfmas(HDM_LIVE_FULL);                     // 2048
HDM_HD constexpr long hdm_block_mfmas(const HdmLive (&t)[HDM_KBLOCK_PAIRS]) {
    long s = 0;
    for (int p = 0; p < HDM_KBLOCK_PAIRS; ++p) s += hdm_pair_mfmas(t[p]);
    return s;
}
// the cell paths run a run-time stage count in pairs: an odd count ends with a stage of zeros
HDM_HD constexpr long hdm_even_stages(long nst) { return nst <= 0 ? 0 : ((nst + 1) / 2) * 2; }
constexpr int HDM_DIAG_CELLS = 36;                                               // 16 x 16 cells on or below a full tile's diagonal
HDM_HD constexpr int hdm_diag_short_cells(int RV) { return RV * (RV + 1) / 2; }
HDM_HD constexpr int hdm_edge_cells(int RV) { return 8 * RV; }
// MFMA instructions tile (tm, tn) executes for batch entry z.  The cell paths and the Gram role run the tile's K range; the
// congruence roles' main tiles run straight-line sequences that take their length from the tile's place (gemm_tile.h)
HDM_HD constexpr long hdm_tile_mfmas(const HdmTileGeom &g, int tm, int tn, int z) {
    const long nst = hdm_tile_stages(g, tm, tn, z);
    if (g.role == HDM_ROLE_GENERIC) return hdm_pair_mfmas(HDM_LIVE_FULL) / 2 * nst;        // any stage count, no pairing
    const HdmTileClass c = hdm_tile_class(g, tm, tn);
    switch (c.kind) {
        case HDM_CLS_DIAG_FULL: return 4L * HDM_DIAG_CELLS * hdm_even_stages(nst);         // one MFMA per cell and k-step
        case HDM_CLS_DIAG_SHORT: return 4L * hdm_diag_short_cells(c.RV) * hdm_even_stages(nst);
        case HDM_CLS_EDGE: return 4L * hdm_edge_cells(c.RV) * hdm_even_stages(nst);
        case HDM_CLS_SYMDIAG: return tn * HDM_KBLOCK_MFMAS + hdm_block_mfmas(HDM_LIVE_CONG2D_LAST);
        default: break;
    }
    if (g.role == HDM_ROLE_CONG2) return 2 * (tn * HDM_KBLOCK_MFMAS + hdm_block_mfmas(HDM_LIVE_CONG2_LAST));   // both products
    if (g.role == HDM_ROLE_CONG1)
        return hdm_block_mfmas(HDM_LIVE_CONG1_FIRST) + (tm - tn - 1) * HDM_KBLOCK_MFMAS + hdm_block_mfmas(HDM_LIVE_CONG1_LAST);
    return hdm_pair_mfmas(HDM_LIVE_FULL) / 2 * hdm_even_stages(nst);
}
// of a whole launch's tiles (subset as in hdm_tile_list), one batch entry -- a split-K launch: all its splits
inline long hdm_launch_mfmas(const HdmTileGeom &g, int subset) {
    long mf = 0;
    for (int z = 0; z < (g.slab ? g.batch : 1); ++z)
        for (int tm = 0; tm < hdm_ntiles(g.M); ++tm)
            for (int tn = 0; tn < hdm_ntiles(g.N); ++tn)
                if (hdm_tile_in_subset(g, tm, tn, subset)) mf += hdm_tile_mfmas(g, tm, tn, z);
    return mf;
}

// ---- how far unmasked tile loads reach ----------------------------------------------------------
// Roles 1-3 stage whole 128-row tiles without a row mask: the farthest element + 1, counted from the operand's pointer, that
// a launch can touch -- last batch entry, last tile row, last k of the launch.  `rows`: M for the A side, N for the B side;
// kblk: elements between the 16-deep k blocks of a K-major operand (0: a plain matrix); seg_rows / seg_extra: HdmGemmArgs.
// `sky` (step 1's B operand): the last panel (width w < 128 columns, height w) is read as 128 "rows" of its leading
// dimension, i.e. up to (128 - w) columns' worth past the matrix.
HDM_HD constexpr long hdm_operand_need(const HdmTileGeom &g, bool kmajor, long ld, long kblk, long stride, int rows, long seg_rows,
                                       long seg_extra, bool sky) {
    if (sky) {
        const int t = hdm_ntiles(rows) - 1;
        const long h = rows - 128L * t;
        return (long) (g.batch - 1) * stride + hdm_sky_panel(t, rows) + 127 * h + h;
    }
    const long maxrow = (long) hdm_ntiles(rows) * HDM_TILE - 1;
    const long klast = (g.slab ? hdm_min((long) g.K, g.k_base + (long) g.batch * g.k_chunk) : (long) g.K) - 1;
    long off = ((g.slab ? 1 : g.batch) - 1) * stride;
    if (kmajor) {
        off += (klast / HDM_BK) * (kblk ? kblk : HDM_BK) + maxrow * ld + (HDM_BK - 1);
        if (seg_rows) off += (maxrow / seg_rows) * seg_extra;
    } else {
        off += klast * ld + maxrow;
    }
    return off + 1;
}

// ---- the two work shares of congruence step 2 -------------------------------------------------
// Two different approximations of "how much of step 2 is here", each kept as its caller has always computed it (all sums
// are integers below 2^53: exact in a double, one rounding in the division).  Do not merge them.
//  * by output element: (i, j), i >= j, is 2 products x (j + 1) terms.  The share of the full diagonal tiles among the tile
//    columns of the mask -- what a role-2 launch splits its algorithmic flops by between its two kernels.
inline double hdm_cong2_diag_share(int M, int N, unsigned long long colmask) {
    const unsigned long long mask = hdm_colmask_effective(colmask, hdm_ntiles(N));
    double all = 0.0, diag = 0.0;
    for (int tn = 0; tn < hdm_ntiles(N); ++tn) {
        if (mask && !((mask >> tn) & 1ULL)) continue;
        const int j0 = tn * HDM_TILE, j1 = std::min(N, j0 + HDM_TILE);
        const bool full = hdm_full_diag(M, tn, tn);
        for (int j = j0; j < j1; ++j) {
            all += (double) (M - j) * (j + 1);
            if (full) diag += (double) (j1 - j) * (j + 1);
        }
    }
    return all > 0.0 ? diag / all : 0.0;
}
//  * by tile: tile (tm, tn), tm >= tn, runs tn + 1 K blocks.  The share of the mask's tile columns in the whole step -- what
//    the engine scales a masked launch's algorithmic flops by.
inline double hdm_cong2_mask_share(int NT, unsigned long long colmask) {
    const unsigned long long mask = hdm_colmask_effective(colmask, NT);
    if (!mask) return 1.0;
    double all = 0.0, sel = 0.0;
    for (int tn = 0; tn < NT; ++tn) {
        const double w = (double) (NT - tn) * (double) hdm_tile_weight(HDM_KLIM_BY_N, tn, tn);
        all += w;
        if ((mask >> tn) & 1ULL) sel += w;
    }
    return all > 0.0 ? sel / all : 1.0;
}

// ---- the blocked congruence layout --------------------------------------------------------------
// The lower triangle of an n16 x n16 matrix in 16 x 16 sub-blocks (bi >= bj), numbered column by column; sub-block `sub`
// is the 16 p-blocks 16 sub .. 16 sub + 15, one per matrix column, each holding that column's 16 rows.
HDM_HD constexpr long hdm_blk_col_start(int bj, int nblk) { return (long) bj * nblk - (long) bj * (bj - 1) / 2; }
HDM_HD constexpr long hdm_blk_sub(int bi, int bj, int nblk) { return hdm_blk_col_start(bj, nblk) + (bi - bj); }
// the column whose sub-blocks include `sub` (the last one for anything past the triangle)
HDM_HD constexpr int hdm_blk_col_of(long sub, int nblk) {
    int lo = 0, hi = nblk - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (hdm_blk_col_start(mid, nblk) <= sub) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// p-block q: its sub-block, and the matrix column it holds (its 16 packed columns 16 q + r are the rows 16 bi + r)
struct HdmPBlock { long sub; int bi, bj; long col; };
HDM_HD constexpr HdmPBlock hdm_pblock_decode(long q, int nblk) {
    const long sub = q >> 4;
    const int bj = hdm_blk_col_of(sub, nblk);
    return {sub, bj + (int) (sub - hdm_blk_col_start(bj, nblk)), bj, (long) bj * 16 + (q & 15)};
}
