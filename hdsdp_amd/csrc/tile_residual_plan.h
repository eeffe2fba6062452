// tile_residual_plan.h -- the work list of the tile form's twice-precision residual r = b - M x (refine.hip: hdm_tile_residual_kernel).
// Pure host arithmetic: no HIP call, no engine state; tests/test_tile_residual_plan_cpu.py compiles this header alone.
//
// The tile store (bsparse.h) keeps the lower triangle of the permuted matrix as 128 x 128 tiles, tile number = position in the block
// pattern (bptr, brow).  The residual works on 64 x 64 QUADRANTS, the tile of the dense residual kernel: quadrant (qi, qj) of tile
// (bi, bj) covers the rows of 64-row block I = 2 bi + qi and the columns of 64-row block J = 2 bj + qj of the permuted order.
//
//   jobs    one per stored quadrant with I >= J (a diagonal tile has three, any other four) whose first row and first column are
//           below m; ascending tile number, then quadrant number q = qi + 2 qj.
//   uses    a job is read once and used twice: DIRECT, M_q x_J into the rows of block I, and TRANSPOSED, M_q' x_I into the rows of
//           block J.  In a diagonal quadrant (I == J) the direct use takes the lower triangle with the diagonal and the transposed
//           use the strict lower triangle.
//   slots   every use writes 64 (hi, lo) pairs into a slot of its own: no slot has two writers.  The slots of row block R are
//           numbered slot_ptr[R] .. slot_ptr[R + 1] - 1 in the order (tile number, quadrant, direct before transposed), which is
//           the order the combine pass adds them in.  slot_use[s] = 2 job + (0 direct, 1 transposed) names the writer.
// Tiles that exist only as fill are tiles of zeros like any other; the trash tile (number ntiles) is in no job.
#pragma once
#include <cstddef>
#include <vector>

constexpr int HDM_TILERES_BLOCK = 128;   // tile edge (bsparse.h)
constexpr int HDM_TILERES_QUAD = 64;     // quadrant edge = HDM_SYMRES_TILE (refine.h)

struct HdmTileResJob {
    int tile;          // tile number in the store
    int qi, qj;        // quadrant inside the tile
    int rblk, cblk;    // 64-row blocks I and J of the permuted order
    int slot_direct;   // slot of M_q x_J, in row block I
    int slot_trans;    // slot of M_q' x_I, in row block J
    int diag;          // 1: I == J
};

struct HdmTileResPlan {
    int m = 0, nb = 0, nrb = 0;           // order, 128-blocks, 64-row blocks (2 nb: the padded length / 64)
    std::vector<HdmTileResJob> jobs;
    std::vector<int> slot_ptr;            // nrb + 1
    std::vector<int> slot_use;            // per slot: 2 job + use
    int nslots() const { return (int) slot_use.size(); }
};

// nb block columns, bptr (nb + 1), brow (bptr[nb]): the block pattern of the factor, lower with the diagonal, by block column
inline HdmTileResPlan hdm_tile_residual_plan(int m, int nb, const int *bptr, const int *brow) {
    HdmTileResPlan p;
    p.m = m; p.nb = nb; p.nrb = 2 * nb;
    for (int bj = 0; bj < nb; ++bj)
        for (int t = bptr[bj]; t < bptr[bj + 1]; ++t) {
            const int bi = brow[t];
            for (int q = 0; q < 4; ++q) {
                HdmTileResJob j;
                j.tile = t; j.qi = q & 1; j.qj = q >> 1;
                j.rblk = 2 * bi + j.qi; j.cblk = 2 * bj + j.qj;
                if (j.rblk < j.cblk) continue;                                     // the upper quadrant of a diagonal tile
                if ((long) j.rblk * HDM_TILERES_QUAD >= m || (long) j.cblk * HDM_TILERES_QUAD >= m) continue;   // all padding
                j.diag = j.rblk == j.cblk ? 1 : 0;
                j.slot_direct = j.slot_trans = -1;
                p.jobs.push_back(j);
            }
        }
    p.slot_ptr.assign((size_t) p.nrb + 1, 0);
    for (const HdmTileResJob &j : p.jobs) { p.slot_ptr[(size_t) j.rblk + 1] += 1; p.slot_ptr[(size_t) j.cblk + 1] += 1; }
    for (int R = 0; R < p.nrb; ++R) p.slot_ptr[(size_t) R + 1] += p.slot_ptr[(size_t) R];
    p.slot_use.assign((size_t) p.slot_ptr[(size_t) p.nrb], -1);
    std::vector<int> fill(p.slot_ptr.begin(), p.slot_ptr.end() - 1);
    for (size_t k = 0; k < p.jobs.size(); ++k) {          // jobs in order, direct before transposed: every list comes out sorted
        HdmTileResJob &j = p.jobs[k];
        j.slot_direct = fill[(size_t) j.rblk]++;
        p.slot_use[(size_t) j.slot_direct] = 2 * (int) k;
        j.slot_trans = fill[(size_t) j.cblk]++;
        p.slot_use[(size_t) j.slot_trans] = 2 * (int) k + 1;
    }
    return p;
}
