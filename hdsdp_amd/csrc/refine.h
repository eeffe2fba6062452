// refine.h -- the device side of the refined Schur solve (see refine.hip): the twice-precision residual r = b - M x of a
// symmetric matrix stored as its lower triangle -- a dense column-major array, or the 128 x 128 tile store of bsparse.h -- and the
// small vector kernels of the refinement loop.
#pragma once
#include "hdm_common.h"
#include "tile_residual_plan.h"
#include <vector>

constexpr int HDM_SYMRES_TILE = 64;   // edge of the square tiles the lower triangle is cut into

// r = b - M x and |r|_2^2, every component accumulated in twice the working precision and rounded once.
// M: n x n column-major, leading dimension ld >= n, lower triangle valid; nothing above the diagonal and nothing in rows or
// columns >= n is read.  x, b, r: n entries on the device; norm2_dev: one double on the device.  Deterministic: no atomics,
// a reduction order fixed by n alone.
struct HdmSymRes {
    HdmBuf<double> part;     // per (row block, slot): 64 (hi, lo) pairs -- nbt (nbt + 1) 128 doubles
    HdmBuf<double> npart;    // per row block: (hi, lo) of the sum of its r_i^2
    int reserve(int n);      // work space for matrices up to order n (no-op when held)
    size_t bytes() const { return sizeof(double) * (part.count() + npart.count()); }
    int run(const double *M, long ld, int n, const double *x, const double *b, double *r, double *norm2_dev, hipStream_t s);
};

// dst[perm[i]] = src[i] (perm == nullptr: dst[i] = src[i]), i < n
int hdm_refine_scatter(double *dst, const double *src, const int *perm, int n, hipStream_t s);
// x[i] = (add ? x[i] : 0) + d[perm[i]] (perm == nullptr: d[i]), i < n: the correction x <- x + d, or the solution's way back
int hdm_refine_gather(double *x, const double *d, const int *perm, int n, int add, hipStream_t s);

// The tile form's part of the refined solve (bsparse.h): the residual of a tile store over
// tile_residual_plan.h's jobs, the correction solve through HdmBsp::solve_device, and the loop's vectors.  Everything lives in
// the store's own order: permuted and padded to len = nb * 128, padding rows zero.  Used by the operator's linear system and by
// HMiTileResidualProbe / HMiBspRefinedSolve.  Allocated by prepare / keep_copy, freed by release.
struct HdmBsp;
struct HdmBspRefine {
    HdmBuf<HdmTileResJob> jobs;
    HdmBuf<int> slot_ptr;
    HdmBuf<double> part;     // per slot: 64 (hi, lo) pairs
    HdmBuf<double> npart;    // per 64-row block: (hi, lo) of the sum of its r_i^2
    HdmBuf<double> v;        // 6 len + 8: right-hand side, iterate, previous iterate, unrefined solution, residual, staging; |r|^2
    HdmBuf<double> copy;     // ntiles tiles: the factor store as it was scattered, before the factorisation (mirror on)
    std::vector<double> stage;
    int m = 0, nrb = 0, njobs = 0;
    long len = 0;
    int prepare(const HdmBsp &bs);                       // plan, work space and vectors for this pattern (no-op when held)
    int keep_copy(const HdmBsp &bs, hipStream_t s);      // copy <- the factor store
    double *vec(int k) const { return v.get() + (long) k * len; }
    // r = b - M x and |r|_2^2 of the matrix in `store` (tiles of the pattern prepare saw); x, b, r: len entries, permuted and padded.
    // Nothing in a padding row or column of the store and no entry of x or b past m is read; r is 0 in the padding.
    int residual(const double *store, const double *x, const double *b, double *r, double *norm2_dev, hipStream_t s);
    // x <- M^-1 v, or x <- x + M^-1 v, through the factor's level loops; v and x: len entries (v's padding zero)
    int apply(HdmBsp &bs, const double *v, double *x, bool add, hipStream_t s);
    void release() {
        jobs.reset(); slot_ptr.reset(); part.reset(); npart.reset(); v.reset(); copy.reset();
        stage.clear(); stage.shrink_to_fit(); m = nrb = njobs = 0; len = 0;
    }
    size_t bytes() const {
        return sizeof(HdmTileResJob) * jobs.count() + sizeof(int) * slot_ptr.count() + sizeof(double) * (part.count() + npart.count() + v.count() + copy.count());
    }
};

const void *hdm_module_handle_refine();
