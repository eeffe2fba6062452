// refine.h -- the device side of the refined Schur solve (see refine.hip): the twice-precision residual r = b - M x of a
// symmetric matrix stored as its lower triangle, and the small vector kernels of the refinement loop.
#pragma once
#include "hdm_common.h"

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

const void *hdm_module_handle_refine();
