// refine.hip -- r = b - M x in twice the working precision for the refined Schur solve.
//
// M is symmetric and only its lower triangle exists (column-major): row i of M x needs M[i, 0..i] -- strided in memory -- and
// M[i+1.., i], a column.  The triangle is cut into 64 x 64 tiles (I, J), J <= I, one workgroup each.  A tile is read ONCE, down
// its columns (coalesced), and used twice: as it arrives for the rows of block I (sum over the tile's columns), and, transposed
// through LDS, for the rows of block J (sum over the tile's rows; the diagonal tile's strict lower part only).  Each use leaves
// 64 partial sums as (hi, lo) pairs in a slot of its row block that no other tile writes: row block R has nbt + 1 slots, slot J
// from tile (R, J), J <= R, and slot I + 1 from tile (I, R), I >= R.  A second launch adds a row block's slots in slot order,
// b_i as one more term, rounds once, and leaves the block's sum of squares; a third adds the blocks' sums in block order.
// No atomics, no order that depends on the grid or on timing: two runs give the same bits.
//
// The tile form of a sparse operator (bsparse.h) has no m x m array: its matrix is 128 x 128 tiles inside the block pattern of the
// factor.  The same 64 x 64 body runs on the quadrants of the stored tiles, one workgroup per job of tile_residual_plan.h; the slot
// lists of a row block then have the length its pattern gives them, and the combine pass walks them in list order.
//
// Arithmetic: Dot2 of Ogita, Rump and Oishi -- every product split exactly with an fma (TwoProd), every sum with TwoSum, the
// error terms collected in a second double -- so a component's error is u |r_i| + O(n^2 u^2) (|M| |x| + |b|)_i.
// The error-free transformations need every operation rounded as written: no contraction in this file.
#pragma clang fp contract(off)
#include "refine.h"
#include "bsparse.h"

namespace {
constexpr int RT = HDM_SYMRES_TILE;
constexpr int RLD = RT + 1;       // LDS leading dimension of the tile: the transposed read is conflict-free

// (s, c) += a * b, exactly split
__device__ __forceinline__ void dd_add_prod(double &s, double &c, double a, double b) {
    const double p = a * b;
    const double e = fma(a, b, -p);
    const double t = s + p;
    const double z = t - s;
    c += ((s - (t - z)) + (p - z)) + e;
    s = t;
}
// (s, c) += (h, l)
__device__ __forceinline__ void dd_add(double &s, double &c, double h, double l) {
    const double t = s + h;
    const double z = t - s;
    c += ((s - (t - z)) + (h - z)) + l;
    s = t;
}

// the four 16-wide partial sums of each of 64 rows -> one (hi, lo) pair per row, added in group order, into a slot
__device__ __forceinline__ void reduce_groups_to_slot(double *red, double s, double c, int lane, int grp, double *slot) {
    red[(grp * 2) * RT + lane] = s;
    red[(grp * 2 + 1) * RT + lane] = c;
    __syncthreads();
    if (grp == 0) {
        double S = 0.0, C = 0.0;
        for (int q = 0; q < 4; ++q) dd_add(S, C, red[(q * 2) * RT + lane], red[(q * 2 + 1) * RT + lane]);
        slot[lane] = S;
        slot[RT + lane] = C;
    }
    __syncthreads();
}

// The 64 x 64 tile body shared by the dense and the tile-form kernels: the tile at `base` (column-major, leading dimension ld) is
// read ONCE, down its columns, and used twice.  nr / nc: its rows / columns that exist (the others are padding and are never
// loaded: the loads are predicated, not masked afterwards); diag: only the lower triangle exists.  xcol / xrow: the 64 entries of x
// that face its columns / its rows, in LDS, written by the caller before the call (the barrier below covers them).
//   slot_direct  <- - sum over the tile's columns, per row            (lower triangle with the diagonal in a diagonal tile)
//   slot_trans   <- - sum over the tile's rows, per column, through the LDS transpose   (strictly below the diagonal there)
__device__ __forceinline__ void symres_tile_body(const double *__restrict__ base, long ld, int nr, int nc, bool diag, const double *xcol,
                                                 const double *xrow, double *tile, double *red, int lane, int grp,
                                                 double *__restrict__ slot_direct, double *__restrict__ slot_trans) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int jl = grp * 16 + k;
        v[k] = (lane < nr && jl < nc && (!diag || jl <= lane)) ? base[(long) lane + (long) jl * ld] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) tile[lane + (grp * 16 + k) * RLD] = v[k];
    __syncthreads();
    // the rows of the tile: sum over its columns
    double s = 0.0, c = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int jl = grp * 16 + k;
        if (lane < nr && jl < nc && (!diag || jl <= lane)) dd_add_prod(s, c, -v[k], xcol[jl]);
    }
    reduce_groups_to_slot(red, s, c, lane, grp, slot_direct);
    // the columns of the tile: column `lane`, summed over the tile's rows
    s = 0.0; c = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int il = grp * 16 + k;
        if (il < nr && lane < nc && (!diag || lane < il)) dd_add_prod(s, c, -tile[il + lane * RLD], xrow[il]);
    }
    reduce_groups_to_slot(red, s, c, lane, grp, slot_trans);
}

// one tile (I, J) of the lower triangle: partial sums of -M x for the rows of block I (slot J) and of block J (slot I + 1)
__global__ __launch_bounds__(256) void hdm_symres_tile_kernel(const double *__restrict__ M, long ld, int n, const double *__restrict__ x,
                                                              int nbt, double *__restrict__ part) {
    const int J = blockIdx.x, I = blockIdx.y;
    if (J > I) return;
    __shared__ double tile[RT * RLD];
    __shared__ double red[8 * RT];
    __shared__ double xcol[RT], xrow[RT];
    const int t = threadIdx.x, lane = t & (RT - 1), grp = t >> 6;
    if (t < RT) { const int j = J * RT + t; xcol[t] = j < n ? x[j] : 0.0; }
    else if (t < 2 * RT) { const int i = I * RT + t - RT; xrow[t - RT] = i < n ? x[i] : 0.0; }
    // rows that exist: i < n; columns: j <= i in the diagonal tile, all 64 below it (j < i < n there)
    const int nr = min(RT, n - I * RT);
    symres_tile_body(M + (long) I * RT + (long) J * RT * ld, ld, nr, I == J ? nr : RT, I == J, xcol, xrow, tile, red, lane, grp,
                     part + ((long) I * (nbt + 1) + J) * (2 * RT), part + ((long) J * (nbt + 1) + I + 1) * (2 * RT));
}

// one quadrant job of a tile store (tile_residual_plan.h): the same body on the 64 x 64 quadrant inside its 128 x 128 tile.
// x in the store's permuted, padded order; rows and columns >= m are padding: never loaded, x never read there.
__global__ __launch_bounds__(256) void hdm_tile_residual_kernel(const double *__restrict__ Mstore, const HdmTileResJob *__restrict__ jobs, int m,
                                                                const double *__restrict__ x, double *__restrict__ part) {
    const HdmTileResJob job = jobs[blockIdx.x];
    __shared__ double tile[RT * RLD];
    __shared__ double red[8 * RT];
    __shared__ double xcol[RT], xrow[RT];
    const int t = threadIdx.x, lane = t & (RT - 1), grp = t >> 6;
    const int nr = min(RT, m - job.rblk * RT), nc = min(RT, m - job.cblk * RT);      // both > 0: the plan skips quadrants of padding
    if (t < RT) xcol[t] = t < nc ? x[job.cblk * RT + t] : 0.0;
    else if (t < 2 * RT) xrow[t - RT] = t - RT < nr ? x[job.rblk * RT + t - RT] : 0.0;
    symres_tile_body(Mstore + ((long) job.tile << 14) + RT * job.qi + (long) (RT * job.qj) * HDM_TILERES_BLOCK, HDM_TILERES_BLOCK, nr, nc,
                     job.diag != 0, xcol, xrow, tile, red, lane, grp, part + (long) job.slot_direct * (2 * RT),
                     part + (long) job.slot_trans * (2 * RT));
}

// A row block's slots (`count` of them from `base`) in a fixed order -- four interleaved chains in slot order, then the chains in
// order -- b_i as one more term, one rounding; rows that do not exist give 0.  Leaves the block's sum of squares in npart2.
// Returns r_i to the threads of group 0 (0 elsewhere).
__device__ __forceinline__ double symres_combine_body(const double *__restrict__ base, int count, bool exists, const double *__restrict__ bi,
                                                      double *red, double *sq, int t, double *__restrict__ npart2) {
    const int lane = t & (RT - 1), grp = t >> 6;
    double s = 0.0, c = 0.0;
    for (int sl = grp; sl < count; sl += 4) dd_add(s, c, base[(long) sl * (2 * RT) + lane], base[(long) sl * (2 * RT) + RT + lane]);
    red[(grp * 2) * RT + lane] = s;
    red[(grp * 2 + 1) * RT + lane] = c;
    __syncthreads();
    double ri = 0.0;
    if (grp == 0) {
        double S = 0.0, C = 0.0;
        for (int q = 0; q < 4; ++q) dd_add(S, C, red[(q * 2) * RT + lane], red[(q * 2 + 1) * RT + lane]);
        if (exists) {
            dd_add(S, C, *bi, 0.0);
            ri = S + C;
        }
        const double p = ri * ri;
        sq[lane] = p;
        sq[RT + lane] = fma(ri, ri, -p);
    }
    __syncthreads();
    if (t == 0) {
        double S = 0.0, C = 0.0;
        for (int q = 0; q < RT; ++q) dd_add(S, C, sq[q], sq[RT + q]);
        npart2[0] = S;
        npart2[1] = C;
    }
    return ri;
}

// row block R: its nbt + 1 slots, b_i, one rounding
__global__ __launch_bounds__(256) void hdm_symres_combine_kernel(const double *__restrict__ part, int nbt, int n, const double *__restrict__ b,
                                                                 double *__restrict__ r, double *__restrict__ npart) {
    const int R = blockIdx.x, t = threadIdx.x;
    __shared__ double red[8 * RT];
    __shared__ double sq[2 * RT];
    const int i = R * RT + (t & (RT - 1));
    const bool exists = t < RT && i < n;
    const double ri = symres_combine_body(part + (long) R * (nbt + 1) * (2 * RT), nbt + 1, exists, b + (exists ? i : 0), red, sq, t, npart + 2 * R);
    if (exists) r[i] = ri;
}

// 64-row block R of a tile store's padded order: the slots slot_ptr[R] .. slot_ptr[R + 1] - 1 in list order, b_i, one rounding;
// r is written in the padding rows too, as 0 (it is the next correction solve's right-hand side)
__global__ __launch_bounds__(256) void hdm_tile_combine_kernel(const double *__restrict__ part, const int *__restrict__ slot_ptr, int m,
                                                               const double *__restrict__ b, double *__restrict__ r, double *__restrict__ npart) {
    const int R = blockIdx.x, t = threadIdx.x;
    __shared__ double red[8 * RT];
    __shared__ double sq[2 * RT];
    const int i = R * RT + (t & (RT - 1)), first = slot_ptr[R];
    const bool exists = t < RT && i < m;
    const double ri = symres_combine_body(part + (long) first * (2 * RT), slot_ptr[R + 1] - first, exists, b + (exists ? i : 0), red, sq, t, npart + 2 * R);
    if (t < RT) r[i] = ri;
}

__global__ void hdm_symres_norm_kernel(const double *__restrict__ npart, int nbt, double *__restrict__ norm2) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double S = 0.0, C = 0.0;
    for (int R = 0; R < nbt; ++R) dd_add(S, C, npart[2 * R], npart[2 * R + 1]);
    norm2[0] = S + C;
}

__global__ void hdm_refine_scatter_kernel(double *__restrict__ dst, const double *__restrict__ src, const int *__restrict__ perm, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[perm ? perm[i] : i] = src[i];
}
__global__ void hdm_refine_gather_kernel(double *__restrict__ x, const double *__restrict__ d, const int *__restrict__ perm, int n, int add) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const double di = d[perm ? perm[i] : i];
        x[i] = add ? x[i] + di : di;
    }
}
}  // namespace

int HdmSymRes::reserve(int n) {
    const size_t nbt = (size_t) hdm_roundup(n, RT) / RT;
    HDM_HIP_CHECK(part.reserve(nbt * (nbt + 1) * 2 * RT));
    HDM_HIP_CHECK(npart.reserve(2 * nbt));
    return 0;
}

int HdmSymRes::run(const double *M, long ld, int n, const double *x, const double *b, double *r, double *norm2_dev, hipStream_t s) {
    if (n < 1 || ld < n || !M || !x || !b || !r || !norm2_dev) return 1;
    const int nbt = (int) (hdm_roundup(n, RT) / RT);
    if (nbt > 65535 || reserve(n)) return 1;
    hipLaunchKernelGGL(hdm_symres_tile_kernel, dim3(nbt, nbt), dim3(256), 0, s, M, ld, n, x, nbt, part.get());
    hipLaunchKernelGGL(hdm_symres_combine_kernel, dim3(nbt), dim3(256), 0, s, (const double *) part.get(), nbt, n, b, r, npart.get());
    hipLaunchKernelGGL(hdm_symres_norm_kernel, dim3(1), dim3(64), 0, s, (const double *) npart.get(), nbt, norm2_dev);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_refine_scatter(double *dst, const double *src, const int *perm, int n, hipStream_t s) {
    hipLaunchKernelGGL(hdm_refine_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dst, src, perm, n);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}
int hdm_refine_gather(double *x, const double *d, const int *perm, int n, int add, hipStream_t s) {
    hipLaunchKernelGGL(hdm_refine_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, d, perm, n, add);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the tile form ----
int HdmBspRefine::prepare(const HdmBsp &bs) {
    const long want = (long) bs.nb * HDM_TILERES_BLOCK;
    if (jobs && v && m == bs.m && len == want) return 0;
    const HdmTileResPlan p = hdm_tile_residual_plan(bs.m, bs.nb, bs.bptr.data(), bs.brow.data());
    if (p.jobs.empty()) return 1;
    HDM_HIP_CHECK(jobs.alloc(p.jobs.size()));
    HDM_HIP_CHECK(slot_ptr.alloc(p.slot_ptr.size()));
    HDM_HIP_CHECK(part.alloc((size_t) p.nslots() * 2 * RT));
    HDM_HIP_CHECK(npart.alloc(2 * (size_t) p.nrb));
    HDM_HIP_CHECK(v.alloc(6 * (size_t) want + 8));
    HDM_HIP_CHECK(hdm_memcpy_h2d_sync(jobs.get(), p.jobs.data(), sizeof(HdmTileResJob) * p.jobs.size()));
    HDM_HIP_CHECK(hdm_memcpy_h2d_sync(slot_ptr.get(), p.slot_ptr.data(), sizeof(int) * p.slot_ptr.size()));
    m = bs.m; nrb = p.nrb; njobs = (int) p.jobs.size(); len = want;
    return 0;
}

int HdmBspRefine::keep_copy(const HdmBsp &bs, hipStream_t s) {
    const size_t count = (size_t) bs.ntiles << 14;
    HDM_HIP_CHECK(copy.reserve(count));
    HDM_HIP_CHECK(hipMemcpyAsync(copy.get(), bs.Lval.get(), sizeof(double) * count, hipMemcpyDeviceToDevice, s));
    return 0;
}

int HdmBspRefine::residual(const double *store, const double *x, const double *b, double *r, double *norm2_dev, hipStream_t s) {
    if (!store || !x || !b || !r || !norm2_dev || njobs < 1 || !jobs || !part) return 1;
    hipLaunchKernelGGL(hdm_tile_residual_kernel, dim3(njobs), dim3(256), 0, s, store, (const HdmTileResJob *) jobs.get(), m, x, part.get());
    hipLaunchKernelGGL(hdm_tile_combine_kernel, dim3(nrb), dim3(256), 0, s, (const double *) part.get(), (const int *) slot_ptr.get(), m, b, r, npart.get());
    hipLaunchKernelGGL(hdm_symres_norm_kernel, dim3(1), dim3(64), 0, s, (const double *) npart.get(), nrb, norm2_dev);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int HdmBspRefine::apply(HdmBsp &bs, const double *rhs, double *x, bool add, hipStream_t s) {
    if (!bs.factored || len != (long) bs.nb * HDM_TILERES_BLOCK) return 1;
    HDM_HIP_CHECK(hipMemcpyAsync(bs.vec.get(), rhs, sizeof(double) * (size_t) len, hipMemcpyDeviceToDevice, s));
    if (bs.solve_device(bs.vec.get(), s)) return 1;
    return hdm_refine_gather(x, bs.vec.get(), nullptr, (int) len, add ? 1 : 0, s);
}

const void *hdm_module_handle_refine() { return (const void *) hdm_refine_gather_kernel; }
