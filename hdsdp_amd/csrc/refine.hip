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
// Arithmetic: Dot2 of Ogita, Rump and Oishi -- every product split exactly with an fma (TwoProd), every sum with TwoSum, the
// error terms collected in a second double -- so a component's error is u |r_i| + O(n^2 u^2) (|M| |x| + |b|)_i.
// The error-free transformations need every operation rounded as written: no contraction in this file.
#pragma clang fp contract(off)
#include "refine.h"

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
    // the thread's 16 elements of row `lane`: loaded where they exist (i < n, j <= i, hence j < n), zero elsewhere
    const int i = I * RT + lane;
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int j = J * RT + grp * 16 + k;
        v[k] = (i < n && j <= i) ? M[(long) i + (long) j * ld] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) tile[lane + (grp * 16 + k) * RLD] = v[k];
    __syncthreads();
    // rows of block I: sum over the tile's columns
    double s = 0.0, c = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int j = J * RT + grp * 16 + k;
        if (i < n && j <= i) dd_add_prod(s, c, -v[k], xcol[grp * 16 + k]);
    }
    reduce_groups_to_slot(red, s, c, lane, grp, part + ((long) I * (nbt + 1) + J) * (2 * RT));
    // rows of block J: column `lane` of the tile, summed over the tile's rows (strictly below the diagonal in a diagonal tile)
    const int j = J * RT + lane;
    s = 0.0; c = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int il = grp * 16 + k, ii = I * RT + il;
        if (ii < n && j < ii) dd_add_prod(s, c, -tile[il + lane * RLD], xrow[il]);
    }
    reduce_groups_to_slot(red, s, c, lane, grp, part + ((long) J * (nbt + 1) + I + 1) * (2 * RT));
}

// row block R: its nbt + 1 slots in a fixed order (four interleaved chains, then the chains in order), b_i, one rounding
__global__ __launch_bounds__(256) void hdm_symres_combine_kernel(const double *__restrict__ part, int nbt, int n, const double *__restrict__ b,
                                                                 double *__restrict__ r, double *__restrict__ npart) {
    const int R = blockIdx.x, t = threadIdx.x, lane = t & (RT - 1), grp = t >> 6;
    __shared__ double red[8 * RT];
    __shared__ double sq[2 * RT];
    const double *base = part + (long) R * (nbt + 1) * (2 * RT);
    double s = 0.0, c = 0.0;
    for (int sl = grp; sl <= nbt; sl += 4) dd_add(s, c, base[(long) sl * (2 * RT) + lane], base[(long) sl * (2 * RT) + RT + lane]);
    red[(grp * 2) * RT + lane] = s;
    red[(grp * 2 + 1) * RT + lane] = c;
    __syncthreads();
    if (grp == 0) {
        double S = 0.0, C = 0.0;
        for (int q = 0; q < 4; ++q) dd_add(S, C, red[(q * 2) * RT + lane], red[(q * 2 + 1) * RT + lane]);
        const int i = R * RT + lane;
        double ri = 0.0;
        if (i < n) {
            dd_add(S, C, b[i], 0.0);
            ri = S + C;
            r[i] = ri;
        }
        const double p = ri * ri;
        sq[lane] = p;
        sq[RT + lane] = fma(ri, ri, -p);
    }
    __syncthreads();
    if (t == 0) {
        double S = 0.0, C = 0.0;
        for (int q = 0; q < RT; ++q) dd_add(S, C, sq[q], sq[RT + q]);
        npart[2 * R] = S;
        npart[2 * R + 1] = C;
    }
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

const void *hdm_module_handle_refine() { return (const void *) hdm_refine_gather_kernel; }
