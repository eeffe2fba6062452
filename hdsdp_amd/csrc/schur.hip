// schur.hip -- data-movement and reduction kernels of the Schur build (all HBM-bound).
//
//   * hdm_unpack_sym_kernel     packed lower (reference DENSE layout, def_hdsdp_sdpdata.h:107-113,
//                               PACK_IDX hdsdp_utils.h:49-53) -> full symmetric column-major, via an
//                               LDS tile transpose so both triangles are written coalesced
//   * hdm_synth_kernel          SURVEY.md 8(d) splitmix64 generator evaluated counter-based on device
//   * hdm_blocked_eye_kernel    identity in the 16x16-blocked congruence layout (the "S row")
//   * hdm_direct_rows_kernel    low-rank constraint rows straight into that layout (direct_rows.h)
//   * hdm_slab_reduce_kernel    split-K slab reduction of the Gram GEMM (deterministic order)
//   * hdm_extract_kernel        scatter Gram rows/cols into M, ASinv, ASinvRdSinv, ASinvCSinv, scalars
//   * hdm_sym_combine_kernel    S = tau*C - sum_i y_i A_i - Rd*I  (hdsdp_conic_sdp.c:343-402), lower part
//   * hdm_r1_* kernels          rank-one (M2) path: M_ij = s_i s_j (a_i' S^-1 a_j)^2
//                               (hdsdp_conic_sdp.c:687-778, hdsdp_sdpdata.c:1003-1118)
#include "hdm_common.h"
#include "schur.h"
#include <vector>
#include <map>
#include "bsparse.h"
#include <algorithm>

// ------------------------------------------------------------------------------------------
// symmetric tile writer: a 32x32 lower tile source -> dst (full symmetric)
// ------------------------------------------------------------------------------------------
struct PackedSrc {
    const double *p;  // packed lower, column-major
    int n;
    __device__ double operator()(int i, int j) const {  // i >= j, both < n
        return p[(long) (2 * n - j - 1) * j / 2 + i];
    }
};

__device__ __forceinline__ double hdm_splitmix_u(uint64_t t) {
    // draw number t (0-based) of the SURVEY 8(d) stream: state s0 + (t+1)*gamma
    const uint64_t g = 0x9E3779B97F4A7C15ULL;
    uint64_t z = g + (t + 1) * g;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z = z ^ (z >> 31);
    return 2.0 * ((double) (z >> 11) / 9007199254740992.0) - 1.0;
}

struct SynthSrc {
    uint64_t base;  // 2 * c * P
    int n;
    __device__ double operator()(int i, int j) const {
        uint64_t k = (uint64_t) ((long) (2 * n - j - 1) * j / 2 + i);
        double v = hdm_splitmix_u(base + 2 * k);
        double w = hdm_splitmix_u(base + 2 * k + 1);
        return (i == j || w >= 0.2) ? v : 0.0;
    }
};

template <class Src>
__device__ __forceinline__ void write_sym_tile(const Src &src, double *__restrict__ dst, long ld, int n, int ti, int tj) {
    // workgroup = 32 x 8 threads; tile (ti >= tj) of 32x32
    __shared__ double tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int jj = ty; jj < 32; jj += 8) {
        int i = ti * 32 + tx, j = tj * 32 + jj;
        double v = 0.0;
        if (i < n && j < n) v = (i >= j) ? src(i, j) : src(j, i);
        tile[jj][tx] = v;
        if (i < ld && j < ld) dst[i + (long) j * ld] = v;
    }
    if (ti == tj) return;
    __syncthreads();
    for (int jj = ty; jj < 32; jj += 8) {
        // transposed tile: element (row = tj*32 + tx, col = ti*32 + jj) = tile[tx][jj]
        int i = tj * 32 + tx, j = ti * 32 + jj;
        if (i < ld && j < ld) dst[i + (long) j * ld] = tile[tx][jj];
    }
}

// "A_L" form of a symmetric matrix: strict lower triangle + HALF the diagonal, zeros above, so that A = A_L + A_L^T.
// The congruence kernels multiply with A_L only (triangular times triangular: n^3/3 instead of n^3 flops).
template <class Src>
__device__ __forceinline__ void write_low_tile(const Src &src, double *__restrict__ dst, long ld, int n, int ti, int tj) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int jj = ty; jj < 32; jj += 8) {
        const int i = ti * 32 + tx, j = tj * 32 + jj;
        if (i < ld && j < ld && i >= (j & ~127)) {      // skyline storage (gemm_geom.h): nothing above a panel's top block
            double v = 0.0;
            if (i < n && j < n && i >= j) v = (i == j) ? 0.5 * src(i, j) : src(i, j);
            dst[hdm_sky_off(i, j, (int) ld)] = v;
        }
    }
}

__global__ __launch_bounds__(256) void hdm_synth_low_kernel(double *__restrict__ full, long fstride, int n, int ld, int nt,
                                                             int c0) {
    int t = blockIdx.x, tj = 0;
    while (t >= nt - tj) { t -= nt - tj; ++tj; }
    const uint64_t P = (uint64_t) n * (n + 1) / 2;
    SynthSrc s{2 * (uint64_t) (c0 + blockIdx.y) * P, n};
    write_low_tile(s, full + (long) blockIdx.y * fstride, (long) ld, n, tj + t, tj);
}

// Entries (packed lower index, value) of a batch of matrices -> A_L form in skyline storage, scattered on the device: row q's
// entries are ent[beg[q] .. beg[q + 1]).  The target was zeroed by the caller; the diagonal takes half its value (A_L form).
// Column of a packed position p: the largest j with j (2n - j + 1) / 2 <= p, from the quadratic's root in fp64 and corrected.
__global__ __launch_bounds__(256) void hdm_scatter_low_kernel(const int *__restrict__ idx, const double *__restrict__ val,
                                                               const long *__restrict__ beg, double *__restrict__ full,
                                                               long fstride, int n, int ld) {
    const int q = blockIdx.y;
    const long e0 = beg[q], e1 = beg[q + 1];
    double *dst = full + (long) q * fstride;
    const double tn1 = 2.0 * n + 1.0;
    for (long e = e0 + (long) blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += (long) gridDim.x * blockDim.x) {
        const long p = idx[e];
        long j = (long) ((tn1 - sqrt(tn1 * tn1 - 8.0 * (double) p)) * 0.5);
        if (j < 0) j = 0;
        if (j > n - 1) j = n - 1;
        while (j + 1 < n && (j + 1) * (2L * n - (j + 1) + 1) / 2 <= p) ++j;
        while (j > 0 && j * (2L * n - j + 1) / 2 > p) --j;
        const long i = j + (p - j * (2L * n - j + 1) / 2);
        const double v = val[e];
        dst[hdm_sky_off((int) i, (int) j, ld)] = (i == j) ? 0.5 * v : v;
    }
}

// full symmetric -> A_L form in skyline storage (objective matrix)
__global__ void hdm_lower_half_kernel(const double *__restrict__ full, double *__restrict__ low, int n, long ld) {
    long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long) ld * ld) return;
    int i = (int) (e % ld), j = (int) (e / ld);
    if (i < (j & ~127)) return;
    double v = 0.0;
    if (i < n && j < n && i >= j) v = (i == j) ? 0.5 * full[e] : full[e];
    low[hdm_sky_off(i, j, (int) ld)] = v;
}

__global__ __launch_bounds__(256) void hdm_unpack_sym_kernel(const double *__restrict__ packed, long pstride,
                                                              double *__restrict__ full, long fstride, int n, int ld,
                                                              int nt) {
    // grid.x = nt*(nt+1)/2 lower tiles, grid.y = matrix in batch
    int t = blockIdx.x;
    int tj = 0;
    while (t >= nt - tj) { t -= nt - tj; ++tj; }
    int ti = tj + t;
    PackedSrc s{packed + (long) blockIdx.y * pstride, n};
    write_sym_tile(s, full + (long) blockIdx.y * fstride, (long) ld, n, ti, tj);
}

__global__ __launch_bounds__(256) void hdm_synth_kernel(double *__restrict__ full, long fstride, int n, int ld, int nt,
                                                         int c0) {
    int t = blockIdx.x;
    int tj = 0;
    while (t >= nt - tj) { t -= nt - tj; ++tj; }
    int ti = tj + t;
    const uint64_t P = (uint64_t) n * (n + 1) / 2;
    SynthSrc s{2 * (uint64_t) (c0 + blockIdx.y) * P, n};
    write_sym_tile(s, full + (long) blockIdx.y * fstride, (long) ld, n, ti, tj);
}

// C = I + sum_c y0_c A_c accumulated sequentially in c (SURVEY 8(d) step iii), full symmetric output
__global__ void hdm_synth_obj_kernel(double *__restrict__ C, int n, int ld, int m) {
    long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long) n * n) return;
    int i = (int) (e % n), j = (int) (e / n);
    if (i < j) return;
    const uint64_t P = (uint64_t) n * (n + 1) / 2;
    uint64_t k = (uint64_t) ((long) (2 * n - j - 1) * j / 2 + i);
    double acc = (i == j) ? 1.0 : 0.0;
    for (int c = 0; c < m; ++c) {
        uint64_t base = 2 * (uint64_t) c * P;
        double v = hdm_splitmix_u(base + 2 * k);
        double w = hdm_splitmix_u(base + 2 * k + 1);
        double a = (i == j || w >= 0.2) ? v : 0.0;
        double y0 = hdm_splitmix_u(2 * (uint64_t) m * P + c);
        acc += y0 * a;
    }
    C[i + (long) j * ld] = acc;
    C[j + (long) i * ld] = acc;
}

// ------------------------------------------------------------------------------------------
__global__ void hdm_blocked_eye_kernel(double *__restrict__ dst, long row_stride, long row, int nblk, int n) {
    // diagonal sub-blocks (bj == bi) of the "S row": At = L^-1 S L^-T = I (zero in the padding)
    int b = blockIdx.x;  // sub-block index along the diagonal
    int c = threadIdx.x >> 4, r = threadIdx.x & 15;
    long sub = hdm_blk_col_start(b, nblk);
    long pb = sub * 16 + c;
    int g = b * 16 + c;
    dst[(pb * row_stride + row) * 16 + r] = (r == c && g < n) ? 1.0 : 0.0;
}

// The direct rows of a block (direct_rows.h): transformed row d at matrix position (16 bi + r, 16 bj + c) is the sum of its terms,
// c (x_r y_s + y_r x_s), in table order; it goes to dst[((16 sub + c) row_stride + row0 + d) 16 + r], times sqrt(2) off the block
// diagonal as the HDM_EPI_BLOCKED epilogue has it (gemm_tile.h), an exact zero at or beyond n.  HBM-write bound.
// One workgroup = one 16 x 16 sub-block of 16 consecutive direct rows; lane (row, r) holds the 16 values of its matrix row in
// registers and stores them p-block by p-block, so that for a fixed p-block a wave writes four adjacent 128-byte lines.  The
// terms run in chunks of HDM_DR_TCH: a row's x / y slices over the sub-block's columns are staged in LDS (each lane loads one
// entry, all 16 lanes of the row read all of them), its slices over the sub-block's rows stay in registers.
constexpr int HDM_DR_TCH = 8;
constexpr int HDM_DR_LDS_ROW = HDM_DR_TCH * 16 + 2;   // (+2: the four rows of a wave read from different banks)
__global__ __launch_bounds__(256) void hdm_direct_rows_kernel(HdmDirectArgs a) {
    __shared__ double sx[16 * HDM_DR_LDS_ROW], sy[16 * HDM_DR_LDS_ROW];
    const int rl = threadIdx.x >> 4, r = threadIdx.x & 15;
    const long sub = blockIdx.x;
    const int bj = hdm_blk_col_of(sub, a.nblk), bi = bj + (int) (sub - hdm_blk_col_start(bj, a.nblk));
    const long d0 = (long) blockIdx.y * 16, d = d0 + rl;
    const bool live = d < a.nrows;
    const long t0 = live ? a.row_ptr[d] : 0, t1 = live ? a.row_ptr[d + 1] : 0;
    long kgroup = 0;   // the longest row of the group: the barriers below are reached by every lane
    for (int q = 0; q < 16; ++q) {
        const long k = (d0 + q < a.nrows) ? a.row_ptr[d0 + q + 1] - a.row_ptr[d0 + q] : 0;
        kgroup = k > kgroup ? k : kgroup;
    }
    const long gi = 16L * bi + r, gj0 = 16L * bj;
    double *mx = sx + rl * HDM_DR_LDS_ROW, *my = sy + rl * HDM_DR_LDS_ROW;
    double acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.0;
    for (long e0 = 0; e0 < kgroup; e0 += HDM_DR_TCH) {
        __syncthreads();
        for (int t = 0; t < HDM_DR_TCH; ++t) {
            const long e = t0 + e0 + t;
            if (e >= t1) break;
            const HdmDirectTerm tm = a.terms[e];
            mx[t * 16 + r] = hdm_direct_vec(tm.x, gj0 + r, a.Linv, a.ldl, a.U, a.ldu);
            my[t * 16 + r] = hdm_direct_vec(tm.y, gj0 + r, a.Linv, a.ldl, a.U, a.ldu);
        }
        __syncthreads();
        for (int t = 0; t < HDM_DR_TCH; ++t) {
            const long e = t0 + e0 + t;
            if (e >= t1) break;
            const HdmDirectTerm tm = a.terms[e];
            const double xr = hdm_direct_vec(tm.x, gi, a.Linv, a.ldl, a.U, a.ldu);
            const double yr = hdm_direct_vec(tm.y, gi, a.Linv, a.ldl, a.U, a.ldu);
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] = hdm_direct_fma(acc[c], tm.c, xr, my[t * 16 + c], yr, mx[t * 16 + c]);
        }
    }
    if (!live) return;
    const double sc = (bi == bj) ? 1.0 : 1.4142135623730951;
    double *q = a.dst + (sub * 16 * a.row_stride + a.row0 + d) * 16 + r;
#pragma unroll
    for (int c = 0; c < 16; ++c) q[(long) c * a.row_stride * 16] = (gi < a.n && gj0 + c < a.n) ? sc * acc[c] : 0.0;
}

// out = sum over the split-K slabs, in slab order (deterministic).  The Gram launch writes lower 128-tiles only, so
// elements of strictly upper tiles (R > 0: matrices are R x R) are skipped: nothing downstream reads them.
__global__ void hdm_slab_reduce_kernel(const double *__restrict__ slabs, long slab_stride, int nsplit,
                                       double *__restrict__ out, long total, long R) {
    long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    if (R > 0 && ((e / R) >> 7) > ((e % R) >> 7)) return;
    const double *p = slabs + e;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int k = 0;
    for (; k + 3 < nsplit; k += 4) {   // four loads in flight; the sum order is still fixed
        const double a = p[(long) k * slab_stride], b = p[(long) (k + 1) * slab_stride];
        const double c = p[(long) (k + 2) * slab_stride], d = p[(long) (k + 3) * slab_stride];
        s0 += a; s1 += b; s2 += c; s3 += d;
    }
    for (; k < nsplit; ++k) s0 += p[(long) k * slab_stride];
    out[e] = (s0 + s1) + (s2 + s3);
}

// G is the (R x R) augmented Gram matrix in segment order (lower valid, ld = ldg).  rows_seg maps a
// segment-ordered row to its global constraint (-1 padding, <= -2 augmented).  The augmented rows sit in
// segment 0 at pI ("I row": At = Linv Linv^T), pI+1 ("S row": At = I), pI+2 ("C row").
__device__ __forceinline__ double hdm_gsym(const double *__restrict__ G, long ldg, long a, long p) {
    return a >= p ? G[a + p * ldg] : G[p + a * ldg];
}
__global__ void hdm_extract_kernel(const double *__restrict__ G, long ldg, long R, long pI,
                                   const int *__restrict__ rows_seg, HdmMatView Mv,
                                   double *__restrict__ asinv, double *__restrict__ asinvrd,
                                   double *__restrict__ asinvc, double *__restrict__ scal, double Rd, int hsd) {
    long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e < R * R) {
        long a = e % R, b = e / R;
        if (a >= b) {
            int ga = rows_seg[a], gb = rows_seg[b];
            if (ga >= 0 && gb >= 0) {
                int r = ga > gb ? ga : gb, c = ga > gb ? gb : ga;
                *hdm_mat_at(Mv, r, c) += G[a + b * ldg];
            }
        }
    }
    if (e < R) {
        int ga = rows_seg[e];
        if (ga >= 0) {
            asinvrd[ga] += Rd * hdm_gsym(G, ldg, e, pI);
            asinv[ga] += hdm_gsym(G, ldg, e, pI + 1);
            if (hsd) asinvc[ga] += hdm_gsym(G, ldg, e, pI + 2);
        }
    }
    if (e == 0) {
        // scal: [0] TraceSinv [1] CSinv [2] CSinvCSinv [3] CSinvRdSinv
        if (Rd != 0.0) scal[0] += G[pI + 1 + pI * ldg];
        if (hsd) {
            scal[1] += G[pI + 2 + (pI + 1) * ldg];
            scal[2] += G[pI + 2 + (pI + 2) * ldg];
            scal[3] += Rd * G[pI + 2 + pI * ldg];
        }
    }
}

// S(lower incl. diag, full column-major n x n with ld) = tau*C - sum_i y_i A_i + eye*I
__global__ void hdm_sym_combine_kernel(const double *__restrict__ A, long astride, int m,
                                       const double *__restrict__ y, const double *__restrict__ C, double tau,
                                       double eye, double *__restrict__ S, int n, long lda, long lds_) {
    long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long) n * n) return;
    int i = (int) (e % n), j = (int) (e / n);
    if (i < j) return;
    const long off = hdm_sky_off(i, j, (int) lda);   // the constraint matrices: A_L form (half diagonal), skyline storage of dimension lda
    double acc = 0.0;
    for (int c = 0; c < m; ++c) acc -= y[c] * A[(long) c * astride + off];
    if (i == j) acc *= 2.0;
    acc += tau * C[i + (long) j * lda];
    if (i == j) acc += eye;
    S[i + (long) j * lds_] = acc;
}

// The same sum walked in STORAGE order: thread t of a workgroup owns skyline positions s0 + t, + 256, + 512, + 768, so a
// workgroup reads 8 KB of consecutive memory from every constraint matrix (the element-indexed kernel above reads 2 KB
// pieces, one per column segment, and half of its workgroups -- the ones above the diagonal -- leave at once), with four
// independent accumulators per thread (16-byte loads over 16 KB per workgroup measured slower: 6.2 ms against 5.84).  Positions are decoded to (i, j) only once, for the store; the stored zeros of the
// diagonal blocks' upper triangles are skipped there.
__global__ __launch_bounds__(256) void hdm_sym_combine_sky_kernel(const double *__restrict__ A, long astride, int m,
                                                                  const double *__restrict__ y, const double *__restrict__ C,
                                                                  double tau, double eye, double *__restrict__ S, int n, int lda,
                                                                  long lds_, long sky) {
    const long s0 = (long) blockIdx.x * 1024 + threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (s0 + 768 < sky) {                          // (workgroup-uniform except in the last workgroup)
        const double *p = A + s0;
#pragma unroll 4
        for (int c = 0; c < m; ++c, p += astride) {
            const double yc = y[c];
            acc[0] -= yc * p[0]; acc[1] -= yc * p[256]; acc[2] -= yc * p[512]; acc[3] -= yc * p[768];
        }
    } else {
        for (int c = 0; c < m; ++c) {
            const double yc = y[c];
            const double *p = A + (long) c * astride + s0;
#pragma unroll
            for (int q = 0; q < 4; ++q) if (s0 + 256 * q < sky) acc[q] -= yc * p[256 * q];
        }
    }
    const int tlast = (lda + 127) / 128 - 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long sp = s0 + 256 * q;
        if (sp >= sky) continue;
        int t = 0;
        while (t < tlast && hdm_sky_panel(t + 1, lda) <= sp) ++t;
        const long local = sp - hdm_sky_panel(t, lda);
        const int ldp = lda - 128 * t;
        const int i = 128 * t + (int) (local % ldp), j = 128 * t + (int) (local / ldp);
        if (i < j || i >= n || j >= n) continue;
        double v = acc[q];
        if (i == j) v *= 2.0;
        v += tau * C[i + (long) j * lda];
        if (i == j) v += eye;
        S[i + (long) j * lds_] = v;
    }
}

// ------------------------------------------------------------------------------------------
// zero-suppressed sweep format (schur.h: HdmZs).  Workgroup b owns skyline positions 1024 b .. 1024 b + 1023 = 16 mask words of
// every matrix; bit l of word w is position 1024 b + 64 w + l.  The two builder kernels run four waves of four words each, the
// sweep two waves of eight; a wave's mask words and offsets are wave-uniform: scalar loads.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned hdm_lanes_below(unsigned long long mask) {   // set bits of `mask` below this lane
    return __builtin_amdgcn_mbcnt_hi((unsigned) (mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) mask, 0u));
}

// pass 1: non-zeros per chunk of the m matrices at A, ADDED to total[] (the builder walks the data batch by batch)
__global__ __launch_bounds__(256) void hdm_zs_count_kernel(const double *__restrict__ A, long astride, int m, long sky,
                                                            unsigned long long *__restrict__ total) {
    __shared__ unsigned long long wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long p0 = (long) blockIdx.x * 1024 + 256 * wave + lane;
    unsigned long long cnt = 0;
    for (int c = 0; c < m; ++c) {
        const double *a = A + (long) c * astride;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long p = p0 + 64 * q;
            const double v = (p < sky) ? a[p] : 0.0;
            cnt += (unsigned long long) __popcll(__ballot(v != 0.0));
        }
    }
    if (lane == 0) wsum[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) total[blockIdx.x] += wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// pass 2: masks, offsets and values of chunk b, matrix after matrix (the offsets run on through the chunk's range).  The m
// matrices at A are matrices c0 .. c0 + m - 1 of mtot; run[b] carries the chunk's fill from one batch to the next.
__global__ __launch_bounds__(256) void hdm_zs_fill_kernel(const double *__restrict__ A, long astride, int m, long sky,
                                                           const unsigned long long *__restrict__ base,
                                                           unsigned long long *__restrict__ meta, double *__restrict__ val,
                                                           int c0, int mtot, unsigned *__restrict__ run) {
    __shared__ unsigned pc[2][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long p0 = (long) blockIdx.x * 1024 + 256 * wave + lane;
    double *out = val + base[blockIdx.x];
    unsigned running = run[blockIdx.x];
    for (int c = 0; c < m; ++c) {
        const double *a = A + (long) c * astride;
        double v[4];
        unsigned long long mk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long p = p0 + 64 * q;
            v[q] = (p < sky) ? a[p] : 0.0;
            mk[q] = __ballot(v[q] != 0.0);
            if (lane == 0) pc[c & 1][4 * wave + q] = (unsigned) __popcll(mk[q]);
        }
        __syncthreads();                     // (two buffers: the next matrix writes the other one before anyone can lag two behind)
        unsigned before = running, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const unsigned k = pc[c & 1][w];
            if (w < 4 * wave) before += k;
            all += k;
        }
        unsigned long long *rec = meta + ((long) blockIdx.x * mtot + c0 + c) * 24;
        unsigned off = before;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (lane == 0) {
                rec[4 * wave + q] = mk[q];
                reinterpret_cast<unsigned *>(rec + 16)[4 * wave + q] = off;
            }
            if ((mk[q] >> lane) & 1ULL) out[off + hdm_lanes_below(mk[q])] = v[q];
            off += (unsigned) __popcll(mk[q]);
        }
        running += all;
    }
    __syncthreads();
    if (threadIdx.x == 0) run[blockIdx.x] = running;
}

// The copy back into A_L-form skyline storage: matrices c0 .. c0 + count - 1 of the copy, chunk by chunk (zeros where the mask has
// none).  A cone whose ingested rows are too many to stay resident keeps ONLY the copy and expands a batch of rows whenever the
// congruence (or any other reader of the dense form) asks for one -- what the counter-based generator does for the synthetic
// family (engine_rows.h: MiRows::rows).  blockIdx.y splits the matrices of a chunk over several workgroups.
__global__ __launch_bounds__(256) void hdm_zs_expand_kernel(const unsigned long long *__restrict__ meta, const double *__restrict__ val,
                                                             const unsigned long long *__restrict__ base, int mtot, int c0, int count,
                                                             double *__restrict__ A, long astride, long sky) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long p0 = (long) blockIdx.x * 1024 + 256 * wave + lane;
    const double *src = val + base[blockIdx.x];
    for (int c = blockIdx.y; c < count; c += gridDim.y) {
        const unsigned long long *rec = meta + ((long) blockIdx.x * mtot + c0 + c) * 24;
        double *a = A + (long) c * astride;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long mk = rec[4 * wave + q];
            const unsigned off = reinterpret_cast<const unsigned *>(rec + 16)[4 * wave + q];
            const long p = p0 + 64 * q;
            const double v = ((mk >> lane) & 1ULL) ? src[off + hdm_lanes_below(mk)] : 0.0;
            if (p < sky) a[p] = v;
        }
    }
}

// S(lower incl. diag) = tau*C - sum_i y_i A_i + eye*I from the zero-suppressed copy: the sums of hdm_sym_combine_sky_kernel
// term by term in the same order, without the terms whose a is an exact zero.
// Workgroup = one chunk, two waves: wave w owns mask words 8 w .. 8 w + 7 (lane l of word q = position 1024 b + 512 w + 64 q + l),
// so a chunk row is 4160 waves at n16 = 2000 -- all resident at once (the 2080 four-wave workgroups of the dense sweep need a
// second, nearly empty round).  Two matrices per trip: their 16 mask words, first offsets and multipliers sit in SGPRs (a word
// is its own lane mask: the loads of a word's zeros are switched off by it, v_cndmask takes it as is; the offsets of words
// 1..7 are running popcounts); the metadata of the NEXT trip is requested after this trip's value loads have been issued and
// before they are waited for, so its latency hides behind theirs (scalar loads return out of order: any wait for them is a
// wait for all, which is why the request may not come earlier).
struct HdmZsTrip { unsigned long long mk[2][8]; unsigned off[2]; double y[2]; };
__global__ __launch_bounds__(128) void hdm_sym_combine_zs_kernel(const unsigned long long *__restrict__ meta,
                                                                  const double *__restrict__ val,
                                                                  const unsigned long long *__restrict__ base, int m,
                                                                  const double *__restrict__ y, const double *__restrict__ C,
                                                                  double tau, double eye, double *__restrict__ S, int n, int lda,
                                                                  long lds_, long sky) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double *v0 = val + base[blockIdx.x];
    const unsigned long long *rec = meta + (long) blockIdx.x * m * 24 + 8 * wave;                                   // this wave's 8 mask words of matrix 0
    const unsigned *offp = reinterpret_cast<const unsigned *>(meta + (long) blockIdx.x * m * 24 + 16) + 8 * wave;   // offset of its first word
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    auto load_trip = [&](HdmZsTrip &t, int c) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const unsigned long long *r = rec + (long) (c + u) * 24;
#pragma unroll
            for (int q = 0; q < 8; ++q) t.mk[u][q] = r[q];
            t.off[u] = offp[(long) (c + u) * 48];
            t.y[u] = y[c + u];
        }
    };
    auto issue = [&](const HdmZsTrip &t, double (&a)[2][8]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            unsigned o = t.off[u];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                a[u][q] = v0[o + hdm_lanes_below(t.mk[u][q])];      // (unconditional: the lanes of a word's zeros read a neighbour's value and drop it below)
                o += (unsigned) __popcll(t.mk[u][q]);
            }
        }
    };
    auto accumulate = [&](const HdmZsTrip &t, const double (&a)[2][8]) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] -= t.y[u] * (__builtin_amdgcn_inverse_ballot_w64(t.mk[u][q]) ? a[u][q] : 0.0);
    };
    HdmZsTrip A, B;
    double a[2][8];
    const int mp = m & ~1;
    int c = 0;
    if (mp >= 2) load_trip(A, 0);
    for (; c + 4 <= mp; c += 4) {
        issue(A, a);
        __builtin_amdgcn_sched_barrier(0);
        load_trip(B, c + 2);
        __builtin_amdgcn_sched_barrier(0);
        accumulate(A, a);
        issue(B, a);
        __builtin_amdgcn_sched_barrier(0);
        load_trip(A, min(c + 4, mp - 2));
        __builtin_amdgcn_sched_barrier(0);
        accumulate(B, a);
    }
    if (c + 2 <= mp) { issue(A, a); accumulate(A, a); c += 2; }
    if (c < m) {                                  // odd count: the last matrix alone
        const unsigned long long *r = rec + (long) c * 24;
        unsigned o = offp[(long) c * 48];
        const double yc = y[c];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const unsigned long long mk = r[q];
            const double v = __builtin_amdgcn_inverse_ballot_w64(mk) ? v0[o + hdm_lanes_below(mk)] : 0.0;
            o += (unsigned) __popcll(mk);
            acc[q] -= yc * v;
        }
    }
    const int tlast = (lda + 127) / 128 - 1;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const long sp = (long) blockIdx.x * 1024 + 512 * wave + 64 * q + lane;
        if (sp >= sky) continue;
        int t = 0;
        while (t < tlast && hdm_sky_panel(t + 1, lda) <= sp) ++t;
        const long local = sp - hdm_sky_panel(t, lda);
        const int ldp = lda - 128 * t;
        const int i = 128 * t + (int) (local % ldp), j = 128 * t + (int) (local / ldp);
        if (i < j || i >= n || j >= n) continue;
        double v = acc[q];
        if (i == j) v *= 2.0;
        v += tau * C[i + (long) j * lda];
        if (i == j) v += eye;
        S[i + (long) j * lds_] = v;
    }
}

// <A_c, X> and <A_c, Y> for all matrices from the zero-suppressed copy (the corrector's two dot products per constraint,
// hdsdp_conic_sdp.c:1035-1056; primal recovery): workgroup = one chunk, two waves of eight words as in the sweep above.  A lane
// keeps the X and Y elements of its eight positions in registers for the whole pass -- X and Y are read ONCE, where the dense
// kernel re-reads them for every group of four matrices -- and multiplies them with the values of matrix after matrix; the
// per-lane products of 16 matrices are parked in LDS and added up across the lanes by 16 x 4 lanes at a time (two shuffles to
// finish), so a matrix costs four LDS accesses per lane instead of a dozen cross-lane steps.  Partial sums per (chunk, wave,
// matrix) go to `part`, folded in fixed order by the two kernels below.
#define ZS_DB 16
__global__ __launch_bounds__(128) void hdm_sym_dot2_zs_kernel(const unsigned long long *__restrict__ meta,
                                                               const double *__restrict__ val,
                                                               const unsigned long long *__restrict__ base, int m,
                                                               const double *__restrict__ X, const double *__restrict__ Y, long ldx,
                                                               int n, int lda, long sky, double *__restrict__ part) {
    __shared__ double tile[2][2][ZS_DB][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double *v0 = val + base[blockIdx.x];
    const unsigned long long *rec = meta + (long) blockIdx.x * m * 24 + 8 * wave;
    const unsigned *offp = reinterpret_cast<const unsigned *>(meta + (long) blockIdx.x * m * 24 + 16) + 8 * wave;
    double xv[8], yv[8];
    const int tlast = (lda + 127) / 128 - 1;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const long sp = (long) blockIdx.x * 1024 + 512 * wave + 64 * q + lane;
        xv[q] = 0.0; yv[q] = 0.0;
        if (sp < sky) {
            int t = 0;
            while (t < tlast && hdm_sky_panel(t + 1, lda) <= sp) ++t;
            const long local = sp - hdm_sky_panel(t, lda);
            const int ldp = lda - 128 * t;
            const int i = 128 * t + (int) (local % ldp), j = 128 * t + (int) (local / ldp);
            if (i >= j && i < n && j < n) {
                xv[q] = X[i + (long) j * ldx];
                if (Y) yv[q] = Y[i + (long) j * ldx];
            }
        }
    }
    double *prow = part + ((long) (blockIdx.x * 2 + wave) * m) * 2;
    // two matrices per trip, the next trip's metadata requested behind this trip's value loads (as in the sweep above)
    auto load_trip = [&](HdmZsTrip &t, int c) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int cc = min(c + u, m - 1);          // (an odd count repeats the last matrix; its products are not kept)
            const unsigned long long *r = rec + (long) cc * 24;
#pragma unroll
            for (int q = 0; q < 8; ++q) t.mk[u][q] = r[q];
            t.off[u] = offp[(long) cc * 48];
        }
    };
    auto issue = [&](const HdmZsTrip &t, double (&a)[2][8]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            unsigned o = t.off[u];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                a[u][q] = v0[o + hdm_lanes_below(t.mk[u][q])];      // (unconditional, as in the sweep)
                o += (unsigned) __popcll(t.mk[u][q]);
            }
        }
    };
    auto park = [&](const HdmZsTrip &t, const double (&a)[2][8], int slot) {   // products of the trip's two matrices into tile rows slot, slot + 1
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            double px = 0.0, py = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const double av = __builtin_amdgcn_inverse_ballot_w64(t.mk[u][q]) ? a[u][q] : 0.0;
                px += av * xv[q]; py += av * yv[q];
            }
            tile[wave][0][slot + u][lane] = px;
            tile[wave][1][slot + u][lane] = py;
        }
    };
    HdmZsTrip A, B;
    double a[2][8];
    load_trip(A, 0);
    for (int c0 = 0; c0 < m; c0 += ZS_DB) {
        const int nb = min(ZS_DB, m - c0);
        // (ZS_DB / 2 = 8 trips per batch, A and B alternating; trips past the end of the data reload the last matrix and park
        // products nobody reads -- the loop stays uniform)
#pragma unroll
        for (int tr = 0; tr < ZS_DB / 2; tr += 2) {
            issue(A, a);
            __builtin_amdgcn_sched_barrier(0);
            load_trip(B, c0 + 2 * tr + 2);
            __builtin_amdgcn_sched_barrier(0);
            park(A, a, 2 * tr);
            issue(B, a);
            __builtin_amdgcn_sched_barrier(0);
            load_trip(A, c0 + 2 * tr + 4);
            __builtin_amdgcn_sched_barrier(0);
            park(B, a, 2 * tr + 2);
        }
        __syncthreads();
        {
            const int u = lane & 15, qt = lane >> 4;
            double sx = 0.0, sy = 0.0;
#pragma unroll
            for (int t = 0; t < 16; ++t) { sx += tile[wave][0][u][qt * 16 + t]; sy += tile[wave][1][u][qt * 16 + t]; }
            sx += __shfl_xor(sx, 16, 64); sy += __shfl_xor(sy, 16, 64);
            sx += __shfl_xor(sx, 32, 64); sy += __shfl_xor(sy, 32, 64);
            if (lane < nb) { prow[(long) (c0 + lane) * 2] = sx; prow[(long) (c0 + lane) * 2 + 1] = sy; }
        }
        __syncthreads();
    }
}

// out[y][c][v] = sum over the rows r = y, y + nfold, ... of part[r][c][v]   (first level of the fold; the second is
// hdm_sym_dot2_reduce_kernel over the nfold rows)
__global__ void hdm_dot2_fold_kernel(const double *__restrict__ part, long rows, int count, int nfold, double *__restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (c >= count) return;
    double tx = 0.0, ty = 0.0;
    for (long r = y; r < rows; r += nfold) {
        const double2 v = *reinterpret_cast<const double2 *>(part + (r * count + c) * 2);
        tx += v.x; ty += v.y;
    }
    out[((long) y * count + c) * 2] = tx;
    out[((long) y * count + c) * 2 + 1] = ty;
}

// ------------------------------------------------------------------------------------------
// rank-one (M2) path.  U = Linv * [a_1 .. a_m] (n x m), Gm = U^T U  =>  Gm_ij = a_i' S^-1 a_j
//   M_ij = s_i s_j Gm_ij^2 ; ASinv_i = s_i Gm_ii ; ASinvRdSinv_i = Rd s_i |S^-1 a_i|^2 = Rd s_i |Linv^T u_i|^2
// ------------------------------------------------------------------------------------------
__global__ void hdm_r1_hadamard_kernel(const double *__restrict__ Gm, long ldg, const double *__restrict__ sgn,
                                       const int *__restrict__ rows_global, int mloc, HdmMatView Mv,
                                       double *__restrict__ asinv) {
    long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long) mloc * mloc) return;
    int i = (int) (e % mloc), j = (int) (e / mloc);
    if (i < j) return;
    double g = Gm[i + (long) j * ldg];
    int gi = rows_global[i], gj = rows_global[j];
    int r = gi > gj ? gi : gj, c = gi > gj ? gj : gi;
    *hdm_mat_at(Mv, r, c) += sgn[i] * sgn[j] * g * g;
    if (i == j) asinv[gi] += sgn[i] * g;
}

__global__ void hdm_r1_colnorm_kernel(const double *__restrict__ V, long ldv, int n, const double *__restrict__ sgn,
                                      const int *__restrict__ rows_global, int mloc, double Rd,
                                      double *__restrict__ asinvrd) {
    // one wave per column
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int c = blockIdx.x * 4 + wave;
    if (c >= mloc) return;
    double s = 0.0;
    for (int i = lane; i < n; i += 64) { double v = V[i + (long) c * ldv]; s += v * v; }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) asinvrd[rows_global[c]] += Rd * sgn[c] * s;
}

// <A_i, X> for full symmetric A_i, X (both n x n, ld): one workgroup per constraint (corrector, M5 traces)
// <A_i, X> and <A_i, Y> for a group of 4 constraints and one chunk of columns, lower triangle only (the constraint
// matrices are stored in A_L form: nothing above the diagonal): every X / Y element is loaded once for four A's, and
// the first version's full-square sweep with X and Y re-read per constraint (200 % overhead, 18 ms per corrector build
// at n = m = 2000) becomes one pass over the 32 GB of lower triangles.  Partial sums go to part[chunk][constraint][2]
// and are added up in chunk order by hdm_sym_dot2_reduce_kernel (deterministic, no atomics).
#define DOT2_G 4
__global__ __launch_bounds__(256) void hdm_sym_dot2_kernel(const double *__restrict__ A, long astride, int n, long lda,
                                                            int count, const double *__restrict__ X,
                                                            const double *__restrict__ Y, long ldx, int nchunk,
                                                            double *__restrict__ part) {
    __shared__ double red[2 * DOT2_G][4];
    const int g0 = blockIdx.x * DOT2_G, ch = blockIdx.y;
    const int cw = (n + nchunk - 1) / nchunk, j0 = ch * cw, j1 = min(n, j0 + cw);
    const double *Aq[DOT2_G];
#pragma unroll
    for (int q = 0; q < DOT2_G; ++q) Aq[q] = A + (long) min(g0 + q, count - 1) * astride;   // clamped: surplus slots repeat the last one
    double ax[DOT2_G], ay[DOT2_G];
#pragma unroll
    for (int q = 0; q < DOT2_G; ++q) { ax[q] = 0.0; ay[q] = 0.0; }
    for (int j = j0; j < j1; ++j) {
        const double *xc = X + (long) j * ldx, *yc = Y ? Y + (long) j * ldx : nullptr;
        const long cj = hdm_sky_off(0, j, (int) lda);      // column j of a skyline-stored A_L matrix (element (i, j) at cj + i)
        for (int i = j + threadIdx.x; i < n; i += 256) {
            const double x = xc[i], y = yc ? yc[i] : 0.0;
#pragma unroll
            for (int q = 0; q < DOT2_G; ++q) {
                const double a = Aq[q][cj + i];
                ax[q] += a * x;
                ay[q] += a * y;
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < DOT2_G; ++q) {
        double sx = ax[q], sy = ay[q];
        for (int off = 32; off > 0; off >>= 1) { sx += __shfl_down(sx, off, 64); sy += __shfl_down(sy, off, 64); }
        if (lane == 0) { red[2 * q][wave] = sx; red[2 * q + 1][wave] = sy; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * DOT2_G) {
        const int q = threadIdx.x >> 1, which = threadIdx.x & 1;
        if (g0 + q < count)
            part[((long) ch * count + g0 + q) * 2 + which] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    }
}

__global__ void hdm_sym_dot2_reduce_kernel(const double *__restrict__ part, int count, int nchunk, int has_y,
                                           double *__restrict__ outx, double *__restrict__ outy,
                                           const int *__restrict__ rows_global, double sx, double sy) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    double tx = 0.0, ty = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) { tx += part[((long) ch * count + c) * 2]; ty += part[((long) ch * count + c) * 2 + 1]; }
    const int gi = rows_global[c];
    outx[gi] += sx * tx;
    if (has_y) outy[gi] += sy * ty;
}

// ------------------------------------------------------------------------------------------
// sparse (M5) path: no intermediate matrix, entries of X = S^-1 are gathered per pair of nonzeros
// (reference: KKT5Pair_Sparse_Sparse, linalg/hdsdp_sdpdata.c:1711-1760, and its rank-one variants).
// Constraint i is a list of lower triplets (p >= q, a); one wavefront per pair (i >= j):
//   M_ij = sum_{(p,q,a) in A_i} sum_{(r,s,b) in A_j} a b [ X_qr X_sp + (r!=s) X_qs X_rp + (p!=q) X_pr X_sq + (p!=q)(r!=s) X_ps X_rq ]
// lanes stride over the nnz_i x nnz_j products, the partial sums are reduced with wave shuffles.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hdm_sparse_pair_kernel(const int *__restrict__ rp, const int *__restrict__ ti,
                                                               const int *__restrict__ tj, const double *__restrict__ tv,
                                                               const double *__restrict__ X, long ldx, int mloc,
                                                               const int *__restrict__ rows_global,
                                                               HdmMatView Mv) {
    const int lane = threadIdx.x & 63;
    const long t = (long) blockIdx.x * 4 + (threadIdx.x >> 6);
    const long npairs = (long) mloc * (mloc + 1) / 2;
    if (t >= npairs) return;
    long i = (long) ((sqrt(8.0 * (double) t + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    const long j = t - i * (i + 1) / 2;
    const int bi = rp[i], ni = rp[i + 1] - bi, bj = rp[j], nj = rp[j + 1] - bj;
    double acc = 0.0;
    const long tot = (long) ni * nj;
    for (long e = lane; e < tot; e += 64) {
        const int ei = bi + (int) (e / nj), ej = bj + (int) (e % nj);
        const int p = ti[ei], q = tj[ei], r = ti[ej], s = tj[ej];
        double g = X[q + r * ldx] * X[s + p * ldx];
        if (r != s) g += X[q + s * ldx] * X[r + p * ldx];
        if (p != q) {
            g += X[p + r * ldx] * X[s + q * ldx];
            if (r != s) g += X[p + s * ldx] * X[r + q * ldx];
        }
        acc += tv[ei] * tv[ej] * g;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0 && tot > 0) {
        const int gi = rows_global[i], gj = rows_global[j];
        const int rr = gi > gj ? gi : gj, cc = gi > gj ? gj : gi;
        *hdm_mat_at(Mv, rr, cc) += acc;
    }
}

// out[row] += scale * <A_row, Y> for triplet rows and a full symmetric Y: one wavefront per row
__global__ __launch_bounds__(256) void hdm_sparse_dot_kernel(const int *__restrict__ rp, const int *__restrict__ ti,
                                                              const int *__restrict__ tj, const double *__restrict__ tv,
                                                              const double *__restrict__ Y, long ldy, int mloc,
                                                              const int *__restrict__ rows_global, double scale,
                                                              double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= mloc) return;
    double acc = 0.0;
    for (int e = rp[i] + lane; e < rp[i + 1]; e += 64) {
        const int p = ti[e], q = tj[e];
        acc += tv[e] * Y[p + q * ldy] * (p != q ? 2.0 : 1.0);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) out[rows_global[i]] += scale * acc;
}

// ------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------
int hdm_scatter_low(const int *idx, const double *val, const long *beg, long max_per_row, double *full, long fstride, int n, int ld,
                    int batch, hipStream_t s) {
    if (batch <= 0) return 0;
    const unsigned gx = (unsigned) std::max(1L, std::min(256L, (max_per_row + 1023) / 1024));
    hipLaunchKernelGGL(hdm_scatter_low_kernel, dim3(gx, batch), dim3(256), 0, s, idx, val, beg, full, fstride, n, ld);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_synth_fill_low(double *full, long fstride, int n, int ld, int c0, int batch, hipStream_t s) {
    int nt = (ld + 31) / 32;
    dim3 grid(nt * (nt + 1) / 2, batch), block(32, 8);
    hipLaunchKernelGGL(hdm_synth_low_kernel, grid, block, 0, s, full, fstride, n, ld, nt, c0);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_lower_half(const double *full, double *low, int n, long ld, hipStream_t s) {
    long tot = ld * ld;
    hipLaunchKernelGGL(hdm_lower_half_kernel, dim3((unsigned) ((tot + 255) / 256)), dim3(256), 0, s, full, low, n, ld);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_unpack_sym(const double *packed, long pstride, double *full, long fstride, int n, int ld, int batch, hipStream_t s) {
    int nt = (ld + 31) / 32;
    dim3 grid(nt * (nt + 1) / 2, batch), block(32, 8);
    hipLaunchKernelGGL(hdm_unpack_sym_kernel, grid, block, 0, s, packed, pstride, full, fstride, n, ld, nt);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_synth_fill(double *full, long fstride, int n, int ld, int c0, int batch, hipStream_t s) {
    int nt = (ld + 31) / 32;
    dim3 grid(nt * (nt + 1) / 2, batch), block(32, 8);
    hipLaunchKernelGGL(hdm_synth_kernel, grid, block, 0, s, full, fstride, n, ld, nt, c0);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_synth_obj(double *C, int n, int ld, int m, hipStream_t s) {
    long tot = (long) n * n;
    hipLaunchKernelGGL(hdm_synth_obj_kernel, dim3((unsigned) ((tot + 255) / 256)), dim3(256), 0, s, C, n, ld, m);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_blocked_eye(double *dst, long row_stride, long row, int nblk, int n, hipStream_t s) {
    hipLaunchKernelGGL(hdm_blocked_eye_kernel, dim3(nblk), dim3(256), 0, s, dst, row_stride, row, nblk, n);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// Bounds of a direct-rows launch, checked here before it runs.  Stores: the last line written is that of local row
// row0 + nrows - 1 in p-block 16 nsub - 1, i.e. element ((16 nsub - 1) row_stride + row0 + nrows - 1) 16 + 15 of dst.  Loads: entry
// i <= 16 nblk - 1 of column v <= max_lcol of Linv (element i + v ldl) or of column j < nu of U (element i + j ldu); the terms and
// row_ptr are the cone's own table, whose vector indices were held to max_lcol and nu when it was made.
int hdm_direct_rows(const HdmDirectArgs &a, hipStream_t s) {
    if (a.nrows <= 0) return 0;
    const long n16 = 16L * a.nblk, nsub = (long) a.nblk * (a.nblk + 1) / 2, groups = (a.nrows + 15L) / 16;
    const long dst_need = ((16 * nsub - 1) * a.row_stride + a.row0 + a.nrows - 1) * 16 + 16;
    const long linv_need = a.max_lcol >= 0 ? (long) a.max_lcol * a.ldl + n16 : 0;
    const long u_need = a.nu > 0 ? (long) (a.nu - 1) * a.ldu + n16 : 0;
    if (a.row0 < 0 || a.row0 + a.nrows > a.row_stride || a.n > n16 || a.max_lcol >= a.n || a.ldl < n16 || a.ldu < n16 ||
        dst_need > a.dst_span || linv_need > a.linv_span || u_need > a.u_span || groups > 65535 || nsub > 2147483647L) {
        fprintf(stderr, "[hdsdp_mi355x] direct rows: the launch needs %ld / %ld / %ld elements of the row buffer, the factor inverse and "
                        "the transformed factors, the caller vouches for %ld / %ld / %ld: launch refused\n",
                dst_need, linv_need, u_need, a.dst_span, a.linv_span, a.u_span);
        return 1;
    }
    hipLaunchKernelGGL(hdm_direct_rows_kernel, dim3((unsigned) nsub, (unsigned) groups), dim3(256), 0, s, a);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_slab_reduce(const double *slabs, long slab_stride, int nsplit, double *out, long total, long R, hipStream_t s) {
    hipLaunchKernelGGL(hdm_slab_reduce_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, s, slabs,
                       slab_stride, nsplit, out, total, R);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_extract(const double *G, long ldg, long R, long pI, const int *rows_seg, const HdmMatView &Mv, double *asinv,
                double *asinvrd, double *asinvc, double *scal, double Rd, int hsd, hipStream_t s) {
    long tot = R * R;
    hipLaunchKernelGGL(hdm_extract_kernel, dim3((unsigned) ((tot + 255) / 256)), dim3(256), 0, s, G, ldg, R, pI,
                       rows_seg, Mv, asinv, asinvrd, asinvc, scal, Rd, hsd);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_sym_combine(const double *A, long astride, int m, const double *y, const double *C, double tau, double eye,
                    double *S, int n, long lda, long lds_, hipStream_t s) {
    const bool sky_order = hdm_env_on<ENV_SYM_COMBINE_SKY>();
    const long sky = hdm_sky_size((int) lda);
    if (sky_order && m > 0) {
        hipLaunchKernelGGL(hdm_sym_combine_sky_kernel, dim3((unsigned) ((sky + 1023) / 1024)), dim3(256), 0, s, A, astride, m, y, C,
                           tau, eye, S, n, (int) lda, lds_, sky);
        HDM_HIP_CHECK(hipGetLastError());
        return 0;
    }
    long tot = (long) n * n;
    hipLaunchKernelGGL(hdm_sym_combine_kernel, dim3((unsigned) ((tot + 255) / 256)), dim3(256), 0, s, A, astride, m, y,
                       C, tau, eye, S, n, lda, lds_);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_zs_build_from(const std::function<const double *(int, int)> &source, int batch, long astride, int m, long sky,
                      double max_fill, HdmZs *out, hipStream_t s) {
    *out = HdmZs();
    if (m <= 0 || sky <= 0 || batch <= 0) return 0;
    const long nchunk = (sky + 1023) / 1024;
    if ((double) m * 1024.0 >= 4.0e9) return 0;           // a chunk's offsets are 32-bit
    HdmBuf<unsigned long long> total_own;
    HdmBuf<unsigned> run_own;
    // every way out below leaves nothing behind: the two locals go with the scope, `out` is emptied
    auto fail = [&](int rc) { (void) hipGetLastError(); hdm_zs_free(out); return rc; };
    if (total_own.alloc((size_t) nchunk) != hipSuccess) return fail(1);
    unsigned long long *total = total_own.get();
    if (hipMemsetAsync(total, 0, sizeof(unsigned long long) * nchunk, s) != hipSuccess) return fail(1);
    for (int c0 = 0; c0 < m; c0 += batch) {
        const int nb = std::min(batch, m - c0);
        const double *A = source(c0, nb);
        if (!A) return fail(1);
        hipLaunchKernelGGL(hdm_zs_count_kernel, dim3((unsigned) nchunk), dim3(256), 0, s, A, astride, nb, sky, total);
        if (hipGetLastError() != hipSuccess) return fail(1);
    }
    std::vector<unsigned long long> h(nchunk);
    if (hipMemcpyAsync(h.data(), total, sizeof(unsigned long long) * nchunk, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) return fail(1);
    unsigned long long run = 0;
    for (long b = 0; b < nchunk; ++b) { const unsigned long long k = h[b]; h[b] = run; run += k; }
    if ((double) run > max_fill * (double) m * (double) sky) return fail(0);   // not worth the memory
    out->base = std::move(total_own);                      // reused: counts -> exclusive offsets
    if (hipMemcpyAsync(out->base.get(), h.data(), sizeof(unsigned long long) * nchunk, hipMemcpyHostToDevice, s) != hipSuccess) return fail(1);
    // (+ 64 values of slack: the lanes behind a word's last non-zero read the slot that follows)
    if (out->val.alloc((size_t) (run + 64)) != hipSuccess || out->meta.alloc(24 * (size_t) nchunk * m) != hipSuccess ||
        run_own.alloc((size_t) nchunk) != hipSuccess)
        return fail(0);                                    // no memory for the copy: the dense sweep stays
    unsigned *run_dev = run_own.get();
    if (hipMemsetAsync(out->val.get() + run, 0, sizeof(double) * 64, s) != hipSuccess ||
        hipMemsetAsync(run_dev, 0, sizeof(unsigned) * nchunk, s) != hipSuccess) return fail(1);
    for (int c0 = 0; c0 < m; c0 += batch) {
        const int nb = std::min(batch, m - c0);
        const double *A = source(c0, nb);
        if (!A) return fail(1);
        hipLaunchKernelGGL(hdm_zs_fill_kernel, dim3((unsigned) nchunk), dim3(256), 0, s, A, astride, nb, sky, out->base.get(), out->meta.get(), out->val.get(),
                           c0, m, run_dev);
        if (hipGetLastError() != hipSuccess) return fail(1);
    }
    if (hipStreamSynchronize(s) != hipSuccess) return fail(1);
    out->nchunk = nchunk; out->sky = sky; out->nnz = (long) run; out->m = m;
    return 0;
}

int hdm_zs_expand(const HdmZs &z, int c0, int count, double *A, long astride, hipStream_t s) {
    if (!z.val || c0 < 0 || count < 0 || c0 + count > z.m) return 1;
    if (count == 0) return 0;
    const unsigned gy = (unsigned) std::max(1, std::min(count, 16));
    hipLaunchKernelGGL(hdm_zs_expand_kernel, dim3((unsigned) z.nchunk, gy), dim3(256), 0, s, z.meta.get(), z.val.get(), z.base.get(), z.m, c0, count, A, astride, z.sky);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_zs_build(const double *A, long astride, int m, long sky, double max_fill, HdmZs *out, hipStream_t s) {
    return hdm_zs_build_from([&](int c0, int) { return A + (long) c0 * astride; }, std::max(1, m), astride, m, sky, max_fill, out, s);
}

void hdm_zs_free(HdmZs *z) { *z = HdmZs(); }

int hdm_sym_combine_zs(const HdmZs &z, const double *y, const double *C, double tau, double eye, double *S, int n, long lda,
                       long lds_, hipStream_t s) {
    hipLaunchKernelGGL(hdm_sym_combine_zs_kernel, dim3((unsigned) z.nchunk), dim3(128), 0, s, z.meta.get(), z.val.get(), z.base.get(), z.m, y, C, tau,
                       eye, S, n, (int) lda, lds_, z.sky);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// partial-sum scratch of the two dot-product sweeps: one buffer per host thread AND device (a host thread normally drives one
// device -- the caller's, or one shard of a device group -- but the caller's thread may move to another one over its life:
// HMiDeviceInit on another id, HMiSetDevices followed by plain cones; a buffer bound to the device of the first call would then
// be read by a kernel on the other).  Kept until the process ends: thread-local storage, so a raw pointer on purpose (an owning
// type's destructor would call hipFree at thread or process exit, after the runtime may have shut down).
static double *dot2_scratch(size_t need) {
    struct Buf { double *p = nullptr; size_t cap = 0; };
    static thread_local std::map<int, Buf> bufs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    Buf &b = bufs[dev];
    if (need > b.cap) {
        if (b.p) (void) hipFree(b.p);
        b.p = nullptr; b.cap = 0;
        if (hdm_malloc((void **) &b.p, need) != hipSuccess) { (void) hipGetLastError(); b.p = nullptr; return nullptr; }
        b.cap = need;
    }
    return b.p;
}

int hdm_sym_dot2_zs(const HdmZs &z, int n, long lda, const double *X, const double *Y, long ldx, double *outx, double *outy,
                    const int *rows_global, double sx, double sy, hipStream_t s) {
    if (z.m <= 0) return 0;
    const int nfold = 64;
    const long rows = 2 * z.nchunk;
    double *part = dot2_scratch(sizeof(double) * 2 * (size_t) z.m * (size_t) (rows + nfold));
    if (!part) return 1;
    double *folded = part + 2 * (size_t) z.m * rows;
    hipLaunchKernelGGL(hdm_sym_dot2_zs_kernel, dim3((unsigned) z.nchunk), dim3(128), 0, s, z.meta.get(), z.val.get(), z.base.get(), z.m, X, Y, ldx, n,
                       (int) lda, z.sky, part);
    hipLaunchKernelGGL(hdm_dot2_fold_kernel, dim3((z.m + 255) / 256, nfold), dim3(256), 0, s, part, rows, z.m, nfold, folded);
    hipLaunchKernelGGL(hdm_sym_dot2_reduce_kernel, dim3((z.m + 255) / 256), dim3(256), 0, s, folded, z.m, nfold, Y ? 1 : 0, outx,
                       outy, rows_global, sx, sy);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_r1_hadamard(const double *Gm, long ldg, const double *sgn, const int *rows_global, int mloc, const HdmMatView &Mv,
                    double *asinv, hipStream_t s) {
    long tot = (long) mloc * mloc;
    hipLaunchKernelGGL(hdm_r1_hadamard_kernel, dim3((unsigned) ((tot + 255) / 256)), dim3(256), 0, s, Gm, ldg, sgn,
                       rows_global, mloc, Mv, asinv);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_r1_colnorm(const double *V, long ldv, int n, const double *sgn, const int *rows_global, int mloc, double Rd,
                   double *asinvrd, hipStream_t s) {
    hipLaunchKernelGGL(hdm_r1_colnorm_kernel, dim3((mloc + 3) / 4), dim3(256), 0, s, V, ldv, n, sgn, rows_global, mloc,
                       Rd, asinvrd);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_sym_dot2(const double *A, long astride, int n, long lda, int count, const double *X, const double *Y, long ldx,
                 double *outx, double *outy, const int *rows_global, double sx, double sy, hipStream_t s) {
    if (count <= 0) return 0;
    // enough (group, chunk) workgroups to fill the device several times over; the partials buffer is cached
    const int groups = (count + DOT2_G - 1) / DOT2_G;
    int nchunk = std::max(1, std::min(64, 4096 / std::max(1, groups)));
    nchunk = std::min(nchunk, std::max(1, n / 16));
    double *part = dot2_scratch(sizeof(double) * 2 * (size_t) nchunk * count);
    if (!part) return 1;
    hipLaunchKernelGGL(hdm_sym_dot2_kernel, dim3(groups, nchunk), dim3(256), 0, s, A, astride, n, lda, count, X, Y, ldx,
                       nchunk, part);
    hipLaunchKernelGGL(hdm_sym_dot2_reduce_kernel, dim3((count + 255) / 256), dim3(256), 0, s, part, count, nchunk,
                       Y ? 1 : 0, outx, outy, rows_global, sx, sy);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_sparse_pairs(const int *rp, const int *ti, const int *tj, const double *tv, const double *X, long ldx, int mloc,
                     const int *rows_global, const HdmMatView &Mv, hipStream_t s) {
    const long npairs = (long) mloc * (mloc + 1) / 2;
    if (npairs <= 0) return 0;
    hipLaunchKernelGGL(hdm_sparse_pair_kernel, dim3((unsigned) ((npairs + 3) / 4)), dim3(256), 0, s, rp, ti, tj, tv, X, ldx,
                       mloc, rows_global, Mv);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_sparse_dot(const int *rp, const int *ti, const int *tj, const double *tv, const double *Y, long ldy, int mloc,
                   const int *rows_global, double scale, double *out, hipStream_t s) {
    if (mloc <= 0) return 0;
    hipLaunchKernelGGL(hdm_sparse_dot_kernel, dim3((mloc + 3) / 4), dim3(256), 0, s, rp, ti, tj, tv, Y, ldy, mloc,
                       rows_global, scale, out);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// The congruence's first step writes the lower triangle of its output's diagonal tiles only, the second step reads those
// tiles whole (gemm_f64.hip): the strict upper part has to read as zero.  One workgroup per (matrix, diagonal tile);
// thread t owns column pair (2t, 2t+1) of the tile... kept simple: 256 threads sweep the 128 columns, 128 rows each.
__global__ void hdm_zero_diag_upper_kernel(double *__restrict__ T, long tstride, int n) {
    const int tile = blockIdx.x, z = blockIdx.y;
    const int base = tile * 128;
    double *M = T + (long) z * tstride;
    for (int e = threadIdx.x; e < 128 * 128; e += 256) {
        const int i = base + (e & 127), j = base + (e >> 7);
        if (i < j && j < n) M[i + (long) j * n] = 0.0;
    }
}
int hdm_zero_diag_upper(double *T, long tstride, int n, int batch, hipStream_t s) {
    if (batch <= 0) return 0;
    hipLaunchKernelGGL(hdm_zero_diag_upper_kernel, dim3((n + 127) / 128, batch), dim3(256), 0, s, T, tstride, n);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// skyline-stored A_L matrix -> square column-major n x n (ld = n), zeros above the diagonal blocks' lower part
__global__ void hdm_sky_to_square_kernel(const double *__restrict__ sky, double *__restrict__ sq, int n) {
    const long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long) n * n) return;
    const int i = (int) (e % n), j = (int) (e / n);
    sq[e] = (i >= (j & ~127)) ? sky[hdm_sky_off(i, j, n)] : 0.0;
}
int hdm_sky_to_square(const double *sky, double *sq, int n, hipStream_t s) {
    const long tot = (long) n * n;
    hipLaunchKernelGGL(hdm_sky_to_square_kernel, dim3((unsigned) ((tot + 255) / 256)), dim3(256), 0, s, sky, sq, n);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// one kernel of this translation unit (= one code object): what the preload thread asks the runtime about (engine.hip: preload_modules)
const void *hdm_module_handle_schur() { return (const void *) hdm_scatter_low_kernel; }
