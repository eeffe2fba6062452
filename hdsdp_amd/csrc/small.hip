// small.hip -- one launch for a whole Phase-A pass on a small rank-one block (BASELINE configs 2-3: mcp100, gpp100).
//
// Reference path being replaced (one pass = interface/hdsdp_algo.c:1082-1101 on a block whose constraints are all
// A_i = s_i a_i a_i', the reference's all-M2 plans, hdsdp_conic_sdp.c:687-778):
//     S = tau C - sum y_i A_i - Rd I -> Cholesky (PSD check, log det) -> S^-1 -> M_ij = s_i s_j (a_i' S^-1 a_j)^2,
//     ASinv_i = s_i a_i' S^-1 a_i,  ASinvRdSinv_i = Rd s_i |S^-1 a_i|^2,  tr S^-1 -> Cholesky of M -> three solves.
// On the multi-launch path that is about forty launches and six host synchronisations for 0.2 MB of operands: 0.6 ms,
// twice what one host core needs.  Here it is ONE workgroup of 512 threads and one synchronisation.
//
// Layout.  n, m <= 128.  A 128 x 128 matrix lives in REGISTERS, dealt cyclically over a 16 x 32 thread grid: thread
// (ty, tx) holds rows ty + 16 r (r < 8) of columns tx + 32 c (c < 4), 32 doubles per matrix.  The cyclic deal keeps
// every thread busy through a triangular sweep.
//
// The sweep (sm_sweep) is a right-looking Cholesky in which step k also finishes row k of W = L^-1 (forward substitution
// on the identity, carried along as a second register matrix): the column of A and the row of R that step k needs are put
// into LDS by their owners, one barrier, and every thread updates its own elements; rows / columns that a step cannot
// touch are skipped with wave-uniform bounds.  One pass over k = 0 .. n-1 with ONE barrier per step (the two LDS lines are
// double-buffered) yields L, L^-1 and log det S.  S^-1 = W'W follows in n / 4 independent rounds (sm_wtw).  (Carrying X
// along in the same sweep as a third register matrix spilled 118 VGPRs at two waves per SIMD.)
//
// The factors are left where the multi-launch path keeps them (HdmChol::L and ::Dinv of the dual matrix and of the Schur
// system -- for one 128-block, Dinv IS the triangular inverse), so every later call on the same state (HKKTSolve, log
// barrier, ratio test) finds what it expects.
#include "small.h"
#include <algorithm>
#include <cmath>

#include "sweep128.h"
#include "lanczos.h"

// x = W'W for the lower-triangular W in registers (x_ij = sum_k W_ki W_kj).  Every thread owns exactly one row of each
// block of sixteen rows (row 16 KR + ty, its local row KR), so a block is published by ALL threads at once -- no owner
// test, constant register indices -- and consumed as sixteen outer products: eight rounds of two barriers for the whole
// product.  buf: 16 x 128 doubles of LDS.  Row k of W is zero right of column k: rows / columns beyond the block's last row
// are skipped.
template <int KR>
__device__ __forceinline__ void sm_wtw_block(int n, const double (&w)[SM_NR][SM_NC], double (&x)[SM_NR][SM_NC], double *buf, int ty, int tx) {
    constexpr int KC = KR / 2;
#pragma unroll
    for (int c = 0; c < SM_NC; ++c) buf[ty * SMALL_P + tx + 32 * c] = (16 * KR + ty < n) ? w[KR][c] : 0.0;
    __syncthreads();
    const int qend = min(16, n - 16 * KR);
    for (int q = 0; q < qend; ++q) {
        const double *row = buf + q * SMALL_P;
        double wi[SM_NR], wj[SM_NC];
#pragma unroll
        for (int r = 0; r <= KR; ++r) wi[r] = row[ty + 16 * r];
#pragma unroll
        for (int c = 0; c <= KC; ++c) wj[c] = row[tx + 32 * c];
#pragma unroll
        for (int r = 0; r <= KR; ++r)
#pragma unroll
            for (int c = 0; c <= KC; ++c) x[r][c] += wi[r] * wj[c];
    }
    __syncthreads();
}
__device__ __forceinline__ void sm_wtw(int n, const double (&w)[SM_NR][SM_NC], double (&x)[SM_NR][SM_NC], double *buf, int ty, int tx) {
#pragma unroll
    for (int r = 0; r < SM_NR; ++r)
#pragma unroll
        for (int c = 0; c < SM_NC; ++c) x[r][c] = 0.0;
    if (n > 0) sm_wtw_block<0>(n, w, x, buf, ty, tx);
    if (n > 16) sm_wtw_block<1>(n, w, x, buf, ty, tx);
    if (n > 32) sm_wtw_block<2>(n, w, x, buf, ty, tx);
    if (n > 48) sm_wtw_block<3>(n, w, x, buf, ty, tx);
    if (n > 64) sm_wtw_block<4>(n, w, x, buf, ty, tx);
    if (n > 80) sm_wtw_block<5>(n, w, x, buf, ty, tx);
    if (n > 96) sm_wtw_block<6>(n, w, x, buf, ty, tx);
    if (n > 112) sm_wtw_block<7>(n, w, x, buf, ty, tx);
}

// x = W' (W b) for the lower-triangular W held in registers; b, t: LDS vectors; part: 16 x 128 LDS doubles; out: m results
__device__ __forceinline__ void sm_solve(int m, const double (&w)[SM_NR][SM_NC], const double *b, double *t, double *part,
                                         double *out, int ty, int tx, int tid) {
    double s[SM_NR];
#pragma unroll
    for (int r = 0; r < SM_NR; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < SM_NC; ++c) acc += w[r][c] * b[tx + 32 * c];
        for (int off = 16; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 32);     // over the 32 threads of one ty
        s[r] = acc;
    }
    if (tx == 0) {
#pragma unroll
        for (int r = 0; r < SM_NR; ++r) t[ty + 16 * r] = s[r];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < SM_NC; ++c) {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < SM_NR; ++r) acc += w[r][c] * t[ty + 16 * r];
        part[ty * SMALL_P + tx + 32 * c] = acc;
    }
    __syncthreads();
    if (tid < m) {
        double acc = 0.0;
        for (int q = 0; q < 16; ++q) acc += part[q * SMALL_P + tid];
        out[tid] = acc;
    }
    __syncthreads();
}

__global__ __launch_bounds__(SM_T) void hdm_small_phase_a_kernel(HdmSmallArgs p) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int n = p.n, m = p.m;
    const int ld = SMALL_P + 1;
    double *Xl = sm;                                   // S, later X = S^-1, later solve scratch: 128 x 129 (its first 2 x 1024 doubles: the sweeps' block images)
    double *vden = sm + (long) SMALL_P * ld;           // SMALL_NDENSE x 128: X a_d of the dense factors
    double *asinv = vden + SMALL_NDENSE * SMALL_P;     // 128
    double *asinvrd = asinv + SMALL_P;                 // 128
    double *tvec = asinvrd + SMALL_P;                  // 128
    double *bvec = tvec + SMALL_P;                     // 128 (+ 128 behind it: the sweep's deferred scale factors)
    // the rank-one factors' CSR, staged once: every later use is a handful of dependent reads per pair of constraints,
    // which from global memory cost an L2 round trip each (the build took 25-45 us that way)
    double *fvl = bvec + 2 * SMALL_P;                  // SMALL_P * SMALL_SPMAX values of the sparse factors
    double *sgl = fvl + SMALL_P * SMALL_SPMAX;         // 128 signs
    int *fil = (int *) (sgl + SMALL_P);                // SMALL_P * SMALL_SPMAX indices
    int *fpl = fil + SMALL_P * SMALL_SPMAX;            // 129 row starts INTO fvl / fil (dense rows: empty)
    int *fnl = fpl + SMALL_P + 4;                      // 128: entries per row (a dense row: n, its values stay in global memory)
    int *dol = fnl + SMALL_P;                          // 128: dense_of
    const int tid = threadIdx.x, ty = tid >> 5, tx = tid & 31;
    // phase stamps (100 MHz wall clock) behind the results: [0] start, [1] S assembled, [2] factor + inverse of S,
    // [3] S^-1, [4] Schur build, [5] factor + inverse of M, [6] solves
    double *stamp = p.out + 4 + 5 * m;
#define SM_STAMP(i) if (tid == 0) stamp[i] = (double) __builtin_amdgcn_s_memrealtime();
    SM_STAMP(0)
    const unsigned long long clk0 = __builtin_amdgcn_s_memtime();

    // ---- S = tau C - sum y_i s_i a_i a_i' + eye I, assembled in LDS (full symmetric)
    // (thread = row tid mod 128 of the columns tid / 128, + 4, ...: no integer division, and the loads of an unrolled
    // group are in flight together -- one load per trip of a divided index ran at a memory round trip per element)
    const int ei = tid & (SMALL_P - 1), ej0 = tid >> 7;
    if (ei < n) {
#pragma unroll 8
        for (int j = ej0; j < n; j += SM_T / SMALL_P)
            Xl[ei + j * ld] = p.tau * p.C[ei + (long) j * p.ldc] + ((ei == j) ? p.eye : 0.0);
    }
    if (tid < SMALL_P) {                               // (entries past m meet zeros of the padded factor in the solves: they must be numbers)
        bvec[tid] = (tid < m) ? p.b[tid] : 0.0;
        asinv[tid] = 0.0; asinvrd[tid] = 0.0; tvec[tid] = 0.0;
    }
    if (tid == 0) {                                    // row starts of the staged (sparse-only) CSR: a serial scan of <= 128 rows
        int pos = 0;
        for (int q = 0; q < m; ++q) {
            const int cnt = p.fp[q + 1] - p.fp[q];
            fpl[q] = pos; fnl[q] = cnt;
            if (cnt <= SMALL_SPMAX) pos += cnt;
        }
        fpl[m] = pos;
    }
    if (tid < m) { sgl[tid] = p.sgn[tid]; dol[tid] = p.dense_of[tid]; }
    __syncthreads();
    for (int q = tid; q < m; q += SM_T) {
        const int f0 = p.fp[q], cnt = fnl[q];
        if (cnt <= SMALL_SPMAX)
            for (int u = 0; u < cnt; ++u) { fvl[fpl[q] + u] = p.fv[f0 + u]; fil[fpl[q] + u] = p.fi[f0 + u]; }
    }
    __syncthreads();
    for (int q = tid; q < m; q += SM_T) {              // sparse factors: a handful of entries each
        if (fnl[q] > SMALL_SPMAX) continue;
        const int f0 = fpl[q], f1 = f0 + fnl[q];
        const double coef = -p.y[q] * sgl[q];
        if (coef == 0.0) continue;
        for (int u = f0; u < f1; ++u)
            for (int v = f0; v < f1; ++v) atomicAdd(&Xl[fil[u] + fil[v] * ld], coef * fvl[u] * fvl[v]);
    }
    __syncthreads();
    for (int d = 0; d < p.ndense; ++d) {               // dense factors: the whole workgroup per row
        const int q = p.dense_rows[d];
        const double coef = -p.y[q] * p.sgn[q];
        const double *av = p.fv + p.fp[q];             // all n entries are listed
        if (coef != 0.0)
            if (ei < n) {
                const double ai = coef * av[ei];
                for (int j = ej0; j < n; j += SM_T / SMALL_P) Xl[ei + j * ld] += ai * av[j];
            }
        __syncthreads();
    }
    if (ei < n) {                                      // the dual matrix itself stays resident for the other cone slots
#pragma unroll 8
        for (int j = ej0; j <= ei; j += SM_T / SMALL_P) p.Sout[ei + (long) j * p.lds] = Xl[ei + j * ld];
    }
    double a[SM_NR][SM_NC], rr[SM_NR][SM_NC];
#pragma unroll
    for (int r = 0; r < SM_NR; ++r)
#pragma unroll
        for (int c = 0; c < SM_NC; ++c) {
            const int i = ty + 16 * r, j = tx + 32 * c;
            a[r][c] = (i < n && j < n) ? Xl[i + j * ld] : ((i == j) ? 1.0 : 0.0);
        }
    __syncthreads();
    SM_STAMP(1)

    // ---- factor S, invert the factor, form S^-1: one sweep
    double logdet = 0.0;
    const int infoS = sm_sweep(n, a, rr, Xl, bvec + SMALL_P, ty, tx, &logdet);
    SM_STAMP(2)
    if (infoS) {
        if (tid == 0) { p.out[0] = (double) infoS; p.out[1] = 0.0; p.out[2] = 0.0; p.out[3] = 0.0; }
        return;
    }
    sm_store_factor(n, a, rr, Xl, p.LS, p.WS, ty, tx, tid);
    __syncthreads();
    sm_wtw(n, rr, a, Xl, ty, tx);                      // (the S image in LDS is free: 16 x 128 doubles of it serve as the row buffer; `a` is free too)
#pragma unroll
    for (int r = 0; r < SM_NR; ++r)
#pragma unroll
        for (int c = 0; c < SM_NC; ++c) {
            const int i = ty + 16 * r, j = tx + 32 * c;
            if (i < n && j < n) Xl[i + j * ld] = a[r][c];
        }
    __syncthreads();

    SM_STAMP(3)
    // ---- the rank-one Schur build on X = S^-1
    for (int d = 0; d < p.ndense; ++d) {               // v_d = X a_d
        const double *av = p.fv + p.fp[p.dense_rows[d]];
        for (int r = tid; r < n; r += SM_T) {
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc += av[k] * Xl[r + k * ld];
            vden[d * SMALL_P + r] = acc;
        }
    }
    __syncthreads();
    for (int q = tid; q < m; q += SM_T) {              // Gamma_qq and |X a_q|^2
        const int dq = dol[q];
        double gii = 0.0, nrm = 0.0;
        if (dq >= 0) {
            const double *v = vden + dq * SMALL_P, *av = p.fv + p.fp[q];
            for (int k = 0; k < n; ++k) { gii += av[k] * v[k]; nrm += v[k] * v[k]; }
        } else {
            const int f0 = fpl[q], f1 = f0 + fnl[q];
            for (int u = f0; u < f1; ++u)
                for (int v = f0; v < f1; ++v) gii += fvl[u] * fvl[v] * Xl[fil[u] + fil[v] * ld];
            for (int r = 0; r < n; ++r) {
                double t = 0.0;
                for (int u = f0; u < f1; ++u) t += fvl[u] * Xl[r + fil[u] * ld];
                nrm += t * t;
            }
        }
        asinv[q] = sgl[q] * gii;
        asinvrd[q] = p.Rd * sgl[q] * nrm;
    }
    {   // M_ji = s_i s_j (a_i' X a_j)^2 for j >= i: thread t keeps ROW j = t mod 128 (its factor in registers) and walks
        // the columns i = t / 128, +4, ... <= j; the column's data are the same address for a whole wave (LDS broadcasts),
        // and the 64 stores of a wave are consecutive rows of one column (full lines)
        const int j = tid & (SMALL_P - 1);
        if (j < m) {
            const int dj = dol[j], j0 = fpl[j], jn = (dj >= 0) ? 0 : fnl[j];
            const double aj0 = (jn > 0) ? fvl[j0] : 0.0;               // the common case: one entry per factor
            const int ij0 = (jn > 0) ? fil[j0] : 0;
            const double sj = sgl[j];
            for (int i = tid >> 7; i <= j; i += 4) {
                const int di = dol[i];
                double gam = 0.0;
                if (di >= 0 && dj >= 0) {                  // both dense (a handful of pairs at most): a_i from global memory
                    const double *v = vden + dj * SMALL_P, *av = p.fv + p.fp[i];
                    for (int k = 0; k < n; ++k) gam += av[k] * v[k];
                } else if (dj >= 0) {
                    const double *v = vden + dj * SMALL_P;
                    for (int u = fpl[i]; u < fpl[i] + fnl[i]; ++u) gam += fvl[u] * v[fil[u]];
                } else if (di >= 0) {
                    const double *v = vden + di * SMALL_P;
                    for (int u = j0; u < j0 + jn; ++u) gam += fvl[u] * v[fil[u]];
                } else {
                    const int i0 = fpl[i], in_ = fnl[i];
                    if (in_ == 1 && jn == 1) gam = fvl[i0] * aj0 * Xl[fil[i0] + ij0 * ld];
                    else
                        for (int u = 0; u < in_; ++u) {
                            const double *xc = Xl + fil[i0 + u];       // row index of X from a_i, column from a_j
                            double t = 0.0;
                            for (int v = j0; v < j0 + jn; ++v) t += fvl[v] * xc[fil[v] * ld];
                            gam += fvl[i0 + u] * t;
                        }
                }
                p.M[j + (long) i * p.ldm] = sgl[i] * sj * gam * gam;
            }
        }
    }
    double trs = 0.0;
    if (tid < 64) {                                    // tr S^-1: one wave, two entries per lane, shuffles
        double t = ((tid < n) ? Xl[tid + tid * ld] : 0.0) + ((tid + 64 < n) ? Xl[(tid + 64) + (tid + 64) * ld] : 0.0);
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        trs = t;
    }
    __threadfence();
    __syncthreads();
    if (tid < m) { p.out[4 + tid] = asinv[tid]; p.out[4 + m + tid] = asinvrd[tid]; }

    SM_STAMP(4)
    // ---- factor M, invert the factor, three solves
    // M comes back through the LDS image (X is dead): full-line loads of the lower triangle, and the rest of the 128 x 128
    // device matrix is zeroed on the way -- the state HKKTBuildUp leaves (hdsdp_schur.c:141-165), without a memset launch
    if (ei < SMALL_P) {
#pragma unroll 8
        for (int j = ej0; j < SMALL_P; j += SM_T / SMALL_P) {
            const bool low = (ei < m && j <= ei);
            double v = 0.0;
            if (low) v = p.M[ei + (long) j * p.ldm];
            else p.M[ei + (long) j * p.ldm] = 0.0;
            Xl[ei + j * ld] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SM_NR; ++r)
#pragma unroll
        for (int c = 0; c < SM_NC; ++c) {
            const int i = ty + 16 * r, j = tx + 32 * c;
            const int hi = max(i, j), lo = min(i, j);
            a[r][c] = (i < m && j < m) ? Xl[hi + lo * ld] : ((i == j) ? 1.0 : 0.0);
        }
    __syncthreads();
    double logdetM = 0.0;
    const int infoM = sm_sweep(m, a, rr, Xl, bvec + SMALL_P, ty, tx, &logdetM);
    if (tid == 0) { p.out[0] = 0.0; p.out[1] = (double) infoM; p.out[2] = logdet; p.out[3] = trs; }
    if (infoM) return;
    sm_store_factor(m, a, rr, Xl, p.LM, p.WM, ty, tx, tid);
    __syncthreads();
    SM_STAMP(5)
    double *part = Xl;                                 // X is no longer needed: 16 x 128 partial sums
    sm_solve(m, rr, bvec, tvec, part, p.out + 4 + 2 * m, ty, tx, tid);
    sm_solve(m, rr, asinv, tvec, part, p.out + 4 + 3 * m, ty, tx, tid);
    sm_solve(m, rr, asinvrd, tvec, part, p.out + 4 + 4 * m, ty, tx, tid);
    SM_STAMP(6)
    if (tid == 0) stamp[7] = (double) (__builtin_amdgcn_s_memtime() - clk0);      // shader-clock cycles of the whole pass
#undef SM_STAMP
}

// ---- interior check of a small block in one launch (see small.h) ------------------------------------------------------
// The body: one workgroup, one block.  It reads its arguments and the block's data, writes the block's S, L, W and report words
// and nothing else; `sm` is the workgroup's dynamic LDS (128 x 129 + 128 + m doubles).
__device__ __forceinline__ void sm_check_body(const HdmSmallCheckArgs &p, double *sm) {
    constexpr int ld = SMALL_P + 1;
    double *Xl = sm;                                   // S, full symmetric: 128 x 129 (its head: the sweep's block images)
    double *rsv = sm + (long) SMALL_P * ld;            // 128 deferred scale factors
    double *yl = rsv + SMALL_P;                        // the multipliers, staged once
    const int n = p.n, n16 = p.n16, m = p.m;
    const int tid = threadIdx.x, ty = tid >> 5, tx = tid & 31;
    for (int q = tid; q < m; q += SM_T) yl[q] = p.y[q];
    __syncthreads();
    // lower triangle, column by column: thread = row (tid mod 128) of the columns tid / 128, + 4, ...
    const int ei = tid & (SMALL_P - 1), ej0 = tid >> 7;
    if (ei < n) {
        for (int j = ej0; j <= ei; j += SM_T / SMALL_P) {
            const double *a = p.A + ei + (long) j * n16;
            double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // eight loads in flight per thread
            int q = 0;
            for (; q + 7 < m; q += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] -= yl[q + u] * a[(long) (q + u) * p.astride];
            }
            for (; q < m; ++q) acc[0] -= yl[q] * a[(long) q * p.astride];
            double v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
            if (ei == j) v *= 2.0;                     // A_L form: half the diagonal is stored
            v += p.tau * p.C[ei + (long) j * n16];
            if (ei == j) v += p.eye;
            Xl[ei + j * ld] = v;
            Xl[j + ei * ld] = v;
            p.Sout[ei + (long) j * n16] = v;
        }
    }
    __syncthreads();
    double a[SM_NR][SM_NC], rr[SM_NR][SM_NC];
#pragma unroll
    for (int r = 0; r < SM_NR; ++r)
#pragma unroll
        for (int c = 0; c < SM_NC; ++c) {
            const int i = ty + 16 * r, j = tx + 32 * c;
            a[r][c] = (i < n && j < n) ? Xl[i + j * ld] : ((i == j) ? 1.0 : 0.0);
        }
    __syncthreads();
    double logdet = 0.0;
    const int info = sm_sweep(n, a, rr, Xl, rsv, ty, tx, &logdet);
    if (tid == 0) { p.out[0] = (double) info; p.out[1] = logdet; }
    if (info) return;
    sm_store_factor(n, a, rr, Xl, p.L, p.W, ty, tx, tid);
}

__global__ __launch_bounds__(SM_T) void hdm_small_check_kernel(HdmSmallCheckArgs p) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    sm_check_body(p, sm);
}

// The grouped form: workgroup b runs the same body on table[b].  The workgroups are independent: none waits for another, none
// reads a word another writes, and any number of them may be resident at a time.
__global__ __launch_bounds__(SM_T) void hdm_grouped_check_kernel(const HdmSmallCheckArgs *__restrict__ table, int count) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if ((int) blockIdx.x >= count) return;
    const HdmSmallCheckArgs p = table[blockIdx.x];
    sm_check_body(p, sm);
}

static bool sm_check_args_ok(const HdmSmallCheckArgs &a) {
    return !(a.n < 1 || a.n > SMALL_P || a.n16 > SMALL_P || a.m < 0 || a.m > 4096) && hdm_small_check_lds_bytes(a.m) <= HDM_SMALL_CHECK_LDS_MAX;
}

int hdm_small_check(const HdmSmallCheckArgs &args, hipStream_t s) {
    if (!sm_check_args_ok(args)) return 1;
    const size_t lds = (size_t) hdm_small_check_lds_bytes(args.m);
    static thread_local int configured_dev = -1;
    int dev = 0;
    HDM_HIP_CHECK(hipGetDevice(&dev));
    if (configured_dev != dev) {
        HDM_HIP_CHECK(hipFuncSetAttribute((const void *) hdm_small_check_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) HDM_SMALL_CHECK_LDS_MAX));
        configured_dev = dev;
    }
    hipLaunchKernelGGL(hdm_small_check_kernel, dim3(1), dim3(SM_T), lds, s, args);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_grouped_check(const HdmSmallCheckArgs *table_host, const HdmSmallCheckArgs *table_dev, int count, int max_m, hipStream_t s) {
    if (!table_host || !table_dev || count < 1) return 1;
    for (int k = 0; k < count; ++k)
        if (!sm_check_args_ok(table_host[k]) || table_host[k].m > max_m) return 1;
    if (max_m < 0 || max_m > 4096 || hdm_small_check_lds_bytes(max_m) > HDM_SMALL_CHECK_LDS_MAX) return 1;
    const size_t lds = (size_t) hdm_small_check_lds_bytes(max_m);
    static thread_local int configured_dev = -1;
    int dev = 0;
    HDM_HIP_CHECK(hipGetDevice(&dev));
    if (configured_dev != dev) {
        HDM_HIP_CHECK(hipFuncSetAttribute((const void *) hdm_grouped_check_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) HDM_SMALL_CHECK_LDS_MAX));
        configured_dev = dev;
    }
    hipLaunchKernelGGL(hdm_grouped_check_kernel, dim3((unsigned) count), dim3(SM_T), lds, s, table_dev, count);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the grouped ratio test's safeguard (lanczos.h: HdmGroupedRatioArgs) ---------------------------------
// Queued behind hdm_grouped_ratio_kernel on the same stream.  Workgroup b reads the step its member's test has just reported and,
// where that is a finite step inside (0, 1e6), factors S + (1 - 1e-3) step dS with the sweep HdmChol::factor runs on a one-block
// object (the lower triangle and the identity padding are what the sweep reads); the word it writes is that factorisation's info,
// 0 otherwise.  No factor is stored: only yes / no is used (engine_cone.h: ratio_safeguard).  Independent workgroups.
__global__ __launch_bounds__(SM_T) void hdm_grouped_safeguard_kernel(const HdmGroupedRatioArgs *__restrict__ table, int count) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if ((int) blockIdx.x >= count) return;
    const HdmGroupedRatioArgs p = table[blockIdx.x];
    constexpr int ld = SMALL_P + 1;
    double *Xl = sm;                                   // 128 x 129 (its head: the sweep's block images)
    double *rsv = sm + (long) SMALL_P * ld;            // 128 deferred scale factors
    const int n = p.n, n16 = p.n16;
    const int tid = threadIdx.x, ty = tid >> 5, tx = tid & 31;
    const double step = p.out[0], status = p.out[2];
    if (status != 0.0 || !(step > 0.0) || !(step < 1e6)) {      // (uniform: every thread read the same two words)
        if (tid == 0) p.out[3] = 0.0;
        return;
    }
    const double st = (1.0 - 1e-3) * step;
    const int ei = tid & (SMALL_P - 1), ej0 = tid >> 7;
    if (ei < n) {
        for (int j = ej0; j <= ei; j += SM_T / SMALL_P) {
            const long e = ei + (long) j * n16;
            const double v = hdm_axpy_elem(p.S[e], p.dS[e], st);
            Xl[ei + j * ld] = v;
            Xl[j + ei * ld] = v;
        }
    }
    __syncthreads();
    double a[SM_NR][SM_NC], rr[SM_NR][SM_NC];
#pragma unroll
    for (int r = 0; r < SM_NR; ++r)
#pragma unroll
        for (int c = 0; c < SM_NC; ++c) {
            const int i = ty + 16 * r, j = tx + 32 * c;
            a[r][c] = (i < n && j < n) ? Xl[i + j * ld] : ((i == j) ? 1.0 : 0.0);
        }
    __syncthreads();
    double unused;
    const int info = sm_sweep<false>(n, a, rr, Xl, rsv, ty, tx, &unused);
    if (tid == 0) p.out[3] = (double) info;
}

int hdm_grouped_safeguard(const HdmGroupedRatioArgs *table_dev, int count, hipStream_t s) {
    if (!table_dev || count < 1) return 1;
    const size_t lds = (size_t) hdm_small_check_lds_bytes(0);
    static thread_local int configured_dev = -1;
    int dev = 0;
    HDM_HIP_CHECK(hipGetDevice(&dev));
    if (configured_dev != dev) {
        HDM_HIP_CHECK(hipFuncSetAttribute((const void *) hdm_grouped_safeguard_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) HDM_SMALL_CHECK_LDS_MAX));
        configured_dev = dev;
    }
    hipLaunchKernelGGL(hdm_grouped_safeguard_kernel, dim3((unsigned) count), dim3(SM_T), lds, s, table_dev, count);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the safeguard's rest, second half (lanczos.h: HdmGroupedRestArgs) --------------------------------------
// Queued behind hdm_grouped_fresh_kernel.  Workgroup b leaves at once where the safeguard word of table[b] is 0.  Otherwise what
// ratio_safeguard_rest (engine_cone.h) does on the host after its fresh-start test, with the same expressions in the same order on
// the same doubles: the smaller of the two steps (the fresh one only where that test reported success), then at most 64 rounds of
// "factor S + (1 - 1e-3) step dS; stop if it factors; step *= 0.9", each round the safeguard kernel's own element expression
// (hdm_axpy_elem) and sweep.  The sweep's info is the same in every thread; it still goes through LDS and a barrier before the
// loop branches on it, so that the exit is uniform whatever a later change to the sweep does.  Independent workgroups.
__global__ __launch_bounds__(SM_T) void hdm_grouped_cuts_kernel(const HdmGroupedRatioArgs *__restrict__ table,
                                                                const HdmGroupedRestArgs *__restrict__ rest, int count) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if ((int) blockIdx.x >= count) return;
    const HdmGroupedRatioArgs p = table[blockIdx.x];
    if (!(p.out[3] > 0.0)) return;                     // (uniform: every thread read the same word)
    const HdmGroupedRestArgs q = rest[blockIdx.x];
    constexpr int ld = SMALL_P + 1;
    double *Xl = sm;                                   // 128 x 129 (its head: the sweep's block images)
    double *rsv = sm + (long) SMALL_P * ld;            // 128 deferred scale factors
    // the round's info, broadcast: the one double hdm_small_check_lds_bytes(0) has behind them (no static LDS: the kernel may ask
    // for all 160 KB as dynamic)
    int *sh_info = reinterpret_cast<int *>(rsv + SMALL_P);
    const int n = p.n, n16 = p.n16;
    const int tid = threadIdx.x;
    const int ei = tid & (SMALL_P - 1), ej0 = tid >> 7;
    double step = p.out[0];
    const double fresh = (q.fresh_out[2] == 0.0) ? q.fresh_out[0] : INFINITY;
    if (fresh < step) step = fresh;
    int cuts = 0, ok = 0;
#pragma unroll 1
    for (int it = 0; it < 64; ++it) {
        // (a round's index arithmetic and bound predicates are redone from these two, not kept in registers across the sweep:
        // hoisted out of the loop they were 30 spilled VGPRs and 30 spilled SGPRs on top of the safeguard kernel's 233)
        int ty = tid >> 5, tx = tid & 31;
        asm volatile("" : "+v"(ty), "+v"(tx));
        const double st = (1.0 - 1e-3) * step;
        if (ei < n) {
            for (int j = ej0; j <= ei; j += SM_T / SMALL_P) {
                const long e = ei + (long) j * n16;
                const double v = hdm_axpy_elem(p.S[e], p.dS[e], st);
                Xl[ei + j * ld] = v;
                Xl[j + ei * ld] = v;
            }
        }
        __syncthreads();
        double a[SM_NR][SM_NC], rr[SM_NR][SM_NC];
#pragma unroll
        for (int r = 0; r < SM_NR; ++r)
#pragma unroll
            for (int c = 0; c < SM_NC; ++c) {
                const int i = ty + 16 * r, j = tx + 32 * c;
                a[r][c] = (i < n && j < n) ? Xl[i + j * ld] : ((i == j) ? 1.0 : 0.0);
            }
        __syncthreads();
        double unused;
        const int info = sm_sweep<false>(n, a, rr, Xl, rsv, ty, tx, &unused);
        if (tid == 0) *sh_info = info;
        __syncthreads();                               // (also: every read of this round's images is over before the next round writes)
        if (*sh_info == 0) { ok = 1; break; }
        step *= 0.9;
        cuts += 1;
    }
    if (tid == 0) { q.rest[0] = step; q.rest[2] = (double) cuts; q.rest[3] = fresh; q.rest[1] = (double) ok; }
}

int hdm_grouped_cuts(const HdmGroupedRatioArgs *table_dev, const HdmGroupedRestArgs *rest_dev, int count, hipStream_t s) {
    if (!table_dev || !rest_dev || count < 1) return 1;
    const size_t lds = (size_t) hdm_small_check_lds_bytes(0);
    static thread_local int configured_dev = -1;
    int dev = 0;
    HDM_HIP_CHECK(hipGetDevice(&dev));
    if (configured_dev != dev) {
        HDM_HIP_CHECK(hipFuncSetAttribute((const void *) hdm_grouped_cuts_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) HDM_SMALL_CHECK_LDS_MAX));
        configured_dev = dev;
    }
    hipLaunchKernelGGL(hdm_grouped_cuts_kernel, dim3((unsigned) count), dim3(SM_T), lds, s, table_dev, rest_dev, count);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the grouped step-and-check (small.h: HdmGroupedStepArgs) --------------------------------------------
// Workgroup b puts table[b]'s checker at S + dStep dS: what cone_axpy_check does for one cone in five launches -- hdm_axpy_mat into
// Scheck, the rectangle copy into the checker object's L, the identity padding, the cleared info word, the diagonal-block sweep --
// and leaves the same bits everywhere those launches write.  One pass over the 128 x 128 index square forms every element of the
// n16 x n16 sum once: it goes to Scheck; inside n x n its lower part goes into the LDS image the sweep starts from (zeros above the
// diagonal, the identity in the padding: what hdm_potrf_diag_sweep_body reads back from L), its strict upper part into L, where the
// rectangle copy would have put it and the sweep's store leaves it.  Then that body's own steps: sm_sweep<false> over the n pivots,
// L's lower triangle and all of Dinv stored whether or not a pivot failed, the first bad pivot reported.  Independent workgroups:
// none waits for another, none reads a word another writes.
__global__ __launch_bounds__(SM_T) void hdm_grouped_step_check_kernel(const HdmGroupedStepArgs *__restrict__ table, int count) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if ((int) blockIdx.x >= count) return;
    const HdmGroupedStepArgs p = table[blockIdx.x];
    constexpr int ldi = SMALL_P + 1;
    double *img = sm;                                  // 128 x 129 staging image; its head doubles as the sweep's block images
    double *rsv = sm + SMALL_P * (SMALL_P + 1);        // 128 deferred scale factors
    const int n = p.n, n16 = p.n16;
    const int tid = threadIdx.x, ty = tid >> 5, tx = tid & 31;
    const int ei = tid & (SMALL_P - 1), ej0 = tid >> 7;
#pragma unroll 8
    for (int j = ej0; j < SMALL_P; j += SM_T / SMALL_P) {
        double v = 0.0;
        if (ei < n16 && j < n16) {
            const long e = ei + (long) j * n16;
            v = hdm_axpy_elem(p.S[e], p.dS[e], p.dStep);
            p.Scheck[e] = v;
        }
        const bool in = (ei < n && j < n);
        if (ei >= j) img[ei + j * ldi] = in ? v : ((ei == j) ? 1.0 : 0.0);
        else {
            img[ei + j * ldi] = 0.0;
            p.L[ei + (long) j * SMALL_P] = in ? v : 0.0;
        }
    }
    __syncthreads();
    double a[SM_NR][SM_NC], rr[SM_NR][SM_NC];
#pragma unroll
    for (int r = 0; r < SM_NR; ++r)
#pragma unroll
        for (int c = 0; c < SM_NC; ++c) a[r][c] = img[(ty + 16 * r) + (tx + 32 * c) * ldi];
    __syncthreads();
    double unused;
    const int bad = sm_sweep<false>(n, a, rr, img, rsv, ty, tx, &unused);
    __syncthreads();
    sm_store_one<true>(SMALL_P, a, img, p.L, SMALL_P, ty, tx, tid);
    sm_store_one<false>(SMALL_P, rr, img, p.Dinv, SMALL_P, ty, tx, tid);
    if (tid == 0) *p.info = bad;
}

int hdm_grouped_step_check(const HdmGroupedStepArgs *table_host, const HdmGroupedStepArgs *table_dev, int count, hipStream_t s) {
    if (!table_host || !table_dev || count < 1) return 1;
    for (int k = 0; k < count; ++k) {
        const HdmGroupedStepArgs &a = table_host[k];
        if (a.n < 1 || a.n > SMALL_P || a.n16 < a.n || a.n16 > SMALL_P || (a.n16 & 15)) return 1;
        if (!a.S || !a.dS || !a.Scheck || !a.L || !a.Dinv || !a.info) return 1;
    }
    const size_t lds = (size_t) hdm_small_check_lds_bytes(0);
    static thread_local int configured_dev = -1;
    int dev = 0;
    HDM_HIP_CHECK(hipGetDevice(&dev));
    if (configured_dev != dev) {
        HDM_HIP_CHECK(hipFuncSetAttribute((const void *) hdm_grouped_step_check_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) HDM_SMALL_CHECK_LDS_MAX));
        configured_dev = dev;
    }
    hipLaunchKernelGGL(hdm_grouped_step_check_kernel, dim3((unsigned) count), dim3(SM_T), lds, s, table_dev, count);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

size_t hdm_small_lds_bytes() {
    return sizeof(double) * ((size_t) SMALL_P * (SMALL_P + 1) + SMALL_NDENSE * SMALL_P + 5 * SMALL_P + SMALL_P * SMALL_SPMAX + SMALL_P) +
           sizeof(int) * ((size_t) SMALL_P * SMALL_SPMAX + (SMALL_P + 4) + 2 * SMALL_P);
}

int hdm_small_phase_a(const HdmSmallArgs &args, hipStream_t s) {
    if (args.n < 1 || args.n > SMALL_P || args.m < 1 || args.m > SMALL_P || args.ndense > SMALL_NDENSE) return 1;
    static thread_local int configured_dev = -1;
    int dev = 0;
    HDM_HIP_CHECK(hipGetDevice(&dev));
    if (configured_dev != dev) {
        HDM_HIP_CHECK(hipFuncSetAttribute((const void *) hdm_small_phase_a_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int) hdm_small_lds_bytes()));
        configured_dev = dev;
    }
    hipLaunchKernelGGL(hdm_small_phase_a_kernel, dim3(1), dim3(SM_T), hdm_small_lds_bytes(), s, args);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the grouped Schur build (see small.h, grouped_plan.h) ----------------------------------------------
// Three launches for all grouped cones of an operator, whatever their number: plain independent workgroups, no workgroup waits
// for another one, nothing is accumulated with atomics -- every staging word has one writer, every destination one adder.
#define GR_T 256
#define GR_W (GR_T / 64)
typedef double gr_c4 __attribute__((ext_vector_type(4)));

// Launch 1.  X = S^-1 = W'W from the triangular inverse W = L^-1 the cone's factor object holds (row k of W is zero right of column
// k, and the padding of the 128-block is the identity: only rows below n enter).  Full symmetric n16 x n16, zero in the padding.
__global__ __launch_bounds__(GR_T) void hdm_grouped_inverse_kernel(HdmGroupedArgs a) {
    __shared__ double Wl[HDM_GROUPED_MAX_N * (HDM_GROUPED_MAX_N + 1)];   // W(k, i) at k + 65 i
    const HdmGroupedConeDev c = a.cones[blockIdx.x];
    const int n = c.n, n16 = c.n16, tid = threadIdx.x;
    constexpr int ldw = HDM_GROUPED_MAX_N + 1;
    for (int e = tid; e < n * n; e += GR_T) {
        const int k = e % n, i = e / n;
        Wl[k + i * ldw] = (k >= i) ? c.W[k + (long) i * SMALL_P] : 0.0;
    }
    __syncthreads();
    double *X = a.X + c.xoff;
    for (int e = tid; e < n16 * n16; e += GR_T) {
        const int i = e % n16, j = e / n16;
        if (i < j) continue;
        double v = 0.0;
        if (i < n)
            for (int k = i; k < n; ++k) v += Wl[k + i * ldw] * Wl[k + j * ldw];
        X[i + (long) j * n16] = v;
        X[j + (long) i * n16] = v;
    }
}

// out(j, i) = sum_k P(i, k) Q(k, j) on the fp64 MFMA, every operand from LDS: P's element (i, k) is read at Pl[i + k ld], Q's
// element (k, j) at Ql[j + k ld] -- both fragments are sixteen consecutive doubles per k -- and the 16 x 16 result tile (lane l,
// register r: row (l >> 4) + 4 r, column l & 15) is stored transposed, which makes its stores consecutive as well.  The callers
// choose P and Q among symmetric matrices and transposes so that what lands in `out` is the column-major product they want.
__device__ __forceinline__ void gr_product(const double *Pl, const double *Ql, double *out, int nb, int ld, int wave, int lane) {
    const int l15 = lane & 15, lq = lane >> 4;
    for (int t = wave; t < nb * nb; t += GR_W) {
        const int ti = t % nb, tj = t / nb;
        const double *pa = Pl + ti * 16 + l15 + lq * ld, *pb = Ql + tj * 16 + l15 + lq * ld;
        gr_c4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < 4 * nb; ++k) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * k * ld], pb[4 * k * ld], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) out[tj * 16 + l15 + (ti * 16 + lq + 4 * r) * ld] = acc[r];
    }
}

__device__ __forceinline__ double gr_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The symmetric matrix in Al (a constraint matrix, or the objective) against X: T = X Al, B = T X, and the three sums
// s[0] = <Al, X>, s[1] = <T, X> = <Al, X^2>, s[2] = <B, C>; thread 0 returns with them.  Products and sums the build type or a zero Rd
// does not ask for are skipped (their sums come back as 0).  Ends behind a barrier: B and Al stay valid until the caller's next one.
__device__ __forceinline__ void gr_row(const double *Xl, const double *Al, double *Tl, double *Bl, const double *C, double *red,
                                       int n16, bool needT, bool needB, bool needC, double (&s)[3]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = n16 >> 4, nn = n16 * n16;
    if (needT) gr_product(Al, Xl, Tl, nb, n16, wave, lane);      // (Al X)(i, j) stored at j + i ld: column-major X Al
    __syncthreads();
    if (needB) gr_product(Xl, Tl, Bl, nb, n16, wave, lane);      // Q(k, j) = T(j, k): (X T')(i, j) = (X Al X)(i, j) stored at j + i ld
    __syncthreads();
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    for (int e = tid; e < nn; e += GR_T) {
        const double x = Xl[e];
        p0 += Al[e] * x;
        if (needT) p1 += Tl[e] * x;
        if (needC) p2 += Bl[e] * C[e];
    }
    p0 = gr_wave_sum(p0); p1 = gr_wave_sum(p1); p2 = gr_wave_sum(p2);
    if (lane == 0) { red[wave * 3] = p0; red[wave * 3 + 1] = p1; red[wave * 3 + 2] = p2; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = (red[k] + red[3 + k]) + (red[6 + k] + red[9 + k]);
    __syncthreads();
}

// Launch 2.  One workgroup per job (grouped_plan.h): X in LDS, then row after row of the job.  Writes staging only: the local vectors
// of its rows, column q of the cone's local lower Gram, and -- the cone's first job -- the four scalars.
__global__ __launch_bounds__(GR_T) void hdm_grouped_jobs_kernel(HdmGroupedArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const HdmGroupedJob job = a.jobs[blockIdx.x];
    const HdmGroupedConeDev c = a.cones[job.slot];
    const int n16 = c.n16, nn = n16 * n16, mloc = c.mloc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *Xl = sm, *Al = sm + nn, *Tl = sm + 2 * nn, *Bl = sm + 3 * nn, *red = sm + 4 * nn;
    const bool corrector = a.typeKKT == 1, hsd = a.typeKKT == 2, rd = c.Rd != 0.0;
    const double *X = a.X + c.xoff;
    double *V = a.V + c.voff, *G = a.G + c.goff;
    for (int e = tid; e < nn; e += GR_T) Xl[e] = X[e];
    double s[3];
    if (job.first) {
        // TraceSinv (Rd != 0), and under HSD the objective as one more row: CSinv = <C, X>, CSinvCSinv = <X C X, C>, CSinvRdSinv = Rd <C, X^2>
        double sc[4] = {0.0, 0.0, 0.0, 0.0};
        if (hsd) {
            for (int e = tid; e < nn; e += GR_T) Al[e] = c.C[e];
            __syncthreads();
            gr_row(Xl, Al, Tl, Bl, c.C, red, n16, true, true, true, s);
            sc[1] = s[0]; sc[2] = s[2];
            if (rd) sc[3] = c.Rd * s[1];
        } else __syncthreads();
        if (tid == 0) {
            if (rd && !corrector)
                for (int i = 0; i < c.n; ++i) sc[0] += Xl[i + i * n16];
            for (int k = 0; k < 4; ++k) V[3 * mloc + k] = sc[k];
        }
    }
    for (int q = job.q0; q < job.q1; ++q) {
        __syncthreads();                                   // the previous row's images are done with
        const double *AL = c.A + (long) q * nn;            // (n16 <= 64: the skyline storage of an A_L form is the plain square)
        for (int e = tid; e < nn; e += GR_T) {
            const int i = e % n16, j = e / n16;
            if (i < j) continue;
            const double v = AL[e];
            if (i == j) Al[e] = 2.0 * v;                   // A_L form: half the diagonal is stored
            else { Al[e] = v; Al[j + i * n16] = v; }
        }
        __syncthreads();
        gr_row(Xl, Al, Tl, Bl, c.C, red, n16, rd || !corrector, !corrector, hsd, s);
        if (tid == 0) {
            V[q] = s[0];
            V[mloc + q] = rd ? c.Rd * s[1] : 0.0;
            V[2 * mloc + q] = hsd ? s[2] : 0.0;
        }
        if (corrector) continue;
        // column q of the local Gram: <B_q, A_p> = sum over the stored triangle of A_L,p (i, j) (B(i, j) + B(j, i)), one wave per p
        for (int p = q + wave; p < mloc; p += GR_W) {
            const double *AP = c.A + (long) p * nn;
            double acc = 0.0;
            for (int e = lane; e < nn; e += 64) {
                const int i = e % n16, j = e / n16;
                if (i >= j) acc += AP[e] * (Bl[e] + Bl[j + i * n16]);
            }
            acc = gr_wave_sum(acc);
            if (lane == 0) G[hdm_grouped_gidx(p, q, mloc)] = acc;
        }
    }
}

// Launch 3.  One thread per destination: an entry of M's lower triangle, a row of the m-vectors, or (the last thread) the four
// scalars.  It sums its contributors in list order -- ascending cone order -- and adds the sum where the per-cone builders add
// theirs.  A corrector build has no M: its threads start behind M's destinations.
__global__ __launch_bounds__(GR_T) void hdm_grouped_scatter_kernel(HdmGroupedScatterArgs a, HdmMatView Mv) {
    const bool corrector = a.typeKKT == 1, hsd = a.typeKKT == 2;
    const long t = (long) blockIdx.x * GR_T + threadIdx.x + (corrector ? a.nM : 0L);
    if (t < a.nM) {
        double acc = 0.0;
        for (long k = a.m_ptr[t]; k < a.m_ptr[t + 1]; ++k) acc += a.G[a.cones[a.m_slot[k]].goff + a.m_idx[k]];
        *hdm_mat_at(Mv, a.m_row[t], a.m_col[t]) += acc;
    } else if (t < a.nM + a.nV) {
        const long r = t - a.nM;
        for (int v = 0; v < (hsd ? 3 : 2); ++v) {
            double acc = 0.0;
            for (long k = a.v_ptr[r]; k < a.v_ptr[r + 1]; ++k) {
                const HdmGroupedConeDev &c = a.cones[a.v_slot[k]];
                acc += a.V[c.voff + (long) v * c.mloc + a.v_idx[k]];
            }
            a.vecs[(long) v * a.m + a.v_row[r]] += acc;
        }
    } else if (t == a.nM + a.nV) {
        for (int k = 0; k < 4; ++k) {
            double acc = 0.0;
            for (int s = 0; s < a.ncones; ++s) acc += a.V[a.cones[s].voff + 3L * a.cones[s].mloc + k];
            a.vecs[3L * a.m + k] += acc;
        }
    }
}

size_t hdm_grouped_lds_bytes(int n16) { return sizeof(double) * (4 * (size_t) n16 * n16 + 3 * GR_W + 4); }

int hdm_grouped_inverses(const HdmGroupedArgs &a, hipStream_t s) {
    if (a.ncones < 1 || a.max_n16 > HDM_GROUPED_MAX_N) return 1;
    hipLaunchKernelGGL(hdm_grouped_inverse_kernel, dim3(a.ncones), dim3(GR_T), 0, s, a);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_grouped_jobs(const HdmGroupedArgs &a, hipStream_t s) {
    if (a.njobs < 1 || a.max_n16 < 16 || a.max_n16 > HDM_GROUPED_MAX_N || (a.max_n16 & 15) || a.typeKKT < 0 || a.typeKKT > 2) return 1;
    const size_t lds = hdm_grouped_lds_bytes(a.max_n16);
    if (lds > 160 * 1024) return 1;
    static thread_local int configured_dev = -1;
    int dev = 0;
    HDM_HIP_CHECK(hipGetDevice(&dev));
    if (configured_dev != dev) {
        HDM_HIP_CHECK(hipFuncSetAttribute((const void *) hdm_grouped_jobs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        configured_dev = dev;
    }
    hipLaunchKernelGGL(hdm_grouped_jobs_kernel, dim3(a.njobs), dim3(GR_T), lds, s, a);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

int hdm_grouped_scatter(const HdmGroupedScatterArgs &a, const HdmMatView &Mv, hipStream_t s) {
    if (a.ncones < 1 || a.typeKKT < 0 || a.typeKKT > 2) return 1;
    const long threads = (a.typeKKT == 1 ? 0L : a.nM) + a.nV + 1;
    hipLaunchKernelGGL(hdm_grouped_scatter_kernel, dim3((unsigned) ((threads + GR_T - 1) / GR_T)), dim3(GR_T), 0, s, a, Mv);
    HDM_HIP_CHECK(hipGetLastError());
    return 0;
}

// one kernel of this translation unit (= one code object): what the preload thread asks the runtime about (engine.hip: preload_modules)
const void *hdm_module_handle_small() { return (const void *) hdm_small_phase_a_kernel; }
