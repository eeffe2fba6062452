// lp_kernels.h -- device kernels of the LP cone (engine_lp.h).  Implementation header of engine.hip: included once, at global
// scope, ahead of the anonymous namespace that holds the cone itself.  Every reduction runs in a fixed order, so two builds of
// the same state are bit-identical.
#pragma once

// out[j] = sum_i (a * y_i) * A_ij over LP column j's entries in ascending constraint order: the reference's csp_Axpy
// (linalg/sparse_opts.c:21-34) restated column by column, with the same rounding (no contraction into fused multiply-adds),
// so that the dual buffers the host finishes from it are the reference's to the last bit
__global__ void lp_col_axpy_kernel(int n, const int *__restrict__ cbeg, const int *__restrict__ cidx, const double *__restrict__ cval,
                                   double a, const double *__restrict__ y, double *__restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double t = 0.0;
    for (int e = cbeg[j]; e < cbeg[j + 1]; ++e) t = __dadd_rn(t, __dmul_rn(__dmul_rn(a, y[cidx[e]]), cval[e]));
    out[j] = t;
}

// one workgroup per constraint row i (the reference's rowMatBeg layout), fixed-order tree reduction:
//   vecs[i]         += sum_j A_ij d_j                  ASinv
//   vecs[m + i]     += sum_j A_ij Rd d_j^2             ASinvRdSinv  (Rd != 0)
//   vecs[2 m + i]   += sum_j A_ij c_j d_j^2            ASinvCSinv   (homogeneous)
// (hdsdp_conic_lp.c:271-326: d = 1/s, or the registered primal X for KKT_TYPE_PRIMAL)
__global__ void __launch_bounds__(256) lp_vecs_kernel(int m, const int *__restrict__ rbeg, const int *__restrict__ ridx,
                                                      const double *__restrict__ rval, const double *__restrict__ d,
                                                      const double *__restrict__ obj, double Rd, int homo, double *__restrict__ vecs) {
    __shared__ double red[3][256];
    const int i = blockIdx.x, t = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int e = rbeg[i] + t; e < rbeg[i + 1]; e += 256) {
        const int j = ridx[e];
        const double v = rval[e], dj = d[j], d2 = dj * dj;
        s0 += v * dj;
        s1 += v * (Rd * d2);
        if (homo) s2 += v * (obj[j] * d2);
    }
    red[0][t] = s0; red[1][t] = s1; red[2][t] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; red[2][t] += red[2][t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        vecs[i] += red[0][0];
        if (Rd != 0.0) vecs[m + i] += red[1][0];
        if (homo) vecs[2 * (long) m + i] += red[2][0];
    }
}

// dense path: LP columns c0 .. c0 + kc - 1 of W = A diag(d) into the K-major, 16-deep blocked operand of the Gram role,
// element (i, k) at W[(k / 16) * ldb + i * 16 + k % 16] (ldb = padded rows * 16); the buffer was zeroed before
__global__ void lp_scatter_kernel(int c0, int kc, const int *__restrict__ cbeg, const int *__restrict__ cidx, const double *__restrict__ cval,
                                  const double *__restrict__ d, long ldb, double *__restrict__ W) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= kc) return;
    const int j = c0 + k;
    const double dj = d[j];
    double *col = W + (long) (k >> 4) * ldb + (k & 15);
    for (int e = cbeg[j]; e < cbeg[j + 1]; ++e) col[(long) cidx[e] * 16] = cval[e] * dj;
}

// sparse path: pair q = (row i, column j), i >= j, with terms (k, A_ik A_jk) in ascending k:  M(i, j) += sum A_ik A_jk d_k^2
__global__ void lp_pairs_kernel(long npair, const int *__restrict__ prow, const int *__restrict__ pcol, const long *__restrict__ pbeg,
                                const int *__restrict__ tcol, const double *__restrict__ tval, const double *__restrict__ d,
                                double *__restrict__ M, long ldm) {
    const long q = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npair) return;
    double s = 0.0;
    for (long e = pbeg[q]; e < pbeg[q + 1]; ++e) {
        const double dk = d[tcol[e]];
        s += tval[e] * (dk * dk);
    }
    M[prow[q] + (long) pcol[q] * ldm] += s;
}
