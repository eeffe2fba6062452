// primal_kernels.h -- device kernels of the signed congruence route of KKT_TYPE_PRIMAL (engine_build.h: build_primal, route 1).
// Implementation header of engine.hip: included once, at global scope, ahead of the anonymous namespace that holds the cone.
// Every reduction runs in a fixed order: two builds of the same state are bit-identical.
#pragma once

#define MI_PSIG_BLOCKS 256   // partial sums of the factor's acceptance check (one per workgroup, summed by one workgroup)

// Ws = diag(sig) W: row i of the npad x npad matrix W scaled by sig[i]
__global__ void mi_psig_rowscale_kernel(const double *__restrict__ W, const double *__restrict__ sig, double *__restrict__ Ws,
                                        long ld, int npad) {
    const long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long) npad * npad) return;
    const int i = (int) (e % npad), j = (int) (e / npad);
    Ws[i + (long) j * ld] = sig[i] * W[i + (long) j * ld];
}

// partial sums over the n x n valid part: [0] |Y - X|^2, [1] |X|^2, [2] |W|^2 (Y = W^T diag(sig) W), workgroup b at part + 3 b
__global__ __launch_bounds__(256) void mi_psig_norms_kernel(const double *__restrict__ Y, const double *__restrict__ X,
                                                            const double *__restrict__ W, long ld, int n, double *__restrict__ part) {
    __shared__ double red[3][256];
    double d = 0.0, x = 0.0, w = 0.0;
    const long tot = (long) n * n;
    for (long e = (long) blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long) gridDim.x * blockDim.x) {
        const long o = (e % n) + (e / n) * ld;
        const double xv = X[o], r = Y[o] - xv, wv = W[o];
        d += r * r; x += xv * xv; w += wv * wv;
    }
    red[0][threadIdx.x] = d; red[1][threadIdx.x] = x; red[2][threadIdx.x] = w;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int) threadIdx.x < s)
            for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 3) part[3 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}
__global__ void mi_psig_norms_final_kernel(const double *__restrict__ part, int nb, double *__restrict__ out) {
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += part[3 * b + threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// the "S row" of the Gram operand (At = I on the other routes) as diag(sig): <At_i, diag(sig)> under the signed weights is
// tr(A_i W^T diag(sig) W) = tr(A_i X); written to the diagonal sub-blocks only (the off-diagonal ones stay zero, as for I)
__global__ void mi_psig_srow_kernel(double *__restrict__ dst, long row_stride, long row, int nblk, int n, const double *__restrict__ sig) {
    const int b = blockIdx.x;
    const int c = threadIdx.x >> 4, r = threadIdx.x & 15;
    const long sub = hdm_blk_col_start(b, nblk);
    const long pb = sub * 16 + c;
    const int gi = b * 16 + c;
    dst[(pb * row_stride + row) * 16 + r] = (r == c && gi < n) ? sig[gi] : 0.0;
}

// Gather of the packed columns of one sign into a compact K-major operand for the Gram role:
//   dst[(j / 16) R 16 + r 16 + j % 16] = Ahat(row r, packed column cols[j])       (zero for ncols <= j < ncols16)
// Ahat in the layout the Gram product reads ([segment][p-block][Lr][16], p-blocks counted from pb0 on this rank); Gram row r
// lies in segment r / Lr.  Threads run along j inside a row: every 16 of them write one 128-byte line.
__global__ void mi_psig_gather_kernel(const double *__restrict__ src, long seg_stride, int Lr, long R, const int *__restrict__ cols,
                                      long ncols, long ncols16, long pb0, double *__restrict__ dst) {
    const long tot = R * ncols16;
    for (long e = (long) blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long) gridDim.x * blockDim.x) {
        const long jl = e & 15, r = (e >> 4) % R, jb = (e >> 4) / R;
        const long j = jb * 16 + jl;
        double v = 0.0;
        if (j < ncols) {
            const int k = cols[j];
            v = src[(r / Lr) * seg_stride + (((long) (k >> 4) - pb0) * Lr + (r % Lr)) * 16 + (k & 15)];
        }
        dst[e] = v;
    }
}

// Gm = beta Gm + sum_z slab_z over the lower 128-tiles (what the Gram launch writes), slabs summed in a fixed order
__global__ void mi_psig_combine_kernel(double *__restrict__ Gm, const double *__restrict__ slabs, long slab_stride, int nz, long R,
                                       double beta) {
    const long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= R * R) return;
    if (((e / R) >> 7) > ((e % R) >> 7)) return;
    double s = 0.0;
    for (int z = 0; z < nz; ++z) s += slabs[e + (long) z * slab_stride];
    Gm[e] = beta * Gm[e] + s;
}
