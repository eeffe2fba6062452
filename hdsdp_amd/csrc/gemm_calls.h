// gemm_calls.h -- the argument block of the fp64 MFMA GEMM family (HdmGemmArgs) and the call forms that fill it: the plain
// product, and the launches of a dense block's Schur build (congruence step 1 and 2, the "I row", the Gram splits, the gathered
// Gram product of the signed route, the LP cone's Gram-role product).  A call site is one form followed by hdm_launch_gemm; no
// other file assigns a field (the launcher, gemm_f64.hip, splits role 2 into its two kernels and defaults a_kblk / b_kblk).
// A Schur form states the whole contract of its role -- storage classes, K limit, the mirrored second pair, the blocked
// destination, the row segments of a sharded Gram operand, the spans that vouch for the unmasked tile loads (work_plan.h, beside
// the byte counts that size the same buffers), the algorithmic flops of the roofline -- so what the launcher would refuse at run
// time cannot be written, and tests/test_gemm_calls_cpu.py checks every field without a device.
// Pure host arithmetic: no HIP header, no allocation, no environment, no I/O, no state.
#pragma once
#include "gemm_geom.h"
#include "work_plan.h"

// ---------------------------------------------------------------------------------------------
// GEMM family (gemm_f64.hip).  Everything is column-major fp64.
//   C[M x N] = alpha * A[M x K] * B[N x K]^T + beta * C
// Operand storage is selected per operand:
//   M-major ("N"): element (i,k) at X[i + k*ld]  (rows contiguous: a column-major M x K matrix)
//   K-major ("T"): element (i,k) at X[i*ld + k]  (k contiguous: the transpose is column-major)
// ---------------------------------------------------------------------------------------------
struct HdmGemmArgs {
    const double *A, *B;
    double *C;
    // optional second product accumulated into the same tile (SYR2K form): C = alpha (A B^T + A2 B2^T) + beta C,
    // same shapes, storage classes and K range as the first pair; A2 == nullptr: single product
    const double *A2, *B2;
    long lda2, ldb2, strideA2, strideB2;
    int b_sky;        // congruence step 1: the B operand is a batch of skyline-stored A_L matrices (N = their dimension)
    // roles 1-3 (unmasked tile loads): elements readable from each operand pointer, slack included; checked at launch
    long spanA, spanB, spanA2, spanB2;
    long lda, ldb, ldc;
    long strideA, strideB, strideC;  // batch strides (elements) along blockIdx.z (batch) -- 0 = shared
    int M, N, K;
    int a_kmajor, b_kmajor;
    long a_kblk, b_kblk;  // K-major operands: elements between consecutive 16-deep k blocks (16 for a plain matrix)
    // K-major operands may be cut into row segments (one per source rank after the multi-GPU transpose):
    // element offset += (row / seg_rows) * seg_extra.  seg_rows == 0: one segment.
    long seg_rows, seg_extra;
    int klimit;       // HdmKLimit: triangular operand => shorter K loop for early tiles
    int lower_only;   // only tiles with tile_m >= tile_n are computed (C symmetric / lower)
    unsigned long long tile_col_mask;  // != 0: only tile columns whose bit is set are computed (N <= 64 tiles; multi-GPU
                                       // builds run congruence step 2 by packed-index range, see engine.hip)
    int epilogue;     // HdmEpilogue
    int batch;        // number of batch entries (grid z for STORE/BLOCKED), or #K-splits for SLAB
    int queue_global; // persistent launches: ONE job queue for the whole chip, batch entry (K split) by batch entry in order,
                      // instead of one queue per XCD over the entries x, x + 8, ... (gemm_tile.h: hdm_gemm_persist_kernel)
    double alpha, beta;
    int role;         // HdmRole
    double flops;     // algorithmic flops of this launch (valid data only), for the live roofline
    // BLOCKED epilogue: destination chunk layout  dst[((blk*16 + c_local) * rowStride + row) * 16 + r_local]
    long blk_row_stride;  // = m_pad (number of constraint rows per 16-wide p-block)
    long blk_row0;        // constraint row of batch entry 0
    int nblk;             // n/16: sub-blocks per matrix edge
    // SLAB epilogue / split-K
    long k_chunk;         // K range per split (multiple of HDM_BK)
    long k_base;          // first k of split 0 (a launch may cover a sub-range of the splits; C then points at its first slab)
    long slab_stride;     // elements between slabs
};

// ---- the plain product ------------------------------------------------------------------------
// C = alpha op(A) op(B)^T + beta C: generic role, STORE epilogue.  An operand is pointer, leading dimension, storage class and
// the stride between the matrices of a batch.  The rare options follow beta as one value that names them where it is written:
// hdm_klimit(HDM_KLIM_BY_M), hdm_lower(), hdm_batched(count, strideC), chained with a dot where a product has several.
struct HdmOperand { const double *p; long ld; int kmajor; long stride; };
inline HdmOperand hdm_operand(const double *p, long ld, int kmajor, long stride = 0) { return {p, ld, kmajor, stride}; }
inline HdmOperand hdm_mmajor(const double *p, long ld, long stride = 0) { return {p, ld, 0, stride}; }
inline HdmOperand hdm_kmajor(const double *p, long ld, long stride = 0) { return {p, ld, 1, stride}; }

struct HdmGemmOpt {
    int klim = HDM_KLIM_NONE, lower_only = 0, batch = 1;
    long strideC = 0;
    HdmGemmOpt klimit(int k) const { HdmGemmOpt o = *this; o.klim = k; return o; }                  // HdmKLimit: a triangular operand
    HdmGemmOpt lower(int on = 1) const { HdmGemmOpt o = *this; o.lower_only = on; return o; }        // only tiles with tile_m >= tile_n
    HdmGemmOpt batched(int count, long strideC_) const { HdmGemmOpt o = *this; o.batch = count; o.strideC = strideC_; return o; }
};
inline HdmGemmOpt hdm_klimit(int k) { return HdmGemmOpt().klimit(k); }
inline HdmGemmOpt hdm_lower() { return HdmGemmOpt().lower(); }
inline HdmGemmOpt hdm_batched(int count, long strideC) { return HdmGemmOpt().batched(count, strideC); }

inline HdmGemmArgs hdm_gemm_product(double *C, long ldc, int M, int N, int K, double alpha, HdmOperand A, HdmOperand B, double beta = 0.0,
                                    HdmGemmOpt o = {}) {
    HdmGemmArgs a = {};
    a.A = A.p; a.lda = A.ld; a.a_kmajor = A.kmajor; a.strideA = A.stride;
    a.B = B.p; a.ldb = B.ld; a.b_kmajor = B.kmajor; a.strideB = B.stride;
    a.C = C; a.ldc = ldc; a.strideC = o.strideC;
    a.M = M; a.N = N; a.K = K; a.batch = o.batch; a.alpha = alpha; a.beta = beta;
    a.klimit = o.klim; a.lower_only = o.lower_only; a.epilogue = HDM_EPI_STORE; a.role = HDM_ROLE_GENERIC;
    return a;
}

// ---- the congruence -----------------------------------------------------------------------------
// rows of AhatLoc  <-  blocked( Linv * A * Linv^T ),  A = A_L + A_L^T given in A_L form:
//   step 1  U  = Linv * A_L                 (lower x lower = lower triangular: k in [col tile, row tile], n^3/3)
//   step 2  At = U * Linv^T + Linv * U^T    (SYR2K form, lower tiles, k <= col tile, 2n^3/3)
// i.e. n^3 flops per constraint instead of the 4/3 n^3 of (Linv A) Linv^T, and half the intermediate traffic.
// `Linv`, `ldl`: the factor inverse, npad x npad with leading dimension npad; `n`: the block's dimension before padding.
//
// Step 1 of the `nb` matrices from `b0` on of a source buffer that holds `src_rows` skyline matrices: T[0 .. nb) = Linv * A_L.
inline HdmGemmArgs hdm_cong_step1(const HdmLayout &L, int n, const double *Linv, long ldl, const double *Asrc, long src_rows, long b0,
                                  int nb, double *T) {
    const long nn = (long) L.n16 * L.n16;
    HdmGemmArgs a = hdm_gemm_product(T, L.n16, L.n16, L.n16, L.n16, 1.0, hdm_mmajor(Linv, ldl), hdm_kmajor(Asrc + b0 * L.astride, L.n16, L.astride),
                                     0.0, hdm_klimit(HDM_KLIM_BAND).lower().batched(nb, nn));
    a.b_sky = 1; a.role = HDM_ROLE_CONG1;
    a.spanA = hdm_linv_span(ldl); a.spanB = hdm_afull_span(L, src_rows) - b0 * L.astride;
    a.flops = (double) nb * ((double) n * n * n) / 3.0;
    return a;
}
// Step 2 of the `nb` matrices step 1 left in T, into constraint rows blk_row0 .. of the blocked destination; `colmask` != 0:
// only the tile columns of the mask.  The second pair mirrors the first by construction.
inline HdmGemmArgs hdm_cong_step2(const HdmLayout &L, int n, long Bc, const double *Linv, long ldl, const double *T, int nb, double *dst,
                                  long blk_row0, unsigned long long colmask = 0) {
    const long nn = (long) L.n16 * L.n16;
    HdmGemmArgs a = hdm_gemm_product(dst, 0, L.n16, L.n16, L.n16, 1.0, hdm_mmajor(T, L.n16, nn), hdm_mmajor(Linv, ldl), 0.0,
                                     hdm_klimit(HDM_KLIM_BY_N).lower().batched(nb, 0));
    a.A2 = a.B; a.lda2 = a.ldb; a.strideA2 = a.strideB;
    a.B2 = a.A; a.ldb2 = a.lda; a.strideB2 = a.strideA;
    a.epilogue = HDM_EPI_BLOCKED; a.blk_row_stride = L.Lr; a.blk_row0 = blk_row0; a.nblk = L.nblk; a.role = HDM_ROLE_CONG2;
    a.tile_col_mask = colmask;
    a.spanA = a.spanB2 = hdm_t_span(L, Bc); a.spanB = a.spanA2 = hdm_linv_span(ldl);
    a.flops = (double) nb * ((double) n * n * n) * 2.0 / 3.0 * hdm_cong2_mask_share(hdm_ntiles(L.n16), colmask);
    return a;
}
// The "I row": A = I => T = Linv, At = Linv Linv^T.  Step 2's product with T := Linv, one pair, generic role.
inline HdmGemmArgs hdm_cong_irow(const HdmLayout &L, const double *Linv, long ldl, double *dst, long blk_row0) {
    HdmGemmArgs a = hdm_gemm_product(dst, 0, L.n16, L.n16, L.n16, 1.0, hdm_mmajor(Linv, ldl), hdm_mmajor(Linv, ldl), 0.0, hdm_klimit(HDM_KLIM_BY_N).lower());
    a.epilogue = HDM_EPI_BLOCKED; a.blk_row_stride = L.Lr; a.blk_row0 = blk_row0; a.nblk = L.nblk;
    return a;
}

// ---- the Gram role --------------------------------------------------------------------------------
// lower(C) (+)= alpha W W^T over W in [k block][row][16] storage: both operands K-major, 16 between rows, `kblk` between k blocks
inline HdmGemmArgs hdm_gram_product(double *C, long ldc, int rows, int K, double alpha, double beta, const double *W, long kblk, long span) {
    HdmGemmArgs a = hdm_gemm_product(C, ldc, rows, rows, K, alpha, hdm_kmajor(W, 16), hdm_kmajor(W, 16), beta, hdm_lower());
    a.a_kblk = a.b_kblk = kblk; a.spanA = a.spanB = span; a.role = HDM_ROLE_GRAM;
    return a;
}
inline HdmGemmArgs hdm_gram_slabs(HdmGemmArgs a, int nz, long k_chunk, long k_base, int queue_global) {
    a.epilogue = HDM_EPI_SLAB; a.batch = nz; a.k_chunk = k_chunk; a.k_base = k_base; a.slab_stride = a.ldc * a.ldc; a.queue_global = queue_global;
    return a;
}
// p-blocks per K split of a block's Gram product: the one statement of it (the splits below; the exchange pieces of a sharded
// build, whole groups of splits -- engine_build.h: piece_range)
inline long hdm_gram_chunk(const HdmLayout &L, long nsplit) { return (L.npb_loc + nsplit - 1) / nsplit; }
// p-blocks [lo, hi) of every destination's chunk that piece k of P carries: the K ranges of the splits [k nsplit / P, (k + 1) nsplit / P)
inline void hdm_piece_range(const HdmLayout &L, long nsplit, int k, int P, long *lo, long *hi) {
    const long chunk = hdm_gram_chunk(L, nsplit), zper = nsplit / P;
    *lo = std::min<long>(L.npb_loc, (long) k * zper * chunk);
    *hi = (k == P - 1) ? L.npb_loc : std::min<long>(L.npb_loc, (long) (k + 1) * zper * chunk);
}
// The K splits [z0, z0 + nz) of `nsplit`: slabs `slab` .. <- (or +=, `accumulate`) Ahat * Ahat^T over their share of this rank's
// p-range; rows in segment order, one segment per source rank.  `n`, `m`: the block's dimension and constraint count.
inline HdmGemmArgs hdm_gram_splits(const HdmLayout &L, int n, int m, long nsplit, int z0, int nz, const double *Ahat, double *slab, bool accumulate,
                                   bool queue_global) {
    const long chunk = hdm_gram_chunk(L, nsplit) * 16;
    HdmGemmArgs a = hdm_gram_slabs(hdm_gram_product(slab, L.R, (int) L.R, (int) (L.npb_loc * 16), 1.0, accumulate ? 1.0 : 0.0, Ahat, (long) L.Lr * 16,
                                                    hdm_exchange_span(L)), nz, chunk, (long) z0 * chunk, queue_global ? 1 : 0);
    if (L.world > 1) { a.seg_rows = L.Lr; a.seg_extra = L.npb_loc * L.Lr * 16 - (long) L.Lr * 16; }
    // (m+3)(m+4)/2 inner products of length n(n+1)/2 (this rank's share), 2 flops each
    const double rows = (double) m + 3.0;
    a.flops = rows * (rows + 1.0) * 0.5 * ((double) n * (n + 1) * 0.5) * 2.0 / L.world * ((double) nz / nsplit);
    return a;
}
// The gathered Gram product of the signed route (engine_build.h: signed_correction): `nc` gathered columns (nc16 = nc rounded
// up to 16) of R rows in `nz` splits into the first nz slabs; `span`: the gather buffer's size.
inline HdmGemmArgs hdm_gram_gathered(long R, long nc, long nc16, int nz, double alpha, bool accumulate, const double *gat, long span, double *slabs,
                                     bool queue_global) {
    HdmGemmArgs a = hdm_gram_slabs(hdm_gram_product(slabs, R, (int) R, (int) nc16, alpha, accumulate ? 1.0 : 0.0, gat, R * 16, span), nz,
                                   (nc16 / 16 + nz - 1) / nz * 16, 0, queue_global ? 1 : 0);
    a.flops = (double) R * (R + 1) * 0.5 * (double) nc * 2.0;
    return a;
}
// The LP cone's product (engine_lp.h): M(lower) += W W^T over a chunk of `kv` columns (kp = kv rounded up to 16; chunks of at
// most `kc`) of the m16 padded rows of W, `mpad` rows per k block; STORE epilogue with beta = 1.
inline HdmGemmArgs hdm_gram_lp(int m, int m16, int mpad, int kc, int kv, int kp, const double *W, double *M, long ldm) {
    HdmGemmArgs a = hdm_gram_product(M, ldm, m16, kp, 1.0, 1.0, W, (long) mpad * 16, hdm_lp_span(kc, mpad));
    a.flops = (double) m * (m + 1) * (double) kv;     // lower triangle, 2 flops a term
    return a;
}
