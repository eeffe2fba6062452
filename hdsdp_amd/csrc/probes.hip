// probes.hip -- raw kernels exported for unit tests and micro-benchmarks, and the measurement probes (fp64 MFMA peak / issue
// rate, diagonal-block kernel, envelope Cholesky).  Its own translation unit: nothing here is on the product path; it reaches
// the engine only through the C ABI (HMiStream) and the kernel objects' headers.  Split out of engine.hip in round 3.
#include "../../include/hdsdp_mi355x.h"
#include "chol.h"
#include "hdm_common.h"
#include "refine.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {
// the engine's stream (HMiStream brings the context up) and two events of this file's own
struct ProbeCtx { hipStream_t stream = nullptr; hipEvent_t ev[8] = {}; bool init = false; };
ProbeCtx g;
int ensure_ctx() {
    if (g.init) return 0;
    g.stream = (hipStream_t) HMiStream();
    if (!g.stream) return 1;
    for (int i = 6; i < 8; ++i) if (hipEventCreate(&g.ev[i]) != hipSuccess) return 1;
    g.init = true;
    return 0;
}
}  // namespace

__device__ __forceinline__ double mi_hash_unit(unsigned x) {  // pseudo-random in (-1, 1)
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return (double) (int) x / 2147483648.0;
}
// same loop on full-range pseudo-random operands (data-dependent power -> sustained clock)
__global__ __launch_bounds__(256, 2) void mi_mfma_probe_rand_kernel(double *out, int iters) {
    hdm_d4 acc[4][4];
    const unsigned gid = blockIdx.x * 256 + threadIdx.x;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i)
            for (int r = 0; r < 4; ++r) acc[j][i][r] = mi_hash_unit(gid * 64 + j * 16 + i * 4 + r);
    double fa[4], fb[4];
    for (int i = 0; i < 4; ++i) { fa[i] = mi_hash_unit(gid * 8 + i + 1000003u); fb[i] = mi_hash_unit(gid * 8 + 4 + i + 7000001u); }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[j], fb[i], acc[j][i], 0, 0, 0);
    }
    double s = 0.0;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) s += acc[j][i][0] + acc[j][i][1] + acc[j][i][2] + acc[j][i][3];
    if (s == 12345.678) out[0] = s;
}

__global__ void mi_mfma_probe_kernel(double *out, int iters) {
    hdm_d4 acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = (hdm_d4){0.0, 0.0, 0.0, 0.0};
    double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0.0;
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) out[0] = s;  // keep the loop alive
}

// GEMM-shaped MFMA issue probe: 16 accumulators fed by 4 + 4 operand registers exactly like the GEMM inner loop,
// no memory traffic at all.  NW = waves per workgroup.
template <int MODE>
__global__ __launch_bounds__(256, 2) void mi_mfma_probe2_kernel(double *out, int iters) {
    hdm_d4 acc[4][4];
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) acc[j][i] = (hdm_d4){0.0, 0.0, 0.0, 0.0};
    double fa[4], fb[4];
    for (int i = 0; i < 4; ++i) { fa[i] = 1.0 + threadIdx.x * 1e-9 * (i + 1); fb[i] = 1.0 - threadIdx.x * 1e-9 * (i + 2); }
    for (int it = 0; it < iters; ++it) {
        if (MODE == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[j], fb[i], acc[j][i], 0, 0, 0);
        } else if (MODE == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[0], fb[0], acc[j][i], 0, 0, 0);
        } else {  // 8 accumulators only (2 x 4), GEMM operand pattern
#pragma unroll
            for (int rep = 0; rep < 2; ++rep)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[j][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[j], fb[i], acc[j][i], 0, 0, 0);
        }
    }
    double s = 0.0;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) s += acc[j][i][0] + acc[j][i][1] + acc[j][i][2] + acc[j][i][3];
    if (s == 12345.678) out[0] = s;
}

template <int NACC, int LB>
__global__ __launch_bounds__(256, LB) void mi_mfma_probe3_kernel(double *out, int iters) {
    hdm_d4 acc[NACC];
    for (int i = 0; i < NACC; ++i) acc[i] = (hdm_d4){0.0, 0.0, 0.0, 0.0};
    double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0.0;
    for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) out[0] = s;
}


extern "C" {

// ---------------------------------------------------------------- raw kernels for tests
int HMiGemmNT(const double *A, int64_t lda, int aKMajor, const double *B, int64_t ldb, int bKMajor, double *C,
              int64_t ldc, int M, int N, int K, double alpha, double beta, int kLimit, int lowerOnly) {
    if (ensure_ctx()) return 1;
    if (hdm_launch_gemm(hdm_gemm_product(C, ldc, M, N, K, alpha, hdm_operand(A, lda, aKMajor), hdm_operand(B, ldb, bKMajor), beta, hdm_klimit(kLimit).lower(lowerOnly)),
                        g.stream)) return 1;
    HDM_HIP_CHECK(hipStreamSynchronize(g.stream));
    return 0;
}

// The call forms of a dense block's Schur build (gemm_calls.h), one launch each on the caller's device buffers.  The caller
// says how many doubles every buffer holds; an entry refuses (returns 1, launches nothing) when an operand buffer is smaller
// than the span its form vouches for or the destination smaller than what the form writes, so that no argument a test can
// write makes a kernel read or write outside an allocation (the launcher checks the unmasked loads' reach against the span).
// Each is one form followed by hdm_launch_gemm and a synchronise: no field is assigned here.
namespace {
int run_form(const HdmGemmArgs &a) {
    if (ensure_ctx()) return 1;
    if (hdm_launch_gemm(a, g.stream)) return 1;
    HDM_HIP_CHECK(hipStreamSynchronize(g.stream));
    return 0;
}
bool layout_args_ok(int n, int world, int maxloc) { return n >= 1 && n <= (1 << 15) && world >= 1 && world <= 64 && maxloc >= 0 && maxloc <= (1 << 20); }
// doubles of a blocked congruence destination: every p-block of the triangle, Lr constraint rows of 16 each
long blocked_doubles(const HdmLayout &L) { return L.npb * L.Lr * 16; }
bool linv_ok(const HdmLayout &L, int64_t ldl, int64_t linv_len) { return ldl >= hdm_roundup(L.n16, HDM_TILE) && ldl <= (1 << 20) && linv_len >= hdm_linv_span(ldl); }
}  // namespace

int HMiGemmRoleLayout(int n, int world, int maxloc, int64_t *out, int cap) {
    if (!out || cap < 7 || !layout_args_ok(n, world, maxloc)) return -7;
    const HdmLayout L = hdm_layout(n, world, maxloc);
    const int64_t v[7] = {L.n16, L.nblk, L.npb, L.npb_loc, L.Lr, L.R, L.astride};
    std::copy(v, v + 7, out);
    return 7;
}
int64_t HMiGemmRoleSpan(int which, int n, int world, int maxloc, int64_t a0, int64_t a1) {
    if (!layout_args_ok(n, world, maxloc) || a0 < 0 || a1 < 0 || a0 > (1 << 20) || a1 > (1 << 20)) return -1;
    const HdmLayout L = hdm_layout(n, world, maxloc);
    switch (which) {
        case 0: return hdm_t_span(L, a0);
        case 1: return hdm_linv_span(a0);
        case 2: return hdm_afull_span(L, a0);
        case 3: return hdm_exchange_span(L);
        case 4: return hdm_lp_span((int) a0, (int) a1);
        default: return -1;
    }
}
int HMiCongStep1(int n, int world, int maxloc, const double *Linv, int64_t linv_len, int64_t ldl, const double *Asrc, int64_t asrc_len,
                 int64_t src_rows, int64_t b0, int nb, double *T, int64_t t_len) {
    if (!layout_args_ok(n, world, maxloc) || !Linv || !Asrc || !T) return 1;
    const HdmLayout L = hdm_layout(n, world, maxloc);
    if (!linv_ok(L, ldl, linv_len) || nb < 1 || b0 < 0 || src_rows < b0 + nb || asrc_len < hdm_afull_span(L, src_rows) ||
        t_len < (int64_t) nb * L.n16 * L.n16) return 1;
    return run_form(hdm_cong_step1(L, n, Linv, ldl, Asrc, src_rows, b0, nb, T));
}
int HMiCongStep2(int n, int world, int maxloc, int64_t Bc, const double *Linv, int64_t linv_len, int64_t ldl, const double *T, int64_t t_len,
                 int nb, double *dst, int64_t dst_len, int64_t blk_row0, uint64_t colmask) {
    if (!layout_args_ok(n, world, maxloc) || !Linv || !T || !dst) return 1;
    const HdmLayout L = hdm_layout(n, world, maxloc);
    if (!linv_ok(L, ldl, linv_len) || nb < 1 || Bc < nb || t_len < hdm_t_span(L, Bc) || blk_row0 < 0 || blk_row0 + nb > L.Lr ||
        dst_len < blocked_doubles(L)) return 1;
    return run_form(hdm_cong_step2(L, n, Bc, Linv, ldl, T, nb, dst, blk_row0, colmask));
}
int HMiCongIRow(int n, int world, int maxloc, const double *Linv, int64_t linv_len, int64_t ldl, double *dst, int64_t dst_len, int64_t blk_row0) {
    if (!layout_args_ok(n, world, maxloc) || !Linv || !dst) return 1;
    const HdmLayout L = hdm_layout(n, world, maxloc);
    if (!linv_ok(L, ldl, linv_len) || blk_row0 < 0 || blk_row0 >= L.Lr || dst_len < blocked_doubles(L)) return 1;
    return run_form(hdm_cong_irow(L, Linv, ldl, dst, blk_row0));
}
int HMiGramSplits(int n, int world, int maxloc, int m, int64_t nsplit, int z0, int nz, const double *Ahat, int64_t ahat_len, double *slab,
                  int64_t slab_len, int accumulate, int queue_global) {
    if (!layout_args_ok(n, world, maxloc) || !Ahat || !slab) return 1;
    const HdmLayout L = hdm_layout(n, world, maxloc);
    if (nsplit < 1 || nsplit > L.npb_loc || z0 < 0 || nz < 1 || z0 + (int64_t) nz > nsplit || ahat_len < hdm_exchange_span(L) ||
        slab_len < (int64_t) nz * L.R * L.R) return 1;
    return run_form(hdm_gram_splits(L, n, m, nsplit, z0, nz, Ahat, slab, accumulate != 0, queue_global != 0));
}
int HMiGramGathered(int64_t R, int64_t nc, int nz, double alpha, int accumulate, const double *gat, int64_t gat_len, double *slabs,
                    int64_t slabs_len, int queue_global) {
    if (!gat || !slabs || R < 8 || R > (1 << 20) || (R % 8) || nc < 1 || nc > (1 << 24) || nz < 1 || nz > 4096) return 1;
    const long nc16 = hdm_roundup(nc, 16);
    if (gat_len < nc16 * R || slabs_len < (int64_t) nz * R * R) return 1;
    return run_form(hdm_gram_gathered(R, nc, nc16, nz, alpha, accumulate != 0, gat, gat_len, slabs, queue_global != 0));
}
int HMiGramLp(int m, int mpad, int kc, int kv, const double *W, int64_t w_len, double *M, int64_t m_len, int64_t ldm) {
    if (!W || !M || m < 1 || mpad < 1 || mpad > (1 << 20) || kc < 16 || (kc % 16) || kv < 1 || kv > kc) return 1;
    const int m16 = (int) hdm_roundup(m, 16), kp = (int) hdm_roundup(kv, 16);
    if (m16 > mpad || w_len < hdm_lp_span(kc, mpad) || ldm < m16 || m_len < (int64_t) (m16 - 1) * ldm + m16) return 1;
    return run_form(hdm_gram_lp(m, m16, mpad, kc, kv, kp, W, M, ldm));
}

// blocked Cholesky + solve of a host matrix (lower triangle, column-major, leading dimension n) whose structural zeros are
// described by a block envelope: first[i] = first 128-block column with an entry in block row i (NULL = dense)
int HMiCholEnvelopeSolve(const double *A_host, int n, const int *first, const double *b, double *x, double *L_host, int *info) {
    if (ensure_ctx()) return 1;
    HdmChol ch;
    if (ch.init(n)) return 1;
    int rc = 1;
    do {
        if (first && ch.set_envelope(first)) break;
        if (ch.load_host(A_host, n, g.stream)) break;
        if (ch.factor(g.stream, info)) break;
        if (info && *info != 0) { rc = 0; break; }
        if (b && x && ch.solve_host(b, x, 1, 0, g.stream)) break;
        if (L_host && hipMemcpy2D(L_host, sizeof(double) * n, ch.L.get(), sizeof(double) * ch.npad, sizeof(double) * n, n, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = 0;
    } while (0);
    return rc;
}

// the refined solve's residual kernel (refine.hip) on host arrays: M goes up exactly as given -- ld x n doubles, whatever lies
// above the diagonal and in rows >= n included -- and r = b - M x and |r|_2^2 come back
int HMiSymResidualProbe(int n, const double *Mlower, long ld, const double *x, const double *b, double *r, double *norm2) {
    if (n < 1 || ld < n || !Mlower || !x || !b || !r || !norm2 || ensure_ctx()) return 1;
    HdmBuf<double> M, v;
    HdmSymRes res;
    if (M.alloc((size_t) ld * n) != hipSuccess || v.alloc(3 * (size_t) n + 1) != hipSuccess || res.reserve(n)) return 1;
    double *xd = v.get(), *bd = xd + n, *rd = bd + n, *nd = rd + n;
    if (hipMemcpyAsync(M.get(), Mlower, sizeof(double) * (size_t) ld * n, hipMemcpyHostToDevice, g.stream) != hipSuccess ||
        hipMemcpyAsync(xd, x, sizeof(double) * (size_t) n, hipMemcpyHostToDevice, g.stream) != hipSuccess ||
        hipMemcpyAsync(bd, b, sizeof(double) * (size_t) n, hipMemcpyHostToDevice, g.stream) != hipSuccess) return 1;
    if (res.run(M.get(), ld, n, xd, bd, rd, nd, g.stream)) return 1;
    if (hipMemcpyAsync(r, rd, sizeof(double) * (size_t) n, hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
        hipMemcpyAsync(norm2, nd, sizeof(double), hipMemcpyDeviceToHost, g.stream) != hipSuccess ||
        hipStreamSynchronize(g.stream) != hipSuccess) return 1;
    return 0;
}

// diagnostic: factorisation time (ms, HIP events) of an n x n matrix whose pattern is a band of
// `band` 128-blocks below the diagonal block, once as a dense matrix and once on its block envelope
__global__ void mi_band_spd_kernel(double *A, long ld, int n, int band) {
    const long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long) n * n) return;
    const int i = (int) (e % n), j = (int) (e / n);
    double v = 0.0;
    if (i == j) v = 4.0 * (band + 1) * 128.0;
    else if (i > j && i / 128 - j / 128 <= band) v = ((i * 31 + j * 17) % 13 == 0) ? 1.0 / (1.0 + ((i + j) % 7)) : 0.0;
    A[i + (long) j * ld] = v;
}
int HMiCholEnvelopeProbe(int n, int band, int reps, double *ms_dense, double *ms_env) {
    if (ensure_ctx()) return 1;
    double *A = nullptr;
    if (hdm_malloc((void **) &A, sizeof(double) * (size_t) n * n) != hipSuccess) return 1;
    hipLaunchKernelGGL(mi_band_spd_kernel, dim3((unsigned) (((long) n * n + 255) / 256)), dim3(256), 0, g.stream, A, (long) n, n, band);
    int rc = 0;
    for (int pass = 0; pass < 2 && !rc; ++pass) {
        HdmChol ch;
        if (ch.init(n)) { rc = 1; break; }
        std::vector<int> first(ch.nblk);
        for (int b = 0; b < ch.nblk; ++b) first[b] = std::max(0, b - band);
        if (pass == 1 && ch.set_envelope(first.data())) rc = 1;
        float total = 0.f;
        for (int r = -2; r < reps && !rc; ++r) {
            int info = 0;
            if (ch.load_device(A, n, g.stream)) { rc = 1; break; }
            (void) hipEventRecord(g.ev[6], g.stream);
            if (ch.factor(g.stream, &info) || info != 0) { rc = 1; break; }
            (void) hipEventRecord(g.ev[7], g.stream);
            (void) hipEventSynchronize(g.ev[7]);
            float ms = 0.f;
            (void) hipEventElapsedTime(&ms, g.ev[6], g.ev[7]);
            if (r >= 0) total += ms;
        }
        *(pass == 0 ? ms_dense : ms_env) = total / std::max(1, reps);
    }
    (void) hipFree(A);
    return rc;
}

int HMiPotrf(double *A_dev, int n, int64_t lda, int *info) {
    if (ensure_ctx()) return 1;
    HdmChol ch;
    if (ch.init(n)) return 1;
    if (ch.load_device(A_dev, lda, g.stream)) return 1;
    if (ch.factor(g.stream, info)) return 1;
    HDM_HIP_CHECK(hipMemcpy2DAsync(A_dev, sizeof(double) * lda, ch.L.get(), sizeof(double) * ch.npad, sizeof(double) * n, n,
                                   hipMemcpyDeviceToDevice, g.stream));
    HDM_HIP_CHECK(hipStreamSynchronize(g.stream));
    return 0;
}

double HMiDiagBlockProbe(int variant, int reps) {
    if (ensure_ctx()) return -1.0;
    return hdm_diag_block_probe(variant, reps, g.stream);
}

double HMiMfmaPeakProbe(int iters) {
    if (ensure_ctx()) return -1.0;
    double *out = nullptr;
    if (hdm_malloc((void **) &out, 8) != hipSuccess) return -1.0;
    const int blocks = 256 * 8, threads = 256;
    hipLaunchKernelGGL(mi_mfma_probe_kernel, dim3(blocks), dim3(threads), 0, g.stream, out, 16);
    (void) hipEventRecord(g.ev[6], g.stream);
    hipLaunchKernelGGL(mi_mfma_probe_kernel, dim3(blocks), dim3(threads), 0, g.stream, out, iters);
    (void) hipEventRecord(g.ev[7], g.stream);
    (void) hipEventSynchronize(g.ev[7]);
    float ms = 0;
    (void) hipEventElapsedTime(&ms, g.ev[6], g.ev[7]);
    (void) hipFree(out);
    const double flops = (double) blocks * (threads / 64) * (double) iters * 8 * 2.0 * 16 * 16 * 4;
    return flops / (ms * 1e-3) / 1e12;
}

// mode 0: GEMM operand pattern, mode 1: one operand pair; wgPerCu workgroups of 256 threads per CU
double HMiMfmaIssueProbe(int mode, int wgPerCu, int iters) {
    if (ensure_ctx()) return -1.0;
    double *out = nullptr;
    if (hdm_malloc((void **) &out, 8) != hipSuccess) return -1.0;
    const int blocks = 256 * wgPerCu, threads = 256;
    for (int rep = 0; rep < 2; ++rep) {
        if (rep == 1) (void) hipEventRecord(g.ev[6], g.stream);
        if (mode == 300) {
            hipLaunchKernelGGL(mi_mfma_probe_rand_kernel, dim3(blocks), dim3(threads), 0, g.stream, out, iters);
        } else if (mode == 200) {
            hipLaunchKernelGGL(mi_mfma_probe_kernel, dim3(blocks), dim3(threads), 0, g.stream, out, iters * 2);
        } else if (mode >= 100) {
            const int it3 = iters * 16 / (mode % 100);
            switch (mode) {
                case 104: hipLaunchKernelGGL((mi_mfma_probe3_kernel<4, 1>), dim3(blocks), dim3(threads), 0, g.stream, out, it3); break;
                case 108: hipLaunchKernelGGL((mi_mfma_probe3_kernel<8, 1>), dim3(blocks), dim3(threads), 0, g.stream, out, it3); break;
                case 112: hipLaunchKernelGGL((mi_mfma_probe3_kernel<12, 1>), dim3(blocks), dim3(threads), 0, g.stream, out, it3); break;
                case 116: hipLaunchKernelGGL((mi_mfma_probe3_kernel<16, 1>), dim3(blocks), dim3(threads), 0, g.stream, out, it3); break;
                case 124: hipLaunchKernelGGL((mi_mfma_probe3_kernel<24, 1>), dim3(blocks), dim3(threads), 0, g.stream, out, it3); break;
                default: break;
            }
        } else if (mode == 0) hipLaunchKernelGGL(mi_mfma_probe2_kernel<0>, dim3(blocks), dim3(threads), 0, g.stream, out, iters);
        else if (mode == 1) hipLaunchKernelGGL(mi_mfma_probe2_kernel<1>, dim3(blocks), dim3(threads), 0, g.stream, out, iters);
        else hipLaunchKernelGGL(mi_mfma_probe2_kernel<2>, dim3(blocks), dim3(threads), 0, g.stream, out, iters);
    }
    (void) hipEventRecord(g.ev[7], g.stream);
    (void) hipEventSynchronize(g.ev[7]);
    float ms = 0;
    (void) hipEventElapsedTime(&ms, g.ev[6], g.ev[7]);
    (void) hipFree(out);
    const double flops = (double) blocks * (threads / 64) * (double) iters * 16 * 2.0 * 16 * 16 * 4;
    return flops / (ms * 1e-3) / 1e12;
}

}  // extern "C"
