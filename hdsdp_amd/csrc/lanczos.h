// lanczos.h -- device-resident ratio test (see lanczos.hip)
#pragma once
#include <vector>
#include "hdm_common.h"
#include "lanczos_host.h"   // the rules (lanczos_rule.h), the host driver, the start vector
#include "small_ratio_rule.h"

struct HdmLanczos {
    int n = 0, n16 = 0;
    int nComputed = 0;        // calls so far: the second and later calls warm-start (hdsdp_lanczos.c:166-181)
    HdmBuf<double> V;         // n16 x (LZ_MD + 1) Lanczos basis
    HdmBuf<double> bv, b1, b2, bw, bz;   // n16 x 8 vector blocks (column 0 used)
    HdmBuf<double> warm, tmp, startd;   // startd: device copy of `start`, zero padded
    HdmBuf<double> part;      // LZ_NCHUNK x n16 partial sums of the plain matrix-vector product
    HdmBuf<double> LT;        // n16 x n16 transposed copy of Linv (large blocks, hdm_lanczos_group_kernel), made per test
    HdmBuf<unsigned> gsync;    // its grid barrier: counter, give-up word
    bool big_ok = true;        // no grid-wide wait of this object has run out
    int cus = 0;               // compute units of the device (0: not known), for hdm_lz_form
    unsigned sync_epoch = 0;   // barrier epochs handed out so far
    HdmPinned<double> scal_h;  // the mailbox (lanczos_rule.h: HdmLzMailbox) in mapped pinned memory: the kernels get dev()
    std::vector<double> start;   // the reference's pseudo-random start vector (host)

    int init(int n);
    int apply(const double *Linv, long ldl, const double *dS, long ldd, const double *in, double *out, hipStream_t s);
    // max step of  S + alpha dS >= 0  given Linv (S = L L^T) and the full symmetric dS; INFINITY if unbounded
    int solve(const double *Linv, long ldl, const double *dS, long ldd, hipStream_t s, double *maxStep, int *steps);
};

int hdm_mirror_lower(double *A, long ld, int n, hipStream_t s);
int hdm_sym_scale(double *A, long ld, int n, double diag_add, double scale, hipStream_t s);   // A <- scale*(sym(A) + diag_add*I)
int hdm_axpy_mat(double *out, const double *S, const double *dS, double step, long count, hipStream_t s);   // out = S + step*dS
int hdm_axpy_mat_eye(double *out, const double *S, const double *dS, double step, double eye, long ld, int n, hipStream_t s);   // out = S + step*dS + eye*I
#if defined(__HIPCC__)
// one element of out = S + step * dS: hdm_axpy_mat's kernel and the grouped safeguard (small.hip) share the expression
__device__ __forceinline__ double hdm_axpy_elem(double s, double d, double step) { return s + step * d; }
#endif

// ---- the grouped ratio test (small_ratio_rule.h has the rule, engine_ratio_set.h the set) -----------------
// One table entry per launched member, in mapped pinned memory.  Two launches work on the table, queued back to back:
// hdm_grouped_ratio_kernel (lanczos.hip) forms the member's step matrix and runs the one-launch Lanczos test's body on it,
// hdm_grouped_safeguard_kernel (small.hip) factors S + (1 - 1e-3) step dS and reports whether that succeeded.
struct HdmGroupedRatioArgs {
    int n, n16, m;                      // block dimension, its leading dimension, rows that enter the sum (0: every owned multiplier is zero)
    int fresh;                          // the member's Lanczos object has computed nothing yet: no warm start
    const double *A; long astride;      // m matrices in A_L form (strict lower + half diagonal), column-major n16 x n16
    const double *C;                    // objective, full symmetric, ld n16
    const double *y;                    // m multipliers (mapped host or device)
    double tau, eye;
    double *dS;                         // the member's step matrix, ld n16: both triangles of the leading n x n are written
    const double *S;                    // the member's dual matrix (lower triangle read), ld n16
    const double *Linv;                 // 128 x 128 triangular inverse of the dual factor (HdmChol::Dinv of a one-block factor)
    double *V, *warm;                   // HdmLanczos::V, ::warm
    const double *start;                // HdmLanczos::startd
    double *out;                        // mailbox + LZ_MB_WHOLE: [0] step [1] Lanczos steps [2] status [3] safeguard: 0, or first bad pivot + 1
};
int hdm_grouped_ratio(const HdmGroupedRatioArgs *table_host, const HdmGroupedRatioArgs *table_dev, int count, hipStream_t s);
int hdm_grouped_safeguard(const HdmGroupedRatioArgs *table_dev, int count, hipStream_t s);   // small.hip

// ---- the safeguard's rest in the grouped launch ------------------------------------------------------------
// A second table, indexed like the first (entry b goes with table[b]); the first table's struct, which the two kernels above copy,
// stays as it is.  Two more launches work on the pair, queued behind the two above; a workgroup whose member's safeguard word
// (table[b].out[3]) is 0 leaves at once.
// hdm_grouped_fresh_kernel (lanczos.hip) runs the one-launch Lanczos test's body from the fresh start vector on the member's
// lanczos_fresh object, with the Linv and dS of table[b]; hdm_grouped_cuts_kernel (small.hip) takes the smaller of the two steps
// and cuts it by 10 % until S + (1 - 1e-3) step dS factors (engine_cone.h: ratio_safeguard_rest, the same expressions in the same
// order).
struct HdmGroupedRestArgs {
    double *V, *warm;                   // the member's lanczos_fresh object: HdmLanczos::V, ::warm
    const double *start;                // its ::startd
    double *fresh_out;                  // its mailbox + LZ_MB_WHOLE: [0] step [1] Lanczos steps [2] status
    double *rest;                       // the rest's report words: [0] final step [1] a round succeeded (1 / 0; -1: nothing reported)
                                        // [2] cuts made [3] the fresh-start step (infinite where that test failed)
};
constexpr int HDM_GROUPED_REST_WORDS = 4;
int hdm_grouped_fresh(const HdmGroupedRatioArgs *table_host, const HdmGroupedRatioArgs *table_dev, const HdmGroupedRestArgs *rest_host,
                      const HdmGroupedRestArgs *rest_dev, int count, hipStream_t s);
int hdm_grouped_cuts(const HdmGroupedRatioArgs *table_dev, const HdmGroupedRestArgs *rest_dev, int count, hipStream_t s);   // small.hip
