// lanczos.h -- device-resident ratio test (see lanczos.hip)
#pragma once
#include <vector>
#include "hdm_common.h"
#include "lanczos_host.h"   // the rules (lanczos_rule.h), the host driver, the start vector

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
