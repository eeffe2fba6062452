// small.h -- the fused single-launch Phase-A pass for small rank-one blocks (small.hip)
#pragma once
#include "hdm_common.h"
#include "bsparse.h"
#include "grouped_plan.h"
#include "small_check_rule.h"

#define SMALL_P 128       // padded dimension: n, m <= 128
static_assert(SMALL_P == HDM_SMALL_CHECK_P, "small_check_rule.h states the sweep's padded dimension");
#define SMALL_SPMAX 8      // a rank-one factor with more entries than this is treated as dense
#define SMALL_NDENSE 4     // at most this many dense factors per block

struct HdmSmallArgs {
    int n, m;
    const double *C; long ldc;          // objective, full symmetric n x n (device)
    const int *fp, *fi;                 // rank-one factors as CSR over the m rows (a dense factor lists all n entries)
    const double *fv;
    const double *sgn;                  // m signs
    const int *dense_of;                // m: index into dense_rows, or -1
    int ndense;
    const int *dense_rows;              // ndense row indices (device)
    const double *y, *b;                // m multipliers, m right-hand side of the first solve (mapped host or device)
    double tau, eye, Rd;                // S = tau C - sum y_i A_i + eye I  (eye = -Rd + perturbation)
    double *Sout; long lds;             // the dual matrix, lower triangle (the cone's resident S)
    double *LS, *WS;                    // 128 x 128: Cholesky factor of S and its inverse (HdmChol::L, ::Dinv)
    double *M; long ldm;                // Schur matrix, lower triangle (device)
    double *LM, *WM;                    // 128 x 128: factor of M and its inverse
    double *out;                        // [0] info S, [1] info M, [2] logdet S, [3] tr S^-1, then ASinv, ASinvRdSinv, d1, d2, d3 (m each),
                                        // then 8 phase stamps (s_memrealtime, 100 MHz)
};

// One launch for an interior check of a small block (n <= 128, any device path): S = tau C - sum y_i A_i + eye I from the
// resident A_L-form constraint matrices (n16 x n16 each, n16 <= 128: skyline storage is a plain square there), the Cholesky
// factor with the triangular inverse, the pivot information and log det S.  What the call-by-call form does in seven
// operations and two synchronisations (pinned copy of y, assembly kernel, rectangle copy into the factor object, padding
// kernel, memset, sweep kernel, copy back): 88 us on a 100 x 100 block, 56 us on truss1's 21 x 21 ones, of which the
// reference's driver runs thousands.
struct HdmSmallCheckArgs {
    int n, n16, m;                      // block dimension, its leading dimension, constraint matrices resident
    const double *A; long astride;      // m matrices in A_L form (strict lower + half diagonal), column-major n16 x n16
    const double *C;                    // objective, full symmetric, ld n16
    const double *y;                    // m multipliers (mapped host or device)
    double tau, eye;
    double *Sout;                       // the dual matrix buffer (lower triangle written), ld n16
    double *L, *W;                      // 128 x 128: Cholesky factor and its inverse (HdmChol::L, ::Dinv)
    double *out;                        // [0] info (0, or first non-positive pivot + 1), [1] log det S
};
int hdm_small_check(const HdmSmallCheckArgs &args, hipStream_t s);
// The grouped form (hdm_grouped_check_kernel): ONE launch of `count` independent workgroups, workgroup b running the same body
// on table[b]; the dynamic LDS is sized for max_m, the largest m of the table.  The table is a mapped pinned block: the checks
// hdm_small_check makes on its argument are made on every entry through the host's address, the kernel reads the device's.
int hdm_grouped_check(const HdmSmallCheckArgs *table_host, const HdmSmallCheckArgs *table_dev, int count, int max_m, hipStream_t s);

// The grouped step-and-check (small_step_rule.h has the rule, engine_step_set.h the set): ONE launch of `count`
// independent workgroups.  Workgroup b writes table[b]'s checker buffer, Scheck = S + dStep dS over all n16 x n16 elements (what
// hdm_axpy_mat writes), factors it with the sweep HdmChol::factor runs on a one-block object, leaves L and Dinv as that path
// leaves them (L's strict upper triangle too: what the rectangle copy and the padding put there), and reports the sweep's info.
struct HdmGroupedStepArgs {
    int n, n16;                         // block dimension, leading dimension of S, dS, Scheck
    const double *S, *dS;               // the dual matrix and the step matrix, n16 x n16
    double dStep;
    double *Scheck;                     // n16 x n16, all of it written
    double *L, *Dinv;                   // 128 x 128 each: the checker factor object's HdmChol::L and ::Dinv
    int *info;                          // the report word (mapped host): preset to -1, "nothing reported"
};
int hdm_grouped_step_check(const HdmGroupedStepArgs *table_host, const HdmGroupedStepArgs *table_dev, int count, hipStream_t s);

size_t hdm_small_lds_bytes();
int hdm_small_phase_a(const HdmSmallArgs &args, hipStream_t s);

// ---- the grouped Schur build: every eligible small SDP block of an operator in three launches (grouped_plan.h has the rule and
// the plan, DESIGN.md section 17 the whole story) -------------------------------------------------------------------------
struct HdmGroupedConeDev {              // one grouped cone as the kernels see it
    int n, n16, mloc, pad;
    const double *W;                    // 128 x 128 triangular inverse of the dual factor (HdmChol::Dinv of a one-block factor)
    const double *A;                    // mloc matrices in A_L form, column-major n16 x n16 each
    const double *C;                    // objective, full symmetric, ld n16
    double Rd;
    long xoff, goff, voff;              // this cone's places in the three staging buffers (doubles)
};
struct HdmGroupedArgs {
    const HdmGroupedConeDev *cones; int ncones;
    const HdmGroupedJob *jobs; int njobs;
    int max_n16;                        // the largest n16 among the cones (sizes the jobs' LDS)
    int typeKKT;                        // KKT_TYPE_INFEASIBLE 0, _CORRECTOR 1, _HOMOGENEOUS 2
    double *X, *G, *V;                  // staging: S^-1 per cone; packed local lower Gram; ASinv, ASinvRdSinv, ASinvCSinv (mloc each) + 4 scalars
};
struct HdmGroupedScatterArgs {
    const HdmGroupedConeDev *cones; int ncones;
    long nM; const int *m_row, *m_col; const long *m_ptr; const int *m_slot, *m_idx;   // destinations of M and their contributors (CSR)
    int nV; const int *v_row; const long *v_ptr; const int *v_slot, *v_idx;           // rows of the m-vectors and theirs
    const double *G, *V;
    double *vecs; int m;                // the operator's accumulators: ASinv[m], ASinvRdSinv[m], ASinvCSinv[m], scal[4]
    int typeKKT;
};
size_t hdm_grouped_lds_bytes(int n16);
int hdm_grouped_inverses(const HdmGroupedArgs &a, hipStream_t s);                               // launch 1: one workgroup per cone
int hdm_grouped_jobs(const HdmGroupedArgs &a, hipStream_t s);                                   // launch 2: one workgroup per job
int hdm_grouped_scatter(const HdmGroupedScatterArgs &a, const HdmMatView &Mv, hipStream_t s);   // launch 3: one thread per destination
