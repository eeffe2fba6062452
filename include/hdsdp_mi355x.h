/* hdsdp_mi355x.h -- C ABI of the MI355X-native Schur-complement / Cholesky engine for HDSDP.
 *
 * Drop-in boundary: this library exports the reference's own operator surface for the hot path,
 *   HKKT*      (interface/hdsdp_schur.h:10-22)      -- Schur operator
 *   HFpLinsys* (linalg/hdsdp_linsolver.h:16-28)     -- dense factor / solve operator
 * with binary-compatible structs (hdsdp_kkt: interface/def_hdsdp_schur.h:32-68; hdsdp_linsys_fp:
 * linalg/def_hdsdp_linsolver.h:40-63; hdsdp_cone: interface/def_hdsdp_conic.h:56-107), so that
 * interface/hdsdp_algo.c keeps calling HKKTBuildUp / HKKTFactorize / HKKTSolve unchanged.
 * Return codes and error behaviour follow interface/hdsdp.h:42-48 and hdsdp_utils.h:32-45
 * ("not PSD" is a value, not an error: linalg/hdsdp_linsolver.c:1133-1140).
 *
 * The per-cone plug point is the reference's `coneBuildSchur` vtable slot
 * (def_hdsdp_conic.h:80-81, wired at interface/hdsdp_conic.c:140-141): HKKTBuildUp calls
 * cone->coneBuildSchur(cone->coneData, cone->iCone, kkt, typeKKT) exactly as
 * HConeBuildSchurComplement does (interface/hdsdp_conic.c:308-328).  HMiCone* below creates a cone
 * whose slot is the GPU builder (replacing sdpDenseConeGetKKT, hdsdp_conic_sdp.c:1726-1812).
 *
 * Plain C: pointers + sizes only.  All exported calls are synchronous on return for host-visible
 * outputs.  One solver instance per process/GPU (as the reference: single-threaded caller).
 */
#ifndef HDSDP_MI355X_H
#define HDSDP_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Everything declared in this header is the library's exported surface and nothing else is: the library is built with
 * -fvisibility=hidden, these declarations carry default visibility. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- interface/hdsdp.h:42-48 ---- */
typedef enum { HDSDP_RETCODE_OK, HDSDP_RETCODE_FAILED, HDSDP_RETCODE_MEMORY } hdsdp_retcode;

/* ---- interface/hdsdp_conic.h:16-19 ---- */
#define KKT_TYPE_INFEASIBLE  (0)
#define KKT_TYPE_CORRECTOR   (1)
#define KKT_TYPE_HOMOGENEOUS (2)
#define KKT_TYPE_PRIMAL      (3)

/* ---- interface/def_hdsdp_schur.h:26-30 ---- */
#define KKT_M1 (0)
#define KKT_M2 (1)
#define KKT_M3 (2)
#define KKT_M4 (3)
#define KKT_M5 (4)

/* ---- linalg/def_hdsdp_linsolver.h:26-38 ---- */
typedef enum {
    HDSDP_LINSYS_DENSE_DIRECT,
    HDSDP_LINSYS_SMALL_DIRECT,
    HDSDP_LINSYS_SPARSE_DIRECT,
    HDSDP_LINSYS_SPARSE_INDEFINITE,
    HDSDP_LINSYS_SPARSE_ITERATIVE,
    HDSDP_LINSYS_DENSE_ITERATIVE,
    HDSDP_LINSYS_DENSE_INDEFINITE
} linsys_type;

/* ---- linalg/def_hdsdp_linsolver.h:40-63 (field order is ABI) ---- */
typedef struct {
    int nCol;
    void *chol;
    linsys_type LinType;
    hdsdp_retcode (*cholCreate)(void **, int);
    void (*cholSetParam)(void *, void *);
    hdsdp_retcode (*cholSymbolic)(void *, int *, int *);
    hdsdp_retcode (*cholNumeric)(void *, int *, int *, double *);
    hdsdp_retcode (*cholPsdCheck)(void *, int *, int *, double *, int *);
    void (*cholFSolve)(void *, int, double *, double *);
    void (*cholBSolve)(void *, int, double *, double *);
    hdsdp_retcode (*cholSolve)(void *, int, double *, double *);
    hdsdp_retcode (*cholGetDiag)(void *, double *);
    void (*cholInvert)(void *, double *, double *);
    void (*cholDestroy)(void **);
    int nSolves;
    int nFactorizes;
} hdsdp_linsys_fp;

/* ---- interface/def_hdsdp_conic.h:21-31, :56-107 (field order is ABI) ---- */
typedef enum {
    HDSDP_CONETYPE_UNKNOWN,
    HDSDP_CONETYPE_LP,
    HDSDP_CONETYPE_BOUND,
    HDSDP_CONETYPE_SCALAR_BOUND,
    HDSDP_CONETYPE_DENSE_SDP,
    HDSDP_CONETYPE_SPARSE_SDP,
    HDSDP_CONETYPE_SOCP
} cone_type;

typedef struct {
    int iCone;
    cone_type cone;
    void *usrData;
    void *coneData;
    hdsdp_retcode (*coneCreate)(void **);
    hdsdp_retcode (*coneProcData)(void *, int, int, int *, int *, double *);
    hdsdp_retcode (*conePresolveData)(void *);
    void (*coneDestroyData)(void **);
    void (*coneSetStart)(void *, double);
    void (*coneUpdate)(void *, double, double *);
    hdsdp_retcode (*coneRatioTest)(void *, double, double *, double, int, double *);
    int64_t (*coneGetSymNnz)(void *);
    int (*coneGetDim)(void *);
    void (*coneAddSymNz)(void *, int, int *);
    void (*coneGetKKTMap)(void *, int, int *);
    hdsdp_retcode (*coneBuildSchur)(void *, int, void *, int);
    hdsdp_retcode (*coneBuildSchurFixed)(void *, int, void *, int, int);
    void (*coneBuildPrimalDirection)(void *, void *, double *, double *, int);
    hdsdp_retcode (*coneInteriorCheck)(void *, double, double *, int *);
    hdsdp_retcode (*coneInteriorCheckExpert)(void *, double, double, double *, double, int, int *);
    hdsdp_retcode (*coneGetBarrier)(void *, double, double *, int, double *);
    hdsdp_retcode (*coneAxpyBufferAndCheck)(void *, double, int, int *);
    void (*coneReduceResi)(void *, double);
    void (*coneSetPerturb)(void *, double);
    void (*conePRecover)(void *, double, double *, double *, double *, double *);
    void (*coneDRecover)(void *, double *, double *);
    void (*coneATimesXpy)(void *, double *, double *);
    double (*coneTraceCX)(void *, double *);
    double (*coneXDotS)(void *, double *);
    double (*coneGetCoeffNorm)(void *, int);
    double (*coneGetObjNorm)(void *, int);
    void (*coneScal)(void *, double);
    void (*coneView)(void *);
    void (*getstat)(void *, double *, int[20], double[20]);
} hdsdp_cone;

/* ---- interface/def_hdsdp_schur.h:32-68 (field order is ABI) ---- */
typedef struct {
    int nRow;
    int nCones;
    int maxConeDim;
    hdsdp_cone **cones;
    int isKKTSparse;
    hdsdp_linsys_fp *kktM;
    double *invBuffer;
    double *kktBuffer;
    double *kktBuffer2;
    int *kktMatBeg;
    int *kktMatIdx;
    double *kktMatElem;
    double **kktDiag;
    double *dASinvVec;
    double *dASinvCSinvVec;
    double *dASinvRdSinvVec;
    double dCSinvCSinv;
    double dCSinvRdSinv;
    double dCSinv;
    double dTraceSinv;
    double **dPrimalX;
} hdsdp_kkt;

/* =====================  Schur operator: interface/hdsdp_schur.h:10-22  ===================== */
hdsdp_retcode HKKTCreate(hdsdp_kkt **pHKKT);                                              /* hdsdp_schur.c:167 */
hdsdp_retcode HKKTInit(hdsdp_kkt *HKKT, int nRow, int nCones, hdsdp_cone **cones);        /* :181 */
hdsdp_retcode HKKTBuildUp(hdsdp_kkt *HKKT, int typeKKT);                                  /* :256 */
hdsdp_retcode HKKTBuildUpExtraCone(hdsdp_kkt *HKKT, hdsdp_cone *cone, int typeKKT);       /* :270 */
hdsdp_retcode HKKTBuildUpFixed(hdsdp_kkt *HKKT, int typeKKT, int kktStrategy);            /* :279 */
void HKKTExport(hdsdp_kkt *HKKT, double *dKKTASinvVec, double *dKKTASinvRdSinvVec, double *dKKTASinvCSinvVec,
                double *dCSinvCSinv, double *dCSinv, double *dCSinvRdCSinv, double *dTraceSinv); /* :293 */
hdsdp_retcode HKKTFactorize(hdsdp_kkt *HKKT);                                             /* :328 */
hdsdp_retcode HKKTSolve(hdsdp_kkt *HKKT, double *dRhsVec, double *dLhsVec);               /* :338 */
void HKKTRegularize(hdsdp_kkt *HKKT, double dKKTReg);                                     /* :348 */
void HKKTRegisterPSDP(hdsdp_kkt *HKKT, double **dPrimalScalX);                            /* :375 */
void HKKTClear(hdsdp_kkt *HKKT);                                                          /* :382 */
void HKKTDestroy(hdsdp_kkt **pHKKT);                                                      /* :408 */

/* ==================  linear-system operator: linalg/hdsdp_linsolver.h:16-28  ================
 * DENSE_DIRECT (the dual matrix S): blocked Cholesky on the device; "not positive definite" is a value of PsdCheck
 * and a failure of Numeric, as in lapackLinSolver* (hdsdp_linsolver.c:1082-1144).
 * SPARSE_DIRECT (a sparse dual matrix S; QDLDL in the reference, hdsdp_linsolver.c:509-809): Symbolic takes the lower-
 * triangular CSC pattern, Numeric / PsdCheck the values; the matrix is factored densely on the device.  Result-equivalent:
 * QDLDL's forward / backward solves carry the D^-1/2 scaling, GetDiag returns sqrt(D), Invert the full inverse.
 * DENSE_ITERATIVE (the Schur matrix M): the same direct Cholesky instead of the reference's PCG.  When M is not
 * numerically positive definite -- Numeric's factorisation fails, or Solve returns NaN -- the object switches itself to
 * DENSE_INDEFINITE like HFpLinsysSwitchToIndefinite (hdsdp_linsolver.c:1827-1857, called at :2034-2039 and :2098-2103)
 * and from then on factors with a pivoted device factorisation (csrc/lu.hip; same solutions as the reference's
 * dsytrf/dsytrs to rounding); LinType reads DENSE_INDEFINITE afterwards, PsdCheck / GetDiag fail and FSolve / BSolve /
 * Invert do nothing on such an object (:1729-1797). */
hdsdp_retcode HFpLinsysCreate(hdsdp_linsys_fp **pHLin, int nCol, linsys_type Ltype);      /* hdsdp_linsolver.c:1859 */
void HFpLinsysSetParam(hdsdp_linsys_fp *HLin, double relTol, double absTol, int nThreads, int maxIter,
                       int nRestartFreq);                                                 /* :2000 */
hdsdp_retcode HFpLinsysSymbolic(hdsdp_linsys_fp *HLin, int *colMatBeg, int *colMatIdx);   /* :2020 */
hdsdp_retcode HFpLinsysNumeric(hdsdp_linsys_fp *HLin, int *colMatBeg, int *colMatIdx, double *colMatElem); /* :2026 */
hdsdp_retcode HFpLinsysSwitchToBackUp(hdsdp_linsys_fp *HLin);                             /* :2047 */
hdsdp_retcode HFpLinsysPsdCheck(hdsdp_linsys_fp *HLin, int *colMatBeg, int *colMatIdx, double *colMatElem,
                                int *isPsd);                                              /* :2059 */
void HFpLinsysFSolve(hdsdp_linsys_fp *HLin, int nRhs, double *rhsVec, double *solVec);    /* :2065 */
void HFpLinsysBSolve(hdsdp_linsys_fp *HLin, int nRhs, double *rhsVec, double *solVec);    /* :2072 */
hdsdp_retcode HFpLinsysSolve(hdsdp_linsys_fp *HLin, int nRhs, double *rhsVec, double *solVec); /* :2079 */
hdsdp_retcode HFpLinsysGetDiag(hdsdp_linsys_fp *HLin, double *diagElem);                  /* :2113 */
void HFpLinsysInvert(hdsdp_linsys_fp *HLin, double *dFullMatrix, double *dAuxiMatrix);    /* :2119 */
void HFpLinsysClear(hdsdp_linsys_fp *HLin);                                               /* :2126 */
void HFpLinsysDestroy(hdsdp_linsys_fp **HLin);                                            /* :2138 */
/* The refined solve (csrc/refine_rule.h, csrc/refine.hip).  HFpLinsysSolve on a DENSE_DIRECT, SPARSE_DIRECT or
 * DENSE_ITERATIVE object (switched to the pivoted solver or not) then iterates on the true residual b - M x, formed on the
 * device in twice the working precision: solve, residual, and while the residual's 2-norm is not below
 *     tol = max(min(absTol, relTol |b|), 0.1 absTol)      (the reference's formula; HFpLinsysSetParam's values, 1e-6 where unset)
 * a correction solve with the same factor, x <- x + d, the new residual.  Off by default, and with it off nothing changes.
 * HMiLinsysSetRefine: maxSteps = 0 turns it off (and frees its device memory), anything above is the step cap, clamped to 8.
 * The residual needs the matrix the factor was made from: turn refinement on BEFORE HFpLinsysNumeric / HKKTFactorize.
 * HMiLinsysGetRefine: the last HFpLinsysSolve (its last right-hand side) and the running totals; returns the step cap (0: off).
 *   status   0 OFF  1 CONVERGED  2 STAGNATED (the residual did not halve: the iterate with the smaller residual went back)
 *            3 MAXSTEPS  4 NUMERICAL (a residual was not finite: the unrefined solution went back)  5 NO_MATRIX (the factorised
 *            matrix is not at hand -- refinement was off when it was factorised, or a later build has overwritten the device
 *            matrix: the solve ran unrefined)  6 NOT_AVAILABLE (the tile form of a sparse operator without its own switch, below: the solve ran unrefined)
 *   steps    corrections in the solution that went back;  resid0, resid: |b - M x|_2 before and after;  tol: as above
 *   solves, totalSteps: refined right-hand sides and correction solves since the object was created
 * Stopping short of tol is a status, not a failure: nothing switches solvers.  FSolve / BSolve are not refined.
 * HMiLinsysRefineBytes: device memory the refined solve holds for this object (0 while it is off).
 * HMiKKTSetRefine: the same switch on the operator's linear system (kktM).
 * The TILE form of a sparse operator (HMiKKTTileInfo) has a switch of its own on top of the cap: HMiLinsysSetRefineTiles /
 * HMiKKTSetRefineTiles(.., 1).  With the cap on and this switch off (the default) a tile operator answers NOT_AVAILABLE, solves
 * unrefined and holds no memory, as before; with both on BEFORE HKKTFactorize its solves are refined by the same loop, the
 * residual formed from the tile store (the accumulation store in place with the host mirror off -- valid until the next build
 * zeroes it, then NO_MATRIX -- or, with the mirror on, a device copy of the scattered factor store taken before the
 * factorisation).  Switching it off frees what it allocated (HMiLinsysRefineBytes counts it).  HMiLinsysGetRefineTiles: 1 on,
 * 0 off, -1 for a bad handle. */
int HMiLinsysSetRefine(hdsdp_linsys_fp *HLin, int maxSteps);
int HMiLinsysGetRefine(hdsdp_linsys_fp *HLin, int *status, int *steps, double *resid0, double *resid, double *tol, int64_t *solves,
                       int64_t *totalSteps);
int64_t HMiLinsysRefineBytes(hdsdp_linsys_fp *HLin);
int HMiKKTSetRefine(hdsdp_kkt *HKKT, int maxSteps);
int HMiLinsysSetRefineTiles(hdsdp_linsys_fp *HLin, int on);
int HMiLinsysGetRefineTiles(hdsdp_linsys_fp *HLin);
int HMiKKTSetRefineTiles(hdsdp_kkt *HKKT, int on);

/* ==========  MI355X SDP cone: the reference's cone slots that feed the Schur path  ==========
 * HMiConeCreateSDP    = HUserDataSetConeData + HConeCreate/SetData/ProcData/PresolveData for one
 *                       HDSDP_CONETYPE_DENSE_SDP block (tests/test_file_io.c:402-416): the CSC input is
 *                       the reference's user_data layout, shape n(n+1)/2 x (m+1), column 0 = C
 *                       (interface/def_hdsdp_user_data.h:16-32).  Coefficient data is uploaded to HBM once.
 * HMiConeCreateSynthetic builds the SURVEY.md 8(d) synthetic dense family directly in HBM (64-bit
 *                       offsets; the reference's int32 CSC cannot hold n=m=2000 fully dense).
 * rank/world shard the constraint rows (row i is owned by rank i % world); pass 0,1 for one GPU.
 * The remaining functions dispatch through the cone vtable like interface/hdsdp_conic.c:203-330.
 */
hdsdp_retcode HMiConeCreateSDP(hdsdp_cone **pCone, int iCone, int nRow, int nCol, const int *coneMatBeg,
                               const int *coneMatIdx, const double *coneMatElem, int rank, int world);
hdsdp_retcode HMiConeCreateSynthetic(hdsdp_cone **pCone, int iCone, int nCol, int nRow, int rank, int world);
/* 64-bit ingest (SURVEY finding 6, row f3).  The reference's user data is ONE CSC with `int` column pointers
 * (interface/def_hdsdp_user_data.h:22-32): a block whose columns hold more than 2^31 - 1 entries together -- fully dense
 * n = m = 2000 is 4.0e9 -- cannot be expressed in it.  Two ways in that can:
 *   HMiConeCreateSDP64   the same CSC with 64-bit column pointers (row indices stay `int`: a packed index is below
 *                        n(n+1)/2 < 2^31 for n <= 65535, the largest block dimension accepted);
 *   HMiConeBuilder*      column by column: Begin, then AddColumn once per non-zero column in any order (iCol 0 = the objective
 *                        C, iCol i = A_i; entries = packed lower index + value, any order, at most n(n+1)/2 of them), then
 *                        Finish, which returns the cone (columns never given are zero matrices).  A column is classified as it
 *                        arrives and the caller's arrays are not kept, so the caller may generate, hand over and free one
 *                        column at a time and never holds a 2^31-entry array; the library's own host copy goes back as soon as
 *                        the block's device layout is written (blocks on the congruence + Gram path).
 * Both give the device data HMiConeCreateSDP gives on the same entries (tests/test_gpu_ingest.py: bit-identical dual matrix and
 * Schur matrix on every CSC golden).  All three ways in refuse (RETCODE_FAILED) a column whose pointers run backwards, a packed
 * index outside [0, n(n+1)/2) and a packed index named twice in one column (tests/test_abi_cpu.py::
 * test_presolve_refuses_malformed_columns). */
hdsdp_retcode HMiConeCreateSDP64(hdsdp_cone **pCone, int iCone, int nRow, int nCol, const int64_t *coneMatBeg,
                                 const int *coneMatIdx, const double *coneMatElem, int rank, int world);
typedef struct HMiConeBuilder_s HMiConeBuilder;
hdsdp_retcode HMiConeBuilderBegin(HMiConeBuilder **pBuilder, int iCone, int nRow, int nCol, int rank, int world);
hdsdp_retcode HMiConeBuilderAddColumn(HMiConeBuilder *builder, int iCol, int64_t nnz, const int *packedIdx, const double *val);
int64_t HMiConeBuilderStored(const HMiConeBuilder *builder);          /* entries handed in so far */
hdsdp_retcode HMiConeBuilderFinish(HMiConeBuilder **pBuilder, hdsdp_cone **pCone);   /* frees the builder either way */
void HMiConeBuilderAbort(HMiConeBuilder **pBuilder);
/* ==========  LP cone: the SDPA diagonal block (interface/hdsdp_conic_lp.c)  ==========
 * HMiConeCreateLP      = HConeCreate/SetData/ProcData for one HDSDP_CONETYPE_LP block (LPConeProcDataImpl :101-160): the CSC
 *                        input has nCol rows (LP columns) and nRow + 1 columns, column 0 = the objective c (the layout of
 *                        HMiSDPAGetLPBlock and of the reference's reader, hdsdp_file_io.c:185-310).  The returned cone has
 *                        cone = HDSDP_CONETYPE_LP and the reference's slots, quirks included (HMiCone* above dispatch to them):
 *                        updates with dualPerturb on the non-step buffers (:46-83), a ratio test of 100 when no component
 *                        blocks (:223-259), primal recovery that prints "Recovery step is infeasible" and leaves the output
 *                        untouched when the recovery point is not interior (:466-487), ScalByConstant dividing (rscl, :205-209),
 *                        GetSymNnz = nRow^2 (the Schur matrix of an operator with an LP cone is dense), feature detection of
 *                        implied y bounds and free variables (:567-667).  Its coneBuildSchur slot (LPConeGetKKT, :266-348)
 *                        runs on the device: the vectors into the operator's device accumulators, M += A diag(d)^2 A^T into
 *                        the device matrix, d = 1/s (or the registered primal X for KKT_TYPE_PRIMAL).  So an operator of
 *                        engine SDP cones and LP cones counts no host cone and accepts HMiKKTSetHostMirror(0).  HKKTInit
 *                        refuses an operator holding an LP cone and a device-group cone (HMiSetDevices).  The SDP-only
 *                        accessors below (GetDualMatrix, GetTraces, GetPath, GetPresolve, SweepInfo, GetStreaming,
 *                        UseSweepCopy, GetBuildProfile, the exchange calls) fail or return their neutral value on an LP cone.
 * HMiConeLPSetSchurPath  how M is built: 0 = by the cost rule, 1 = dense (chunks of W = A diag(d) scattered on the
 *                        device, M += W W^T on the fp64 matrix pipe), 2 = sparse (a pair list made once at creation: one
 *                        fixed-order segmented sum per lower entry of M).  0 on success; 1 if the path cannot be set up (the
 *                        pair list would exceed 1 GiB) or the cone is not an LP cone.
 * HMiConeLPGetSchurPath  the path builds use (1 dense, 2 sparse; -1: not an LP cone), the two modelled build times in seconds
 *                        and the pair list's bytes. */
hdsdp_retcode HMiConeCreateLP(hdsdp_cone **pCone, int iCone, int nRow, int nCol, const int *coneMatBeg, const int *coneMatIdx,
                              const double *coneMatElem);
int HMiConeLPSetSchurPath(hdsdp_cone *cone, int path);
int HMiConeLPGetSchurPath(hdsdp_cone *cone, double *costDense, double *costSparse, int64_t *pairBytes);
void HMiConeDestroy(hdsdp_cone **pCone);
void HMiConeSetStart(hdsdp_cone *cone, double dConeStartVal);                   /* HConeSetStart  hdsdp_conic.c:222 */
void HMiConeUpdate(hdsdp_cone *cone, double barHsdTau, double *rowDual);        /* HConeUpdate    :228 */
hdsdp_retcode HMiConeCheckIsInterior(hdsdp_cone *cone, double barHsdTau, double *rowDual, int *isInterior);
hdsdp_retcode HMiConeGetLogBarrier(hdsdp_cone *cone, double barHsdTau, double *rowDual, int whichBuffer,
                                   double *logdet);
/* HConeRatioTest (hdsdp_conic.c:270; sdpDenseConeRatioTestImpl hdsdp_conic_sdp.c:1640-1686 + HLanczosSolve
 * linalg/hdsdp_lanczos.c:161-292) on the device: largest step with S + step * dS >= 0, where
 * dS = barHsdTauStep*C - sum rowDualStep_i A_i + dAdaRatio*Rd*I and S is the matrix of the chosen buffer: the current
 * dual matrix (BUFFER_DUALVAR, 0) or the trial point factored last in the checker (BUFFER_DUALCHECK, 1).  Also reachable
 * through the cone's coneRatioTest slot. */
hdsdp_retcode HMiConeRatioTest(hdsdp_cone *cone, double barHsdTauStep, double *rowDualStep, double dAdaRatio,
                               int whichBuffer, double *maxStep);
/* the rest of the dual line search, device resident (hdsdp_conic.c:350-387, :410-421; hdsdp_conic_sdp.c:2192-2241,
 * :2333-2361): an interior check of dCCoef*C + dACoefScal*sum dACoef_i A_i + dEyeCoef*I in either buffer, S + dStep*dS
 * with the dS of the last ratio test (in place for BUFFER_DUALVAR, into the checker for BUFFER_DUALCHECK), and the two
 * scalar setters.  HMiConeGetLogBarrier(whichBuffer = 1, rowDual = NULL) reads the checker's factor. */
hdsdp_retcode HMiConeCheckIsInteriorExpert(hdsdp_cone *cone, double dCCoef, double dACoefScal, double *dACoef, double dEyeCoef,
                                           int whichBuffer, int *isInterior);
hdsdp_retcode HMiConeAddStepToBufferAndCheck(hdsdp_cone *cone, double dStep, int whichBuffer, int *isInterior);
/* HConeDetectFeature (interface/hdsdp_conic.c:423-428): the cone's `getstat` slot -- class counts, "no primal interior", implied
 * trace bound, "very dense" as the reference's feature detection decides them (interface/hdsdp_conic_sdp.c:2651-2758), answered
 * from the engine's own presolve: a driver whose SDP blocks live here needs no CPU cone beside them.
 * Entries the cone does not decide are left as the caller set them. */
void HMiConeDetectFeature(hdsdp_cone *cone, double *rowRHS, int coneIntFeatures[20], double coneDblFeatures[20]);
void HMiConeReduceResi(hdsdp_cone *cone, double dResiReduction);
void HMiConeSetPerturb(hdsdp_cone *cone, double dDualPerturb);
/* the remaining HCone* utilities of a dense SDP block (hdsdp_conic.h:44-61; hdsdp_conic_sdp.c:1558-1614, :2470-2560):
 * data norms (whichNorm: ABS_NORM 1 = sum |a_ij|, FRO_NORM 2, over the full symmetric matrices; rows: sum resp. root of the
 * sum of squares over the constraints), scaling of the objective, and for a primal matrix X (host, n x n, symmetric)
 * y_i += <A_i, X>, <C, X>, <X, S>; HMiConeGetDual copies S (symmetrised) to the host. */
double HMiConeGetCoeffNorm(hdsdp_cone *cone, int whichNorm);
double HMiConeGetObjNorm(hdsdp_cone *cone, int whichNorm);
void HMiConeScalByConstant(hdsdp_cone *cone, double dScal);
void HMiConeComputeATimesXpy(hdsdp_cone *cone, double *dConePrimal, double *dATimesX);
double HMiConeComputeXDotS(hdsdp_cone *cone, double *dConePrimal);
double HMiConeComputeTraceCX(hdsdp_cone *cone, double *dConePrimal);
void HMiConeGetDual(hdsdp_cone *cone, double *dConeDual, double *dConeDual2);
/* HConeGetPrimal (hdsdp_conic.c:389; sdpDenseConeGetPrimal hdsdp_conic_sdp.c:2393-2446): primal recovery
 * X = mu * L^-T (sym(L^-1 dS L^-T) + I) L^-1 with S = C - sum rowDual_i A_i = L L^T and dS = sum rowDualStep_i A_i;
 * dConePrimal receives the n x n matrix (host, column-major), dConePrimal2 is unused scratch.  If S is not positive
 * definite a message is printed and dConePrimal is left untouched, like the reference.  Also the conePRecover slot. */
void HMiConeGetPrimal(hdsdp_cone *cone, double dBarrierMu, double *dRowDual, double *dRowDualStep, double *dConePrimal,
                      double *dConePrimal2);
/* the pseudo-random Lanczos start vector of the reference (HLanczosIPrepare, hdsdp_lanczos.c:33-42), host only */
void HMiLanczosStartVector(int n, double *v);
/* presolve results (classification hdsdp_sdpdata.c:2321-2458, ordering + plan hdsdp_conic_sdp.c:539-676);
 * each output may be NULL; arrays have nRow entries */
void HMiConeGetPresolve(hdsdp_cone *cone, int *coefType, int *coefRank, int *coefNnz, int *kktPerm,
                        int *kktStrategy, int *objType);
/* the same presolve without creating a cone (host only, touches no device): for CPU-side checks */
hdsdp_retcode HMiPresolveCSC(int nRow, int nCol, const int *coneMatBeg, const int *coneMatIdx,
                             const double *coneMatElem, int *coefType, int *coefRank, int *coefNnz, int *kktPerm,
                             int *kktStrategy, int *objType);
/* host copies of device state for parity checks: S (n x n, lower valid), b_i = tr(A_i) */
hdsdp_retcode HMiConeGetDualMatrix(hdsdp_cone *cone, double *S);
/* read-only observer for tests: the checker buffer (n16 x n16 doubles, n16 = n rounded up to 16, column-major) and the checker factor
 * object's L and Dinv (128 x 128 each) as the last step-and-check, expert check or primal recovery left them; any of the three may be
 * NULL.  Fails for a cone without a checker object yet, for n > 128, and for a cone that is not an SDP cone of the engine. */
hdsdp_retcode HMiConeGetChecker(hdsdp_cone *cone, double *Scheck, double *L, double *Dinv);
hdsdp_retcode HMiConeGetTraces(hdsdp_cone *cone, double *trA);
/* which device path the cone's builder uses: 0 = dense congruence + Gram (MFMA), 1 = rank-one */
int HMiConeGetPath(hdsdp_cone *cone);
/* Direct rows (csrc/direct_rows.h): on the congruence + Gram path of one device, rows of rank one and
 * triplet rows of at most *kmax entries are written into the transformed-row buffer in closed form, without the congruence;
 * the block's other non-zero rows are its congruence rows.  *nDirect such rows, *nRankOne of them rank one, *nCongruence others,
 * *kmax the entry limit in force.  All zero for a cone without the form (sharded, synthetic, streamed, forced path, below the size
 * floor, no eligible row, switched off) and for a group cone; HMiConeGetPath still answers 0 for a block with direct rows.
 * Each output may be NULL.  HDSDP_MI355X_DIRECT_ROWS in the table below. */
void HMiConeGetDirectRows(hdsdp_cone *cone, int *nDirect, int *nRankOne, int *nCongruence, int *kmax);
/* the zero-suppressed copy of the constraint data the S / dS sweeps read (csrc/schur.h: HdmZs): returns 1 and the number of
 * stored values / of skyline positions it stands for when the cone has built one, 0 when its sweeps read the dense storage */
int HMiConeSweepInfo(hdsdp_cone *cone, int64_t *values, int64_t *positions);
/* Streamed constraint data (synthetic family; csrc/row_store_rule.h): when the A_L forms of all owned rows do
 * not fit next to what a build needs -- BASELINE configs[4], n = 2000, m = 8000, on ONE device: 136 GB of them beside 130 GB of
 * transformed rows -- HMiConeCreateSynthetic keeps none of them: every consumer (congruence batches, S / dS sweeps without a
 * sweep copy, corrector dots, norms, A X) regenerates the rows it needs into a batch buffer from the counter-based generator,
 * same bits every time.  Returns 1 and the batch size in rows for such a cone, 0 for resident data.  HDSDP_MI355X_STREAM_A
 * forces either way. */
int HMiConeGetStreaming(hdsdp_cone *cone, int *batchRows);
/* on = 1: build the copy now whatever the block's size and fill, and sweep from it; on = 0: sweep from the dense storage
 * (a copy that exists is kept).  For tests and A/B runs; the default is the rule of HDSDP_MI355X_ZS in the table below. */
int HMiConeUseSweepCopy(hdsdp_cone *cone, int on);

/* ===============================  device-resident fast path  ===============================
 * The reference boundary hands host buffers (S in, M out).  For benchmarking with inputs resident in
 * HBM, these keep M on the device between BuildUp / Factorize / Solve (no PCIe round trip of M).  */
void HMiKKTSetHostMirror(hdsdp_kkt *HKKT, int mirrorM);   /* default 1: kktMatElem is refreshed after BuildUp; with 0
                                                              HKKTRegularize / Factorize / Solve act on the device copy */
/* The diagonal channel.  With the mirror off, kktDiag[i] points into a pinned m-vector instead of
 * kktMatElem: host cones handed to HKKTBuildUpExtraCone (the driver's bound cone on y) add their diagonal terms there.  A
 * build (not KKT_TYPE_CORRECTOR) zeroes it; the first HKKTRegularize or HKKTFactorize after the build uploads it (8 m bytes)
 * and adds it to the device matrix's diagonal, and HKKTRegularize takes its minimum over M_ii + channel_i, so the factor
 * input is (M_ii + channel_i) + reg, bit for bit the host mirror's.  Host cones that write M off the diagonal need the mirror.
 * HMiKKTGetDiagTarget: 0 = kktDiag points into kktMatElem (mirror on), 1 = into the channel, -1 = operator not initialised. */
int HMiKKTGetDiagTarget(hdsdp_kkt *HKKT);
/* bytes of M (and of the channel) moved between host and device since HKKTInit: the mirror's copy after a build, its upload
 * for a factorisation, the channel's uploads, rows read by HMiKKTGetRows.  The operator's vectors and scalars are not counted. */
void HMiKKTGetMatrixTraffic(hdsdp_kkt *HKKT, int64_t *bytesToHost, int64_t *bytesToDevice);
/* The grouped Schur build (csrc/grouped_plan.h, csrc/small.hip).  An SDP with many small blocks spends its
 * Schur builds on launch latency: the per-cone builders issue 4 to 16 launches per block.  With the switch on, every eligible
 * cone of the operator -- an engine SDP cone on one device, not synthetic, not streamed, constraint data resident, n <= 64 and
 * mloc * n16 * n16 <= 2^19 -- is built in ONE pass of three launches (inverses, row jobs, ordered scatter), whatever the number of
 * cones, provided at least two cones are eligible; every other cone goes through its own slot as before, and KKT_TYPE_PRIMAL builds
 * never group.  Off by default.  The cones' factor objects are read and left as they are.
 * HMiKKTSetGroupedBuild: after HKKTInit; returns the number of cones that will be grouped (0: off, or fewer than two eligible).
 * HMiKKTGetGroupedBuild: the last HKKTBuildUp / HKKTBuildUpFixed -- cones grouped, jobs (workgroups of the second launch), kernel
 * launches the grouped pass issued (the clean's memsets and the pull's copies are not counted); returns 1 if the pass ran, else 0.
 * HMiGroupedPlanQuery: the plan for an operator described by arrays; host arithmetic only, opens no context, works without a
 * device.  Cone k has dimension dims[k], owns the global rows rows[rowBeg[k] .. rowBeg[k + 1]) (its local order) and kindOk[k] says
 * whether it is a cone of the kind above (what only the engine can know); the dimension and data bounds are applied here.
 * counts (8): [0] grouped cones [1] jobs [2] destinations in M's lower triangle [3] their contributors [4] rows of the m-vectors
 * touched [5] their contributors [6] doubles of staging memory [7] eligible cones.  Every other output may be NULL; sized by a
 * first call: eligible, slotOf (nCones: 0 / 1; position among the grouped cones or -1), jobs (4 per job: slot, first row, end row,
 * 1 = the cone's first job, which also computes its scalars), the destinations of M (mRow >= mCol) with their contributors as a CSR
 * (mPtr: [2] + 1 entries; mSlot, mIdx: slot and index into the cone's local lower Gram, packed by columns) and the same for the
 * vectors' rows (vIdx: the cone's local row).  Contributors of a destination are listed in ascending cone order: that is the order
 * the scatter sums them in.  Returns 8, or -1 for a bad argument. */
int HMiKKTSetGroupedBuild(hdsdp_kkt *HKKT, int on);
int HMiKKTGetGroupedBuild(hdsdp_kkt *HKKT, int *cones, int *jobs, int *launches);
int HMiGroupedPlanQuery(int nRow, int nCones, const int *dims, const int *kindOk, const int *rowBeg, const int *rows, int64_t *counts,
                        int *eligible, int *slotOf, int *jobs, int *mRow, int *mCol, int64_t *mPtr, int *mSlot, int *mIdx, int *vRow,
                        int64_t *vPtr, int *vSlot, int *vIdx);
/* The grouped interior check (csrc/small_check_rule.h, csrc/small.hip, csrc/engine_check_set.h).  The
 * reference's line search puts every point question -- "interior at (tau, y)?", "log det S at (tau, y)" -- to all cones in a loop
 * with the same arguments; a small SDP cone answers each in one launch and one synchronisation of its own.  With the switch on,
 * the first such question put to a member of the operator's check set at a new point puts EVERY member there in one launch
 * (one workgroup per member, the one-launch check's own body: the same bits), and the loop's later calls are answered from the
 * members' state with no device work.  Members: the engine SDP cones of cones[] on one device whose own one-launch check would run
 * (n <= 128, constraint data resident, mloc * n16 * n16 <= 2^19 for n16 <= 64 and <= 2^17 above), not held by another operator's
 * active set.  Only the dual buffer's point questions group: the expert form, the checker buffer, step-and-check and the ratio test
 * stay on their own paths.  One difference from the loop: a question put to one member moves every member's dual buffer and dual
 * factor to that point, also those behind a cone at which the loop breaks.  Off by default.
 * HMiKKTSetGroupedCheck: after HKKTInit; returns the number of members (0: off, or fewer than two members).
 * HMiKKTGetGroupedCheck: out[0] members [1] grouped launches since HKKTInit [2] cones in the last launch [3] cones launched in all
 * [4] per-cone calls answered from state since the switch went on [5] members left out of the last launch because they already
 * stood at the point; returns 1 if the switch is on, else 0.
 * HMiKKTCheckIsInterior: the whole-operator question.  Every cone of cones[] in order, without early exit, through its own
 * coneInteriorCheck and (where interior) coneGetBarrier slots: flags[k], logdets[k] (NaN where flags[k] == 0) and *all (1 if every
 * cone is interior); any of the three may be NULL.  With the switch off it is the plain loop; with it on the members are
 * answered by one launch.  Returns the first retcode of a slot that was not OK. */
int HMiKKTSetGroupedCheck(hdsdp_kkt *HKKT, int on);
int HMiKKTGetGroupedCheck(hdsdp_kkt *HKKT, long out[6]);
hdsdp_retcode HMiKKTCheckIsInterior(hdsdp_kkt *HKKT, double tau, const double *y, int *flags, double *logdets, int *all);
/* The grouped ratio test (csrc/small_ratio_rule.h, csrc/lanczos.hip, csrc/small.hip,
 * csrc/engine_ratio_set.h).  The reference's line search puts "how far along (dTauStep, dy)?" to all cones in a loop with the same
 * arguments; a small SDP cone answers in five launches and two or three synchronisations of its own.  With the switch on, a
 * question on BUFFER_DUALVAR that a member's slot does not hold runs EVERY member's test in one pair of launches and one
 * synchronisation (one workgroup per member: the per-cone sweep's sums, the one-launch Lanczos test's own body, the safeguard's
 * factorisation: the same bits), and the loop's later calls fetch their answers from the members' slots, each exactly once and only
 * while the member's dual matrix, step matrix and factor have not moved.  Members: the check set's population (above) with n >= 2
 * whose Lanczos form is the LDS-resident one-launch test (HDM_LANCZOS_WHOLE not 0) and with mloc <= n16 (n16 + 1).  The checker
 * buffer, n = 1 and larger blocks keep their own paths.  One difference from the loop: a question put to one member runs every
 * member's test -- a member that is never asked that question has its warm-start state one test further and its step matrix
 * overwritten.  Off by default.
 * HMiKKTSetGroupedRatio: after HKKTInit; returns the number of members (0: off, or fewer than two members).
 * HMiKKTGetGroupedRatio: out[0] members [1] grouped launch pairs since HKKTInit [2] cones in the last one [3] cones launched in all
 * [4] answers served from slots since the switch went on [5] members left out of the last launch (dual factor not in place, or an
 * unfetched answer to the same question) [6] safeguard fallbacks (steps that left the cone and took the host's fresh-start test);
 * returns 1 if the switch is on, else 0.
 * HMiKKTRatioTest: the whole-operator question.  Every cone of cones[] in order, without early exit, through its own coneRatioTest
 * slot: steps[k] (NaN where the slot failed; may be NULL) and *minStep, the smallest step of the cones that answered (infinite if
 * none bounds it; may be NULL).  With the switch off it is the plain loop.  Returns the first retcode of a slot that was not OK. */
int HMiKKTSetGroupedRatio(hdsdp_kkt *HKKT, int on);
int HMiKKTGetGroupedRatio(hdsdp_kkt *HKKT, long out[7]);
hdsdp_retcode HMiKKTRatioTest(hdsdp_kkt *HKKT, double dTauStep, const double *dy, double dAdaRatio, int whichBuffer, double *steps,
                              double *minStep);
/* Two opt-ins of the grouped ratio test, each off by default and acting only while HMiKKTSetGroupedRatio is
 * on; switching, releasing or re-initialising the ratio set turns both off again.
 * HMiKKTSetGroupedRatioChecker: the set also answers a question on BUFFER_DUALCHECK -- the same two launches, reading the checker
 * buffer and the checker's factor.  A member whose checker object is missing or of another shape takes its own path; one whose
 * checker holds no factorisation is left out and its own call fails, as it does per cone.  A checker answer is served once, to the
 * same question on the same buffer, while neither the checker (buffer or factor) nor the member's step matrix has been written.
 * HMiKKTSetGroupedRatioRest: where a member's step leaves the cone, the rest of the safeguard -- the fresh-start Lanczos test and
 * the 10 % cuts -- runs in two more launches behind the same synchronisation instead of on the host for that member alone; the
 * step is the host's, bit for bit.  Turning it on makes each member's fresh-start Lanczos object.
 * Both return the number of members when the opt-in is on afterwards, else 0.
 * HMiKKTGetGroupedRatioDetail: out[0] the checker opt-in (1 / 0) [1] the rest opt-in [2] grouped launches that asked the checker,
 * since HKKTInit [3] members given the rest on the device [4] cuts made on the device [5] host fallbacks (HMiKKTGetGroupedRatio's
 * [6]); returns 1 if the grouped ratio test is on, else 0. */
int HMiKKTSetGroupedRatioChecker(hdsdp_kkt *HKKT, int on);
int HMiKKTSetGroupedRatioRest(hdsdp_kkt *HKKT, int on);
int HMiKKTGetGroupedRatioDetail(hdsdp_kkt *HKKT, long out[6]);
/* The grouped step-and-check (csrc/small_step_rule.h, csrc/small.hip, csrc/engine_step_set.h).  Between the
 * ratio test and the barrier the reference's line search asks every cone "is S + dStep dS still inside?" on BUFFER_DUALCHECK, and
 * again with a smaller step until all are; a small SDP cone answers in five launches and one synchronisation of its own.  With the
 * switch on, a step on BUFFER_DUALCHECK that a member's slot does not hold puts EVERY member's checker buffer and checker factor at
 * that step in one launch and one synchronisation (one workgroup per member, the per-cone path's sums and its diagonal-block sweep:
 * the same bits), and the loop's later calls answer from the members' slots -- any number of times, while dStep is exactly the
 * same and nothing has been written to the member's S, dS, checker buffer or checker factor.  Members: the check set's population
 * (above) whose checker object is one 128-block too, with HDM_DIAG_SWEEP not 0; n = 1 is a member.  BUFFER_DUALVAR, the ratio test
 * on the checker and larger blocks keep their own paths.  One difference from the loop: a step put to one member moves every
 * member's checker there, also those behind a cone at which the loop breaks.  Turning the switch on makes each member's checker
 * object and step buffer; a member that has had no ratio test yet has no step matrix: it is left out and its own call fails, as it
 * does per cone.  Off by default.
 * HMiKKTSetGroupedStep: after HKKTInit; returns the number of members (0: off, or fewer than two members).
 * HMiKKTGetGroupedStep: out[0] members [1] grouped launches since HKKTInit [2] cones in the last launch [3] cones launched in all
 * [4] answers served from slots since the switch went on [5] members left out of the last launch (no step matrix, or a slot that
 * serves this step already); returns 1 if the switch is on, else 0.
 * HMiKKTAddStepToBufferAndCheck: the whole-operator question.  Every cone of cones[] in order, without early exit, through its own
 * coneAxpyBufferAndCheck slot: flags[k] (0 where the slot failed; may be NULL) and *allInterior (1 if every cone is inside; may be
 * NULL).  With the switch off it is the plain loop.  Returns the first retcode of a slot that was not OK. */
int HMiKKTSetGroupedStep(hdsdp_kkt *HKKT, int on);
int HMiKKTGetGroupedStep(hdsdp_kkt *HKKT, long out[6]);
hdsdp_retcode HMiKKTAddStepToBufferAndCheck(hdsdp_kkt *HKKT, double dStep, int whichBuffer, int *flags, int *allInterior);
/* multi-GPU (world > 1): constraint rows are sharded (row i on rank i % world).  Each rank congruence-
 * transforms its own rows, a transpose (all-to-all) re-shards the transformed data from "by constraint"
 * to "by packed-index range", each rank forms the Gram partial sum over its range, and an all-reduce
 * (sum) assembles the augmented Gram matrix on every rank.  The two collectives are supplied by the host
 * program (torch.distributed over RCCL in hdsdp_amd/dist.py); both are called with the engine stream
 * idle and must return with the data in place.
 *   alltoall(ctx): send chunk r of the send buffer to rank r, receive chunk r of the recv buffer from rank r
 *   allreduce(ctx, buf, count): in-place sum of `count` doubles at device pointer `buf` over all ranks */
typedef int (*hmi_alltoall_fn)(void *ctx);
typedef int (*hmi_allreduce_fn)(void *ctx, void *buf, int64_t count);
void HMiConeSetExchange(hdsdp_cone *cone, hmi_alltoall_fn a2a, hmi_allreduce_fn ar, void *ctx);
/* optional: the all-to-all in `npieces` pieces along the packed index, so that the Gram product over a piece's index
 * range runs while the later pieces are still in flight.  start(ctx, offset, count, piece): begin exchanging the `count`
 * doubles at `offset` of EVERY chunk (send chunk r -> rank r, into recv chunk <source rank> at the same offset), may
 * return before the data has arrived; wait(ctx, piece): return once that piece is in place.  Pieces are started in
 * order 0..npieces-1 and waited for in that order.  start(.., piece) is called once the send ranges of that piece are
 * final; the engine stream may still be computing the ranges of LATER pieces (the congruence's second step runs by
 * packed-index range in piece order, so the exchange also overlaps the congruence; HDSDP_MI355X_STAGED_A2A=0 restores
 * "congruence complete, stream idle, then exchange"), so start() must only touch the ranges it is given. */
typedef int (*hmi_alltoall_piece_fn)(void *ctx, int64_t offset, int64_t count, int piece);
typedef int (*hmi_alltoall_wait_fn)(void *ctx, int piece);
void HMiConeSetExchangePieces(hdsdp_cone *cone, hmi_alltoall_piece_fn start, hmi_alltoall_wait_fn wait, int npieces);
/* HConeBuildPrimalXSXDirection (interface/hdsdp_conic.c:335-338; the cone's coneBuildPrimalDirection slot, used by the primal
 * refinement hdsdp_psdp.c:236,295): XSX += X^T D X, D = the resident dual matrix (iDualMat != 0) or the dual step of the last
 * ratio test; X and XSX are n x n column-major host matrices */
void HMiConeBuildPrimalXSXDirection(hdsdp_cone *cone, double *dPrimalScalMatrix, double *dPrimalXSXBuffer, int iDualMat);
/* what the last HKKTBuildUp did: pieces of the exchange (1 = one blocking all-to-all) and, when the congruence's second
 * step was staged by packed-index range, the number of launches it was cut into (0 = not staged) */
void HMiConeGetExchangeStats(hdsdp_cone *cone, int *pieces, int *stagedLaunches);
/* the last KKT_TYPE_PRIMAL build of the cone (for a group cone: shard 0's): returns its route -- 0 = X positive definite, Cholesky
 * factor and congruence + Gram path; 1 = X indefinite, the signed factor X = W^T diag(sigma) W passed its acceptance test and the
 * congruence + Gram path ran with the signed Gram correction; 2 = neither, the row-by-row fallback (one device) or a refusal
 * (sharded block) -- with *negativePivots = q, the number of negative pivots of the signed factor, and *growth = |W|_F^2 / |X|_F
 * (both 0 when no signed factor was formed: route 0, route 2 after a zero pivot or with HDSDP_MI355X_PRIMAL_SIGNED=0).
 * -1: not an SDP cone of the engine, or no KKT_TYPE_PRIMAL build yet. */
int HMiConeGetPrimalRoute(hdsdp_cone *cone, int *negativePivots, double *growth);
/* where the last route-1 KKT_TYPE_PRIMAL build (shard 0 of a group cone) spent the time of its signed part, in ms: ms[0] signed
 * factor + acceptance test (host clock, includes the upload of X), ms[1] gathers of the correction's packed columns, ms[2] the
 * correction's Gram launches, ms[3] the final combination into the Gram matrix; *columns = packed columns gathered.  1 if the
 * last KKT_TYPE_PRIMAL build was not on route 1. */
int HMiConeGetPrimalProfile(hdsdp_cone *cone, double *ms, int64_t *columns);
/* Where the last SHARDED Schur build (world > 1) of one shard spent its time, so that a multi-GPU bench line says where a step went
 * and not only how long it took (the cone loop being sharded: interface/hdsdp_schur.c:256-268).  `shard`: index inside an in-process
 * device group (0 for a process-per-GPU cone).  Milliseconds; device times are differences of HIP events on the shard's engine stream,
 * host times wall clock around the two blocking hooks.  Layout of `out` (8 + 6 * pieces doubles):
 *   [0] pieces of the exchange   [1] 1 = congruence step 2 ran by packed-index range (staged)   [2] triangular inverse of the factor
 *   [3] congruence step 1 (staged) or both congruence steps (not staged)   [4] slab reduction   [5] all-reduce of the Gram matrix (host)
 *   [6] extraction into M and the vectors   [7] world
 *   then per piece k:  [8+6k] step 2 of the tile columns piece k needs   [+1] engine stream idle before piece k's Gram splits (the
 *   piece had not arrived: the exchange WAIT)   [+2] host time inside the wait hook   [+3] Gram splits of piece k   [+4] bytes this shard
 *   sent for piece k   [+5] host time from handing piece k to the transport until its wait returned
 * Returns the doubles written, 0 when no sharded build has run, -(doubles needed) when `cap` is too small, -1 for a bad shard. */
int HMiConeGetBuildProfile(hdsdp_cone *cone, int shard, double *out, int cap);
/* exchange buffers (device pointers, `world` chunks of *chunkCount doubles each); the caller may instead
 * supply its own (e.g. torch-allocated) buffers before the first HKKTBuildUp: world * chunkCount doubles of payload
 * plus 8192 doubles of slack behind it (the Gram kernel stages whole 128-row tiles without a row mask) */
hdsdp_retcode HMiConeGetExchangeBuffers(hdsdp_cone *cone, void **sendBuf, void **recvBuf, int64_t *chunkCount);
hdsdp_retcode HMiConeSetExchangeBuffers(hdsdp_cone *cone, void *sendBuf, void *recvBuf);
void *HMiKKTDeviceMatrix(hdsdp_kkt *HKKT, int64_t *ld);   /* device pointer of M (m x m, lower valid) */
/* nRows full symmetric rows of the device copy of M after a build (out: nRows x m doubles, row by row): what a caller that
 * keeps M on the device (host mirror off, m = 8000: 512 MB) needs for a row-subset check against tests/golden/full8000_rows.npz */
hdsdp_retcode HMiKKTGetRows(hdsdp_kkt *HKKT, int nRows, const int *rows, double *out);

/* ======================  several GPUs behind the C ABI (one process, one caller thread)  ======================
 * The reference's driver is a single-threaded process (tests/sdpasolve.c; interface/hdsdp_algo.c:1082-1101 calls
 * HKKTBuildUp / Factorize / Solve in sequence), so for it the sharding has to happen below these calls.
 * HMiSetDevices(n, ids), or HDSDP_MI355X_GPUS=n in the environment of an UNCHANGED driver (devices 0..n-1), configures a
 * device group before the first cone is created.  From then on HMiConeCreateSDP / HMiConeCreateSynthetic (called with
 * rank 0, world 1) return a GROUP CONE for every dense block of dimension >= HMiSetShardMinDim (default 512, env
 * HDSDP_MI355X_SHARD_MIN_N) that takes the congruence + Gram path: its constraint rows are dealt cyclically over n shards,
 * one per device, each with its own stream and host worker thread; every cone slot fans out to the shards, the all-to-all
 * and the all-reduce of the sharded build run over RCCL inside the library (grouped ncclSend/ncclRecv per piece of the
 * exchange, ncclAllReduce), and only shard 0 writes into the caller's Schur operator, which lives on ids[0].  Blocks on
 * the rank-one / sparse paths and small blocks stay plain single-device cones on ids[0].
 * Device ids may repeat (HDSDP_MI355X_LOOPBACK=1 with the environment form: shard r on device r mod visible): the
 * shards then share a device and exchange by device-to-device copies -- a rehearsal of world = n on a 1-GPU box; the same
 * copy transport can be forced between distinct, peer-accessible devices with HDSDP_MI355X_TRANSPORT=copy.
 * The process-per-GPU mode above (HMiConeSetExchange*, torchrun) is unaffected.  All return 0 on success. */
int HMiSetDevices(int nDevices, const int *deviceIds);
/* the same with the transport stated by the caller: 0 = device copies (peer access), 1 = RCCL (one device per shard; with
 * shared devices the group falls back to copies and HMiGetDeviceGroup says so), -1 = HDSDP_MI355X_TRANSPORT, else copies.
 * tests/test_gpu_group.py::test_config5_at_size_on_eight_devices asks for each in turn; bench.py --gpus N asks for RCCL once
 * HMiRcclGroupSelfTest has passed over the same devices in a child process. */
int HMiSetDevicesEx(int nDevices, const int *deviceIds, int transport);
int HMiGetDeviceGroup(int *deviceIds, int maxIds, int *transport);   /* returns the shard count (1 = no group); transport
                                                                        0 = device copies, 1 = RCCL, -1 = none */
void HMiSetShardMinDim(int nMin);
int HMiConeGetShardCount(hdsdp_cone *cone);                          /* 1 for a plain cone */
void HMiConeGetGroupTraffic(hdsdp_cone *cone, int64_t *bytesAllToAll, int64_t *bytesAllReduce);   /* sent by shard 0 so far */
/* One launch for a whole Phase-A pass of a SMALL rank-one block (BASELINE configs 2-3; csrc/small.hip).  The sequence
 *     HConeCheckIsInterior(tau, y) -> HKKTBuildUp(KKT_TYPE_INFEASIBLE) -> HKKTFactorize -> HKKTSolve x 3
 * (interface/hdsdp_algo.c:1082-1101: right-hand sides rhs, ASinv, ASinvRdSinv) is forty launches and six host
 * synchronisations on the call-by-call path, which is what a 100 x 100 block costs there, not its arithmetic.  For an
 * operator with ONE engine cone whose constraints are all rank one (n, m <= 128, at most 4 dense factors) this entry does
 * the whole sequence in one single-workgroup kernel and one synchronisation, with the same results: *isInterior and the
 * log-determinant of S, the operator's dASinvVec / dASinvRdSinvVec / dTraceSinv (and kktMatElem with the host mirror on),
 * the three solutions; the Cholesky factors of S and M are left in the objects HFpLinsys* / HKKTSolve use, so any later call
 * on the same state works as after the separate calls.  HMiKKTPhaseAEligible says whether the operator qualifies; the call
 * itself returns HDSDP_RETCODE_FAILED if not (nothing has been touched then).  The reference's call sites stay as they are:
 * this is an additional entry for drivers that want the latency, used by bench.py's small-config lines. */
int HMiKKTPhaseAEligible(hdsdp_kkt *HKKT);
hdsdp_retcode HMiKKTPhaseA(hdsdp_kkt *HKKT, double barHsdTau, double *rowDual, double *rhs, double *d1, double *d2, double *d3,
                           int *isInterior, double *logdet);
/* wall time the caller's thread has spent below this C ABI, by category (outermost entry only, so the categories add up):
 * [0] HKKTBuildUp of the M-forming types, [1] HKKTBuildUp(KKT_TYPE_CORRECTOR), [2] HKKTFactorize, [3] HKKTSolve,
 * [4] cone slots that assemble and factor S (update, interior checks, barrier, line search), [5] ratio test, [6] primal
 * recovery and the cone utilities, [7] HFpLinsys* called directly (the reference's CPU cones).  Returns the number of
 * categories.  HDSDP_MI355X_CALL_STATS=1 in the environment prints the table on stderr when the process exits. */
int HMiGetCallStats(double *seconds, int64_t *calls, int n);
const char *HMiCallStatName(int k);
void HMiResetCallStats(void);
/* how the requests for a dual or step matrix of single-device blocks were answered so far (csrc/dual_state.h: hdm_dual_plan):
 * [0] the buffer already held the point, [1] a copy of S, [2] S + alpha dS (+ delta I) on the last ratio test's line, [3] a
 * sweep for a dual matrix off that line, [4] a refresh sweep after 16 in-place updates, [5] a step-matrix sweep, [6] a sweep of a
 * block that does not track points.  Process-wide, never reset (the table HDSDP_MI355X_CALL_STATS=1 prints at exit).  Fills up
 * to n entries; returns the number of counters. */
int HMiGetAssembleCounts(int64_t *counts, int n);
int HMiRcclSelfTest(int device);   /* one-rank communicator on `device` (-1: the engine's): all-reduce + grouped send/recv, checked */
/* the same over a whole group of distinct devices, one host thread per device as the group's workers drive it: communicators,
 * an all-reduce, and the grouped ncclSend/ncclRecv of one piece of the sharded build's exchange, values compared bit for bit;
 * every wait is bounded by timeoutMs (<= 0: 60 s) and a rank that fails aborts its communicator so that no peer blocks.
 * 0 = passed, else the first failing stage (csrc/group_impl.h: rccl_group_self_test).  Touches no engine state. */
int HMiRcclGroupSelfTest(int nDevices, const int *deviceIds, int timeoutMs);

/* ================================  ingest (host only)  ================================
 * SDPA sparse format reader with the reference's semantics (interface/hdsdp_file_io.c:34-381): one CSC per
 * SDP block, shape n(n+1)/2 x (m+1), column 0 = C = -F0; rhs = the c vector.  Pointers stay valid until
 * HMiSDPAFree. */
typedef struct HMiSDPA_s HMiSDPA;
hdsdp_retcode HMiReadSDPA(const char *fname, HMiSDPA **out);
void HMiSDPAGetDims(const HMiSDPA *p, int *nConstrs, int *nBlks, int *nLpCols);
hdsdp_retcode HMiSDPAGetBlock(const HMiSDPA *p, int iBlk, int *dim, const int **beg, const int **idx,
                              const double **val);
/* the same with the 64-bit column pointers the reader keeps (a block may hold more than 2^31 - 1 entries; HMiSDPAGetBlock
 * refuses such a block): feeds HMiConeCreateSDP64 */
hdsdp_retcode HMiSDPAGetBlock64(const HMiSDPA *p, int iBlk, int *dim, const int64_t **beg, const int **idx,
                                const double **val);
/* the LP (diagonal) block, hdsdp_file_io.c:185-310: CSC of nCol rows and m + 1 columns, column 0 = the objective (-F0's
 * entries), entries in file order inside a column; RETCODE_FAILED if the file has no LP block.  Feeds HMiConeCreateLP. */
hdsdp_retcode HMiSDPAGetLPBlock(const HMiSDPA *p, int *nCol, const int **beg, const int **idx, const double **val);
const double *HMiSDPAGetRHS(const HMiSDPA *p);
void HMiSDPAFree(HMiSDPA **pp);


/* =====================================  environment switches  =====================================
 * Every environment variable the shipped library reads.  The table is held to the one list the library reads them through,
 * csrc/env_switches.h -- which also states how each text is parsed and when it is read -- by tests/test_abi_cpu.py and
 * tests/test_env_switches_cpu.py, both ways, on name and default.
 * "other position" tests: tests/test_gpu_switches.py runs every device path under the non-default setting in a child
 * process and compares with the default run.  A -DHDM_DIAGNOSTICS build (python -m hdsdp_amd.build --diagnostics) reads
 * three more -- HDM_VAR, HDM_CONG2_DIRECT, HDM_DBG_SYNC -- for stamped kernels and timing ablations; the product never does.
 *
 *  variable                       default   meaning                                                      covered by
 *  -- configuration ---------------------------------------------------------------------------------------------------
 *  LOCAL_RANK                     0         device of the caller's context (process-per-GPU mode)         test_gpu_dist.py
 *  HDSDP_MI355X_GPUS              1         shards of the in-process device group (unchanged driver)      test_gpu_group.py::test_unchanged_driver_shards_by_environment
 *  HDSDP_MI355X_LOOPBACK          0         shards may share devices (rehearsal)                          same
 *  HDSDP_MI355X_SHARD_MIN_N       512       smallest block dimension that is sharded                      same
 *  HDSDP_MI355X_TRANSPORT         copy      device group transport when the caller states none            test_gpu_group.py::test_config5_at_size_on_eight_devices[rccl|copy]
 *                                           (HMiSetDevices, HDSDP_MI355X_GPUS): copy | rccl                (needs 8 devices), test_transport_request_is_honoured
 *  HDSDP_MI355X_A2A_PIECES        8         pieces of the sharded build's exchange                        test_gpu_switches.py
 *  HDSDP_MI355X_STAGED_A2A        1         step 2 by packed-index range, pieces leave as they finish     test_gpu_switches.py
 *  HDSDP_MI355X_FORCE_GEMM        0         every block takes the congruence + Gram path                  test_gpu_switches.py, test_gpu_parity.py
 *  HDSDP_MI355X_FORCE_PATH        -         force device path 0 / 1 / 2 (tests)                           test_gpu_parity.py::test_every_device_path_gives_the_same_numbers
 *  HDSDP_MI355X_SPARSE_KKT        1         0: always the dense Schur matrix                              test_gpu_switches.py
 *  HDSDP_MI355X_KKT_ENVELOPE      1         block-envelope factorisation of a sparse operator             test_gpu_switches.py
 *  HDSDP_MI355X_KKT_RCM           1         reverse Cuthill-McKee order of a sparse operator              test_gpu_switches.py
 *  HDSDP_MI355X_KKT_TILES         1         tile form of a sparse operator when it pays (bsparse.h)       test_gpu_switches.py
 *  HDSDP_MI355X_AFFINE_S          by cost   0 / 1 / 2: dual matrix short-cuts (dual_state.h)              test_gpu_switches.py
 *  HDSDP_MI355X_SMALL_CHECK       1         one-launch interior check of small blocks                     test_gpu_switches.py
 *  HDSDP_MI355X_ZS                by cost   0 / 1 / 2: zero-suppressed copy for the S / dS sweeps (schur.h) test_gpu_switches.py
 *  HDSDP_MI355X_PRIMAL_SIGNED     1         KKT_TYPE_PRIMAL with an indefinite X: signed factor + signed  test_gpu_primal_signed.py
 *                                           Gram correction (route 1); 0: row-by-row fallback / refusal
 *  HDSDP_MI355X_DIRECT_ROWS       by size   rank-one and short triplet rows of a congruence + Gram block   test_gpu_direct_rows.py
 *                                           built without the congruence (direct_rows.h); 0: off; k > 0: on
 *                                           whatever the size, up to k entries per row.  Read at cone creation
 *  HDSDP_MI355X_STREAM_A          by memory 0 / 1: synthetic constraint data resident / regenerated per     test_gpu_streamed.py
 *                                           batch
 *  HDSDP_MI355X_DEVICE_M          0         1: HKKTInit turns the host mirror of M off when no cone of    test_gpu_device_m.py
 *                                           cones[] is a host cone (diagonal channel); else one stderr line
 *  HDSDP_MI355X_GROUPED_BUILD     0         1: HKKTInit turns the grouped Schur build on (all eligible    test_gpu_grouped_build.py
 *                                           small SDP cones of an operator in three launches)
 *  HDSDP_MI355X_GROUPED_CHECK     0         1: HKKTInit turns the grouped interior check on (a point      test_gpu_grouped_check.py
 *                                           question to one small SDP cone answers all in one launch)
 *  HDSDP_MI355X_GROUPED_RATIO     0         1: HKKTInit turns the grouped ratio test on (a ratio test     test_gpu_grouped_ratio.py
 *                                           asked of one small SDP cone runs all in one launch pair)
 *  HDSDP_MI355X_GRATIO_CHECKER    0         1: with HDSDP_MI355X_GROUPED_RATIO=1, HKKTInit lets the ratio test_gpu_grouped_ratio_checker.py
 *                                           set answer BUFFER_DUALCHECK too (HMiKKTSetGroupedRatioChecker)
 *  HDSDP_MI355X_GRATIO_REST       0         1: with HDSDP_MI355X_GROUPED_RATIO=1, the safeguard's fresh-   test_gpu_grouped_ratio_checker.py
 *                                           start test and cuts run in the launch (HMiKKTSetGroupedRatioRest)
 *  HDSDP_MI355X_GROUPED_STEP      0         1: HKKTInit turns the grouped step-and-check on (a step asked test_gpu_grouped_step.py
 *                                           of one small SDP cone's checker puts all there in one launch)
 *  HDSDP_MI355X_REFINE            0         k > 0: HKKTInit turns the refined Schur solve on, at most k   test_gpu_refine.py::test_the_environment_switch_turns_refinement_on
 *                                           steps (HMiKKTSetRefine)
 *  HDSDP_MI355X_REFINE_TILES      0         1: HKKTInit turns the tile form's refined solve on as well    test_gpu_refine_tiles.py::test_the_environment_switches_refine_a_tile_operator
 *                                           (HMiKKTSetRefineTiles; needs HDSDP_MI355X_REFINE=k too)
 *  -- the next six are the work plan's knobs: all read in csrc/work_plan.h (hdm_knobs_from_env), per allocation; HMiWorkPlanQuery sees them too --
 *  HDM_TCAP_GIB                   32        GiB of congruence intermediates per launch group              test_gpu_switches.py, test_gpu_group.py
 *  HDM_BC                         1024      constraints per congruence launch (upper bound)               test_gpu_switches.py
 *  HDM_NSPLIT                     by size   slabs of the Gram product's K splits                          test_gpu_switches.py
 *  HDM_GRAM_KSTAGES               by size   stages (16 k) per (split, tile) job of the Gram product on one    test_gpu_switches.py (with HDM_NSPLIT=8: more
 *                                           device; more splits than slabs run in groups (gram_all)           splits than slabs)
 *  HDM_GRAM_QUEUE                 1         Gram jobs from ONE queue in split order; 0: one queue per XCD      test_gpu_switches.py
 *  HDM_SHARE_T_SLABS              1         intermediates and Gram slabs share one buffer (one GPU)       test_gpu_switches.py
 *  HDSDP_MI355X_HOST_THREADS      min(16,   host threads of the ingest (presolve per column, staging of the    test_gpu_switches.py; the threaded form: test_gpu_ingest.py (syn2000x32)
 *                                 cores)    upload)
 *  -- fallbacks kept reachable (the default is the fast form) ----------------------------------------------------------
 *  HDM_PERSIST                    1         persistent GEMM workgroups; 0: one workgroup per tile         test_gpu_switches.py, test_gpu_kernels.py
 *  HDM_PERSIST_RESERVE_CUS        0 / 8     CUs a persistent launch leaves to the collectives             test_gpu_switches.py, test_gpu_kernels.py
 *  HDM_DIAG_SWEEP                 1         register-sweep diagonal block; 0: LDS-panel kernel            test_gpu_switches.py, test_gpu_kernels.py
 *  HDM_CHOL_K128                  1         Cholesky panel / update as 64-row tiles straight from global  test_gpu_switches.py, test_gpu_kernels.py
 *                                           memory; 0: the general GEMM kernel
 *  HDM_TRSV_FLOW                  1         single-launch substitution; 0: per-block launches             test_gpu_switches.py, test_gpu_kernels.py
 *  HDM_TRSV_FLOW_FAIL_ONCE        0         test hook: throw the first single-launch result away          test_gpu_kernels.py::test_fallback_chains_of_the_factor_and_solve_kernels
 *  HDM_SYM_COMBINE_SKY            1         S assembly in storage order; 0: element-indexed kernel        test_gpu_switches.py
 *  HDM_LANCZOS_WHOLE              1         small blocks: whole ratio test in one launch                  test_gpu_switches.py
 *  HDM_LANCZOS_FUSED              1         small blocks: three Lanczos steps per launch                  test_gpu_switches.py
 *  HDM_LANCZOS_GROUP              1         large blocks: steps between Ritz checks queued back to back   test_gpu_switches.py
 *  HDM_LANCZOS_BIG                1         large blocks: those steps in one launch of co-resident groups test_gpu_switches.py
 *  HDSDP_MI355X_PRELOAD           1         code objects are loaded on a helper thread when the first    test_gpu_switches.py
 *                                           context opens; 0: each on its first launch
 *  -- output only (no code path changes) --------------------------------------------------------------------------------
 *  HDSDP_MI355X_CALL_STATS        0         table of wall time below the C ABI at exit                    tools/small_driver_stats.sh
 *  HDSDP_MI355X_TRACE             0         synchronise and report after every entry                      (diagnostic)
 *  HDSDP_MI355X_RATIO_DEBUG       0         one line per ratio test: Lanczos steps, time                  (diagnostic)
 *  HDSDP_MI355X_AFFINE_DEBUG      0         one line per dual-matrix request that missed the last ratio    (diagnostic)
 *                                           test's line (dual_state.h: hdm_dual_print_miss)
 *  HDM_POISON                     0         new device memory is filled with 0xFF (NaN): a read of         (diagnostic; tools/poison_run.sh)
 *                                           never-written memory turns the results into NaNs
 */

/* ==================================  utilities  ================================== */
int HMiDeviceInit(int device);         /* hipSetDevice + stream; returns 0 on success */
int HMiDeviceSynchronize(void);
void *HMiStream(void);                 /* hipStream_t all kernels are launched on */
const char *HMiVersion(void);
/* timing of the last HKKTBuildUp / HKKTFactorize / HKKTSolve stages measured with HIP events on the
 * engine stream, milliseconds: [0] factor inverse, [1] congruence, [2] gram, [3] reduce+extract,
 * [4] gram kernel launches, [5] congruence kernel launches */
void HMiGetStageTimes(double *ms, int n);

/* The work plan of a dense block's Schur build on the congruence + Gram path (csrc/work_plan.h): constraints per congruence launch,
 * K splits and slabs of the Gram product, buffer sizes.
 * HMiWorkPlanQuery: what the engine would plan in THIS process (its HDM_* knobs as the environment states them now) for rank `rank`
 * of `world` on a block of dimension n with m constraints, all rows resident and none dropped as zero.  Host arithmetic only: opens no
 * context, touches no device, works without one.  out (cap >= 17): [0] n16 [1] nblk [2] npb [3] npb_loc [4] Lr [5] R [6] elements per
 * constraint matrix (skyline) [7] rows owned [8] Bc [9] K splits [10] slabs [11] intermediates and slabs share one buffer [12] one Gram
 * job queue [13] bytes of the intermediates T [14] of the slabs [15] of the exchange buffers [16] of the Gram matrix (payloads; the
 * operand slack behind a buffer is not counted; with [11] set the one buffer has the larger of [13] and [14]).  Returns 17, or -17
 * for a bad argument.
 * HMiConeGetWorkPlan: what a cone HOLDS after its first build allocated the work space (for a group cone: shard 0's) -- the plan above
 * unless device memory was short and an allocation was halved.  out (cap >= 7): [0] Bc [1] K splits [2] slabs [3] shared buffer
 * [4] one Gram job queue [5] bytes of T (of the shared buffer, with [3]) [6] bytes of the slabs.  Returns 7, 0 before the first build
 * (or for a cone on another path), -1 if `cone` is not an SDP cone of the engine. */
int HMiWorkPlanQuery(int n, int m, int world, int rank, int64_t *out, int cap);
int HMiConeGetWorkPlan(hdsdp_cone *cone, int64_t *out, int cap);

/* live per-kernel timing with HIP events on the engine stream (for bench.py's roofline block): roles are
 * [0] helper GEMMs (Cholesky/TRTRI), [1] congruence step 1 (T = Linv A), [2] congruence step 2 without its full diagonal
 * tiles, [3] Gram, [4] the full diagonal tiles of congruence step 2 (a kernel of their own: P + P^T from one product).
 * Each array has 5 entries: total ms, algorithmic flops and launch count since the last call. */
void HMiSetKernelTiming(int on);
int HMiGetKernelTiming(double *ms, double *flops, int64_t *launches);
/* the same with a fourth array: the flops the launches' MFMA instructions EXECUTED (2048 per v_mfma_f64_16x16x4_f64), counted on the
 * host from the tile lists and the kernels' stage sequences -- issued / algorithmic is the granularity loss of a role (sub-blocks that
 * straddle a diagonal, live ranges of triangular K blocks, padding rows); bench.py: roofline.issued_over_valid */
int HMiGetKernelTimingEx(double *ms, double *flops, double *issued, int64_t *launches);
/* diagnostic builds (HDM_VAR=32): per-workgroup s_memtime stamps of launches with the given role, 8 words each */
void HMiSetDebugBuffer(void *dev, int role);

/* raw kernels (device pointers) exported for unit tests and micro-benchmarks */
int HMiGemmNT(const double *A, int64_t lda, int aKMajor, const double *B, int64_t ldb, int bKMajor, double *C,
              int64_t ldc, int M, int N, int K, double alpha, double beta, int kLimit, int lowerOnly);
/* The call forms of a dense block's Schur build (csrc/gemm_calls.h: hdm_cong_step1, hdm_cong_step2, hdm_cong_irow, hdm_gram_splits,
 * hdm_gram_gathered, hdm_gram_lp), ONE launch each on the caller's device buffers, for tests/test_gpu_gemm_roles.py.  (n, world,
 * maxloc) name the block's layout as csrc/work_plan.h: hdm_layout takes them.  Every buffer comes with the number of doubles it
 * holds: an entry returns 1 and launches nothing when an operand buffer is smaller than the span its form vouches for, or the
 * destination smaller than what the form writes (T: nb n16^2; a blocked destination: npb Lr 16; slabs: nz R^2; the LP matrix:
 * (m16 - 1) ldm + m16), or a row range leaves its buffer.  Returns 0 after the launch has completed.
 * HMiGemmRoleLayout (host only): out (cap >= 7) = [0] n16 [1] nblk [2] npb [3] npb_loc [4] Lr [5] R [6] elements per skyline matrix;
 * returns 7, or -7 for a bad argument.
 * HMiGemmRoleSpan (host only): the doubles a form vouches for: which = 0 the intermediates T of a0 matrices, 1 the factor inverse
 * of leading dimension a0, 2 a buffer of a0 skyline matrices, 3 an exchange buffer, 4 the LP cone's dense buffer (kc = a0,
 * mpad = a1); -1 for a bad argument. */
int HMiGemmRoleLayout(int n, int world, int maxloc, int64_t *out, int cap);
int64_t HMiGemmRoleSpan(int which, int n, int world, int maxloc, int64_t a0, int64_t a1);
int HMiCongStep1(int n, int world, int maxloc, const double *Linv, int64_t linv_len, int64_t ldl, const double *Asrc, int64_t asrc_len,
                 int64_t src_rows, int64_t b0, int nb, double *T, int64_t t_len);
int HMiCongStep2(int n, int world, int maxloc, int64_t Bc, const double *Linv, int64_t linv_len, int64_t ldl, const double *T, int64_t t_len,
                 int nb, double *dst, int64_t dst_len, int64_t blk_row0, uint64_t colmask);
int HMiCongIRow(int n, int world, int maxloc, const double *Linv, int64_t linv_len, int64_t ldl, double *dst, int64_t dst_len, int64_t blk_row0);
int HMiGramSplits(int n, int world, int maxloc, int m, int64_t nsplit, int z0, int nz, const double *Ahat, int64_t ahat_len, double *slab,
                  int64_t slab_len, int accumulate, int queue_global);
int HMiGramGathered(int64_t R, int64_t nc, int nz, double alpha, int accumulate, const double *gat, int64_t gat_len, double *slabs,
                    int64_t slabs_len, int queue_global);
int HMiGramLp(int m, int mpad, int kc, int kv, const double *W, int64_t w_len, double *M, int64_t m_len, int64_t ldm);
int HMiPotrf(double *A_dev, int n, int64_t lda, int *info);  /* in place, lower */
/* blocked Cholesky + one solve of a host matrix (lower triangle, column-major, ld = n) with a block envelope: first[i] = first
   128-block column with an entry in block row i, NULL = dense; L_host (n x n) receives the factor if not NULL */
int HMiCholEnvelopeSolve(const double *A_host, int n, const int *first, const double *b, double *x, double *L_host, int *info);
/* host only: the reverse Cuthill-McKee order HKKTInit considers for a sparse Schur pattern (lower-triangular CSC in, perm[old] = new out) */
int HMiRcmOrder(int m, const int *colBeg, const int *rowIdx, int *perm);
/* how the operator's matrix will be factored: *permuted = 1 if the factor object holds P M P' (reverse Cuthill-McKee order of the
   sparse pattern), *fraction = 128-blocks inside the pattern's block envelope / blocks of the dense lower triangle */
void HMiKKTEnvelopeInfo(hdsdp_kkt *HKKT, int *permuted, double *fraction);
/* A sparse Schur operator whose factor's block pattern fills at most half of the triangle is kept in TILE form on the device
   (csrc/bsparse.h): rows reordered (dense rows last, reverse Cuthill-McKee for the rest), matrix and factor stored as the
   128 x 128 tiles inside the block pattern of the Cholesky factor only, factored left-looking by levels of the block elimination
   tree -- the device counterpart of the reference's sparse direct solver behind the aggregated-pattern CSC operator
   (interface/hdsdp_schur.c:46-139, linalg/hdsdp_linsolver.c:509-809).  Returns 1 and fills the outputs when HKKT is in that
   form: tiles stored, tiles of the dense lower triangle, levels, bytes of device memory of the tile stores. */
int HMiKKTTileInfo(hdsdp_kkt *HKKT, int *tiles, int64_t *denseTiles, int *levels, int64_t *bytes);
/* The tile-form factorisation is an LDL' WITHOUT pivoting in signed-Cholesky form, M = L~ S L~' with S = diag(+-1) -- what the
   reference's sparse direct solver does (external/qdldl.c; linalg/hdsdp_linsolver.c:596-626): an indefinite matrix factors and
   solves, only an exactly zero pivot fails HKKTFactorize, and a positive definite matrix gets its Cholesky factor bit for bit.
   Negative pivots of the operator's last factorisation (= negative eigenvalues of M, by inertia); -1 if HKKT is not in tile form
   or not factored. */
int HMiKKTNegativePivots(hdsdp_kkt *HKKT);
/* the tile-form factorisation and solve on a host matrix (lower-triangular CSC, diagonal entry first in every column):
   *info = 0 or first zero pivot + 1; stats[0..3] = block rows, tiles stored, levels, negative pivots; ms (may be NULL) =
   factorisation time, best of three */
int HMiBspSolve(int m, const int *colBeg, const int *rowIdx, const double *val, const double *b, double *x, int *info, int *stats,
                double *ms);
/* host only (no device call): the symbolic phase of that factorisation on a lower-triangular CSC pattern.  perm[old] = new;
   stats[0..4] = block rows, tiles of the factor, levels, rows sent to the dense tail, update source pairs; blockPtr (block rows
   + 1 entries) and blockRow (one per tile) = the factor's block pattern by block column, diagonal first.  Every output may be
   NULL; a first call with blockPtr = blockRow = NULL sizes them through stats.  Returns 1 where HKKTInit would not take the tile
   form (fewer than two block rows, or more tiles than maxFraction of the dense triangle's). */
int HMiBspSymbolic(int m, const int *colBeg, const int *rowIdx, double maxFraction, int *perm, int *stats, int *blockPtr, int *blockRow);
/* the refined solve's residual kernel on host arrays: r = b - M x and |r|_2^2, every component accumulated in twice the working
   precision and rounded once.  Mlower: ld x n column-major, lower triangle valid; it is uploaded exactly as given and nothing above
   the diagonal or in rows >= n is read.  Deterministic: two calls give the same bits. */
int HMiSymResidualProbe(int n, const double *Mlower, long ld, const double *x, const double *b, double *r, double *norm2);
/* the tile form's residual kernel on a host matrix (lower-triangular CSC, diagonal entry first in every column; the pattern must
   take the tile form: m > 128): r = b - M x and |r|_2^2 in twice the working precision, vectors in the caller's order.  The
   padding rows and columns of the tile store and its spare tile are filled with NaN first: nothing of them may be read. */
int HMiTileResidualProbe(int m, const int *colBeg, const int *rowIdx, const double *val, const double *x, const double *b, double *r,
                         double *norm2);
/* HMiBspSolve's factorisation followed by the production refined solve of the tile form (at most maxSteps corrections, tolerances
   as HFpLinsysSetParam takes them).  *info = 0 or first zero pivot + 1 (then nothing is solved); status, steps, resid0, resid, tol
   as HMiLinsysGetRefine; stats[0..3] = block rows, tiles stored, levels, negative pivots.  Every output but x may be NULL. */
int HMiBspRefinedSolve(int m, const int *colBeg, const int *rowIdx, const double *val, const double *b, double *x, int maxSteps, double relTol,
                       double absTol, int *info, int *status, int *steps, double *resid0, double *resid, double *tol, int *stats);
/* what that refined solve costs beside the unrefined one: ONE factorisation, then nVariants variants alternate solve by solve for
   warmup + reps rounds, host clock around each solve (each ends in a stream synchronisation).  caps[v] < 0: the unrefined solve
   (HMiBspSolve's); otherwise the refined solve with that step cap under relTols[v] / absTols[v].  ms[v * reps + r] milliseconds;
   corrections[v] = correction solves over the timed rounds; status[v], resid[2 v] = |r_0| and resid[2 v + 1] = |r| of the last
   solve; stats as HMiBspSolve; *workBytes = device memory the refined solve allocated.  Outputs after ms may be NULL. */
int HMiBspRefineTimingProbe(int m, const int *colBeg, const int *rowIdx, const double *val, const double *b, int nVariants, const int *caps,
                            const double *relTols, const double *absTols, int warmup, int reps, double *ms, int *corrections, int *status,
                            double *resid, int *stats, int64_t *workBytes);
int HMiCholEnvelopeProbe(int n, int band, int reps, double *ms_dense, double *ms_env);   /* factorisation time of a block-banded matrix, dense vs on its envelope */
double HMiDiagBlockProbe(int variant, int reps);   /* us per 128 x 128 diagonal-block kernel of the Cholesky (0: LDS panels, 1: register sweep) */
double HMiMfmaPeakProbe(int iters);    /* measured fp64 MFMA TFLOP/s of a register-only loop */
/* GEMM-shaped issue probe: mode 0 = 16 accumulators x (4+4) operand registers, 1 = one operand pair */
double HMiMfmaIssueProbe(int mode, int wgPerCu, int iters);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* HDSDP_MI355X_H */
