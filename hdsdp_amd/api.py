"""Host-side mirror of the reference operator interface for the Schur path, over the C ABI.

Names, argument meaning and error behaviour follow the reference (interface/hdsdp_schur.h:10-22,
linalg/hdsdp_linsolver.h:16-28, interface/hdsdp_conic.h:27-61): `KKT.build_up(type)` is
HKKTBuildUp, `KKT.factorize()` HKKTFactorize, `KKT.solve(rhs)` HKKTSolve, ... A non-OK
`hdsdp_retcode` raises `HDSDPError` (the reference's `goto exit_cleanup`).

There is NO CPU fallback: importing works without a GPU (symbol checks), any compute call needs
the HIP extension and an MI355X.
"""
import ctypes as C
import os
import sys

import numpy as np

KKT_TYPE_INFEASIBLE, KKT_TYPE_CORRECTOR, KKT_TYPE_HOMOGENEOUS, KKT_TYPE_PRIMAL = 0, 1, 2, 3
KKT_M1, KKT_M2, KKT_M3, KKT_M4, KKT_M5 = 0, 1, 2, 3, 4
HDSDP_LINSYS_DENSE_DIRECT, HDSDP_LINSYS_SPARSE_DIRECT, HDSDP_LINSYS_DENSE_ITERATIVE, HDSDP_LINSYS_DENSE_INDEFINITE = 0, 2, 5, 6
RETCODE_OK, RETCODE_FAILED, RETCODE_MEMORY = 0, 1, 2
BUFFER_DUALVAR, BUFFER_DUALCHECK, BUFFER_DUALSTEP = 0, 1, 2   # interface/hdsdp_conic.h:24-26

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HDSDP_MI355X_LIB") or os.path.join(_PKG, "libhdsdp_mi355x.so")   # override: same-box A/B of two builds

# every symbol include/hdsdp_mi355x.h declares
EXPORTS = [
    "HKKTCreate", "HKKTInit", "HKKTBuildUp", "HKKTBuildUpExtraCone", "HKKTBuildUpFixed", "HKKTExport",
    "HKKTFactorize", "HKKTSolve", "HKKTRegularize", "HKKTRegisterPSDP", "HKKTClear", "HKKTDestroy",
    "HFpLinsysCreate", "HFpLinsysSetParam", "HFpLinsysSymbolic", "HFpLinsysNumeric", "HFpLinsysSwitchToBackUp",
    "HFpLinsysPsdCheck", "HFpLinsysFSolve", "HFpLinsysBSolve", "HFpLinsysSolve", "HFpLinsysGetDiag",
    "HFpLinsysInvert", "HFpLinsysClear", "HFpLinsysDestroy",
    "HMiConeCreateSDP", "HMiConeCreateSDP64", "HMiConeCreateLP", "HMiConeLPSetSchurPath", "HMiConeLPGetSchurPath", "HMiConeBuilderBegin", "HMiConeBuilderAddColumn", "HMiConeBuilderStored", "HMiConeBuilderFinish", "HMiConeBuilderAbort", "HMiConeCreateSynthetic", "HMiConeDestroy", "HMiConeSetStart", "HMiConeUpdate",
    "HMiConeCheckIsInterior", "HMiConeGetLogBarrier", "HMiConeRatioTest", "HMiLanczosStartVector", "HMiConeGetPrimal", "HMiConeCheckIsInteriorExpert",
    "HMiConeAddStepToBufferAndCheck", "HMiConeReduceResi", "HMiConeSetPerturb", "HMiConeGetCoeffNorm", "HMiConeGetObjNorm",
    "HMiConeScalByConstant", "HMiConeComputeATimesXpy", "HMiConeComputeXDotS", "HMiConeComputeTraceCX", "HMiConeGetDual", "HMiConeGetPresolve", "HMiConeDetectFeature", "HMiConeGetDualMatrix",
    "HMiConeGetTraces", "HMiConeGetPath", "HMiConeGetDirectRows", "HMiConeSweepInfo", "HMiConeGetStreaming", "HMiConeUseSweepCopy", "HMiKKTSetHostMirror", "HMiConeSetExchange", "HMiConeSetExchangePieces", "HMiConeGetExchangeStats", "HMiConeGetPrimalRoute", "HMiConeGetPrimalProfile", "HMiConeGetBuildProfile", "HMiConeBuildPrimalXSXDirection",
    "HMiConeGetExchangeBuffers", "HMiConeSetExchangeBuffers", "HMiKKTDeviceMatrix", "HMiKKTGetRows", "HMiKKTGetDiagTarget", "HMiKKTGetMatrixTraffic", "HMiDeviceInit",
    "HMiSetDevices", "HMiSetDevicesEx", "HMiRcclGroupSelfTest", "HMiGetDeviceGroup", "HMiSetShardMinDim", "HMiConeGetShardCount", "HMiConeGetGroupTraffic", "HMiRcclSelfTest", "HMiGetCallStats", "HMiCallStatName", "HMiResetCallStats", "HMiGetAssembleCounts", "HMiKKTPhaseAEligible", "HMiKKTPhaseA",
    "HMiDeviceSynchronize", "HMiStream", "HMiVersion", "HMiGetStageTimes", "HMiGemmNT", "HMiPotrf",
    "HMiMfmaPeakProbe", "HMiDiagBlockProbe", "HMiCholEnvelopeSolve", "HMiCholEnvelopeProbe", "HMiKKTEnvelopeInfo", "HMiKKTTileInfo", "HMiKKTNegativePivots", "HMiBspSolve", "HMiBspSymbolic", "HMiRcmOrder", "HMiSetKernelTiming", "HMiGetKernelTiming", "HMiGetKernelTimingEx", "HMiPresolveCSC", "HMiMfmaIssueProbe", "HMiSetDebugBuffer",
    "HMiGemmRoleLayout", "HMiGemmRoleSpan", "HMiCongStep1", "HMiCongStep2", "HMiCongIRow", "HMiGramSplits", "HMiGramGathered", "HMiGramLp",
    "HMiWorkPlanQuery", "HMiConeGetWorkPlan", "HMiKKTSetGroupedBuild", "HMiKKTGetGroupedBuild", "HMiGroupedPlanQuery",
    "HMiKKTSetGroupedCheck", "HMiKKTGetGroupedCheck", "HMiKKTCheckIsInterior",
    "HMiKKTSetGroupedRatio", "HMiKKTGetGroupedRatio", "HMiKKTRatioTest",
    "HMiKKTSetGroupedRatioChecker", "HMiKKTSetGroupedRatioRest", "HMiKKTGetGroupedRatioDetail",
    "HMiKKTSetGroupedStep", "HMiKKTGetGroupedStep", "HMiKKTAddStepToBufferAndCheck", "HMiConeGetChecker",
    "HMiLinsysSetRefine", "HMiLinsysGetRefine", "HMiLinsysRefineBytes", "HMiKKTSetRefine", "HMiSymResidualProbe",
    "HMiLinsysSetRefineTiles", "HMiLinsysGetRefineTiles", "HMiKKTSetRefineTiles", "HMiTileResidualProbe", "HMiBspRefinedSolve", "HMiBspRefineTimingProbe",
    "HMiReadSDPA", "HMiSDPAGetDims", "HMiSDPAGetBlock", "HMiSDPAGetBlock64", "HMiSDPAGetLPBlock", "HMiSDPAGetRHS", "HMiSDPAFree",
]


class HDSDPError(RuntimeError):
    pass


# status of a refined solve (csrc/refine_rule.h: HdmRefineStatus)
REFINE_OFF, REFINE_CONVERGED, REFINE_STAGNATED, REFINE_MAXSTEPS, REFINE_NUMERICAL, REFINE_NO_MATRIX, REFINE_NOT_AVAILABLE = range(7)
REFINE_STATUS_NAMES = ("OFF", "CONVERGED", "STAGNATED", "MAXSTEPS", "NUMERICAL", "NO_MATRIX", "NOT_AVAILABLE")


def _refine_stats(h):
    """HMiLinsysGetRefine + HMiLinsysRefineBytes of a linear-system handle as a dict"""
    lib = load_library()
    st, steps = C.c_int(0), C.c_int(0)
    r0, r1, tol = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    solves, total = C.c_int64(0), C.c_int64(0)
    cap = lib.HMiLinsysGetRefine(h, C.byref(st), C.byref(steps), C.byref(r0), C.byref(r1), C.byref(tol), C.byref(solves), C.byref(total))
    if cap < 0:
        raise HDSDPError("HMiLinsysGetRefine failed")
    return {"cap": int(cap), "status": st.value, "status_name": REFINE_STATUS_NAMES[st.value], "steps": steps.value, "resid0": r0.value,
            "resid": r1.value, "tol": tol.value, "solves": solves.value, "total_steps": total.value,
            "device_bytes": int(lib.HMiLinsysRefineBytes(h))}


def sym_residual(M, x, b, n=None, ld=None):
    """HMiSymResidualProbe: (r, |r|_2^2) with r = b - M x from the refined solve's residual kernel.  M: the (n, ld) C-order array
    that IS the column-major ld x n matrix (M[j, i] = element (row i, column j)); lower triangle valid, everything else -- the
    upper triangle, rows >= n -- goes to the device as it is and must not be read"""
    M = np.ascontiguousarray(M, dtype=np.float64)
    n = M.shape[0] if n is None else n
    ld = M.shape[1] if ld is None else ld
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if M.size < ld * n or x.size < n or b.size < n:
        raise ValueError("sym_residual: an array is smaller than n and ld say")
    r, nrm = np.zeros(n), C.c_double(0.0)
    _check(load_library().HMiSymResidualProbe(int(n), _dptr(M), int(ld), _dptr(x), _dptr(b), _dptr(r), C.byref(nrm)), "HMiSymResidualProbe")
    return r, nrm.value


def tile_residual(m, beg, idx, val, x, b):
    """HMiTileResidualProbe: (r, |r|_2^2) with r = b - M x from the tile form's residual kernel; M as the lower-triangular CSC
    (beg, idx, val) HMiBspSolve takes, x, b and r in the caller's order.  The tile store's padding and spare tile are NaN."""
    beg, idx = np.ascontiguousarray(beg, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
    val, x, b = (np.ascontiguousarray(a, dtype=np.float64) for a in (val, x, b))
    if beg.size != m + 1 or idx.size < beg[m] or val.size < beg[m] or x.size < m or b.size < m:
        raise ValueError("tile_residual: an array is smaller than m and the pattern say")
    r, nrm = np.zeros(m), C.c_double(0.0)
    _check(load_library().HMiTileResidualProbe(int(m), _iptr(beg), _iptr(idx), _dptr(val), _dptr(x), _dptr(b), _dptr(r), C.byref(nrm)),
           "HMiTileResidualProbe")
    return r, nrm.value


def bsp_refined_solve(m, beg, idx, val, b, max_steps, relTol=0.0, absTol=0.0):
    """HMiBspRefinedSolve: the tile-form factorisation of the CSC matrix and the production refined solve.  Returns (x, info, st):
    st = dict(status, status_name, steps, resid0, resid, tol, block_rows, tiles, levels, negative); x is None where info != 0"""
    beg, idx = np.ascontiguousarray(beg, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
    val, b = np.ascontiguousarray(val, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if beg.size != m + 1 or idx.size < beg[m] or val.size < beg[m] or b.size < m:
        raise ValueError("bsp_refined_solve: an array is smaller than m and the pattern say")
    x, stats = np.zeros(m), np.zeros(4, dtype=np.int32)
    info, status, steps = C.c_int(-1), C.c_int(0), C.c_int(0)
    r0, r1, tol = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    _check(load_library().HMiBspRefinedSolve(int(m), _iptr(beg), _iptr(idx), _dptr(val), _dptr(b), _dptr(x), int(max_steps), float(relTol),
                                             float(absTol), C.byref(info), C.byref(status), C.byref(steps), C.byref(r0), C.byref(r1),
                                             C.byref(tol), _iptr(stats)), "HMiBspRefinedSolve")
    st = {"status": status.value, "status_name": REFINE_STATUS_NAMES[status.value], "steps": steps.value, "resid0": r0.value,
          "resid": r1.value, "tol": tol.value, "block_rows": int(stats[0]), "tiles": int(stats[1]), "levels": int(stats[2]),
          "negative": int(stats[3])}
    return (x if info.value == 0 else None), info.value, st


def bsp_refine_timing(m, beg, idx, val, b, variants, warmup=3, reps=31):
    """HMiBspRefineTimingProbe: one tile-form factorisation of the CSC matrix, then the variants -- (cap, relTol, absTol), cap < 0 =
    the unrefined solve -- alternate solve by solve.  Returns (ms[variant, rep], corrections, status, resid0, resid, stats[4], work bytes)"""
    beg, idx = np.ascontiguousarray(beg, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
    val, b = np.ascontiguousarray(val, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nv = len(variants)
    caps = np.array([v[0] for v in variants], dtype=np.int32)
    rel, ab = np.array([float(v[1]) for v in variants]), np.array([float(v[2]) for v in variants])
    ms, corr, status = np.zeros((nv, reps)), np.zeros(nv, dtype=np.int32), np.zeros(nv, dtype=np.int32)
    resid, stats, work = np.zeros(2 * nv), np.zeros(4, dtype=np.int32), C.c_int64(0)
    _check(load_library().HMiBspRefineTimingProbe(int(m), _iptr(beg), _iptr(idx), _dptr(val), _dptr(b), nv, _iptr(caps), _dptr(rel), _dptr(ab),
                                                  int(warmup), int(reps), _dptr(ms), _iptr(corr), _iptr(status), _dptr(resid), _iptr(stats),
                                                  C.byref(work)), "HMiBspRefineTimingProbe")
    return ms, corr, status, resid[0::2].copy(), resid[1::2].copy(), stats, work.value


class hdsdp_kkt(C.Structure):  # interface/def_hdsdp_schur.h:32-68
    _fields_ = [
        ("nRow", C.c_int), ("nCones", C.c_int), ("maxConeDim", C.c_int), ("cones", C.c_void_p),
        ("isKKTSparse", C.c_int), ("kktM", C.c_void_p),
        ("invBuffer", C.POINTER(C.c_double)), ("kktBuffer", C.POINTER(C.c_double)),
        ("kktBuffer2", C.POINTER(C.c_double)),
        ("kktMatBeg", C.POINTER(C.c_int)), ("kktMatIdx", C.POINTER(C.c_int)),
        ("kktMatElem", C.POINTER(C.c_double)), ("kktDiag", C.POINTER(C.POINTER(C.c_double))),
        ("dASinvVec", C.POINTER(C.c_double)), ("dASinvCSinvVec", C.POINTER(C.c_double)),
        ("dASinvRdSinvVec", C.POINTER(C.c_double)),
        ("dCSinvCSinv", C.c_double), ("dCSinvRdSinv", C.c_double), ("dCSinv", C.c_double),
        ("dTraceSinv", C.c_double), ("dPrimalX", C.c_void_p),
    ]


class hdsdp_linsys_head(C.Structure):  # linalg/def_hdsdp_linsolver.h:40-63, the fields callers read
    _fields_ = [("nCol", C.c_int), ("chol", C.c_void_p), ("LinType", C.c_int)]


def _lin_type(ptr):
    return C.cast(ptr, C.POINTER(hdsdp_linsys_head)).contents.LinType


_lib = None


def load_library():
    """dlopen the in-tree HIP extension; fails loudly if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HDSDPError(f"{LIB_PATH} is missing: run `python -m hdsdp_amd.build` (hipcc, gfx950). "
                         "There is no CPU fallback for the Schur path.")
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7 and loads it by path, the engine
    # links the system one by soname.  Engine first, torch later = two runtimes in one process, and torch then finds
    # "No HIP GPUs"; torch first = the engine's DT_NEEDED resolves to the copy torch already loaded.  So when torch is
    # around (tests, bench, the RCCL exchange), let it load first.  HDSDP_MI355X_NO_TORCH=1 skips this for processes
    # that never touch torch (the C ABI itself has no torch dependency).
    if "torch" not in sys.modules and os.environ.get("HDSDP_MI355X_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = C.CDLL(LIB_PATH)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    kp = C.POINTER(hdsdp_kkt)
    sig = {
        "HKKTCreate": (C.c_int, [C.POINTER(kp)]),
        "HKKTInit": (C.c_int, [kp, C.c_int, C.c_int, C.POINTER(vp)]),
        "HKKTBuildUp": (C.c_int, [kp, C.c_int]),
        "HKKTBuildUpExtraCone": (C.c_int, [kp, vp, C.c_int]),
        "HKKTBuildUpFixed": (C.c_int, [kp, C.c_int, C.c_int]),
        "HKKTExport": (None, [kp, dp, dp, dp, dp, dp, dp, dp]),
        "HKKTFactorize": (C.c_int, [kp]),
        "HKKTSolve": (C.c_int, [kp, dp, dp]),
        "HKKTRegularize": (None, [kp, C.c_double]),
        "HKKTRegisterPSDP": (None, [kp, vp]),
        "HKKTClear": (None, [kp]),
        "HKKTDestroy": (None, [C.POINTER(kp)]),
        "HFpLinsysCreate": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int]),
        "HFpLinsysSetParam": (None, [vp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int]),
        "HFpLinsysSymbolic": (C.c_int, [vp, ip, ip]),
        "HFpLinsysNumeric": (C.c_int, [vp, ip, ip, dp]),
        "HFpLinsysSwitchToBackUp": (C.c_int, [vp]),
        "HFpLinsysPsdCheck": (C.c_int, [vp, ip, ip, dp, ip]),
        "HFpLinsysFSolve": (None, [vp, C.c_int, dp, dp]),
        "HFpLinsysBSolve": (None, [vp, C.c_int, dp, dp]),
        "HFpLinsysSolve": (C.c_int, [vp, C.c_int, dp, dp]),
        "HFpLinsysGetDiag": (C.c_int, [vp, dp]),
        "HFpLinsysInvert": (None, [vp, dp, dp]),
        "HFpLinsysClear": (None, [vp]),
        "HFpLinsysDestroy": (None, [C.POINTER(vp)]),
        "HMiConeCreateSDP": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, ip, ip, dp, C.c_int, C.c_int]),
        "HMiConeCreateLP": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, ip, ip, dp]),
        "HMiConeLPSetSchurPath": (C.c_int, [vp, C.c_int]),
        "HMiConeLPGetSchurPath": (C.c_int, [vp, dp, dp, C.POINTER(C.c_int64)]),
        "HMiConeCreateSynthetic": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "HMiConeDestroy": (None, [C.POINTER(vp)]),
        "HMiConeSetStart": (None, [vp, C.c_double]),
        "HMiConeUpdate": (None, [vp, C.c_double, dp]),
        "HMiConeCheckIsInterior": (C.c_int, [vp, C.c_double, dp, ip]),
        "HMiConeRatioTest": (C.c_int, [vp, C.c_double, dp, C.c_double, C.c_int, dp]),
        "HMiLanczosStartVector": (None, [C.c_int, dp]),
        "HMiConeGetPrimal": (None, [vp, C.c_double, dp, dp, dp, dp]),
        "HMiConeCheckIsInteriorExpert": (C.c_int, [vp, C.c_double, C.c_double, dp, C.c_double, C.c_int, ip]),
        "HMiConeAddStepToBufferAndCheck": (C.c_int, [vp, C.c_double, C.c_int, ip]),
        "HMiConeReduceResi": (None, [vp, C.c_double]),
        "HMiConeSetPerturb": (None, [vp, C.c_double]),
        "HMiConeGetCoeffNorm": (C.c_double, [vp, C.c_int]),
        "HMiConeGetObjNorm": (C.c_double, [vp, C.c_int]),
        "HMiConeScalByConstant": (None, [vp, C.c_double]),
        "HMiConeComputeATimesXpy": (None, [vp, dp, dp]),
        "HMiConeComputeXDotS": (C.c_double, [vp, dp]),
        "HMiConeComputeTraceCX": (C.c_double, [vp, dp]),
        "HMiConeGetDual": (None, [vp, dp, dp]),
        "HMiConeGetLogBarrier": (C.c_int, [vp, C.c_double, dp, C.c_int, dp]),
        "HMiConeGetPresolve": (None, [vp, ip, ip, ip, ip, ip, ip]),
        "HMiConeDetectFeature": (None, [vp, dp, ip, dp]),
        "HMiConeGetDualMatrix": (C.c_int, [vp, dp]),
        "HMiConeGetTraces": (C.c_int, [vp, dp]),
        "HMiConeGetPath": (C.c_int, [vp]),
        "HMiConeGetDirectRows": (None, [vp, ip, ip, ip, ip]),
        "HMiConeSweepInfo": (C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "HMiConeGetStreaming": (C.c_int, [vp, ip]),
        "HMiConeUseSweepCopy": (C.c_int, [vp, C.c_int]),
        "HMiKKTSetHostMirror": (None, [kp, C.c_int]),
        "HMiConeSetExchange": (None, [vp, vp, vp, vp]),
        "HMiConeSetExchangePieces": (None, [vp, vp, vp, C.c_int]),
        "HMiConeGetExchangeStats": (None, [vp, ip, ip]),
        "HMiConeGetPrimalRoute": (C.c_int, [vp, ip, dp]),
        "HMiConeGetPrimalProfile": (C.c_int, [vp, dp, C.POINTER(C.c_int64)]),
        "HMiConeGetBuildProfile": (C.c_int, [vp, C.c_int, dp, C.c_int]),
        "HMiConeBuildPrimalXSXDirection": (None, [vp, dp, dp, C.c_int]),
        "HMiConeGetExchangeBuffers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]),
        "HMiConeSetExchangeBuffers": (C.c_int, [vp, vp, vp]),
        "HMiKKTDeviceMatrix": (vp, [kp, C.POINTER(C.c_int64)]),
        "HMiKKTGetRows": (C.c_int, [kp, C.c_int, ip, dp]),
        "HMiKKTGetDiagTarget": (C.c_int, [kp]),
        "HMiKKTGetMatrixTraffic": (None, [kp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "HMiSetDevices": (C.c_int, [C.c_int, ip]),
        "HMiSetDevicesEx": (C.c_int, [C.c_int, ip, C.c_int]),
        "HMiRcclGroupSelfTest": (C.c_int, [C.c_int, ip, C.c_int]),
        "HMiGetDeviceGroup": (C.c_int, [ip, C.c_int, ip]),
        "HMiSetShardMinDim": (None, [C.c_int]),
        "HMiConeGetShardCount": (C.c_int, [vp]),
        "HMiConeGetGroupTraffic": (None, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "HMiRcclSelfTest": (C.c_int, [C.c_int]),
        "HMiGetCallStats": (C.c_int, [dp, C.POINTER(C.c_int64), C.c_int]),
        "HMiCallStatName": (C.c_char_p, [C.c_int]),
        "HMiResetCallStats": (None, []),
        "HMiGetAssembleCounts": (C.c_int, [C.POINTER(C.c_int64), C.c_int]),
        "HMiKKTPhaseAEligible": (C.c_int, [kp]),
        "HMiKKTPhaseA": (C.c_int, [kp, C.c_double, dp, dp, dp, dp, dp, ip, dp]),
        "HMiDeviceInit": (C.c_int, [C.c_int]),
        "HMiDeviceSynchronize": (C.c_int, []),
        "HMiStream": (vp, []),
        "HMiVersion": (C.c_char_p, []),
        "HMiGetStageTimes": (None, [dp, C.c_int]),
        "HMiGemmNT": (C.c_int, [vp, C.c_int64, C.c_int, vp, C.c_int64, C.c_int, vp, C.c_int64, C.c_int, C.c_int,
                                C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]),
        "HMiGemmRoleLayout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int]),
        "HMiGemmRoleSpan": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64]),
        "HMiCongStep1": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, vp, C.c_int64]),
        "HMiCongStep2": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int, vp, C.c_int64, C.c_int64,
                                   C.c_uint64]),
        "HMiCongIRow": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64]),
        "HMiGramSplits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int]),
        "HMiGramGathered": (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_int, vp, C.c_int64, vp, C.c_int64, C.c_int]),
        "HMiGramLp": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, C.c_int64, C.c_int64]),
        "HMiPotrf": (C.c_int, [vp, C.c_int, C.c_int64, ip]),
        "HMiMfmaPeakProbe": (C.c_double, [C.c_int]),
        "HMiDiagBlockProbe": (C.c_double, [C.c_int, C.c_int]),
        "HMiCholEnvelopeSolve": (C.c_int, [vp, C.c_int, ip, vp, vp, vp, ip]),
        "HMiCholEnvelopeProbe": (C.c_int, [C.c_int, C.c_int, C.c_int, dp, dp]),
        "HMiKKTEnvelopeInfo": (None, [kp, ip, dp]),
        "HMiKKTTileInfo": (C.c_int, [kp, ip, C.POINTER(C.c_int64), ip, C.POINTER(C.c_int64)]),
        "HMiKKTNegativePivots": (C.c_int, [kp]),
        "HMiBspSolve": (C.c_int, [C.c_int, ip, ip, dp, dp, dp, ip, ip, dp]),
        "HMiRcmOrder": (C.c_int, [C.c_int, ip, ip, ip]),
        "HMiBspSymbolic": (C.c_int, [C.c_int, ip, ip, C.c_double, ip, ip, ip, ip]),
        "HMiWorkPlanQuery": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int]),
        "HMiConeGetWorkPlan": (C.c_int, [vp, C.POINTER(C.c_int64), C.c_int]),
        "HMiKKTSetGroupedBuild": (C.c_int, [kp, C.c_int]),
        "HMiKKTGetGroupedBuild": (C.c_int, [kp, ip, ip, ip]),
        "HMiKKTSetGroupedCheck": (C.c_int, [kp, C.c_int]),
        "HMiKKTGetGroupedCheck": (C.c_int, [kp, C.POINTER(C.c_long)]),
        "HMiKKTCheckIsInterior": (C.c_int, [kp, C.c_double, dp, ip, dp, ip]),
        "HMiKKTSetGroupedRatio": (C.c_int, [kp, C.c_int]),
        "HMiKKTGetGroupedRatio": (C.c_int, [kp, C.POINTER(C.c_long)]),
        "HMiKKTRatioTest": (C.c_int, [kp, C.c_double, dp, C.c_double, C.c_int, dp, dp]),
        "HMiKKTSetGroupedRatioChecker": (C.c_int, [kp, C.c_int]),
        "HMiKKTSetGroupedRatioRest": (C.c_int, [kp, C.c_int]),
        "HMiKKTGetGroupedRatioDetail": (C.c_int, [kp, C.POINTER(C.c_long)]),
        "HMiKKTSetGroupedStep": (C.c_int, [kp, C.c_int]),
        "HMiKKTGetGroupedStep": (C.c_int, [kp, C.POINTER(C.c_long)]),
        "HMiKKTAddStepToBufferAndCheck": (C.c_int, [kp, C.c_double, C.c_int, ip, ip]),
        "HMiConeGetChecker": (C.c_int, [vp, dp, dp, dp]),
        "HMiLinsysSetRefine": (C.c_int, [vp, C.c_int]),
        "HMiLinsysGetRefine": (C.c_int, [vp, ip, ip, dp, dp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "HMiLinsysRefineBytes": (C.c_int64, [vp]),
        "HMiKKTSetRefine": (C.c_int, [kp, C.c_int]),
        "HMiSymResidualProbe": (C.c_int, [C.c_int, dp, C.c_long, dp, dp, dp, dp]),
        "HMiLinsysSetRefineTiles": (C.c_int, [vp, C.c_int]),
        "HMiLinsysGetRefineTiles": (C.c_int, [vp]),
        "HMiKKTSetRefineTiles": (C.c_int, [kp, C.c_int]),
        "HMiTileResidualProbe": (C.c_int, [C.c_int, ip, ip, dp, dp, dp, dp, dp]),
        "HMiBspRefineTimingProbe": (C.c_int, [C.c_int, ip, ip, dp, dp, C.c_int, ip, dp, dp, C.c_int, C.c_int, dp, ip, ip, dp, ip, C.POINTER(C.c_int64)]),
        "HMiBspRefinedSolve": (C.c_int, [C.c_int, ip, ip, dp, dp, dp, C.c_int, C.c_double, C.c_double, ip, ip, ip, dp, dp, dp, ip]),
        "HMiGroupedPlanQuery": (C.c_int, [C.c_int, C.c_int, ip, ip, ip, ip, C.POINTER(C.c_int64), ip, ip, ip, ip, ip, C.POINTER(C.c_int64), ip, ip, ip,
                                          C.POINTER(C.c_int64), ip, ip]),
        "HMiPresolveCSC": (C.c_int, [C.c_int, C.c_int, ip, ip, dp, ip, ip, ip, ip, ip, ip]),
        "HMiReadSDPA": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        "HMiSDPAGetDims": (None, [vp, ip, ip, ip]),
        "HMiSDPAGetBlock": (C.c_int, [vp, C.c_int, ip, C.POINTER(ip), C.POINTER(ip), C.POINTER(dp)]),
        "HMiSDPAGetLPBlock": (C.c_int, [vp, ip, C.POINTER(ip), C.POINTER(ip), C.POINTER(dp)]),
        "HMiSDPAGetBlock64": (C.c_int, [vp, C.c_int, ip, C.POINTER(C.POINTER(C.c_int64)), C.POINTER(ip), C.POINTER(dp)]),
        "HMiSDPAGetRHS": (dp, [vp]),
        "HMiConeCreateSDP64": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), ip, dp, C.c_int, C.c_int]),
        "HMiConeBuilderBegin": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "HMiConeBuilderAddColumn": (C.c_int, [vp, C.c_int, C.c_int64, ip, dp]),
        "HMiConeBuilderStored": (C.c_int64, [vp]),
        "HMiConeBuilderFinish": (C.c_int, [C.POINTER(vp), C.POINTER(vp)]),
        "HMiConeBuilderAbort": (None, [C.POINTER(vp)]),
        "HMiSDPAFree": (None, [C.POINTER(vp)]),
        "HMiMfmaIssueProbe": (C.c_double, [C.c_int, C.c_int, C.c_int]),
        "HMiSetDebugBuffer": (None, [vp, C.c_int]),
        "HMiSetKernelTiming": (None, [C.c_int]),
        "HMiGetKernelTiming": (C.c_int, [dp, dp, C.POINTER(C.c_int64)]),
        "HMiGetKernelTimingEx": (C.c_int, [dp, dp, dp, C.POINTER(C.c_int64)]),
    }
    for name in EXPORTS:
        fn = getattr(lib, name)  # AttributeError == missing export
        fn.restype, fn.argtypes = sig[name]
    _lib = lib
    return lib


TRANSPORT_ENV, TRANSPORT_COPY, TRANSPORT_RCCL = -1, 0, 1


def set_devices(ids, shard_min_dim=None, transport=TRANSPORT_ENV):
    """single-process multi-device mode (include/hdsdp_mi355x.h: HMiSetDevicesEx): cones created afterwards with rank 0 of
    world 1 are sharded over `ids` (repeated ids = shards sharing a device, exchanged by device copies).  transport:
    TRANSPORT_COPY / TRANSPORT_RCCL, or TRANSPORT_ENV = what HDSDP_MI355X_TRANSPORT says (default copies)"""
    lib = load_library()
    arr = (C.c_int * len(ids))(*ids)
    if lib.HMiSetDevicesEx(len(ids), arr, int(transport)) != 0:
        raise HDSDPError("HMiSetDevicesEx failed")
    if shard_min_dim is not None:
        lib.HMiSetShardMinDim(int(shard_min_dim))


def rccl_group_self_test(ids, timeout_ms=60000):
    """HMiRcclGroupSelfTest over `ids` (distinct devices): 0 = passed, else the first failing stage"""
    lib = load_library()
    arr = (C.c_int * len(ids))(*ids)
    return int(lib.HMiRcclGroupSelfTest(len(ids), arr, int(timeout_ms)))


def bsp_symbolic(m, beg, idx, max_fraction=1.0):
    """HMiBspSymbolic (host only): (rc, perm, stats[5], blockPtr, blockRow) of the tile form's symbolic phase on a lower-triangular
    CSC pattern; perm and the block pattern are None where rc != 0"""
    lib = load_library()
    ip = C.POINTER(C.c_int)
    beg, idx = np.ascontiguousarray(beg, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
    perm, stats = np.zeros(m, dtype=np.int32), np.zeros(5, dtype=np.int32)
    rc = lib.HMiBspSymbolic(m, beg.ctypes.data_as(ip), idx.ctypes.data_as(ip), float(max_fraction), perm.ctypes.data_as(ip),
                            stats.ctypes.data_as(ip), None, None)
    if rc != 0:
        return rc, None, stats, None, None
    bptr, brow = np.zeros(stats[0] + 1, dtype=np.int32), np.zeros(stats[1], dtype=np.int32)
    rc = lib.HMiBspSymbolic(m, beg.ctypes.data_as(ip), idx.ctypes.data_as(ip), float(max_fraction), perm.ctypes.data_as(ip),
                            stats.ctypes.data_as(ip), bptr.ctypes.data_as(ip), brow.ctypes.data_as(ip))
    return rc, perm, stats, bptr, brow


def chol_envelope_solve(A, first, b):
    """HMiCholEnvelopeSolve: the blocked Cholesky of the symmetric matrix A (its lower triangle is read) on the block envelope
    first[] (None = dense) and one solve.  Returns (x, L, info): L = the lower triangle of the factor, x and L None where
    info != 0."""
    lib = load_library()
    A = np.asfortranarray(A, dtype=np.float64)
    n = A.shape[0]
    b = np.ascontiguousarray(b, dtype=np.float64)
    x, L, info = np.zeros(n), np.zeros((n, n), order="F"), C.c_int(-1)
    fa = None if first is None else np.ascontiguousarray(first, dtype=np.int32)
    rc = lib.HMiCholEnvelopeSolve(A.ctypes.data, n, None if fa is None else fa.ctypes.data_as(C.POINTER(C.c_int)), b.ctypes.data,
                                  x.ctypes.data, L.ctypes.data, C.byref(info))
    if rc != 0:
        raise HDSDPError("HMiCholEnvelopeSolve failed")
    if info.value != 0:
        return None, None, info.value
    return x, np.tril(L), 0


def device_group():
    lib = load_library()
    ids = (C.c_int * 16)()
    tr = C.c_int(-1)
    n = lib.HMiGetDeviceGroup(ids, 16, C.byref(tr))
    return list(ids[:n]), tr.value


def _check(rc, what):
    if rc != RETCODE_OK:
        raise HDSDPError(f"{what} returned hdsdp_retcode {rc}")


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def presolve_csc(n, m, beg, idx, val):
    """host-only presolve of one block (classification, ordering, strategy plan); needs no GPU"""
    lib = load_library()
    beg = np.ascontiguousarray(beg, dtype=np.int32)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    out = {k: np.zeros(m, dtype=np.int32) for k in ("coef_type", "coef_rank", "coef_nnz", "kkt_perm", "kkt_strategy")}
    ot = C.c_int(0)
    _check(lib.HMiPresolveCSC(m, n, _iptr(beg), _iptr(idx), _dptr(val), _iptr(out["coef_type"]),
                              _iptr(out["coef_rank"]), _iptr(out["coef_nnz"]), _iptr(out["kkt_perm"]),
                              _iptr(out["kkt_strategy"]), C.byref(ot)), "HMiPresolveCSC")
    out["obj_type"] = ot.value
    return out


WORK_PLAN_FIELDS = ("n16", "nblk", "npb", "npb_loc", "Lr", "R", "astride", "mloc", "Bc", "nsplit", "nslab", "shared_ts",
                    "gram_queue_global", "t_bytes", "slab_bytes", "exchange_bytes", "gram_bytes")


def work_plan(n, m, world=1, rank=0):
    """what the engine would plan in this process for rank `rank` of `world` on a dense block (csrc/work_plan.h through
    HMiWorkPlanQuery): layout, constraints per congruence launch, K splits and slabs of the Gram product, buffer sizes.
    Host arithmetic under the process's HDM_* knobs; needs no GPU"""
    out = (C.c_int64 * len(WORK_PLAN_FIELDS))()
    if load_library().HMiWorkPlanQuery(n, m, world, rank, out, len(out)) != len(out):
        raise HDSDPError(f"HMiWorkPlanQuery refused n={n} m={m} world={world} rank={rank}")
    return dict(zip(WORK_PLAN_FIELDS, (int(v) for v in out)))


GEMM_ROLE_LAYOUT_FIELDS = ("n16", "nblk", "npb", "npb_loc", "Lr", "R", "astride")
SPAN_T, SPAN_LINV, SPAN_AFULL, SPAN_EXCHANGE, SPAN_LP = range(5)


def gemm_role_layout(n, world=1, maxloc=0):
    """the layout numbers of a dense block (csrc/work_plan.h: hdm_layout through HMiGemmRoleLayout); needs no GPU"""
    out = (C.c_int64 * len(GEMM_ROLE_LAYOUT_FIELDS))()
    if load_library().HMiGemmRoleLayout(n, world, maxloc, out, len(out)) != len(out):
        raise HDSDPError(f"HMiGemmRoleLayout refused n={n} world={world} maxloc={maxloc}")
    return dict(zip(GEMM_ROLE_LAYOUT_FIELDS, (int(v) for v in out)))


def gemm_role_span(which, n=16, world=1, maxloc=0, a0=0, a1=0):
    """doubles an operand buffer of the Schur build's GEMM launches is vouched to hold, slack included (HMiGemmRoleSpan:
    SPAN_T of a0 matrices, SPAN_LINV of leading dimension a0, SPAN_AFULL of a0 skyline matrices, SPAN_EXCHANGE, SPAN_LP of
    kc = a0 and mpad = a1); needs no GPU"""
    v = int(load_library().HMiGemmRoleSpan(which, n, world, maxloc, a0, a1))
    if v < 0:
        raise HDSDPError(f"HMiGemmRoleSpan refused which={which} n={n} world={world} maxloc={maxloc} a0={a0} a1={a1}")
    return v


def grouped_plan(m, cones):
    """the grouped Schur build's plan (csrc/grouped_plan.h through HMiGroupedPlanQuery) for an operator of m rows whose cones are
    given as (n, rows) or (n, rows, kind_ok): block dimension, global rows owned in local order, and whether the cone is of the
    kind the engine groups at all (default True).  Host arithmetic; needs no GPU.  Returns a dict: cones (grouped), n_eligible,
    eligible / slot_of (per cone), jobs (slot, q0, q1, first), the destinations of M (m_row >= m_col) with their contributors as a
    CSR (m_ptr, m_slot, m_idx), the same for the vectors' rows (v_row, v_ptr, v_slot, v_idx), staging_doubles"""
    lib = load_library()
    nc = len(cones)
    dims = np.asarray([int(c[0]) for c in cones], dtype=np.int32).reshape(nc)
    kind = np.asarray([1 if (len(c) < 3 or c[2]) else 0 for c in cones], dtype=np.int32).reshape(nc)
    rows = [np.asarray(c[1], dtype=np.int32).reshape(-1) for c in cones]
    beg = np.zeros(nc + 1, dtype=np.int32)
    beg[1:] = np.cumsum([r.size for r in rows])
    allrows = np.ascontiguousarray(np.concatenate(rows + [np.zeros(1, dtype=np.int32)]), dtype=np.int32)
    counts = (C.c_int64 * 8)()
    el, slot = np.zeros(max(1, nc), dtype=np.int32), np.zeros(max(1, nc), dtype=np.int32)
    head = (int(m), nc, _iptr(dims), _iptr(kind), _iptr(beg), _iptr(allrows), counts, _iptr(el), _iptr(slot))
    if lib.HMiGroupedPlanQuery(*head, *([None] * 10)) != 8:
        raise HDSDPError("HMiGroupedPlanQuery refused the operator")
    ng, nj, nm, nmc, nv, nvc = (int(counts[i]) for i in range(6))
    iz = lambda k: np.zeros(max(1, k), dtype=np.int32)        # noqa: E731
    lz = lambda k: np.zeros(max(1, k), dtype=np.int64)        # noqa: E731
    jobs, mr, mcl, mp, ms, mi, vr, vp_, vs, vi = iz(4 * nj), iz(nm), iz(nm), lz(nm + 1), iz(nmc), iz(nmc), iz(nv), lz(nv + 1), iz(nvc), iz(nvc)
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))     # noqa: E731
    if lib.HMiGroupedPlanQuery(*head, _iptr(jobs), _iptr(mr), _iptr(mcl), lp(mp), _iptr(ms), _iptr(mi), _iptr(vr), lp(vp_), _iptr(vs),
                               _iptr(vi)) != 8:
        raise HDSDPError("HMiGroupedPlanQuery refused the operator")
    return {"cones": ng, "n_eligible": int(counts[7]), "eligible": el[:nc].astype(bool), "slot_of": slot[:nc].copy(),
            "jobs": jobs[:4 * nj].reshape(nj, 4), "m_row": mr[:nm], "m_col": mcl[:nm], "m_ptr": mp[:nm + 1], "m_slot": ms[:nmc],
            "m_idx": mi[:nmc], "v_row": vr[:nv], "v_ptr": vp_[:nv + 1], "v_slot": vs[:nvc], "v_idx": vi[:nvc],
            "staging_doubles": int(counts[6])}


def assemble_counts():
    """process-wide answers to dual / step matrix requests (HMiGetAssembleCounts): [0] already in the buffer, [1] copy of S,
    [2] S + alpha dS on the last ratio test's line, [3] sweep off that line, [4] refresh sweep, [5] step-matrix sweep,
    [6] sweep of an untracked block"""
    out = (C.c_int64 * 7)()
    k = int(load_library().HMiGetAssembleCounts(out, 7))
    return [int(out[i]) for i in range(min(k, 7))]


def lanczos_start_vector(n):
    v = np.zeros(n)
    load_library().HMiLanczosStartVector(int(n), _dptr(v))
    return v


def read_sdpa(fname):
    """SDPA sparse file -> dict(m, b, blocks=[dict(n, beg, idx, val)], n_lp, lp) in the reference's CSC layout; lp = the LP
    block as dict(n, beg, idx, val) (CSC of n rows and m + 1 columns, column 0 = the objective), or None"""
    lib = load_library()
    h = C.c_void_p()
    _check(lib.HMiReadSDPA(os.fsencode(fname), C.byref(h)), f"HMiReadSDPA({fname})")
    try:
        m, nb, nlp = C.c_int(), C.c_int(), C.c_int()
        lib.HMiSDPAGetDims(h, C.byref(m), C.byref(nb), C.byref(nlp))
        b = np.ctypeslib.as_array(lib.HMiSDPAGetRHS(h), shape=(m.value,)).copy()
        blocks = []
        for i in range(nb.value):
            dim = C.c_int()
            pb, pi, pv = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_double)()
            _check(lib.HMiSDPAGetBlock(h, i, C.byref(dim), C.byref(pb), C.byref(pi), C.byref(pv)), "HMiSDPAGetBlock")
            beg = np.ctypeslib.as_array(pb, shape=(m.value + 2,)).copy()
            nnz = int(beg[-1])
            idx = np.ctypeslib.as_array(pi, shape=(max(nnz, 1),))[:nnz].copy()
            val = np.ctypeslib.as_array(pv, shape=(max(nnz, 1),))[:nnz].copy()
            blocks.append({"n": dim.value, "beg": beg, "idx": idx, "val": val})
        lp = None
        if nlp.value > 0:
            ncol = C.c_int()
            pb, pi, pv = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_double)()
            _check(lib.HMiSDPAGetLPBlock(h, C.byref(ncol), C.byref(pb), C.byref(pi), C.byref(pv)), "HMiSDPAGetLPBlock")
            beg = np.ctypeslib.as_array(pb, shape=(m.value + 2,)).copy()
            nnz = int(beg[-1])
            idx = np.ctypeslib.as_array(pi, shape=(max(nnz, 1),))[:nnz].copy()
            val = np.ctypeslib.as_array(pv, shape=(max(nnz, 1),))[:nnz].copy()
            lp = {"n": ncol.value, "beg": beg, "idx": idx, "val": val}
        return {"m": m.value, "b": b, "blocks": blocks, "n_lp": nlp.value, "lp": lp}
    finally:
        lib.HMiSDPAFree(C.byref(h))


class SDPCone:
    """One SDP block living in HBM (the reference's hdsdp_cone with the dense-SDP slots of the Schur path)."""

    def __init__(self, handle, n, m, rank=0, world=1):
        self._h, self.n, self.m, self.rank, self.world = handle, n, m, rank, world

    @classmethod
    def from_csc(cls, n, m, beg, idx, val, iCone=0, rank=0, world=1):
        """CSC of shape n(n+1)/2 x (m+1), column 0 = C (interface/def_hdsdp_user_data.h:16-32)."""
        lib = load_library()
        beg = np.ascontiguousarray(beg, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        assert beg.shape[0] == m + 2
        h = C.c_void_p()
        _check(lib.HMiConeCreateSDP(C.byref(h), iCone, m, n, _iptr(beg), _iptr(idx), _dptr(val), rank, world),
               "HMiConeCreateSDP")
        return cls(h, n, m, rank, world)

    @classmethod
    def from_csc64(cls, n, m, beg, idx, val, iCone=0, rank=0, world=1):
        """the same CSC with 64-bit column pointers (HMiConeCreateSDP64): a block may hold more than 2^31 - 1 entries"""
        lib = load_library()
        beg = np.ascontiguousarray(beg, dtype=np.int64)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        assert beg.shape[0] == m + 2
        h = C.c_void_p()
        _check(lib.HMiConeCreateSDP64(C.byref(h), iCone, m, n, beg.ctypes.data_as(C.POINTER(C.c_int64)), _iptr(idx), _dptr(val),
                                      rank, world), "HMiConeCreateSDP64")
        return cls(h, n, m, rank, world)

    @classmethod
    def from_columns(cls, n, m, columns, iCone=0, rank=0, world=1):
        """column-by-column ingest (HMiConeBuilder*): `columns` yields (iCol, packed_idx, values), iCol 0 = the objective,
        i = A_i, in any order; nothing but the column in hand has to exist on the caller's side"""
        lib = load_library()
        b = C.c_void_p()
        _check(lib.HMiConeBuilderBegin(C.byref(b), iCone, m, n, rank, world), "HMiConeBuilderBegin")
        try:
            for iCol, idx, val in columns:
                idx = np.ascontiguousarray(idx, dtype=np.int32)
                val = np.ascontiguousarray(val, dtype=np.float64)
                assert idx.shape == val.shape
                _check(lib.HMiConeBuilderAddColumn(b, int(iCol), int(idx.shape[0]), _iptr(idx), _dptr(val)), "HMiConeBuilderAddColumn")
            stored = int(lib.HMiConeBuilderStored(b))
            h = C.c_void_p()
            _check(lib.HMiConeBuilderFinish(C.byref(b), C.byref(h)), "HMiConeBuilderFinish")
        finally:
            if b:
                lib.HMiConeBuilderAbort(C.byref(b))
        cone = cls(h, n, m, rank, world)
        cone.stored_entries = stored
        return cone

    @classmethod
    def synthetic(cls, n, m, iCone=0, rank=0, world=1):
        """SURVEY.md 8(d) strictly feasible dense family, generated in HBM."""
        lib = load_library()
        h = C.c_void_p()
        _check(lib.HMiConeCreateSynthetic(C.byref(h), iCone, n, m, rank, world), "HMiConeCreateSynthetic")
        return cls(h, n, m, rank, world)

    def set_start(self, Rd):
        load_library().HMiConeSetStart(self._h, float(Rd))

    def check_is_interior(self, tau, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        ok = C.c_int(0)
        _check(load_library().HMiConeCheckIsInterior(self._h, float(tau), _dptr(y), C.byref(ok)),
               "HConeCheckIsInterior")
        return bool(ok.value)

    def ratio_test(self, dtau_step, dy, ada_ratio=0.0, buffer=BUFFER_DUALVAR):
        """HConeRatioTest: largest step keeping S + step*dS in the cone (inf if unbounded); S = the chosen buffer"""
        dy = np.ascontiguousarray(dy, dtype=np.float64)
        out = C.c_double(0.0)
        _check(load_library().HMiConeRatioTest(self._h, float(dtau_step), _dptr(dy), float(ada_ratio), buffer,
                                               C.byref(out)), "HConeRatioTest")
        return out.value

    def check_is_interior_expert(self, c_coef, a_scal, a_coef, eye_coef, buffer=BUFFER_DUALVAR):
        a_coef = np.ascontiguousarray(a_coef, dtype=np.float64)
        ok = C.c_int(0)
        _check(load_library().HMiConeCheckIsInteriorExpert(self._h, float(c_coef), float(a_scal), _dptr(a_coef),
                                                           float(eye_coef), buffer, C.byref(ok)), "HConeCheckIsInteriorExpert")
        return bool(ok.value)

    def axpy_buffer_and_check(self, step, buffer=BUFFER_DUALCHECK):
        ok = C.c_int(0)
        _check(load_library().HMiConeAddStepToBufferAndCheck(self._h, float(step), buffer, C.byref(ok)), "HConeAddStepToBufferAndCheck")
        return bool(ok.value)

    def log_barrier_of(self, buffer):
        out = C.c_double(0.0)
        _check(load_library().HMiConeGetLogBarrier(self._h, 0.0, None, buffer, C.byref(out)), "HConeGetLogBarrier")
        return out.value

    def coeff_norm(self, which):
        return load_library().HMiConeGetCoeffNorm(self._h, int(which))

    def obj_norm(self, which):
        return load_library().HMiConeGetObjNorm(self._h, int(which))

    def scal_by_constant(self, s):
        load_library().HMiConeScalByConstant(self._h, float(s))

    def a_times_x(self, X, y=None):
        X = np.ascontiguousarray(X, dtype=np.float64)
        out = np.zeros(self.m) if y is None else np.ascontiguousarray(y, dtype=np.float64).copy()
        load_library().HMiConeComputeATimesXpy(self._h, _dptr(X), _dptr(out))
        return out

    def x_dot_s(self, X):
        return load_library().HMiConeComputeXDotS(self._h, _dptr(np.ascontiguousarray(X, dtype=np.float64)))

    def trace_cx(self, X):
        return load_library().HMiConeComputeTraceCX(self._h, _dptr(np.ascontiguousarray(X, dtype=np.float64)))

    def get_dual(self):
        S = np.zeros((self.n, self.n))
        load_library().HMiConeGetDual(self._h, _dptr(S), None)
        return S

    def reduce_resi(self, v):
        load_library().HMiConeReduceResi(self._h, float(v))

    def set_perturb(self, v):
        load_library().HMiConeSetPerturb(self._h, float(v))

    def get_primal(self, mu, y, dy):
        """HConeGetPrimal: n x n primal recovery matrix, or None if S(y) is not positive definite"""
        y = np.ascontiguousarray(y, dtype=np.float64)
        dy = np.ascontiguousarray(dy, dtype=np.float64)
        X = np.full((self.n, self.n), np.nan)
        load_library().HMiConeGetPrimal(self._h, float(mu), _dptr(y), _dptr(dy), _dptr(X), None)
        return None if np.isnan(X[0, 0]) else X

    def log_barrier(self, tau, y=None):
        out = C.c_double(0.0)
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
            yp = _dptr(y)
        _check(load_library().HMiConeGetLogBarrier(self._h, float(tau), yp, BUFFER_DUALVAR, C.byref(out)),
               "HConeGetLogBarrier")
        return out.value

    def build_primal_xsx(self, X, XSX, dual_matrix=True):
        """XSX += X^T D X with D = the dual matrix S (dual_matrix) or the dual step of the last ratio test"""
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert XSX.flags.c_contiguous and XSX.dtype == np.float64
        load_library().HMiConeBuildPrimalXSXDirection(self._h, _dptr(X), _dptr(XSX), 1 if dual_matrix else 0)
        return XSX

    def shard_count(self):
        return int(load_library().HMiConeGetShardCount(self._h))

    def group_traffic(self):
        a, b = C.c_int64(0), C.c_int64(0)
        load_library().HMiConeGetGroupTraffic(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def exchange_stats(self):
        """(pieces of the last build's all-to-all, launches the staged second congruence step was cut into)"""
        p, s = C.c_int(0), C.c_int(0)
        load_library().HMiConeGetExchangeStats(self._h, C.byref(p), C.byref(s))
        return p.value, s.value

    def primal_route(self):
        """(route, q, growth) of the last KKT_TYPE_PRIMAL build (HMiConeGetPrimalRoute): route 0 = X positive definite,
        1 = signed factor + signed Gram correction, 2 = row-by-row fallback or refusal; q = negative pivots of the signed
        factor, growth = |W|_F^2 / |X|_F.  None before the first such build"""
        q, gr = C.c_int(0), C.c_double(0.0)
        r = int(load_library().HMiConeGetPrimalRoute(self._h, C.byref(q), C.byref(gr)))
        return None if r < 0 else (r, q.value, gr.value)

    def primal_profile(self):
        """ms of the signed part of the last route-1 KKT_TYPE_PRIMAL build (HMiConeGetPrimalProfile): dict with the signed
        factor + acceptance test, the gathers, the correction's Gram launches, the combination, and the gathered columns;
        None when the last KKT_TYPE_PRIMAL build was not on route 1"""
        ms, cols = np.zeros(4), C.c_int64(0)
        if load_library().HMiConeGetPrimalProfile(self._h, _dptr(ms), C.byref(cols)):
            return None
        return {"factor_check_ms": float(ms[0]), "gather_ms": float(ms[1]), "correction_ms": float(ms[2]),
                "combine_ms": float(ms[3]), "columns": int(cols.value)}

    def build_profile(self, shard=0):
        """where the last SHARDED Schur build of one shard spent its time (HMiConeGetBuildProfile; ms, bytes): None when no
        sharded build has run on it"""
        buf = np.zeros(8 + 6 * 64)
        k = int(load_library().HMiConeGetBuildProfile(self._h, int(shard), _dptr(buf), int(buf.size)))
        if k <= 0:
            return None
        P = int(buf[0])
        per = buf[8:8 + 6 * P].reshape(P, 6)
        return {"pieces": P, "staged": bool(buf[1]), "invert_ms": float(buf[2]),
                ("congruence_step1_ms" if buf[1] else "congruence_ms"): float(buf[3]), "slab_reduce_ms": float(buf[4]),
                "allreduce_ms": float(buf[5]), "extract_ms": float(buf[6]), "world": int(buf[7]),
                "step2_piece_ms": per[:, 0].tolist(), "exchange_wait_ms": per[:, 1].tolist(),
                "exchange_wait_host_ms": per[:, 2].tolist(), "gram_piece_ms": per[:, 3].tolist(),
                "piece_bytes_sent": per[:, 4].tolist(), "piece_flight_ms": per[:, 5].tolist()}

    def detect_feature(self, b):
        """the cone's getstat slot (HConeDetectFeature): (int features[20], double features[20]), zero where the cone decides nothing"""
        fi, fd = np.zeros(20, dtype=np.int32), np.zeros(20)
        bb = np.ascontiguousarray(b, dtype=np.float64)
        load_library().HMiConeDetectFeature(self._h, _dptr(bb), _iptr(fi), _dptr(fd))
        return fi, fd

    def presolve(self):
        m = self.m
        out = {k: np.zeros(m, dtype=np.int32) for k in ("coef_type", "coef_rank", "coef_nnz", "kkt_perm", "kkt_strategy")}
        ot = C.c_int(0)
        load_library().HMiConeGetPresolve(self._h, _iptr(out["coef_type"]), _iptr(out["coef_rank"]),
                                          _iptr(out["coef_nnz"]), _iptr(out["kkt_perm"]), _iptr(out["kkt_strategy"]),
                                          C.byref(ot))
        out["obj_type"] = ot.value
        return out

    def dual_matrix(self):
        S = np.zeros((self.n, self.n), dtype=np.float64)  # column-major n x n seen as C-order transposed
        _check(load_library().HMiConeGetDualMatrix(self._h, _dptr(S)), "HMiConeGetDualMatrix")
        return S

    def checker_state(self):
        """HMiConeGetChecker: (Scheck, L, Dinv) as the last write of the checker left them -- the checker buffer, n16 x n16,
        and the checker factor object's two 128 x 128 matrices; element (i, j) of each is [j, i] (column-major storage)"""
        n16 = (self.n + 15) // 16 * 16
        Sc, L, D = np.zeros((n16, n16)), np.zeros((128, 128)), np.zeros((128, 128))
        _check(load_library().HMiConeGetChecker(self._h, _dptr(Sc), _dptr(L), _dptr(D)), "HMiConeGetChecker")
        return Sc, L, D

    def traces(self):
        t = np.zeros(self.m, dtype=np.float64)
        _check(load_library().HMiConeGetTraces(self._h, _dptr(t)), "HMiConeGetTraces")
        return t

    @property
    def path(self):
        return load_library().HMiConeGetPath(self._h)

    def direct_rows(self):
        """(direct rows, rank-one ones among them, congruence rows, kmax) of a congruence + Gram block whose low-rank rows are
        built without the congruence (HMiConeGetDirectRows); all zero for a cone without the form"""
        v = [C.c_int(0) for _ in range(4)]
        load_library().HMiConeGetDirectRows(self._h, *[C.byref(x) for x in v])
        return tuple(int(x.value) for x in v)

    def use_sweep_copy(self, on):
        _check(load_library().HMiConeUseSweepCopy(self._h, int(bool(on))), "HMiConeUseSweepCopy")

    def streaming(self):
        """(streamed?, rows per regenerated batch): include/hdsdp_mi355x.h: HMiConeGetStreaming"""
        b = C.c_int(0)
        on = load_library().HMiConeGetStreaming(self._h, C.byref(b))
        return bool(on), int(b.value)

    def sweep_info(self):
        """(in use, stored values, skyline positions they stand for) of the zero-suppressed copy the S / dS sweeps read"""
        v, p = C.c_int64(0), C.c_int64(0)
        on = load_library().HMiConeSweepInfo(self._h, C.byref(v), C.byref(p))
        return bool(on), int(v.value), int(p.value)

    def work_plan(self):
        """what the cone holds once its first build has allocated the work space (a group cone: shard 0), to compare with
        api.work_plan: dict of Bc, nsplit, nslab, shared_ts, gram_queue_global, t_bytes, slab_bytes; None before that"""
        keys = ("Bc", "nsplit", "nslab", "shared_ts", "gram_queue_global", "t_bytes", "slab_bytes")
        out = (C.c_int64 * len(keys))()
        k = load_library().HMiConeGetWorkPlan(self._h, out, len(out))
        if k < 0:
            raise HDSDPError("HMiConeGetWorkPlan: not an SDP cone of the engine")
        return dict(zip(keys, (int(v) for v in out))) if k else None

    def destroy(self):
        if self._h:
            load_library().HMiConeDestroy(C.byref(self._h))
            self._h = None


class LPCone:
    """The LP (diagonal) block of an SDPA problem living in HBM: the reference's hdsdp_cone with the LP slots
    (interface/hdsdp_conic_lp.c), its Schur build on the device.  Vectors (duals, primals) are 1-D arrays of n = nCol."""

    DENSE, SPARSE = 1, 2

    def __init__(self, handle, n, m):
        self._h, self.n, self.m = handle, n, m

    @classmethod
    def from_csc(cls, m, n, beg, idx, val, iCone=0):
        """CSC of n rows (LP columns) and m + 1 columns, column 0 = the objective (LPConeProcDataImpl's input)"""
        lib = load_library()
        beg = np.ascontiguousarray(beg, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        assert beg.shape[0] == m + 2
        h = C.c_void_p()
        _check(lib.HMiConeCreateLP(C.byref(h), iCone, m, n, _iptr(beg), _iptr(idx), _dptr(val)), "HMiConeCreateLP")
        return cls(h, n, m)

    @classmethod
    def from_sdpa(cls, fname, iCone=0):
        """the LP block of an SDPA file (read_sdpa(fname)["lp"])"""
        p = read_sdpa(fname)
        if p["lp"] is None:
            raise HDSDPError(f"{fname} has no LP block")
        lp = p["lp"]
        return cls.from_csc(p["m"], lp["n"], lp["beg"], lp["idx"], lp["val"], iCone=iCone)

    def set_schur_path(self, path):
        """0 = by the cost rule, LPCone.DENSE, LPCone.SPARSE (HMiConeLPSetSchurPath)"""
        if load_library().HMiConeLPSetSchurPath(self._h, int(path)) != 0:
            raise HDSDPError(f"HMiConeLPSetSchurPath({path}) failed")

    def schur_path(self):
        """(path, modelled dense seconds, modelled sparse seconds, pair-list bytes)"""
        a, b, n = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        p = load_library().HMiConeLPGetSchurPath(self._h, C.byref(a), C.byref(b), C.byref(n))
        return p, a.value, b.value, n.value

    set_start = SDPCone.set_start
    check_is_interior = SDPCone.check_is_interior
    ratio_test = SDPCone.ratio_test
    check_is_interior_expert = SDPCone.check_is_interior_expert
    axpy_buffer_and_check = SDPCone.axpy_buffer_and_check
    log_barrier_of = SDPCone.log_barrier_of
    log_barrier = SDPCone.log_barrier
    coeff_norm = SDPCone.coeff_norm
    obj_norm = SDPCone.obj_norm
    scal_by_constant = SDPCone.scal_by_constant
    a_times_x = SDPCone.a_times_x
    x_dot_s = SDPCone.x_dot_s
    trace_cx = SDPCone.trace_cx
    reduce_resi = SDPCone.reduce_resi
    set_perturb = SDPCone.set_perturb
    detect_feature = SDPCone.detect_feature
    destroy = SDPCone.destroy

    def update(self, tau, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        load_library().HMiConeUpdate(self._h, float(tau), _dptr(y))

    def get_dual(self):
        s = np.zeros(self.n)
        load_library().HMiConeGetDual(self._h, _dptr(s), None)
        return s

    def get_primal(self, mu, y, dy):
        """HConeGetPrimal: the nCol primal values, or None if the recovery point is not interior"""
        y = np.ascontiguousarray(y, dtype=np.float64)
        dy = np.ascontiguousarray(dy, dtype=np.float64)
        X = np.full(self.n, np.nan)
        load_library().HMiConeGetPrimal(self._h, float(mu), _dptr(y), _dptr(dy), _dptr(X), None)
        return None if np.isnan(X[0]) else X

    def build_primal_xsx(self, X, XSX, dual_matrix=True):
        """XSX = X * X * s with s = the dual (dual_matrix) or the dual step of the last ratio test"""
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert XSX.flags.c_contiguous and XSX.dtype == np.float64 and XSX.shape == (self.n,)
        load_library().HMiConeBuildPrimalXSXDirection(self._h, _dptr(X), _dptr(XSX), 1 if dual_matrix else 0)
        return XSX


class KKT:
    """hdsdp_kkt: the Schur operator (interface/hdsdp_schur.c)."""

    def __init__(self, m, cones, host_mirror=True):
        lib = load_library()
        self.m = m
        self.cones = list(cones)
        self._k = C.POINTER(hdsdp_kkt)()
        _check(lib.HKKTCreate(C.byref(self._k)), "HKKTCreate")
        self._cone_arr = (C.c_void_p * len(self.cones))(*[c._h for c in self.cones])
        _check(lib.HKKTInit(self._k, m, len(self.cones), self._cone_arr), "HKKTInit")
        if not host_mirror:
            lib.HMiKKTSetHostMirror(self._k, 0)

    def build_up(self, typeKKT=KKT_TYPE_INFEASIBLE):
        _check(load_library().HKKTBuildUp(self._k, typeKKT), "HKKTBuildUp")

    def build_up_fixed(self, typeKKT, strategy):
        _check(load_library().HKKTBuildUpFixed(self._k, typeKKT, strategy), "HKKTBuildUpFixed")

    def register_psdp(self, primal_mats):
        """HKKTRegisterPSDP (interface/hdsdp_schur.c:375-380): borrow one primal per cone -- an n x n column-major matrix for
        an SDP cone, a 1-D array of nCol entries for an LP cone; build_up(KKT_TYPE_PRIMAL) then runs the builder on them
        instead of S^-1"""
        self._psdp = []
        for c, x in zip(self.cones, primal_mats):
            x = np.ascontiguousarray(x, dtype=np.float64)
            if isinstance(c, LPCone) and x.shape != (c.n,):
                raise ValueError(f"LP cone of {c.n} columns: the primal is a 1-D array of {c.n} entries, not {x.shape}")
            self._psdp.append(x)
        self._psdp_arr = (C.POINTER(C.c_double) * len(self._psdp))(*[_dptr(x) for x in self._psdp])
        load_library().HKKTRegisterPSDP(self._k, C.cast(self._psdp_arr, C.c_void_p))

    def factorize(self):
        _check(load_library().HKKTFactorize(self._k), "HKKTFactorize")

    def solve(self, rhs, inplace=False):
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        if inplace:
            _check(load_library().HKKTSolve(self._k, _dptr(rhs), None), "HKKTSolve")
            return rhs
        sol = np.zeros_like(rhs)
        _check(load_library().HKKTSolve(self._k, _dptr(rhs), _dptr(sol)), "HKKTSolve")
        return sol

    def phase_a_eligible(self):
        return bool(load_library().HMiKKTPhaseAEligible(self._k))

    def phase_a(self, tau, y, rhs):
        """HMiKKTPhaseA: interior check + INFEASIBLE build + factorisation + the three solves in ONE launch (small rank-one
        blocks).  Returns (is_interior, logdet S, d1, d2, d3); the operator's host fields are filled as after build_up."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        d1, d2, d3 = (np.zeros(self.m) for _ in range(3))
        ok, ld = C.c_int(0), C.c_double(0.0)
        _check(load_library().HMiKKTPhaseA(self._k, float(tau), _dptr(y), _dptr(rhs), _dptr(d1), _dptr(d2), _dptr(d3),
                                           C.byref(ok), C.byref(ld)), "HMiKKTPhaseA")
        return bool(ok.value), ld.value, d1, d2, d3

    def regularize(self, reg):
        load_library().HKKTRegularize(self._k, float(reg))

    @property
    def lin_type(self):
        """kktM->LinType: DENSE_ITERATIVE until a factorisation fails, DENSE_INDEFINITE afterwards
        (HFpLinsysSwitchToIndefinite, linalg/hdsdp_linsolver.c:1827-1857)"""
        return _lin_type(self._k.contents.kktM)

    def export(self):
        m = self.m
        a, r, c = (np.zeros(m) for _ in range(3))
        s = [C.c_double(0.0) for _ in range(4)]
        load_library().HKKTExport(self._k, _dptr(a), _dptr(r), _dptr(c), C.byref(s[0]), C.byref(s[1]), C.byref(s[2]),
                                  C.byref(s[3]))
        return {"ASinv": a, "ASinvRdSinv": r, "ASinvCSinv": c, "CSinvCSinv": s[0].value, "CSinv": s[1].value,
                "CSinvRdSinv": s[2].value, "TraceSinv": s[3].value}

    @property
    def is_sparse(self):
        """isKKTSparse: the host Schur matrix is the aggregated-pattern CSC of interface/hdsdp_schur.c:46-139"""
        return bool(self._k.contents.isKKTSparse)

    def csc(self):
        """(kktMatBeg, kktMatIdx, kktMatElem) of a sparse operator as numpy views: lower triangle, column by column"""
        k = self._k.contents
        beg = np.ctypeslib.as_array(k.kktMatBeg, shape=(self.m + 1,))
        nnz = int(beg[self.m])
        return beg, np.ctypeslib.as_array(k.kktMatIdx, shape=(nnz,)), np.ctypeslib.as_array(k.kktMatElem, shape=(nnz,))

    @property
    def M(self):
        """kktMatElem as the reference leaves it: m x m column-major, lower triangle valid.
        Returned in numpy C-order, i.e. M[j, i] is element (row i, col j): valid where i >= j.
        For a sparse operator the CSC is expanded into such an array (a copy, not a view)."""
        k = self._k.contents
        if k.isKKTSparse:
            beg, idx, val = self.csc()
            D = np.zeros((self.m, self.m))
            for j in range(self.m):
                D[j, idx[beg[j]:beg[j + 1]]] = val[beg[j]:beg[j + 1]]
            return D
        return np.ctypeslib.as_array(k.kktMatElem, shape=(self.m, self.m))

    def rows(self, rows):
        """full symmetric rows of the DEVICE copy of M after a build (works with the host mirror off)"""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.zeros((rows.size, self.m))
        _check(load_library().HMiKKTGetRows(self._k, int(rows.size), _iptr(rows), _dptr(out)), "HMiKKTGetRows")
        return out

    def set_host_mirror(self, on):
        """HMiKKTSetHostMirror: 1 = the host copy of M is refreshed after every build; 0 = M stays on the device and kktDiag[]
        points into the diagonal channel (refused, with a stderr line, while a host cone sits in the operator)"""
        load_library().HMiKKTSetHostMirror(self._k, 1 if on else 0)

    def set_refine(self, max_steps):
        """HMiKKTSetRefine: HKKTSolve iterates on the true residual, at most max_steps corrections (0: off, the default; clamped
        to 8).  Turn it on before factorize(): the residual reads the matrix the factor was made from."""
        _check(load_library().HMiKKTSetRefine(self._k, int(max_steps)), "HMiKKTSetRefine")

    def set_refine_tiles(self, on):
        """HMiKKTSetRefineTiles: the tile form's own switch on top of set_refine's cap -- a tile operator is refined only with
        both on before factorize(); off (the default) it answers NOT_AVAILABLE and holds no memory"""
        _check(load_library().HMiKKTSetRefineTiles(self._k, 1 if on else 0), "HMiKKTSetRefineTiles")

    def refine_tiles(self):
        """HMiLinsysGetRefineTiles of the operator's linear system"""
        return bool(load_library().HMiLinsysGetRefineTiles(self._k.contents.kktM))

    def set_param(self, relTol=0.0, absTol=0.0, maxIter=-1):
        """HFpLinsysSetParam on the operator's linear system (HKKTInit sets 5e-12 / 1e-12 for m <= 5000): the refined solve's
        tolerances"""
        load_library().HFpLinsysSetParam(self._k.contents.kktM, float(relTol), float(absTol), -1, int(maxIter), -1)

    def refine_stats(self):
        """the operator's linear system: dict(cap, status, status_name, steps, resid0, resid, tol, solves, total_steps, device_bytes)
        of the last solve and the running totals"""
        return _refine_stats(self._k.contents.kktM)

    def set_grouped_build(self, on):
        """HMiKKTSetGroupedBuild: all eligible small SDP cones of the operator are built in one pass of three launches
        (csrc/grouped_plan.h has the rule); returns the number of cones that will be grouped (0: off, or fewer than two eligible)"""
        return int(load_library().HMiKKTSetGroupedBuild(self._k, 1 if on else 0))

    def grouped_build_info(self):
        """HMiKKTGetGroupedBuild: dict(cones, jobs, launches) of the last build's grouped pass (all 0: it did not run)"""
        c, j, l = C.c_int(0), C.c_int(0), C.c_int(0)
        load_library().HMiKKTGetGroupedBuild(self._k, C.byref(c), C.byref(j), C.byref(l))
        return {"cones": c.value, "jobs": j.value, "launches": l.value}

    def _set_grouped(self, kind, on):       # a question set's switch (kind: Check, Ratio, Step) ...
        return int(getattr(load_library(), f"HMiKKTSetGrouped{kind}")(self._k, 1 if on else 0))

    def _grouped_info(self, kind, *own):    # ... and its Get call: on, the counters every kind has, the kind's `own`
        out = (C.c_long * (4 + len(own)))()
        on = getattr(load_library(), f"HMiKKTGetGrouped{kind}")(self._k, out)
        return {"on": bool(on), **dict(zip(("members", "launches", "last_cones", "total_cones") + own, out))}

    def set_grouped_check(self, on):
        """HMiKKTSetGroupedCheck: a point question (check_is_interior, log_barrier with y) put to one member of the operator's
        check set puts every member at that point in one launch (csrc/small_check_rule.h has the rule); returns the number of
        members (0: off, or fewer than two members)"""
        return self._set_grouped("Check", on)

    def grouped_check_info(self):
        """HMiKKTGetGroupedCheck: dict(on, members, launches, last_cones, total_cones, from_state, left_out)"""
        return self._grouped_info("Check", "from_state", "left_out")

    def check_is_interior(self, tau, y):
        """HMiKKTCheckIsInterior: every cone of the operator at (tau, y), in order and without early exit; returns
        (flags, logdets, all): logdets[k] is NaN where flags[k] is False"""
        y = np.ascontiguousarray(y, dtype=np.float64)
        n = len(self.cones)
        flags = np.zeros(n, dtype=np.int32)
        logdets = np.full(n, np.nan)
        every = C.c_int(0)
        _check(load_library().HMiKKTCheckIsInterior(self._k, float(tau), _dptr(y), _iptr(flags), _dptr(logdets), C.byref(every)),
               "HMiKKTCheckIsInterior")
        return flags.astype(bool), logdets, bool(every.value)

    def set_grouped_ratio(self, on):
        """HMiKKTSetGroupedRatio: a ratio test on the dual buffer asked of one member of the operator's ratio set runs every
        member's test in one pair of launches (csrc/small_ratio_rule.h has the rule); the later calls fetch their answers.
        Returns the number of members (0: off, or fewer than two members)"""
        return self._set_grouped("Ratio", on)

    def grouped_ratio_info(self):
        """HMiKKTGetGroupedRatio: dict(on, members, launches, last_cones, total_cones, from_slots, left_out, fallbacks)"""
        return self._grouped_info("Ratio", "from_slots", "left_out", "fallbacks")

    def set_grouped_ratio_checker(self, on):
        """HMiKKTSetGroupedRatioChecker: while the grouped ratio test is on, the set also answers a ratio test on
        BUFFER_DUALCHECK.  Returns the number of members when the opt-in is on afterwards, else 0"""
        return int(load_library().HMiKKTSetGroupedRatioChecker(self._k, 1 if on else 0))

    def set_grouped_ratio_rest(self, on):
        """HMiKKTSetGroupedRatioRest: while the grouped ratio test is on, the rest of the safeguard (fresh-start test and cuts)
        of a member whose step left the cone runs in the grouped launch, not on the host.  Returns the number of members when
        the opt-in is on afterwards, else 0"""
        return int(load_library().HMiKKTSetGroupedRatioRest(self._k, 1 if on else 0))

    def grouped_ratio_detail(self):
        """HMiKKTGetGroupedRatioDetail: dict(on, checker, rest, checker_launches, device_rests, device_cuts, fallbacks)"""
        out = (C.c_long * 6)()
        on = int(load_library().HMiKKTGetGroupedRatioDetail(self._k, out))
        return dict(on=bool(on), checker=bool(out[0]), rest=bool(out[1]), checker_launches=int(out[2]), device_rests=int(out[3]),
                    device_cuts=int(out[4]), fallbacks=int(out[5]))

    def ratio_test(self, dtau_step, dy, ada_ratio=0.0, buffer=BUFFER_DUALVAR):
        """HMiKKTRatioTest: every cone of the operator along (dtau_step, dy), in order and without early exit; returns
        (steps, min_step): steps[k] is NaN where cone k's slot failed"""
        dy = np.ascontiguousarray(dy, dtype=np.float64)
        steps = np.full(len(self.cones), np.nan)
        mn = C.c_double(0.0)
        _check(load_library().HMiKKTRatioTest(self._k, float(dtau_step), _dptr(dy), float(ada_ratio), buffer, _dptr(steps),
                                              C.byref(mn)), "HMiKKTRatioTest")
        return steps, mn.value

    def set_grouped_step(self, on):
        """HMiKKTSetGroupedStep: a step-and-check on the checker buffer asked of one member of the operator's step set puts
        every member's checker at S + step dS in one launch (csrc/small_step_rule.h has the rule); the later calls answer from
        their slots.  Returns the number of members (0: off, or fewer than two members)"""
        return self._set_grouped("Step", on)

    def grouped_step_info(self):
        """HMiKKTGetGroupedStep: dict(on, members, launches, last_cones, total_cones, from_slots, left_out)"""
        return self._grouped_info("Step", "from_slots", "left_out")

    def axpy_buffer_and_check(self, step, buffer=BUFFER_DUALCHECK):
        """HMiKKTAddStepToBufferAndCheck: every cone of the operator at S + step dS, in order and without early exit; returns
        (flags, all, rc): flags[k] is False where cone k is outside or its slot failed, rc the first retcode that was not OK"""
        flags = np.zeros(len(self.cones), dtype=np.int32)
        every = C.c_int(0)
        rc = int(load_library().HMiKKTAddStepToBufferAndCheck(self._k, float(step), buffer, _iptr(flags), C.byref(every)))
        return flags.astype(bool), bool(every.value), rc

    def diag_target(self):
        """HMiKKTGetDiagTarget: 0 = kktDiag[] points into kktMatElem, 1 = into the diagonal channel"""
        return int(load_library().HMiKKTGetDiagTarget(self._k))

    def matrix_traffic(self):
        """HMiKKTGetMatrixTraffic: (bytes of M and channel to the host, to the device) since HKKTInit"""
        h, d = C.c_int64(0), C.c_int64(0)
        load_library().HMiKKTGetMatrixTraffic(self._k, C.byref(h), C.byref(d))
        return h.value, d.value

    def add_to_diag(self, v):
        """what the y-box cone does through kktDiag[] (interface/hdsdp_conic_bound.c:201-229)"""
        if self.is_sparse:
            beg, idx, val = self.csc()
            val[beg[:-1]] += v
            return
        M = self.M
        idx = np.arange(self.m)
        M[idx, idx] += v

    def envelope_info(self):
        """(permuted, fraction): is P M P' factored, and the share of 128-blocks inside the pattern's block envelope"""
        p, f = C.c_int(0), C.c_double(1.0)
        load_library().HMiKKTEnvelopeInfo(self._k, C.byref(p), C.byref(f))
        return bool(p.value), float(f.value)

    def tile_info(self):
        """None, or (tiles stored, tiles of the dense lower triangle, levels, bytes) of a sparse operator kept in tile form"""
        t, lv = C.c_int(0), C.c_int(0)
        dt, by = C.c_int64(0), C.c_int64(0)
        if not load_library().HMiKKTTileInfo(self._k, C.byref(t), C.byref(dt), C.byref(lv), C.byref(by)):
            return None
        return t.value, dt.value, lv.value, by.value

    def negative_pivots(self):
        """negative pivots of the tile-form operator's last LDL' factorisation (-1: not tile form / not factored)"""
        return int(load_library().HMiKKTNegativePivots(self._k))

    def stage_times_ms(self):
        t = np.zeros(8)
        load_library().HMiGetStageTimes(_dptr(t), 8)
        return t

    def destroy(self):
        if self._k:
            load_library().HKKTDestroy(C.byref(self._k))
            self._k = None


class LinSys:
    """hdsdp_linsys_fp, dense direct backend (linalg/hdsdp_linsolver.c:1044-1286)."""

    def __init__(self, n, ltype=HDSDP_LINSYS_DENSE_DIRECT):
        self.n = n
        self._h = C.c_void_p()
        _check(load_library().HFpLinsysCreate(C.byref(self._h), n, ltype), "HFpLinsysCreate")

    def numeric(self, A):
        A = np.ascontiguousarray(A, dtype=np.float64)
        _check(load_library().HFpLinsysNumeric(self._h, None, None, _dptr(A)), "HFpLinsysNumeric")

    @property
    def lin_type(self):
        return _lin_type(self._h)

    def symbolic(self, beg, idx):
        """HFpLinsysSymbolic: the lower-triangular CSC pattern of a SPARSE_DIRECT object"""
        self._beg = np.ascontiguousarray(beg, dtype=np.int32)
        self._idx = np.ascontiguousarray(idx, dtype=np.int32)
        _check(load_library().HFpLinsysSymbolic(self._h, _iptr(self._beg), _iptr(self._idx)), "HFpLinsysSymbolic")

    def psd_check_csc(self, val):
        val = np.ascontiguousarray(val, dtype=np.float64)
        ok = C.c_int(0)
        _check(load_library().HFpLinsysPsdCheck(self._h, _iptr(self._beg), _iptr(self._idx), _dptr(val), C.byref(ok)),
               "HFpLinsysPsdCheck")
        return bool(ok.value)

    def psd_check(self, A):
        A = np.ascontiguousarray(A, dtype=np.float64)
        ok = C.c_int(0)
        _check(load_library().HFpLinsysPsdCheck(self._h, None, None, _dptr(A), C.byref(ok)), "HFpLinsysPsdCheck")
        return bool(ok.value)

    def get_diag(self):
        d = np.zeros(self.n)
        _check(load_library().HFpLinsysGetDiag(self._h, _dptr(d)), "HFpLinsysGetDiag")
        return d

    def _rhs(self, rhs):
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        nrhs = 1 if rhs.ndim == 1 else rhs.shape[0]  # C-order (nrhs, n) == column-major n x nrhs
        return rhs, nrhs

    def solve(self, rhs, inplace=False):
        rhs, nrhs = self._rhs(rhs)
        if inplace:                  # solVec == NULL: the solution replaces the right-hand side
            _check(load_library().HFpLinsysSolve(self._h, nrhs, _dptr(rhs), None), "HFpLinsysSolve")
            return rhs
        sol = np.zeros_like(rhs)
        _check(load_library().HFpLinsysSolve(self._h, nrhs, _dptr(rhs), _dptr(sol)), "HFpLinsysSolve")
        return sol

    def set_param(self, relTol=0.0, absTol=0.0, maxIter=-1):
        """HFpLinsysSetParam: the tolerances of the refined solve (values <= 0: the reference's 1e-6)"""
        load_library().HFpLinsysSetParam(self._h, float(relTol), float(absTol), -1, int(maxIter), -1)

    def set_refine(self, max_steps):
        """HMiLinsysSetRefine: solve() iterates on the true residual, at most max_steps corrections (0: off, the default; clamped
        to 8).  Turn it on before numeric(): the residual reads a device copy of the matrix taken then."""
        _check(load_library().HMiLinsysSetRefine(self._h, int(max_steps)), "HMiLinsysSetRefine")

    def refine_stats(self):
        """dict(cap, status, status_name, steps, resid0, resid, tol, solves, total_steps, device_bytes) of the last solve and the
        running totals"""
        return _refine_stats(self._h)

    def fsolve(self, rhs):
        rhs, nrhs = self._rhs(rhs)
        sol = np.zeros_like(rhs)
        load_library().HFpLinsysFSolve(self._h, nrhs, _dptr(rhs), _dptr(sol))
        return sol

    def bsolve(self, rhs):
        rhs, nrhs = self._rhs(rhs)
        sol = np.zeros_like(rhs)
        load_library().HFpLinsysBSolve(self._h, nrhs, _dptr(rhs), _dptr(sol))
        return sol

    def invert(self):
        out = np.zeros((self.n, self.n))
        aux = np.zeros(1)
        load_library().HFpLinsysInvert(self._h, _dptr(out), _dptr(aux))
        return out

    def destroy(self):
        if self._h:
            load_library().HFpLinsysDestroy(C.byref(self._h))
            self._h = None
