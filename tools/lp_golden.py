"""LP-cone fixtures: tests/golden/lp_<case>.npz from the reference's own LP cone (interface/hdsdp_conic_lp.c), driven through
ctypes in the compiled reference library (oracle/_ref/libhdsdp_ref.so, made by `make -C oracle ref`).

    python tools/lp_golden.py            # writes tests/golden/lp_{small,bounds,wide,mixed}.npz
    python tools/lp_golden.py --check    # regenerates in memory and compares with the committed files

The inputs are not stored: `make_case(name)` generates them from fixed formulas (numpy only), and the tests call it too.  A
fixture holds what the reference computed at the case's state: every KKT type's Schur matrix (lower triangle), vectors and
scalars, and the values of the remaining slots (for the wide case a fixed sample of M's rows and of the nCol-long arrays).
The mixed case adds theta1's SDP block as a second cone of the same operator.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libhdsdp_ref.so")
CASES = ("small", "bounds", "wide", "mixed")
CONE_LP, CONE_DENSE_SDP = 1, 4
KKT_TYPES = (0, 1, 2, 3)   # INFEASIBLE, CORRECTOR, HOMOGENEOUS, PRIMAL


def _csc_from_columns(m, n, rows_of_col, vals_of_col, obj):
    """LPConeProcDataImpl's input: CSC of n rows (LP columns) and m + 1 columns (constraints), column 0 = the objective"""
    trip = [[] for _ in range(m + 1)]
    for j in range(n):
        if obj[j] != 0.0:
            trip[0].append((j, obj[j]))
        for i, v in zip(rows_of_col[j], vals_of_col[j]):
            trip[i + 1].append((j, v))
    beg = np.zeros(m + 2, dtype=np.int32)
    for c in range(m + 1):
        beg[c + 1] = beg[c] + len(trip[c])
    idx = np.array([j for t in trip for j, _ in t], dtype=np.int32)
    val = np.array([v for t in trip for _, v in t], dtype=np.float64)
    return beg, idx, val


def make_case(name):
    """dict(m, n, beg, idx, val, y, Rd, tau, dy, X, sdp=None|theta1 name): data and one interior state"""
    rng = np.random.default_rng({"small": 11, "bounds": 12, "wide": 13, "mixed": 14}[name])
    if name == "small":
        m, n = 40, 300
        rows = [np.arange(m)] * n
        vals = [rng.uniform(-1.0, 1.0, m) for _ in range(n)]
    elif name == "bounds":      # l <= y <= u: +e_i (u_i) for the first m columns, -e_i (-l_i) for the next m
        m = 60
        n = 2 * m
        rows = [np.array([j % m]) for j in range(n)]
        vals = [np.array([1.0 if j < m else -1.0]) for j in range(n)]
    elif name == "wide":
        m, n = 500, 20000
        rows = [np.sort(rng.choice(m, size=10, replace=False)) for _ in range(n)]
        vals = [rng.uniform(-1.0, 1.0, 10) for _ in range(n)]
    elif name == "mixed":       # theta1's constraints plus 150 LP columns of 12 entries each
        g = np.load(os.path.join(GOLDEN, "theta1_A.npz"))
        m, n = int(g["dims"][1]), 150
        rows = [np.sort(rng.choice(m, size=12, replace=False)) for _ in range(n)]
        vals = [rng.uniform(-1.0, 1.0, 12) for _ in range(n)]
    else:
        raise ValueError(name)
    absum = np.array([np.abs(v).sum() for v in vals])
    obj = 0.5 * absum + 1.0 + rng.uniform(0.0, 1.0, n)    # s = c - A^T y > 0 for |y_i| <= 0.5
    beg, idx, val = _csc_from_columns(m, n, rows, vals, obj)
    y = 0.3 * np.sin(1.7 * np.arange(1, m + 1))
    dy = 0.8 * np.cos(0.9 * np.arange(1, m + 1))
    X = 0.5 + 0.25 * np.cos(0.3 * np.arange(n))
    Rd, tau = -20.0, 0.9
    if name == "mixed":         # theta1's block is interior at a smaller y (the state __graft_entry__.smoke uses)
        y, Rd, tau = 0.05 * np.sin(1.7 * np.arange(1, m + 1)), -60.0, 0.8
    return {"m": m, "n": n, "beg": beg, "idx": idx, "val": val, "y": y, "dy": dy, "X": X, "Rd": Rd, "tau": tau,
            "sdp": "theta1" if name == "mixed" else None}


class hdsdp_kkt(C.Structure):   # interface/def_hdsdp_schur.h:32-68
    _fields_ = [("nRow", C.c_int), ("nCones", C.c_int), ("maxConeDim", C.c_int), ("cones", C.c_void_p),
                ("isKKTSparse", C.c_int), ("kktM", C.c_void_p), ("invBuffer", C.c_void_p), ("kktBuffer", C.c_void_p),
                ("kktBuffer2", C.c_void_p), ("kktMatBeg", C.c_void_p), ("kktMatIdx", C.c_void_p),
                ("kktMatElem", C.POINTER(C.c_double)), ("kktDiag", C.c_void_p), ("dASinvVec", C.POINTER(C.c_double)),
                ("dASinvCSinvVec", C.POINTER(C.c_double)), ("dASinvRdSinvVec", C.POINTER(C.c_double)),
                ("dCSinvCSinv", C.c_double), ("dCSinvRdSinv", C.c_double), ("dCSinv", C.c_double), ("dTraceSinv", C.c_double),
                ("dPrimalX", C.c_void_p)]


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class _Ref:
    def __init__(self, path=REF_LIB):
        self.lib = C.CDLL(path, mode=C.RTLD_GLOBAL)   # (MKL loads its CPU-specific kernels against the core library's symbols)
        vp = C.c_void_p
        L = self.lib
        for name, res in (("HConeGetCoeffNorm", C.c_double), ("HConeGetObjNorm", C.c_double), ("HConeComputeXDotS", C.c_double),
                          ("HConeComputeTraceCX", C.c_double)):
            getattr(L, name).restype = res
        L.HConeSetStart.argtypes = [vp, C.c_double]
        L.HConeReduceResi.argtypes = [vp, C.c_double]
        L.HConeSetPerturb.argtypes = [vp, C.c_double]
        L.HConeScalByConstant.argtypes = [vp, C.c_double]
        L.HConeGetCoeffNorm.argtypes = [vp, C.c_int]
        L.HConeGetObjNorm.argtypes = [vp, C.c_int]
        L.HConeCheckIsInterior.argtypes = [vp, C.c_double, vp, vp]
        L.HConeCheckIsInteriorExpert.argtypes = [vp, C.c_double, C.c_double, vp, C.c_double, C.c_int, vp]
        L.HConeRatioTest.argtypes = [vp, C.c_double, vp, C.c_double, C.c_int, vp]
        L.HConeGetLogBarrier.argtypes = [vp, C.c_double, vp, C.c_int, vp]
        L.HConeAddStepToBufferAndCheck.argtypes = [vp, C.c_double, C.c_int, vp]
        L.HConeGetPrimal.argtypes = [vp, C.c_double, vp, vp, vp, vp]
        L.HConeBuildPrimalXSXDirection.argtypes = [vp, vp, vp, vp, C.c_int]
        L.HUserDataSetConeData.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
        L.HKKTInit.argtypes = [vp, C.c_int, C.c_int, vp]
        L.HKKTBuildUp.argtypes = [vp, C.c_int]
        L.HKKTSolve.argtypes = [vp, vp, vp]
        L.HKKTRegisterPSDP.argtypes = [vp, vp]
        self._keep = []

    def cone(self, kind, m, ncol, beg, idx, val, iCone):
        L = self.lib
        beg, idx, val = (np.ascontiguousarray(beg, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32),
                         np.ascontiguousarray(val, dtype=np.float64))
        self._keep += [beg, idx, val]
        ud, h = C.c_void_p(), C.c_void_p()
        assert L.HUserDataCreate(C.byref(ud)) == 0
        L.HUserDataSetConeData(ud, kind, m, ncol, beg.ctypes.data, idx.ctypes.data, val.ctypes.data)
        assert L.HConeCreate(C.byref(h), iCone) == 0
        assert L.HConeSetData(h, ud) == 0 and L.HConeProcData(h) == 0 and L.HConePresolveData(h) == 0
        self._keep.append(ud)
        return h


def reference_outputs(name, lib_path=REF_LIB):
    """everything the fixture holds, computed by the reference library"""
    cs = make_case(name)
    m, n, y, dy, Rd, tau = cs["m"], cs["n"], cs["y"], cs["dy"], cs["Rd"], cs["tau"]
    R = _Ref(lib_path)
    L = R.lib
    cones = []
    if cs["sdp"]:
        g = np.load(os.path.join(GOLDEN, cs["sdp"] + "_A.npz"))
        cones.append(R.cone(CONE_DENSE_SDP, m, int(g["dims"][0]), g["csc_beg"], g["csc_idx"], g["csc_val"], 0))
    lp = R.cone(CONE_LP, m, n, cs["beg"], cs["idx"], cs["val"], len(cones))
    cones.append(lp)
    out = {}
    ok = C.c_int(0)
    for h in cones:
        L.HConeSetStart(h, Rd)
        assert L.HConeCheckIsInterior(h, tau, _d(y), C.byref(ok)) == 0 and ok.value == 1, name
    kkt = C.POINTER(hdsdp_kkt)()
    assert L.HKKTCreate(C.byref(kkt)) == 0
    arr = (C.c_void_p * len(cones))(*[h.value for h in cones])
    assert L.HKKTInit(kkt, m, len(cones), arr) == 0
    k = kkt.contents
    X = np.ascontiguousarray(cs["X"])
    px = (C.POINTER(C.c_double) * 1)(_d(X))      # (KKT_TYPE_PRIMAL is built for the LP cone alone: it is cone 0)
    tril = np.tril_indices(m)
    for t in (KKT_TYPES if not cs["sdp"] else (0,)):
        if t == 3:
            L.HKKTRegisterPSDP(kkt, C.cast(px, C.c_void_p))
        assert L.HKKTBuildUp(kkt, t) == 0, (name, t)
        Mt = np.ctypeslib.as_array(k.kktMatElem, shape=(m, m)).copy()   # C order: Mt[j, i] = element (i, j)
        if t != 1 and not (name == "wide" and t != 0):
            out[f"M{t}"] = Mt.T[tril]          # lower triangle, row-major over (i >= j)
        out[f"ASinv{t}"] = np.ctypeslib.as_array(k.dASinvVec, shape=(m,)).copy()
        out[f"ASinvRdSinv{t}"] = np.ctypeslib.as_array(k.dASinvRdSinvVec, shape=(m,)).copy()
        if t == 2:
            out["ASinvCSinv2"] = np.ctypeslib.as_array(k.dASinvCSinvVec, shape=(m,)).copy()
            out["CSinv2"], out["CSinvCSinv2"] = np.array(k.dCSinv), np.array(k.dCSinvCSinv)
        out[f"TraceSinv{t}"] = np.array(k.dTraceSinv)
    if cs["sdp"]:
        # the operator's solve of one right-hand side after the INFEASIBLE build (the reference factors and solves its own M)
        L.HKKTBuildUp(kkt, 0)
        rhs = np.cos(0.37 * np.arange(m)) + 2.0
        sol = np.zeros(m)
        assert L.HKKTFactorize(kkt) == 0
        assert L.HKKTSolve(kkt, _d(rhs), _d(sol)) == 0
        out["rhs"], out["sol"] = rhs, sol
        return out
    # the remaining slots of the LP cone, in this order (the tests replay it)
    s = C.c_double(0.0)
    L.HConeGetLogBarrier(lp, tau, _d(y), 0, C.byref(s))
    out["barrier"] = np.array(s.value)
    out["dual"] = np.zeros(n)
    L.HConeGetDual(lp, _d(out["dual"]), None)
    L.HConeRatioTest(lp, 0.0, _d(np.zeros(m)), 0.0, 0, C.byref(s))
    out["ratio_none"] = np.array(s.value)
    L.HConeRatioTest(lp, 0.1, _d(dy), 0.5, 0, C.byref(s))
    out["ratio_var"] = np.array(s.value)
    L.HConeAddStepToBufferAndCheck(lp, 0.5 * out["ratio_var"].item(), 1, C.byref(ok))
    out["axpy_chk"] = np.array(ok.value)
    L.HConeGetLogBarrier(lp, 0.0, None, 1, C.byref(s))
    out["barrier_chk"] = np.array(s.value)
    L.HConeRatioTest(lp, 0.1, _d(dy), 0.5, 1, C.byref(s))
    out["ratio_chk"] = np.array(s.value)
    L.HConeAddStepToBufferAndCheck(lp, 3.0 * out["ratio_chk"].item(), 1, C.byref(ok))   # (well past the boundary)
    out["axpy_chk_far"] = np.array(ok.value)
    L.HConeSetPerturb(lp, 0.25)
    L.HConeCheckIsInteriorExpert(lp, 1.0, -1.0, _d(y), -Rd, 1, C.byref(ok))
    out["expert_chk"] = np.array(ok.value)
    L.HConeGetLogBarrier(lp, 0.0, None, 1, C.byref(s))
    out["barrier_expert"] = np.array(s.value)
    L.HConeCheckIsInteriorExpert(lp, 1.0, -1.0, _d(40.0 * np.ones(m)), 0.0, 0, C.byref(ok))
    out["expert_var_far"] = np.array(ok.value)
    L.HConeSetPerturb(lp, 0.0)
    L.HConeCheckIsInterior(lp, tau, _d(y), C.byref(ok))
    out["interior"] = np.array(ok.value)
    L.HConeAddStepToBufferAndCheck(lp, 0.5 * out["ratio_var"].item(), 0, C.byref(ok))
    out["axpy_var"] = np.array(ok.value)
    out["dual_after_step"] = np.zeros(n)
    L.HConeGetDual(lp, _d(out["dual_after_step"]), None)
    xsx = np.zeros(n)
    L.HConeBuildPrimalXSXDirection(lp, None, _d(cs["X"]), _d(xsx), 1)
    out["xsx_dual"] = xsx.copy()
    L.HConeBuildPrimalXSXDirection(lp, None, _d(cs["X"]), _d(xsx), 0)
    out["xsx_step"] = xsx.copy()
    prim = np.zeros(n)
    L.HConeGetPrimal(lp, 0.7, _d(y), _d(dy), _d(prim), None)
    out["primal"] = prim
    out["xdots"] = np.array(L.HConeComputeXDotS(lp, _d(cs["X"])))
    out["tracecx"] = np.array(L.HConeComputeTraceCX(lp, _d(cs["X"])))
    ax = np.ones(m)
    L.HConeComputeATimesXpy(lp, _d(cs["X"]), _d(ax))
    out["atimesx"] = ax
    out["norms"] = np.array([L.HConeGetCoeffNorm(lp, 1), L.HConeGetCoeffNorm(lp, 2), L.HConeGetObjNorm(lp, 1), L.HConeGetObjNorm(lp, 2)])
    fi, fd = np.zeros(20, dtype=np.int32), np.zeros(20)
    L.HConeDetectFeature(lp, _d(np.ones(m)), fi.ctypes.data_as(C.POINTER(C.c_int)), _d(fd))
    out["feat_int"], out["feat_dbl"] = fi, fd
    L.HConeScalByConstant(lp, 3.0)
    out["obj_norm_scaled"] = np.array(L.HConeGetObjNorm(lp, 2))
    return _sampled(out, m, n) if name == "wide" else out


def _sampled(out, m, n):
    """the wide case keeps a fixed sample, so that its fixture stays small: 16 full (symmetric) rows of M and every 40th entry
    of the nCol-long arrays (the tests compare on the same sample and check the whole M against numpy besides)"""
    rows = np.arange(0, m, m // 16)[:16]
    cols = np.arange(0, n, 40)
    res = {"M0_rows_idx": rows, "col_sample": cols}
    for k, v in out.items():
        if k == "M0":
            L = np.zeros((m, m))
            L[np.tril_indices(m)] = v                  # element (i, j), i >= j
            res["M0_rows"] = (L + np.tril(L, -1).T)[rows]
        elif v.ndim == 1 and v.shape[0] == n:
            res[k] = v[cols]
        else:
            res[k] = v
    return res


def main():
    check = "--check" in sys.argv
    bad = 0
    for name in CASES:
        out = reference_outputs(name)
        path = os.path.join(GOLDEN, f"lp_{name}.npz")
        if check:
            g = np.load(path)
            same = sorted(g.files) == sorted(out) and all(np.array_equal(g[k], out[k]) for k in out)
            print(f"{path}: {'same' if same else 'DIFFERS'}")
            bad += not same
        else:
            np.savez_compressed(path, **out)
            print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    return bad


if __name__ == "__main__":
    sys.exit(main())
