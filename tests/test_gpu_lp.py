"""The LP cone on the MI355X (csrc/engine_lp.h) against the reference's own LP cone (interface/hdsdp_conic_lp.c): the fixtures
tests/golden/lp_*.npz hold what the compiled reference computed at each case's state (tools/lp_golden.py makes them; the inputs
are regenerated here from the same formulas)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
from tools.lp_golden import make_case  # noqa: E402

CASES = ["small", "bounds", "wide"]
_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = (make_case(name), np.load(os.path.join(GOLDEN, f"lp_{name}.npz")))
    return _cases[name]


def _rel(a, r):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    den = np.max(np.abs(r)) if r.size else 0.0
    return float(np.max(np.abs(a - r)) / den) if den > 0 else float(np.max(np.abs(a - r), initial=0.0))


def _cone(cs, path=0, iCone=0):
    from hdsdp_amd import api
    c = api.LPCone.from_csc(cs["m"], cs["n"], cs["beg"], cs["idx"], cs["val"], iCone=iCone)
    if path:
        c.set_schur_path(path)
    assert c.schur_path()[0] in (1, 2)
    return c


def _lower(kkt, m):
    return kkt.M.T[np.tril_indices(m)]


def _full(kkt, m):
    """the operator's host matrix as a full symmetric array (only its lower triangle is kept)"""
    L = np.tril(kkt.M.T)
    return L + np.tril(L, -1).T


def _sample(g, name, v, n):
    """the wide fixture holds every 40th entry of the nCol-long arrays (tools/lp_golden.py: _sampled)"""
    if "col_sample" in g.files and np.ndim(v) == 1 and len(v) == n:
        return np.asarray(v)[g["col_sample"]]
    return v


def _dense_A(cs):
    A = np.zeros((cs["m"], cs["n"]))
    beg, idx, val = cs["beg"], cs["idx"], cs["val"]
    for i in range(cs["m"]):
        A[i, idx[beg[i + 1]:beg[i + 2]]] = val[beg[i + 1]:beg[i + 2]]
    return A


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("name", CASES)
def test_every_kkt_type_matches_the_reference(name, path):
    from hdsdp_amd import api
    cs, g = _case(name)
    m = cs["m"]
    cone = _cone(cs, path)
    cone.set_start(cs["Rd"])
    assert cone.check_is_interior(cs["tau"], cs["y"])
    kkt = api.KKT(m, [cone])
    try:
        for t in (0, 1, 2, 3):
            if t == 3:
                kkt.register_psdp([cs["X"]])
            kkt.build_up(t)
            ex = kkt.export()
            if f"M{t}" in g.files:
                assert _rel(_lower(kkt, m), g[f"M{t}"]) < 1e-13, (name, path, t)
            if t == 0 and "M0_rows" in g.files:
                # the fixture's sample of M (full rows), and the whole M against numpy fp64 at the cone's own dual
                assert _rel(_full(kkt, m)[g["M0_rows_idx"]], g["M0_rows"]) < 1e-13, (name, path)
                A, s = _dense_A(cs), cone.get_dual()
                assert _rel(_lower(kkt, m), ((A / s ** 2) @ A.T)[np.tril_indices(m)]) < 1e-13, (name, path)
            assert _rel(ex["ASinv"], g[f"ASinv{t}"]) < 1e-13, (name, path, t)
            assert _rel(ex["ASinvRdSinv"], g[f"ASinvRdSinv{t}"]) < 1e-13, (name, path, t)
            assert _rel(ex["TraceSinv"], g[f"TraceSinv{t}"]) < 1e-12, (name, path, t)
            if t == 2:
                assert _rel(ex["ASinvCSinv"], g["ASinvCSinv2"]) < 1e-13
                assert _rel(ex["CSinv"], g["CSinv2"]) < 1e-12 and _rel(ex["CSinvCSinv"], g["CSinvCSinv2"]) < 1e-12
    finally:
        kkt.destroy()
        cone.destroy()


@pytest.mark.parametrize("name", CASES)
def test_remaining_slots_match_the_reference(name):
    """the generator's sequence of slot calls, replayed (each call sees the buffers the previous ones left)"""
    from hdsdp_amd import api
    cs, g = _case(name)
    m, n, y, dy, X, Rd, tau = cs["m"], cs["n"], cs["y"], cs["dy"], cs["X"], cs["Rd"], cs["tau"]
    V, K = api.BUFFER_DUALVAR, api.BUFFER_DUALCHECK
    c = _cone(cs)
    try:
        c.set_start(Rd)
        assert c.check_is_interior(tau, y)
        got = {"barrier": c.log_barrier(tau, y), "dual": c.get_dual()}
        got["ratio_none"] = c.ratio_test(0.0, np.zeros(m), 0.0, V)
        got["ratio_var"] = c.ratio_test(0.1, dy, 0.5, V)
        got["axpy_chk"] = c.axpy_buffer_and_check(0.5 * g["ratio_var"].item(), K)
        got["barrier_chk"] = c.log_barrier_of(K)
        got["ratio_chk"] = c.ratio_test(0.1, dy, 0.5, K)
        got["axpy_chk_far"] = c.axpy_buffer_and_check(3.0 * g["ratio_chk"].item(), K)
        c.set_perturb(0.25)
        got["expert_chk"] = c.check_is_interior_expert(1.0, -1.0, y, -Rd, K)
        got["barrier_expert"] = c.log_barrier_of(K)
        got["expert_var_far"] = c.check_is_interior_expert(1.0, -1.0, 40.0 * np.ones(m), 0.0, V)
        c.set_perturb(0.0)
        got["interior"] = c.check_is_interior(tau, y)
        got["axpy_var"] = c.axpy_buffer_and_check(0.5 * g["ratio_var"].item(), V)
        got["dual_after_step"] = c.get_dual()
        got["xsx_dual"] = c.build_primal_xsx(X, np.zeros(n), True).copy()
        got["xsx_step"] = c.build_primal_xsx(X, np.zeros(n), False).copy()
        got["primal"] = c.get_primal(0.7, y, dy)
        got["xdots"] = c.x_dot_s(X)
        got["tracecx"] = c.trace_cx(X)
        got["atimesx"] = c.a_times_x(X, np.ones(m))
        got["norms"] = [c.coeff_norm(1), c.coeff_norm(2), c.obj_norm(1), c.obj_norm(2)]
        got["feat_int"], got["feat_dbl"] = c.detect_feature(np.ones(m))
        c.scal_by_constant(3.0)
        got["obj_norm_scaled"] = c.obj_norm(2)
        assert got["ratio_none"] == 100.0                     # no component blocks
        for k, v in got.items():
            r = g[k]
            if v is not None:
                v = _sample(g, name, v, n)
            if r.dtype.kind in "iu" or k in ("axpy_chk", "axpy_chk_far", "expert_chk", "expert_var_far", "interior", "axpy_var"):
                assert np.array_equal(np.asarray(v, dtype=np.int64), r.astype(np.int64)), (name, k, v, r)
            else:
                assert v is not None and _rel(v, r) < 1e-13, (name, k)
        if name == "bounds":
            assert got["feat_int"][6] == 1                    # INT_FEATURE_I_IMPYBOUND
        # recovery point outside the cone: the reference's message, and no primal
        assert c.get_primal(0.7, 40.0 * np.ones(m), dy) is None
    finally:
        c.destroy()


@pytest.mark.parametrize("path", [1, 2])
def test_two_builds_are_bit_identical(path):
    from hdsdp_amd import api
    cs, _ = _case("wide")
    cone = _cone(cs, path)
    cone.set_start(cs["Rd"])
    assert cone.check_is_interior(cs["tau"], cs["y"])
    kkt = api.KKT(cs["m"], [cone])
    try:
        outs = []
        for _ in range(2):
            kkt.build_up(api.KKT_TYPE_HOMOGENEOUS)
            ex = kkt.export()
            outs.append((kkt.M.copy(), ex["ASinv"], ex["ASinvRdSinv"], ex["ASinvCSinv"], ex["CSinv"], ex["TraceSinv"]))
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
    finally:
        kkt.destroy()
        cone.destroy()


@pytest.mark.parametrize("name", CASES)
def test_dense_and_sparse_paths_agree(name):
    from hdsdp_amd import api
    cs, _ = _case(name)
    res = []
    for path in (1, 2):
        cone = _cone(cs, path)
        assert cone.schur_path()[0] == path
        cone.set_start(cs["Rd"])
        assert cone.check_is_interior(cs["tau"], cs["y"])
        kkt = api.KKT(cs["m"], [cone])
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        res.append(_lower(kkt, cs["m"]).copy())
        kkt.destroy()
        cone.destroy()
    assert _rel(res[0], res[1]) < 1e-13


def test_the_path_rule():
    from hdsdp_amd import api
    for name in CASES:
        cs, _ = _case(name)
        c = _cone(cs)
        p, td, tsp, nb = c.schur_path()
        assert p == (2 if tsp < td else 1), (name, p, td, tsp)
        if name == "bounds":
            assert p == 2 and nb < 1 << 20        # one entry per column: a pair list of a few KB
        c.destroy()
    # dense columns at m = 2000: the dense path, and a pair list beyond 1 GiB (128 columns: 2.6e8 terms) cannot be forced
    m = 2000
    c = api.LPCone.from_csc(m, *_dense_csc(np.ones((m, 128)), np.ones(128)))
    try:
        assert c.schur_path()[0] == 1 and c.schur_path()[3] > 1 << 30
        with pytest.raises(api.HDSDPError):
            c.set_schur_path(api.LPCone.SPARSE)
        assert c.schur_path()[0] == 1
    finally:
        c.destroy()


def test_sdp_only_accessors_refuse_an_lp_cone():
    from hdsdp_amd import api
    lib = api.load_library()
    cs, _ = _case("small")
    c = _cone(cs)
    h = c._h
    try:
        buf = np.zeros(max(cs["n"], cs["m"]) ** 2)
        assert lib.HMiConeGetDualMatrix(h, api._dptr(buf)) != 0
        assert lib.HMiConeGetTraces(h, api._dptr(buf)) != 0
        assert lib.HMiConeGetPath(h) == -1
        assert lib.HMiConeSweepInfo(h, None, None) == 0
        assert lib.HMiConeGetStreaming(h, None) == 0
        assert lib.HMiConeUseSweepCopy(h, 1) != 0
        assert lib.HMiConeGetBuildProfile(h, 0, None, 0) == -1
        assert lib.HMiConeGetExchangeBuffers(h, None, None, None) != 0
        assert lib.HMiConeSetExchangeBuffers(h, C.c_void_p(16), C.c_void_p(16)) != 0
        assert lib.HMiConeGetShardCount(h) == 1
        ty = np.full(cs["m"], -7, dtype=np.int32)
        lib.HMiConeGetPresolve(h, api._iptr(ty), None, None, None, None, None)
        assert (ty == -7).all()
        pieces, staged = C.c_int(5), C.c_int(5)
        lib.HMiConeGetExchangeStats(h, C.byref(pieces), C.byref(staged))
        assert pieces.value == 0 and staged.value == 0
        lib.HMiConeSetExchange(h, None, None, None)
        lib.HMiConeSetExchangePieces(h, None, None, 2)
        assert c.check_is_interior(cs["tau"], cs["y"])       # the cone is untouched by all of the above
    finally:
        c.destroy()
    sdp = _theta1()
    assert lib.HMiConeLPSetSchurPath(sdp._h, 1) != 0 and lib.HMiConeLPGetSchurPath(sdp._h, None, None, None) == -1
    sdp.destroy()


def test_register_psdp_takes_a_vector_for_an_lp_cone():
    from hdsdp_amd import api
    cs, _ = _case("small")
    c = _cone(cs)
    kkt = api.KKT(cs["m"], [c])
    try:
        with pytest.raises(ValueError):
            kkt.register_psdp([np.eye(cs["n"])])
        kkt.register_psdp([cs["X"]])
    finally:
        kkt.destroy()
        c.destroy()


def _theta1():
    from hdsdp_amd import api
    g = np.load(os.path.join(GOLDEN, "theta1_A.npz"))
    return api.SDPCone.from_csc(int(g["dims"][0]), int(g["dims"][1]), g["csc_beg"], g["csc_idx"], g["csc_val"])


def test_engine_sdp_and_lp_cones_in_one_operator_without_the_host_copy():
    """theta1 on the engine's SDP cone plus an engine LP cone: no host cone, so HMiKKTSetHostMirror(0) holds; M read from the
    device and the operator's solve equal the reference's HKKTBuildUp / HKKTSolve over its own two cones"""
    from hdsdp_amd import api
    cs, g = _case("mixed")
    m = cs["m"]
    sdp = _theta1()
    lp = _cone(cs, iCone=1)
    try:
        for c in (sdp, lp):
            c.set_start(cs["Rd"])
            assert c.check_is_interior(cs["tau"], cs["y"])
        kkt = api.KKT(m, [sdp, lp], host_mirror=False)
        assert not kkt.phase_a_eligible()
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        assert not np.any(kkt.M)                                    # the host matrix was never written: mirror off
        Mdev = kkt.rows(np.arange(m))
        assert _rel(Mdev[np.tril_indices(m)], g["M0"]) < 1e-13
        ex = kkt.export()
        assert _rel(ex["ASinv"], g["ASinv0"]) < 1e-12 and _rel(ex["ASinvRdSinv"], g["ASinvRdSinv0"]) < 1e-12
        assert _rel(ex["TraceSinv"], g["TraceSinv0"]) < 1e-12
        kkt.factorize()
        sol = kkt.solve(g["rhs"])
        assert _rel(sol, g["sol"]) < 1e-8                            # (the reference solves by PCG to its KKT accuracy)
        assert _rel(Mdev @ sol, g["rhs"]) < 1e-10
        kkt.destroy()
    finally:
        lp.destroy()
        sdp.destroy()


def test_lp_cone_is_refused_beside_a_device_group_cone():
    from hdsdp_amd import api
    cs, _ = _case("mixed")
    api.set_devices([0, 0], shard_min_dim=0)
    try:
        sdp = api.SDPCone.synthetic(96, cs["m"])          # (a dense block on the congruence + Gram path: sharded)
        assert sdp.shard_count() == 2
        lp = _cone(cs, iCone=1)
        with pytest.raises(api.HDSDPError):
            api.KKT(cs["m"], [sdp, lp])
        lp.destroy()
        sdp.destroy()
    finally:
        api.set_devices([0])


def _dense_csc(A, c):
    """LPConeProcDataImpl's CSC of a dense m x n constraint matrix A (row i = constraint i) and objective c"""
    m, n = A.shape
    beg = np.arange(m + 2, dtype=np.int64) * n
    assert beg[-1] < 2 ** 31
    idx = np.tile(np.arange(n, dtype=np.int32), m + 1)
    val = np.concatenate([c, A.ravel()])
    return n, beg.astype(np.int32), idx, val


def test_at_size_dense_against_numpy():
    """m = 2000, 2000 dense LP columns: the dense path's M against A diag(1/s^2) A^T in numpy fp64"""
    from hdsdp_amd import api
    lib = api.load_library()
    m = n = 2000
    rng = np.random.default_rng(21)
    A = rng.uniform(-1.0, 1.0, (m, n))
    c = 0.5 * np.abs(A).sum(axis=0) + 1.0 + rng.uniform(0, 1, n)
    y = 0.3 * np.sin(1.7 * np.arange(1, m + 1))
    Rd, tau = -20.0, 0.9
    cone = api.LPCone.from_csc(m, *_dense_csc(A, c))
    try:
        assert cone.schur_path()[0] == 1
        cone.set_start(Rd)
        assert cone.check_is_interior(tau, y)
        s = tau * c - A.T @ y - Rd
        assert _rel(cone.get_dual(), s) < 1e-13
        kkt = api.KKT(m, [cone])
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        Mref = (A / s ** 2) @ A.T
        tril = np.tril_indices(m)
        err = _rel(kkt.M.T[tril], Mref[tril])
        ex = kkt.export()
        assert err < 1e-13, err
        assert _rel(ex["ASinv"], A @ (1.0 / s)) < 1e-13
        assert _rel(ex["ASinvRdSinv"], A @ (Rd / s ** 2)) < 1e-13
        # timing of the build (the operator's host copy included) and the dense path's GEMM rate, for the record
        lib.HMiSetKernelTiming(1)
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        ms, fl, la = np.zeros(5), np.zeros(5), np.zeros(5, dtype=np.int64)
        lib.HMiGetKernelTiming(api._dptr(ms), api._dptr(fl), la.ctypes.data_as(C.POINTER(C.c_int64)))
        lib.HMiSetKernelTiming(0)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
            t.append(time.perf_counter() - t0)
        print(f"\nLP dense m={m} n={n}: HKKTBuildUp {1e3 * min(t):.3f} ms (min of 5), Gram-role GEMM {ms[3]:.3f} ms, "
              f"{fl[3] / (ms[3] * 1e-3) / 1e12 if ms[3] > 0 else 0.0:.1f} TFLOP/s, rel err {err:.2e}")
        kkt.destroy()
    finally:
        cone.destroy()
