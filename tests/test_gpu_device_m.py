"""The diagonal channel: the Schur matrix M stays on the device while host cones write its diagonal.

With the host mirror off, kktDiag[i] points into a pinned m-vector.  A host cone handed to HKKTBuildUpExtraCone -- the
reference driver's bound cone on y, interface/hdsdp_conic_bound.c:201-249 -- adds its diagonal terms there; the first
HKKTRegularize or HKKTFactorize after the build uploads the vector and adds it to the device matrix's diagonal.  Everything
the factorisation sees must be bit for bit what the host-mirror path factors, and no byte of M may travel to the host."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from util import load_golden, y_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "_ref", "sdpasolve_mi355x")


class HostCone(C.Structure):   # hdsdp_cone, interface/def_hdsdp_conic.h:60-100: 2 ints, 2 pointers, 30 slots
    _fields_ = [("iCone", C.c_int), ("cone", C.c_int), ("usrData", C.c_void_p), ("coneData", C.c_void_p),
                ("slots", C.c_void_p * 30)]


BUILD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int)


def _host_cone(fn):
    cone = HostCone()
    cone.iCone = 9
    cone.slots[11] = C.cast(fn, C.c_void_p)          # coneBuildSchur
    cone._keep = fn
    return cone


def bound_cone(y, lo, up):
    """a stand-in for the y-box cone lo <= y <= up (scalar bounds) at a known y: sBoundConeGetKKT
    (interface/hdsdp_conic_bound.c:201-249) step by step, with dualLower = y - lo and dualUpper = up - y"""
    from hdsdp_amd import api
    y = np.asarray(y, dtype=np.float64)
    li, ui = 1.0 / (y - lo), 1.0 / (up - y)

    @BUILD_FN
    def build(cone_data, icone, kkt_ptr, type_kkt):
        k = C.cast(kkt_ptr, C.POINTER(api.hdsdp_kkt)).contents
        if type_kkt == api.KKT_TYPE_PRIMAL:
            return 1
        for i in range(k.nRow):
            k.dASinvVec[i] -= li[i]
            k.dASinvVec[i] += ui[i]
        if type_kkt == api.KKT_TYPE_CORRECTOR:
            return 0
        for i in range(k.nRow):
            k.kktDiag[i][0] += li[i] * li[i] + ui[i] * ui[i]
        if type_kkt == api.KKT_TYPE_HOMOGENEOUS:
            for i in range(k.nRow):
                k.dCSinv += up * ui[i]
                s = ui[i] * ui[i]
                k.dASinvCSinvVec[i] += up * s
                k.dCSinvCSinv += up * up * s
                k.dCSinv -= lo * li[i]
                s = li[i] * li[i]
                k.dASinvCSinvVec[i] += lo * s
                k.dCSinvCSinv += lo * lo * s
        return 0
    return _host_cone(build)


def diag_cone(d):
    """a host cone that adds the vector d to diag(M) through kktDiag[] (nothing else)"""
    from hdsdp_amd import api
    d = np.asarray(d, dtype=np.float64)

    @BUILD_FN
    def build(cone_data, icone, kkt_ptr, type_kkt):
        if type_kkt == api.KKT_TYPE_CORRECTOR:
            return 0
        k = C.cast(kkt_ptr, C.POINTER(api.hdsdp_kkt)).contents
        for i in range(k.nRow):
            k.kktDiag[i][0] += d[i]
        return 0
    return _host_cone(build)


def extra(kkt, host, typ):
    from hdsdp_amd import api
    assert api.load_library().HKKTBuildUpExtraCone(kkt._k, C.cast(C.pointer(host), C.c_void_p), typ) == 0


def step(kkt, host, typ, regs, rhs):
    """build, the host cone, the regularisations, factorisation, three solves: everything the driver reads afterwards"""
    kkt.build_up(typ)
    if host is not None:
        extra(kkt, host, typ)
    for r in regs:
        kkt.regularize(r)
    kkt.factorize()
    ex = kkt.export()
    out = dict(ex)
    out["d1"] = kkt.solve(rhs)
    out["d2"] = kkt.solve(ex["ASinv"])
    out["d3"] = kkt.solve(ex["ASinvRdSinv"])
    return out


def assert_identical(a, b, what):
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (what, key, np.max(np.abs(np.asarray(a[key]) - np.asarray(b[key]))))


def dev_diag(kkt):
    """the device matrix's diagonal (what the factorisation was handed, channel and regularisation included)"""
    R = kkt.rows(np.arange(kkt.m))
    return np.diag(R).copy()


def host_diag(kkt):
    return np.diag(kkt.M).copy()


@pytest.fixture
def syn64():
    from hdsdp_amd import api
    g = load_golden("syn64")
    n, m = int(g["dims"][0]), int(g["dims"][1])
    cone = api.SDPCone.synthetic(n, m)
    cone.set_start(float(g["Rd"][0]))
    assert cone.check_is_interior(float(g["tau"][0]), y_of(g))
    yield cone, m, y_of(g)
    cone.destroy()


@pytest.mark.parametrize("typ", ["INFEASIBLE", "HOMOGENEOUS"])
def test_bound_cone_through_the_channel_is_bit_identical(syn64, typ):
    """syn64 + the bound-cone stand-in through ExtraCone, Regularize(1e-6), Factorize and three solves: mirror off == mirror
    on bit for bit, and with the mirror off only the channel's 8 m bytes cross the bus (before this, the diagonal was lost)"""
    from hdsdp_amd import api
    cone, m, y = syn64
    t = getattr(api, "KKT_TYPE_" + typ)
    assert np.all(np.abs(y) < 0.5)
    host = bound_cone(y, -1.0, 2.0)
    rhs = np.sin(np.arange(m) + 1.0)
    got = {}
    for mirror in (True, False):
        kkt = api.KKT(m, [cone], host_mirror=mirror)
        assert kkt.diag_target() == (0 if mirror else 1)
        got[mirror] = step(kkt, host, t, [1e-6], rhs)
        th, td = kkt.matrix_traffic()
        if mirror:
            assert (th, td) == (8 * m * m, 8 * m * m)
            Mon = kkt.M.copy()
        else:
            assert (th, td) == (0, 8 * m)
            # and a second build + factorisation costs the channel once more
            step(kkt, host, t, [1e-6], rhs)
            assert kkt.matrix_traffic() == (0, 16 * m)
        kkt.destroy()
    assert_identical(got[True], got[False], typ)
    full = np.triu(Mon) + np.triu(Mon, 1).T
    assert np.linalg.norm(full @ got[False]["d1"] - rhs) <= 1e-10 * np.linalg.norm(rhs)


def test_regularize_edge_cases_follow_the_host_rule(syn64):
    """HKKTRegularize on device M + channel (hdsdp_schur.c:348-373): a regularisation below 1e-14 is none; the minimum is
    taken over M_ii + channel_i; a second call adds on top, ((M_ii + c_i) + r1) + r2, exactly as the host mirror does"""
    from hdsdp_amd import api
    cone, m, y = syn64
    rhs = np.cos(np.arange(m))
    ref = api.KKT(m, [cone])
    ref.build_up(api.KKT_TYPE_INFEASIBLE)
    d0 = host_diag(ref)
    ref.destroy()
    c = 0.1 + 0.37 * np.abs(np.sin(3.1 * np.arange(m)))
    j = int(np.argmax(d0))
    c[j] = 1e-3 * d0.min() - d0[j]                            # the minimum of M_ii + c_i sits at j and comes from the channel
    host = diag_cone(c)
    for regs in ([1e-30], [1e-6], [1e-6, 1e-6], [1e-6, 0.5]):
        got, diag = {}, {}
        for mirror in (True, False):
            kkt = api.KKT(m, [cone], host_mirror=mirror)
            got[mirror] = step(kkt, host, api.KKT_TYPE_INFEASIBLE, regs, rhs)
            diag[mirror] = host_diag(kkt) if mirror else dev_diag(kkt)
            kkt.destroy()
        assert_identical(got[True], got[False], regs)
        assert np.array_equal(diag[True], diag[False]), regs
        base = d0 + c
        want = base.copy()
        for r in regs:
            rr = min(r * want.min(), 1e-5)
            want = want + (rr if rr >= 1e-14 else 0.0)
        assert np.array_equal(diag[False], want), regs
        if regs == [1e-30]:
            assert np.array_equal(diag[False], base)
        if regs == [1e-6]:
            rr = min(1e-6 * base[j], 1e-5)
            assert rr >= 1e-14 and base.min() == base[j] and np.array_equal(diag[False], base + rr)


def test_indefinite_fallback_factors_device_M_plus_channel(syn64, capfd):
    """a channel that makes M + diag(c) indefinite: the Cholesky fails and the pivoted solver takes over
    (lin_switch_indefinite / lin_factor_indef) -- on device M plus the channel, with the mirror-on solution"""
    from hdsdp_amd import api
    cone, m, y = syn64
    ref = api.KKT(m, [cone])
    ref.build_up(api.KKT_TYPE_INFEASIBLE)
    d0 = host_diag(ref)
    ref.destroy()
    c = np.zeros(m)
    c[[3, 17, 40]] = -2.0 * d0[[3, 17, 40]] - 1.0
    host = diag_cone(c)
    rhs = np.sin(0.3 * np.arange(m))
    got = {}
    for mirror in (True, False):
        kkt = api.KKT(m, [cone], host_mirror=mirror)
        got[mirror] = step(kkt, host, api.KKT_TYPE_INFEASIBLE, [], rhs)
        assert kkt.lin_type == api.HDSDP_LINSYS_DENSE_INDEFINITE
        if mirror:
            Mon = kkt.M.copy()
        else:
            assert kkt.matrix_traffic()[0] == 0
        # a second factorisation of the same build stays switched and reads the same matrix (the channel is added once)
        kkt.factorize()
        again = kkt.solve(rhs)
        assert np.array_equal(again, got[mirror]["d1"])
        kkt.destroy()
    assert "Switch to the pivoted" in capfd.readouterr().err
    assert_identical(got[True], got[False], "indefinite")
    full = np.triu(Mon) + np.triu(Mon, 1).T
    assert int(np.sum(np.linalg.eigvalsh(full) < 0)) >= 1
    assert np.linalg.norm(full @ got[False]["d1"] - rhs) <= 1e-9 * np.linalg.norm(rhs)


def test_tile_form_operator_keeps_M_on_the_device():
    """arrow128's sparse Schur operator in tile form (engine cones only): channel + Regularize + LDL' on the tile store
    == the host CSC path, bit for bit; with the mirror off nothing of M comes back"""
    from hdsdp_amd import api
    g = load_golden("arrow128_A")
    m = int(g["mb_dims"][1])
    Rd, tau, y = float(g["Rd"][0]), float(g["tau"][0]), y_of(g)
    prob = api.read_sdpa(os.path.join(ROOT, "tests", "golden", "arrow128.dat-s"))
    cones = [api.SDPCone.from_csc(blk["n"], m, blk["beg"], blk["idx"], blk["val"], iCone=k) for k, blk in enumerate(prob["blocks"])]
    try:
        for cn in cones:
            cn.set_start(Rd)
            assert cn.check_is_interior(tau, y)
        host = bound_cone(0.1 * np.sin(np.arange(m)), -3.0, 5.0)
        got = {}
        for mirror in (True, False):
            kkt = api.KKT(m, cones, host_mirror=mirror)
            assert kkt.is_sparse and kkt.tile_info() is not None
            assert kkt.diag_target() == (0 if mirror else 1)
            got[mirror] = step(kkt, host, api.KKT_TYPE_INFEASIBLE, [1e-6], g["b"])
            th, td = kkt.matrix_traffic()
            if not mirror:
                assert (th, td) == (0, 8 * m)
            else:
                assert th > 0 and td > 0
            kkt.destroy()
        assert_identical(got[True], got[False], "tiles")
    finally:
        for cn in cones:
            cn.destroy()


def test_device_group_operator_keeps_M_on_the_device():
    """a loopback device group (two shards on device 0, HMiSetShardMinDim(0)): M assembled on ids[0], the channel added
    there; INFEASIBLE and HOMOGENEOUS with the bound cone == the mirror-on path"""
    from hdsdp_amd import api
    n, m = 96, 50
    Rd = -2.5 * n
    y = 0.02 * np.sin(1.3 * np.arange(m) + 0.4)
    host = bound_cone(y, -1.0, 1.5)
    rhs = np.sin(np.arange(m) + 0.5)
    api.set_devices([0, 0], shard_min_dim=0)
    try:
        cone = api.SDPCone.synthetic(n, m)
        try:
            assert cone.shard_count() == 2
            cone.set_start(Rd)
            assert cone.check_is_interior(1.0, y)
            for typ in (api.KKT_TYPE_INFEASIBLE, api.KKT_TYPE_HOMOGENEOUS):
                got = {}
                for mirror in (True, False):
                    kkt = api.KKT(m, [cone], host_mirror=mirror)
                    got[mirror] = step(kkt, host, typ, [1e-6], rhs)
                    if not mirror:
                        assert kkt.matrix_traffic() == (0, 8 * m)
                    kkt.destroy()
                assert_identical(got[True], got[False], typ)
        finally:
            cone.destroy()
    finally:
        api.set_devices([0])


def test_switch_turns_the_mirror_off_only_when_eligible(syn64, monkeypatch, capfd):
    """HDSDP_MI355X_DEVICE_M=1: HKKTInit turns the mirror off for an operator of engine cones; with a host cone inside
    cones[] it keeps the mirror, says why on stderr, and computes what it computed before"""
    from hdsdp_amd import api
    cone, m, y = syn64
    lib = api.load_library()
    rhs = np.sin(np.arange(m) + 2.0)
    P = 0.05 * np.cos(np.add.outer(np.arange(m), np.arange(m)))

    @BUILD_FN
    def build(cone_data, icone, kkt_ptr, type_kkt):      # a host cone inside the operator: writes all of M
        k = C.cast(kkt_ptr, C.POINTER(api.hdsdp_kkt)).contents
        for j in range(m):
            for i in range(j, m):
                k.kktMatElem[i + j * m] += P[i, j]
        return 0

    @C.CFUNCTYPE(C.c_int, C.c_void_p)
    def get_dim(cone_data):
        return 3

    @C.CFUNCTYPE(C.c_int64, C.c_void_p)
    def get_nnz(cone_data):
        return m * m
    foreign = HostCone()
    foreign.iCone = 1
    foreign.slots[7] = C.cast(get_nnz, C.c_void_p)       # coneGetSymNnz
    foreign.slots[8] = C.cast(get_dim, C.c_void_p)       # coneGetDim
    foreign.slots[11] = C.cast(build, C.c_void_p)        # coneBuildSchur

    def mixed_run():
        k = C.POINTER(api.hdsdp_kkt)()
        assert lib.HKKTCreate(C.byref(k)) == 0
        arr = (C.c_void_p * 2)(cone._h, C.cast(C.pointer(foreign), C.c_void_p).value)
        assert lib.HKKTInit(k, m, 2, arr) == 0
        target = lib.HMiKKTGetDiagTarget(k)
        assert lib.HKKTBuildUp(k, api.KKT_TYPE_INFEASIBLE) == 0
        lib.HKKTRegularize(k, 1e-6)
        assert lib.HKKTFactorize(k) == 0
        x = np.zeros(m)
        assert lib.HKKTSolve(k, api._dptr(rhs), api._dptr(x)) == 0
        lib.HKKTDestroy(C.byref(k))
        return target, x

    host = bound_cone(y, -1.0, 2.0)
    base_t, base_x = mixed_run()
    kkt = api.KKT(m, [cone])
    base = step(kkt, host, api.KKT_TYPE_INFEASIBLE, [1e-6], rhs)
    kkt.destroy()
    capfd.readouterr()

    monkeypatch.setenv("HDSDP_MI355X_DEVICE_M", "1")
    t, x = mixed_run()
    assert t == base_t == 0
    assert np.array_equal(x, base_x)
    assert "HDSDP_MI355X_DEVICE_M=1: the host copy of M is kept: 1 cone(s) of this operator accumulate on the host" in capfd.readouterr().err
    kkt = api.KKT(m, [cone])
    assert kkt.diag_target() == 1
    got = step(kkt, host, api.KKT_TYPE_INFEASIBLE, [1e-6], rhs)
    assert kkt.matrix_traffic() == (0, 8 * m)
    kkt.set_host_mirror(1)                                   # mode 1 is the mirror again: kktDiag back on kktMatElem
    assert kkt.diag_target() == 0
    again = step(kkt, host, api.KKT_TYPE_INFEASIBLE, [1e-6], rhs)
    kkt.destroy()
    assert_identical(base, got, "switch")
    assert_identical(base, again, "back")
    assert "host copy of M is kept" not in capfd.readouterr().err


def test_primal_build_and_phase_a_with_the_mirror_off():
    """KKT_TYPE_PRIMAL (the primal refinement, with the driver's 1e-16 regularisation) and the one-launch Phase A keep
    working with M on the device: same numbers as with the mirror on"""
    from hdsdp_amd import api
    from util import primal_X
    g = load_golden("syn64")
    n, m = int(g["dims"][0]), int(g["dims"][1])
    cone = api.SDPCone.synthetic(n, m)
    try:
        cone.set_start(float(g["Rd"][0]))
        assert cone.check_is_interior(float(g["tau"][0]), y_of(g))
        X = primal_X(n)
        rhs = np.sin(np.arange(m) + 0.25)
        got = {}
        for mirror in (True, False):
            kkt = api.KKT(m, [cone], host_mirror=mirror)
            kkt.register_psdp([X])
            got[mirror] = step(kkt, None, api.KKT_TYPE_PRIMAL, [1e-16], rhs)
            if not mirror:
                assert kkt.matrix_traffic()[0] == 0
            kkt.destroy()
        assert_identical(got[True], got[False], "primal")
    finally:
        cone.destroy()
    # Phase A: the fused pass of a small rank-one block (mcp100-like), then the multi-launch operations on the same operator
    gg = np.load(os.path.join(ROOT, "tests", "golden", "mcp100_A.npz"))
    n, m = int(gg["dims"][0]), int(gg["dims"][1])
    cone = api.SDPCone.from_csc(n, m, gg["csc_beg"], gg["csc_idx"], gg["csc_val"])
    try:
        cone.set_start(-20.0)
        y = 0.3 * np.sin(1.7 * np.arange(1, m + 1))
        rhs = np.cos(np.arange(m))
        res = {}
        for mirror in (True, False):
            kkt = api.KKT(m, [cone], host_mirror=mirror)
            if not kkt.phase_a_eligible():
                kkt.destroy()
                pytest.skip("mcp100 is not Phase-A eligible on this build")
            ok, ld, d1, d2, d3 = kkt.phase_a(0.7, y, rhs)
            assert ok
            host = diag_cone(0.01 + 0.001 * np.arange(m))
            after = step(kkt, host, api.KKT_TYPE_INFEASIBLE, [1e-6], rhs)
            res[mirror] = (d1, d2, d3, after, kkt.matrix_traffic())
            kkt.destroy()
        for a, b in zip(res[True][:3], res[False][:3]):
            assert np.array_equal(a, b)
        assert_identical(res[True][3], res[False][3], "after phase A")
        assert res[False][4] == (0, 8 * m)
    finally:
        cone.destroy()


# ---------------------------------------------------------------- the unchanged driver

ITER = re.compile(r"^\s+\d+\s+[-+]\d")


def _driver(fname, device_m, attach="2"):
    env = dict(os.environ, HDSDP_DROP_ATTACH=attach)
    env.pop("HDSDP_MI355X_DEVICE_M", None)
    if device_m:
        env["HDSDP_MI355X_DEVICE_M"] = "1"
    r = subprocess.run([EXE, fname], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    # an iteration line without its last column (the elapsed time)
    iters = [l.split()[:-1] for l in r.stdout.splitlines() if ITER.match(l)]
    dobj = float(re.search(r"dObj\s+([-+0-9.eE]+)", r.stdout + r.stderr).group(1))
    return iters, dobj, r.stdout + r.stderr


def _instance(inst, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    if inst.startswith("syn"):
        from synth_sdpa import write_synth_sdpa
        fname = str(tmp_path / (inst + ".dat-s"))
        write_synth_sdpa(int(inst[3:]), int(inst[3:]), fname)
        return fname
    if inst.startswith("blocks"):
        from blocks_sdpa import write_blocks_sdpa
        fname = str(tmp_path / (inst + ".dat-s"))
        write_blocks_sdpa(fname, with_lp=inst.endswith("lp"))
        return fname
    return os.path.join(ROOT, "tests", "golden", inst + ".dat-s")


# optimum as the driver prints it (tests/test_gpu_reference_driver.py: CASES)
DRIVER_CASES = {"theta1": -23.0, "gpp100": 44.9435, "mcp100": -226.15735, "syn120": -36.746433644, "truss1": 8.999996,
                "blockslp": 10.616269973}
ON = "HDSDP_MI355X_DEVICE_M=1: M stays on the device"
KEPT = "HDSDP_MI355X_DEVICE_M=1: the host copy of M is kept"


def _tol(inst):
    return 1e-6 if inst.startswith(("syn", "blocks")) else 1e-4


@pytest.mark.parametrize("inst", ["gpp100", "mcp100", "syn120", "theta1", "truss1"])
def test_unchanged_driver_log_is_unchanged_with_M_on_the_device(inst, tmp_path):
    """engine cones only (HDSDP_DROP_ATTACH=2): the switch takes M off the host, and the iteration log is the same line by
    line -- the factor input is bit for bit the host mirror's"""
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/sdpasolve_mi355x not built (needs the reference at build time: make -C oracle drop)")
    fname = _instance(inst, tmp_path)
    base, dobj0, out0 = _driver(fname, False)
    got, dobj1, out1 = _driver(fname, True)
    assert ON not in out0 and ON in out1 and KEPT not in out1
    assert len(base) > 5 and got == base
    assert dobj1 == dobj0
    assert abs(dobj1 - DRIVER_CASES[inst]) <= _tol(inst) * abs(DRIVER_CASES[inst])


@pytest.mark.parametrize("inst,attach", [("truss1", "0"), ("blockslp", "2")])
def test_unchanged_driver_keeps_the_mirror_beside_a_host_cone(inst, attach, tmp_path):
    """a CPU cone of the reference inside the operator (truss1 with the reference's own cones; blockslp's LP block, which stays a
    CPU LP cone): the switch keeps the mirror, says why once, and the run is the one without the switch"""
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/sdpasolve_mi355x not built (needs the reference at build time: make -C oracle drop)")
    fname = _instance(inst, tmp_path)
    base, dobj0, _ = _driver(fname, False, attach)
    got, dobj1, out = _driver(fname, True, attach)
    assert out.count(KEPT) == 1 and ON not in out
    assert got == base and dobj1 == dobj0
    assert abs(dobj1 - DRIVER_CASES[inst]) <= _tol(inst) * abs(DRIVER_CASES[inst])
