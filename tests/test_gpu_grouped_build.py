"""The grouped Schur build (csrc/grouped_plan.h, csrc/small.hip): every eligible small SDP cone of an
operator built in three launches -- against the compiled reference's goldens, against the per-cone loop of the same library,
against the definition (tests/xprec_ref.py), at the rule's boundaries, and under the reference's unchanged driver through
HDSDP_MI355X_GROUPED_BUILD=1."""
import os
import re
import subprocess

import numpy as np
import pytest

from util import check_close, golden_schur_dense, load_golden, lower_mask, y_of
import xprec_ref as xr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "oracle", "_ref", "sdpasolve_mi355x")
INSTANCES = {"truss1_A": ("truss1.dat-s", 7), "blocks3_A": ("blocks3.dat-s", 3), "chain16_A": ("chain16.dat-s", 16),
             "arrow128_A": ("arrow128.dat-s", 128)}
TYPES = ("HOMOGENEOUS", "CORRECTOR", "INFEASIBLE")


@pytest.fixture(scope="module", params=sorted(INSTANCES))
def instance(request):
    """the cones of a multi-block golden at the golden's state, shared by the tests of this module"""
    from hdsdp_amd import api
    name = request.param
    g = load_golden(name)
    m = int(g["mb_dims"][1])
    prob = api.read_sdpa(os.path.join(GOLDEN, INSTANCES[name][0]))
    cones = [api.SDPCone.from_csc(blk["n"], m, blk["beg"], blk["idx"], blk["val"], iCone=k) for k, blk in enumerate(prob["blocks"])]
    for c in cones:
        c.set_start(float(g["Rd"][0]))
        assert c.check_is_interior(float(g["tau"][0]), y_of(g))
    yield name, g, m, cones
    for c in cones:
        c.destroy()


def _builds(kkt):
    """the three build types of one operator: M (lower triangle), the vectors and the scalars of each"""
    from hdsdp_amd import api
    msk = lower_mask(kkt.m)
    out = {}
    for t in TYPES:
        kkt.build_up(getattr(api, "KKT_TYPE_" + t))
        ex = kkt.export()
        out[t] = {"M": None if t == "CORRECTOR" else kkt.M[msk].copy(), "ASinv": ex["ASinv"].copy(), "ASinvRdSinv": ex["ASinvRdSinv"].copy(),
                  "ASinvCSinv": ex["ASinvCSinv"].copy(),
                  "scalars": np.array([ex["CSinv"], ex["CSinvCSinv"], ex["CSinvRdSinv"], ex["TraceSinv"]]), "info": kkt.grouped_build_info()}
    return out


def _agree(a, b, what, exact=False):
    for t in TYPES:
        for key in ("M", "ASinv", "ASinvRdSinv", "ASinvCSinv", "scalars"):
            if a[t][key] is None or (key == "ASinvCSinv" and t != "HOMOGENEOUS") or (key == "scalars" and t == "CORRECTOR"):
                continue
            x, y = a[t][key], b[t][key]
            if key == "scalars" and t == "INFEASIBLE":
                x, y = x[3:], y[3:]                      # TraceSinv is the one scalar of this type
            if exact:
                assert np.array_equal(x, y), f"{what}: {t} {key} differs"
            else:
                check_close(x, y, f"{what}: {t} {key}")


def _check_goldens(name, g, kkt, ncones):
    from hdsdp_amd import api
    msk = lower_mask(kkt.m)
    assert kkt.is_sparse == bool(int(g["kkt_sparse"][0]))
    kkt.build_up(api.KKT_TYPE_HOMOGENEOUS)
    info = kkt.grouped_build_info()
    assert info["cones"] == ncones and 1 <= info["launches"] <= 3 and info["jobs"] >= ncones, info
    ex = kkt.export()
    if kkt.is_sparse and kkt.diag_target() == 0:
        check_close(kkt.csc()[2], g["M_hsd"], name + " M_hsd (CSC values)")
    if kkt.diag_target() == 0:
        check_close(kkt.M[msk], golden_schur_dense(g, "M_hsd")[msk], name + " M_hsd")
    check_close(ex["ASinv"], g["ASinv_hsd"], name + " ASinv")
    check_close(ex["ASinvRdSinv"], g["ASinvRdSinv_hsd"], name + " ASinvRdSinv")
    check_close(ex["ASinvCSinv"], g["ASinvCSinv_hsd"], name + " ASinvCSinv")
    check_close([ex["CSinv"], ex["CSinvCSinv"], ex["CSinvRdSinv"], ex["TraceSinv"]], g["hsd_scalars"], name + " scalars")
    kkt.build_up(api.KKT_TYPE_CORRECTOR)
    info = kkt.grouped_build_info()
    assert info["cones"] == ncones and 1 <= info["launches"] <= 3, info
    exc = kkt.export()
    check_close(exc["ASinv"], g["ASinv_cor"], name + " ASinv_cor")
    check_close(exc["ASinvRdSinv"], g["ASinvRdSinv_cor"], name + " ASinvRdSinv_cor")
    kkt.build_up(api.KKT_TYPE_INFEASIBLE)
    info = kkt.grouped_build_info()
    assert info["cones"] == ncones and 1 <= info["launches"] <= 3, info
    if kkt.diag_target() == 0:
        check_close(kkt.M[msk], golden_schur_dense(g, "M_inf")[msk], name + " M_inf")
    kkt.factorize()
    x = kkt.solve(g["b"])
    assert np.linalg.norm(x - g["sol_b"]) <= 1e-8 * np.linalg.norm(g["sol_b"])


def test_grouped_build_against_the_reference_goldens(instance):
    """test_multi_block_instance_against_reference's numbers and bars with the grouped pass on: truss1 (dense operator), blocks3
    (three blocks on three per-cone paths, one grouped pass here), chain16 (CSC-mirrored operator) and arrow128 (tile form);
    chain16 once more with the host mirror off"""
    from hdsdp_amd import api
    name, g, m, cones = instance
    ncones = INSTANCES[name][1]
    kkt = api.KKT(m, cones)
    try:
        assert kkt.set_grouped_build(True) == ncones
        if name == "arrow128_A":
            assert kkt.tile_info() is not None
        _check_goldens(name, g, kkt, ncones)
    finally:
        kkt.destroy()
    if name == "chain16_A":
        kdev = api.KKT(m, cones, host_mirror=False)
        try:
            assert kdev.set_grouped_build(True) == ncones and kdev.diag_target() == 1
            _check_goldens(name, g, kdev, ncones)
        finally:
            kdev.destroy()


def test_grouped_build_against_the_loop_and_itself(instance):
    """one operator, one process: switch off, on, on again -- the pass agrees with the per-cone loop under check_close, two
    grouped builds are bit-identical, and switching off again gives the loop's bits back"""
    from hdsdp_amd import api
    name, g, m, cones = instance
    kkt = api.KKT(m, cones)
    try:
        loop = _builds(kkt)
        assert all(loop[t]["info"] == {"cones": 0, "jobs": 0, "launches": 0} for t in TYPES)
        assert kkt.set_grouped_build(True) == INSTANCES[name][1]
        first = _builds(kkt)
        second = _builds(kkt)
        assert all(first[t]["info"]["cones"] == INSTANCES[name][1] for t in TYPES)
        _agree(first, loop, name + " grouped against loop")
        _agree(second, first, name + " two grouped builds", exact=True)
        assert kkt.set_grouped_build(False) == 0
        _agree(_builds(kkt), loop, name + " loop again", exact=True)
    finally:
        kkt.destroy()


# ---- operators from seeded numpy data, compared with the definition ----------------------------------------------------
def _sym(rng, n, density):
    A = rng.uniform(-1.0, 1.0, (n, n)) * (rng.uniform(0.0, 1.0, (n, n)) < density)
    A = np.tril(A) + np.tril(A, -1).T
    if not A.any():
        A[n - 1, n - 1] = 1.0
    return A


def _block(rng, n, m, rows):
    """(cone, C, A): a block of dimension n with seeded data on `rows` of the m constraints; A is m x n x n"""
    from hdsdp_amd import api
    C = 0.1 * _sym(rng, n, 1.0) + 4.0 * np.eye(n)
    A = np.zeros((m, n, n))
    for k, r in enumerate(rows):
        A[r] = _sym(rng, n, 1.0 if k % 3 == 0 else 0.3)
    iu = np.triu_indices(n)                      # (j, i) with i >= j, column by column: the packed lower triangle
    beg, idx, val = [0], [], []
    for mat in [C] + list(A):
        v = mat[iu]
        nz = np.flatnonzero(v)
        idx.extend(nz.tolist()); val.extend(v[nz].tolist()); beg.append(len(idx))
    return api.SDPCone.from_csc(n, m, beg, np.asarray(idx, dtype=np.int32), np.asarray(val)), C, A


def _definition(blocks, m, tau, y, Rd, perturb, typeKKT):
    """sum over the blocks of tests/xprec_ref.py: schur at S = tau C - sum y_i A_i + (perturb - Rd) I"""
    tot = None
    for _, C, A in blocks:
        n = C.shape[0]
        S = tau * C - np.tensordot(y, A, axes=1) + (perturb - Rd) * np.eye(n)
        one = xr.schur(xr.inverse(S), C, Rd, ("dense", A), typeKKT)
        tot = one if tot is None else {k: tot[k] + one[k] for k in one}
    return {k: np.asarray(v, dtype=np.float64) for k, v in tot.items()}


def _check_definition(kkt, blocks, m, tau, y, Rd, perturb, what):
    from hdsdp_amd import api
    msk = lower_mask(m)
    for typ, code in ((api.KKT_TYPE_HOMOGENEOUS, 2), (api.KKT_TYPE_CORRECTOR, 1), (api.KKT_TYPE_INFEASIBLE, 0)):
        ref = _definition(blocks, m, tau, y, Rd, perturb, code)
        kkt.build_up(typ)
        ex = kkt.export()
        check_close(ex["ASinv"], ref["ASinv"], f"{what} type {code} ASinv")
        check_close(ex["ASinvRdSinv"], ref["ASinvRdSinv"], f"{what} type {code} ASinvRdSinv")
        if code != 1:
            check_close(kkt.M[msk], ref["M"][msk], f"{what} type {code} M")
            check_close([ex["TraceSinv"]], [ref["TraceSinv"]], f"{what} type {code} TraceSinv")
        if code == 2:
            check_close(ex["ASinvCSinv"], ref["ASinvCSinv"], f"{what} ASinvCSinv")
            check_close([ex["CSinv"], ex["CSinvCSinv"], ex["CSinvRdSinv"]], [ref["CSinv"], ref["CSinvCSinv"], ref["CSinvRdSinv"]], f"{what} scalars")


def test_grouped_build_at_the_rules_boundaries():
    """block dimensions 1, 16, 17, 48 and 64 and a block no constraint touches in one operator; Rd = 0, Rd != 0, and Rd != 0
    after set_perturb; the block of dimension 17 owns twenty rows (three jobs)"""
    from hdsdp_amd import api
    rng = np.random.default_rng(20240607)
    m = 24
    plan = [(1, [0, 5, 23]), (16, [1, 2, 3, 4, 5, 6]), (17, list(range(4, 24))), (48, [0, 7, 9, 11, 22]), (64, [2, 8, 13, 21]), (5, [])]
    blocks = [_block(rng, n, m, rows) for n, rows in plan]
    cones = [b[0] for b in blocks]
    tau, y = 0.9, rng.uniform(-0.02, 0.02, m)
    try:
        kkt = api.KKT(m, cones)
        assert kkt.set_grouped_build(True) == len(cones)
        for Rd, perturb in ((0.0, 0.0), (-0.3, 0.0), (-0.3, 0.05)):
            for c in cones:
                c.set_start(Rd)
                c.set_perturb(perturb)
                assert c.check_is_interior(tau, y)
            _check_definition(kkt, blocks, m, tau, y, Rd, perturb, f"boundaries Rd {Rd} perturb {perturb}")
            info = kkt.grouped_build_info()
            assert info["cones"] == len(cones) and info["launches"] <= 3
            assert info["jobs"] == 1 + 1 + 3 + 1 + 1 + 1
        kkt.destroy()
    finally:
        for c in cones:
            c.destroy()


def test_mixed_operator_groups_the_small_blocks_only():
    """two small blocks beside blocks of dimension 65 and 129: two cones grouped, the large ones through their own slots;
    against the loop and against the definition"""
    from hdsdp_amd import api
    rng = np.random.default_rng(7)
    m = 12
    plan = [(65, [0, 3, 4, 9]), (12, [0, 1, 2, 3]), (129, [2, 5, 6, 11]), (33, [3, 7, 8, 10, 11])]
    blocks = [_block(rng, n, m, rows) for n, rows in plan]
    cones = [b[0] for b in blocks]
    tau, y, Rd = 1.1, rng.uniform(-0.02, 0.02, m), -0.2
    try:
        for c in cones:
            c.set_start(Rd)
            assert c.check_is_interior(tau, y)
        kkt = api.KKT(m, cones)
        loop = _builds(kkt)
        assert kkt.set_grouped_build(True) == 2
        grouped = _builds(kkt)
        assert all(grouped[t]["info"]["cones"] == 2 and grouped[t]["info"]["launches"] <= 3 for t in TYPES)
        _agree(grouped, loop, "mixed operator")
        _check_definition(kkt, blocks, m, tau, y, Rd, 0.0, "mixed operator")
        kkt.destroy()
    finally:
        for c in cones:
            c.destroy()


def test_grouped_build_refusals(capfd):
    """a grouped cone without a valid factor fails the build as cone_build_schur does, with its message; one eligible cone alone
    is not a group: the pass is not used and the results are the loop's, bit for bit"""
    from hdsdp_amd import api
    rng = np.random.default_rng(11)
    m = 6
    blocks = [_block(rng, n, m, rows) for n, rows in ((9, [0, 1, 2]), (20, [2, 3, 4, 5]))]
    cones = [b[0] for b in blocks]
    tau, y = 1.0, rng.uniform(-0.02, 0.02, m)
    try:
        cones[0].set_start(-0.1)
        cones[1].set_start(-0.1)
        assert cones[0].check_is_interior(tau, y)          # cones[1] is never factored
        kkt = api.KKT(m, cones)
        assert kkt.set_grouped_build(True) == 2
        capfd.readouterr()
        with pytest.raises(api.HDSDPError, match="hdsdp_retcode %d" % api.RETCODE_FAILED):
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        assert "BuildSchur: the dual matrix has no valid Cholesky factor" in capfd.readouterr().err
        assert cones[1].check_is_interior(tau, y)
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)               # and with the factor in place the same operator builds
        assert kkt.grouped_build_info()["cones"] == 2
        kkt.destroy()
    finally:
        for c in cones:
            c.destroy()
    blocks = [_block(rng, n, m, rows) for n, rows in ((9, [0, 1, 2]), (65, [2, 3, 4, 5]))]
    cones = [b[0] for b in blocks]
    try:
        for c in cones:
            c.set_start(-0.1)
            assert c.check_is_interior(tau, y)
        kkt = api.KKT(m, cones)
        loop = _builds(kkt)
        assert kkt.set_grouped_build(True) == 0
        alone = _builds(kkt)
        assert all(alone[t]["info"] == {"cones": 0, "jobs": 0, "launches": 0} for t in TYPES)
        _agree(alone, loop, "one eligible cone", exact=True)
        kkt.destroy()
    finally:
        for c in cones:
            c.destroy()


# the optimum the driver prints, as tests/test_gpu_reference_driver.py expects it for the same files
DRIVER_CASES = {"truss1": 8.999996, "chain16": 74.932288321}


@pytest.mark.parametrize("inst", sorted(DRIVER_CASES))
def test_unchanged_driver_with_the_grouped_build_switched_on(inst):
    """the reference's own driver with its SDP blocks handed to the engine's cones (oracle/drop_attach.c) and
    HDSDP_MI355X_GROUPED_BUILD=1 in the environment: HKKTInit turns the grouped pass on for the operator's small engine cones --
    all sixteen of chain16, all seven of truss1 -- and the solve reaches the optimum tests/test_gpu_reference_driver.py expects for the file"""
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/sdpasolve_mi355x not built (make -C oracle drop needs the reference's sources at build time)")
    opt = DRIVER_CASES[inst]
    env = dict(os.environ, HDSDP_DROP_ATTACH="1", HDSDP_MI355X_GROUPED_BUILD="1")
    r = subprocess.run([EXE, os.path.join(GOLDEN, inst + ".dat-s")], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "SDP Status: Primal dual optimal" in out, out[-3000:]
    said = re.search(r"HDSDP_MI355X_GROUPED_BUILD=1: (\d+) of (\d+) cone", out)
    assert said, out[-3000:]
    print(said.group(0))
    assert int(said.group(1)) >= 2, said.group(0)
    assert said.group(1) == said.group(2) == {"chain16": "16", "truss1": "7"}[inst], said.group(0)
    pobj = float(re.search(r"pObj\s+([-+0-9.eE]+)", out).group(1))
    dobj = float(re.search(r"dObj\s+([-+0-9.eE]+)", out).group(1))
    assert abs(dobj - opt) <= 1e-4 * abs(opt), (dobj, opt)
    assert abs(pobj - dobj) <= 1e-4 * abs(opt), (pobj, dobj)
