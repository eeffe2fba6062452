"""What tests/test_gpu_grouped_{check,ratio,step}.py share, stated once: the multi-block goldens and their cones, seeded operators,
an LP cone, the grouped build's golden comparison and the reference's unchanged driver.  A plain helper module like util.py; where
the three kinds differ a helper takes the kind, and a test file binds its kind with functools.partial under the names its tests
use."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import line_search_model as lm  # noqa: E402
from util import check_close, golden_schur_dense, load_golden, lower_mask  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "oracle", "_ref", "sdpasolve_mi355x")
INSTANCES = {"truss1_A": ("truss1.dat-s", 7), "blocks3_A": ("blocks3.dat-s", 3), "chain16_A": ("chain16.dat-s", 16),
             "arrow128_A": ("arrow128.dat-s", 128)}
GROUPED = ("HDSDP_MI355X_GROUPED_BUILD", "HDSDP_MI355X_GROUPED_CHECK", "HDSDP_MI355X_GROUPED_RATIO", "HDSDP_MI355X_GROUPED_STEP")


def _rule(kind, n, mloc):
    """csrc/small_{check,ratio,step}_rule.h for an engine SDP cone on one device with resident data, one-block factor objects
    (n <= 128) and the default switches.  check: the one-launch check's rule; step: the same (n = 1 is a member); ratio: that,
    n >= 2, and the multipliers fit the packed triangles' region"""
    n16 = (n + 15) // 16 * 16
    check = n16 <= 128 and mloc * n16 * n16 <= ((1 << 19) if n16 <= 64 else (1 << 17))
    return check and (kind != "ratio" or (n >= 2 and mloc <= n16 * (n16 + 1)))


def _golden_cones(rule, name, m):
    from hdsdp_amd import api
    prob = api.read_sdpa(os.path.join(GOLDEN, INSTANCES[name][0]))
    cones = [api.SDPCone.from_csc(blk["n"], m, blk["beg"], blk["idx"], blk["val"], iCone=k) for k, blk in enumerate(prob["blocks"])]
    members = sum(rule(blk["n"], int(np.count_nonzero(np.diff(np.asarray(blk["beg"])[1:])))) for blk in prob["blocks"])
    return cones, members


def instance_of(golden_cones):
    """the module fixture `instance` over a test file's own _golden_cones"""
    @pytest.fixture(scope="module", params=sorted(INSTANCES))
    def instance(request):
        """two sets of cones of a multi-block golden, made from the same file: `loop` is asked cone by cone with the switch off,
        `grp` cone by cone under an operator with the switch on"""
        name = request.param
        g = load_golden(name)
        m = int(g["mb_dims"][1])
        loop, members = golden_cones(name, m)
        grp, _ = golden_cones(name, m)
        for c in loop + grp:
            c.set_start(float(g["Rd"][0]))
        yield name, g, m, loop, grp, members
        for c in loop + grp:
            c.destroy()
    return instance


# ---- operators from seeded numpy data ----------------------------------------------------------------------------------
def _sym(rng, n, density):
    A = rng.uniform(-1.0, 1.0, (n, n)) * (rng.uniform(0.0, 1.0, (n, n)) < density)
    A = np.tril(A) + np.tril(A, -1).T
    if not A.any():
        A[n - 1, n - 1] = 1.0
    return A


def _cone_of(n, m, C, A):
    from hdsdp_amd import api
    beg, idx, val = lm.to_csc([C] + list(A))
    return api.SDPCone.from_csc(n, m, beg, idx, val)


def _block(kind, rng, n, m, rows):
    """(cone, C, A): a block of dimension n with seeded data on `rows` of the m constraints; A is m x n x n.  step: C is 4 I plus
    noise of norm below 0.2, with the largest diagonal entry (6) first and the smallest (2) last (n = 1: 2): along dS = -C the first
    pivot of S + a dS is the first to fail, along dS = -3 I the last one (_pivot_directions)"""
    C = (0.01 if kind == "step" else 0.1) * _sym(rng, n, 1.0) + 4.0 * np.eye(n)
    if kind == "step":
        if n > 1:
            C[0, 0] += 2.0
        C[n - 1, n - 1] -= 2.0
    A = np.zeros((m, n, n))
    for k, r in enumerate(rows):
        A[r] = _sym(rng, n, 1.0 if k % 3 == 0 else 0.3)
    return _cone_of(n, m, C, A), C, A


def _set(kind, seed, m, plan):
    return [_block(kind, np.random.default_rng([seed, k]), n, m, rows) for k, (n, rows) in enumerate(plan)]


def _two_sets(kind, seed, m, plan):
    """the same seeded blocks twice: (loop blocks, grouped blocks)"""
    return _set(kind, seed, m, plan), _set(kind, seed, m, plan)


def _destroy(*sets):
    for s in sets:
        for b in s:
            b[0].destroy()


def _lp_cone(m, ncol, seed):
    from hdsdp_amd import api
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1.0, 1.0, (m, ncol))
    c = 4.0 + rng.uniform(0.0, 1.0, ncol)
    beg = (np.arange(m + 2, dtype=np.int64) * ncol).astype(np.int32)
    idx = np.tile(np.arange(ncol, dtype=np.int32), m + 1)
    return api.LPCone.from_csc(m, ncol, beg, idx, np.concatenate([c, A.ravel()]))


def _check_goldens(name, g, kkt, ncones, full=False):
    """tests/test_gpu_grouped_build.py's golden comparison, same bars; `full` (the check set's tests): the sparse form, the
    scalars and the corrector build as well"""
    from hdsdp_amd import api
    msk = lower_mask(kkt.m)
    if full:
        assert kkt.is_sparse == bool(int(g["kkt_sparse"][0]))
    kkt.build_up(api.KKT_TYPE_HOMOGENEOUS)
    info = kkt.grouped_build_info()
    assert info["cones"] == ncones and 1 <= info["launches"] <= 3 and (not full or info["jobs"] >= ncones), info
    ex = kkt.export()
    if full and kkt.is_sparse and kkt.diag_target() == 0:
        check_close(kkt.csc()[2], g["M_hsd"], name + " M_hsd (CSC values)")
    if kkt.diag_target() == 0:
        check_close(kkt.M[msk], golden_schur_dense(g, "M_hsd")[msk], name + " M_hsd")
    check_close(ex["ASinv"], g["ASinv_hsd"], name + " ASinv")
    check_close(ex["ASinvRdSinv"], g["ASinvRdSinv_hsd"], name + " ASinvRdSinv")
    check_close(ex["ASinvCSinv"], g["ASinvCSinv_hsd"], name + " ASinvCSinv")
    if full:
        check_close([ex["CSinv"], ex["CSinvCSinv"], ex["CSinvRdSinv"], ex["TraceSinv"]], g["hsd_scalars"], name + " scalars")
        kkt.build_up(api.KKT_TYPE_CORRECTOR)
        info = kkt.grouped_build_info()
        assert info["cones"] == ncones and 1 <= info["launches"] <= 3, info
        exc = kkt.export()
        check_close(exc["ASinv"], g["ASinv_cor"], name + " ASinv_cor")
        check_close(exc["ASinvRdSinv"], g["ASinvRdSinv_cor"], name + " ASinvRdSinv_cor")
    kkt.build_up(api.KKT_TYPE_INFEASIBLE)
    if full:
        info = kkt.grouped_build_info()
        assert info["cones"] == ncones and 1 <= info["launches"] <= 3, info
    if kkt.diag_target() == 0:
        check_close(kkt.M[msk], golden_schur_dense(g, "M_inf")[msk], name + " M_inf")
    kkt.factorize()
    x = kkt.solve(g["b"])
    assert np.linalg.norm(x - g["sol_b"]) <= 1e-8 * np.linalg.norm(g["sol_b"])


def _drive(inst, on):
    """the reference's unchanged driver on a golden's file with the grouped switches `on` (names of GROUPED) set to 1, the others
    unset: (output, iteration numbers, printed pObj, printed dObj)"""
    env = dict(os.environ, HDSDP_DROP_ATTACH="1")
    for k in GROUPED:
        env.pop(k, None)
    for k in on:
        env[k] = "1"
    r = subprocess.run([EXE, os.path.join(GOLDEN, inst + ".dat-s")], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "SDP Status: Primal dual optimal" in out, out[-3000:]
    its = [m_.group(1) for m_ in re.finditer(r"^\s+(\d+)\s+[-+]\d\.\d+e[-+]\d+\s+[-+]\d\.\d+e[-+]\d+", out, re.M)]
    return out, its, re.findall(r"pObj\s+([-+0-9.eE]+)", out), re.findall(r"dObj\s+([-+0-9.eE]+)", out)
