"""The LP (diagonal) block of an SDPA file on the host: the reader's LP getter against the reference's own reader (HReadSDPA in the
compiled reference library), and the committed LP-cone fixtures against a fresh run of their generator (tools/lp_golden.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libhdsdp_ref.so")
need_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference library not built (make -C oracle ref)")


def _write(path, m, sizes, rhs, entries):
    with open(path, "w") as f:
        f.write(f"\"LP block test file\n{m}\n{len(sizes)}\n{' '.join(str(s) for s in sizes)}\n")
        f.write(" ".join(repr(float(v)) for v in rhs) + "\n")
        for e in entries:
            f.write("%d %d %d %d %.17g\n" % e)


def _files(tmp_path):
    rng = np.random.default_rng(5)
    out = {}
    # dense LP block only: every (constraint, column) present, objective included
    m, n = 6, 9
    ent = [(k, 1, j + 1, j + 1, rng.uniform(-2, 2)) for k in range(m + 1) for j in range(n)]
    out["dense"] = (m, [-n], ent)
    # bounds only: +-1 entries, two per constraint, objective with a zero entry left out
    m = 5
    ent = [(0, 1, j + 1, j + 1, float(j % 3)) for j in range(2 * m) if j % 3]
    ent += [(i + 1, 1, i + 1, i + 1, 1.0) for i in range(m)] + [(i + 1, 1, m + i + 1, m + i + 1, -1.0) for i in range(m)]
    out["bounds"] = (m, [-2 * m], ent)
    # two SDP blocks then the LP block, entries interleaved across blocks and given out of order
    m = 4
    ent = []
    for k in range(m + 1):
        ent += [(k, 1, 1, 2, rng.uniform(-1, 1)), (k, 2, 3, 3, rng.uniform(-1, 1)), (k, 3, 7 - k, 7 - k, rng.uniform(-1, 1))]
        ent += [(k, 3, 1, 1, rng.uniform(-1, 1)), (k, 1, 3, 3, 1e-14)]       # (below 1e-12: dropped by both readers)
    rng.shuffle(ent)
    out["mixed"] = (m, [3, 4, -7], [tuple(e) for e in ent])
    files = {}
    for name, (m, sizes, ent) in out.items():
        p = str(tmp_path / f"{name}.dat-s")
        _write(p, m, sizes, np.arange(1, m + 1) * 0.5, [(int(a), int(b), int(c), int(d), float(v)) for a, b, c, d, v in ent])
        files[name] = p
    return files


def _ref_read(path):
    lib = C.CDLL(REF_LIB, mode=C.RTLD_GLOBAL)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    m, nb, ncols, nlp, nel = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    dims, rhs = ip(), dp()
    cb, ci, cv = C.POINTER(ip)(), C.POINTER(ip)(), C.POINTER(dp)()
    lb, li, lv = ip(), ip(), dp()
    rc = lib.HReadSDPA(C.c_char_p(os.fsencode(path)), C.byref(m), C.byref(nb), C.byref(dims), C.byref(rhs), C.byref(cb), C.byref(ci),
                       C.byref(cv), C.byref(ncols), C.byref(nlp), C.byref(lb), C.byref(li), C.byref(lv), C.byref(nel))
    assert rc == 0
    beg = np.ctypeslib.as_array(lb, shape=(m.value + 2,)).copy()
    nnz = int(beg[-1])
    return {"m": m.value, "n": nlp.value, "beg": beg, "idx": np.ctypeslib.as_array(li, shape=(max(nnz, 1),))[:nnz].copy(),
            "val": np.ctypeslib.as_array(lv, shape=(max(nnz, 1),))[:nnz].copy()}


@need_ref
@pytest.mark.parametrize("case", ["dense", "bounds", "mixed"])
def test_lp_block_getter_is_the_reference_readers_block(tmp_path, case):
    from hdsdp_amd import api
    path = _files(tmp_path)[case]
    d = api.read_sdpa(path)
    r = _ref_read(path)
    assert d["lp"] is not None and d["n_lp"] == r["n"] == d["lp"]["n"]
    assert d["m"] == r["m"]
    for k in ("beg", "idx", "val"):
        assert np.array_equal(d["lp"][k], r[k]), k
    if case == "mixed":
        assert [b["n"] for b in d["blocks"]] == [3, 4]


def test_lp_block_getter_without_an_lp_block():
    from hdsdp_amd import api
    d = api.read_sdpa(os.path.join(ROOT, "tests", "golden", "theta1.dat-s"))
    assert d["lp"] is None and d["n_lp"] == 0


def test_lp_block_layout_by_hand(tmp_path):
    """column 0 = -F0's entries, file order inside a column, 0-based LP indices"""
    from hdsdp_amd import api
    p = str(tmp_path / "hand.dat-s")
    _write(p, 2, [2, -3], [1.0, 1.0], [(0, 2, 3, 3, 4.0), (1, 2, 2, 2, -1.5), (0, 2, 1, 1, 2.0), (2, 1, 1, 1, 1.0), (1, 2, 1, 1, 0.5)])
    lp = api.read_sdpa(p)["lp"]
    assert lp["n"] == 3
    assert list(lp["beg"]) == [0, 2, 4, 4]
    assert list(lp["idx"]) == [2, 0, 1, 0] and list(lp["val"]) == [-4.0, -2.0, -1.5, 0.5]


@need_ref
def test_lp_fixtures_regenerate_from_the_reference():
    sys.path.insert(0, ROOT)
    from tools import lp_golden
    for name in lp_golden.CASES:
        out = lp_golden.reference_outputs(name)
        g = np.load(os.path.join(ROOT, "tests", "golden", f"lp_{name}.npz"))
        assert sorted(g.files) == sorted(out), name
        for k in out:
            assert np.array_equal(g[k], out[k]), (name, k)
