"""tests/gemm_layouts.py -- the numpy model of the skyline storage, the 16 x 16 blocked congruence output and the Gram operand
that tests/test_gpu_gemm_roles.py packs and unpacks with -- held index by index to what the engine's headers say, without a
device: tests/gemm_layouts_driver.cpp is compiled with the host C++ compiler against csrc/gemm_geom.h, csrc/work_plan.h and
csrc/gemm_calls.h and prints hdm_sky_off, hdm_sky_size, hdm_blk_sub, hdm_pblock_decode, the layout numbers and the Gram
operand's offsets as the kernels' stager adds them up from the fields hdm_gram_splits fills."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gemm_layouts as gl

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_layouts") / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", exe, os.path.join(HERE, "gemm_layouts_driver.cpp")])
    return exe


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n16", [16, 48, 128, 144, 272])
def test_model_and_headers_agree_index_by_index(driver, n16, world):
    maxloc = 21 if world == 1 else 5            # Lr = 24 on one device (no multiple of 16), 128 when sharded
    kstep = 1 if n16 <= 144 else 15             # n16 = 272: the first and the last k of every k block
    raw = np.frombuffer(subprocess.run([driver, str(n16), str(world), str(maxloc), str(kstep)], capture_output=True, check=True).stdout,
                        dtype=np.int64)
    L = gl.layout(n16, world, maxloc)
    nblk, npb = L["nblk"], L["npb"]
    pos = 0

    def take(k):
        nonlocal pos
        pos += k
        return raw[pos - k:pos]

    # skyline
    assert take(1)[0] == gl.sky_size(n16)
    sky = take(n16 * n16).reshape(n16, n16)
    want = np.array([[gl.sky_off(i, j, n16) if i >= 128 * (j // 128) else -1 for j in range(n16)] for i in range(n16)])
    assert np.array_equal(sky, want)
    stored = np.sort(sky[sky >= 0])
    assert np.array_equal(stored, np.arange(gl.sky_size(n16)))      # a bijection onto the storage: nothing shared, nothing unused
    AL = np.tril(np.arange(1.0, n16 * n16 + 1).reshape(n16, n16))
    buf = gl.sky_pack(AL)
    lower = np.tril(np.ones((n16, n16), dtype=bool))
    assert np.array_equal(buf[sky[lower]], AL[lower]) and np.array_equal(gl.sky_unpack(buf, n16), AL)
    # blocked layout
    sub = take(nblk * nblk).reshape(nblk, nblk)
    assert np.array_equal(sub, np.array([[gl.blk_sub(bi, bj, nblk) if bi >= bj else -1 for bj in range(nblk)] for bi in range(nblk)]))
    dec = take(npb * 4).reshape(npb, 4)
    assert np.array_equal(dec, np.array([gl.pblock_decode(q, nblk) for q in range(npb)]))
    idx, w = gl.blocked_index(n16, L["Lr"])
    i, j = np.meshgrid(np.arange(n16), np.arange(n16), indexing="ij")
    keep = i // 16 >= j // 16
    assert np.array_equal(idx[keep], ((sub[i // 16, j // 16] * 16 + j % 16) * L["Lr"] * 16 + i % 16)[keep]) and np.all(idx[~keep] == -1)
    assert np.all(w[i // 16 == j // 16] == 1.0) and np.all(w[i // 16 != j // 16] == np.sqrt(2.0))
    # every p-block the layout addresses decodes to the column it was written for, and the rows of all constraints tile the buffer
    assert np.array_equal(dec[(idx[keep] // (L["Lr"] * 16))][:, 3], j[keep])
    cover = np.concatenate([idx[keep] + 16 * r for r in range(L["Lr"])])
    assert np.array_equal(np.sort(cover), np.arange(gl.blocked_doubles(n16, L["Lr"])))
    At = np.arange(1.0, n16 * n16 + 1).reshape(n16, n16)
    At = At + At.T
    dst = np.full(gl.blocked_doubles(n16, L["Lr"]), -7.0)
    gl.blocked_pack(dst, At, L["Lr"], 2)
    got, w2 = gl.blocked_unpack(dst, n16, L["Lr"], 2)
    assert np.array_equal(got[keep], (w * At)[keep]) and np.all(np.isnan(got[~keep])) and np.array_equal(w, w2)
    assert np.count_nonzero(dst != -7.0) == np.count_nonzero(keep)
    # layout numbers
    assert [int(v) for v in take(7)] == [L[k] for k in ("n16", "nblk", "npb", "npb_loc", "Lr", "R", "astride")]
    # Gram operand
    ks = np.arange(0, 16, kstep)
    off = take(L["R"] * L["npb_loc"] * ks.size).reshape(L["R"], L["npb_loc"], ks.size)
    assert pos == raw.size
    model = gl.gram_index(L["R"], 16 * L["npb_loc"], L["Lr"], L["npb_loc"]).reshape(L["R"], L["npb_loc"], 16)
    assert np.array_equal(off, model[:, :, ks])
    assert np.array_equal(np.sort(model.reshape(-1)), np.arange(L["R"] * L["npb_loc"] * 16))
    if n16 <= 48:
        W = np.arange(1.0, L["R"] * L["npb_loc"] * 16 + 1).reshape(L["R"], -1)
        assert np.array_equal(gl.gram_unpack(gl.gram_pack(W, L["Lr"], L["npb_loc"]), L["R"], L["Lr"], L["npb_loc"]), W)


# ---- which tile classes the GPU cases reach ---------------------------------------------------------------------------------
GENERIC, CONG1, CONG2, GRAM, CONG2D = range(5)                 # HdmRole
KLIM_NONE, KLIM_BY_N, KLIM_BAND = 0, 2, 3                      # HdmKLimit
KINDS = ("DIAG_FULL", "DIAG_SHORT", "EDGE", "SYMDIAG", "MAIN")  # HdmTileKind


def role_case_classes(exe):
    """role -> set of (kind, RV) over the launches of tests/test_gpu_gemm_roles.py, from hdm_tile_class (tests/gemm_geom_driver.cpp)"""
    import test_gpu_gemm_roles as roles
    launches = []
    for n16 in [s[0] for s in roles.CONG_SIZES] + [roles.MASK_N16]:
        launches += [("step 1", CONG1, n16, n16, KLIM_BAND, 0, 1), ("step 2", CONG2, n16, n16, KLIM_BY_N, 0, 2), ("step 2", CONG2D, n16, n16, KLIM_BY_N, 0, 1)]
    Rs = list(roles.GRAM_ROWS) + [gl.layout(roles.GRAM_N16, w, ml)["R"] for w, ml, _ in roles.GRAM_SHARDED] + [136, 80]   # + gathered, LP
    launches += [("Gram", GRAM, R, 16 * 96, KLIM_NONE, 1, 1) for R in Rs]
    lines, keys = [], []
    for name, role, M, K, klim, slab, npass in launches:
        lines.append(f"GEOM {M} {M} {K} {klim} 1 0 {role} {slab} 1 0 {K} {npass}")
        for tm in range((M + 127) // 128):
            for tn in range(tm + 1):
                lines.append(f"TILE {tm} {tn} 0")
                keys.append((name, role, M, tm, tn))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(keys)
    seen = {}
    for (name, role, M, tm, tn), row in zip(keys, out):
        sel, _, _, kind, _, RV, _ = (int(v) for v in row.split())
        full_diag = tm == tn and M - 128 * tm >= 113
        if sel and (role not in (CONG2, CONG2D) or (role == CONG2D) == full_diag):     # step 2's two kernels split the tile list
            seen.setdefault(name, set()).add((KINDS[kind], RV))
    return seen


def test_gpu_role_cases_reach_every_tile_class(tmp_path):
    exe = str(tmp_path / "geom_driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-I", CSRC, "-o", exe, os.path.join(HERE, "gemm_geom_driver.cpp")])
    seen = role_case_classes(exe)
    cells = {(k, rv) for k in ("DIAG_SHORT", "EDGE") for rv in (4, 5, 6, 7)}
    for name in sorted(seen):
        print(f"\n{name}: " + ", ".join(f"{k} RV={rv}" if k in ("DIAG_SHORT", "EDGE") else k for k, rv in sorted(seen[name])))
    assert seen["step 1"] == cells | {("DIAG_FULL", 8), ("MAIN", 8)}
    assert seen["step 2"] == cells | {("SYMDIAG", 8), ("MAIN", 8)}
    assert seen["Gram"] == cells | {("DIAG_FULL", 8), ("MAIN", 8)}
