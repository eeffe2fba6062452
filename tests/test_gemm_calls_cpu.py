"""The call forms of the fp64 GEMM family (csrc/gemm_calls.h), without a device: the header is compiled alone with the host C++
compiler beside tests/gemm_calls_driver.cpp, which prints every field of each form's HdmGemmArgs and re-evaluates the launcher's
checks on it with gemm_geom.h's own functions.

- The expected value of every field is written here from the rules as DESIGN.md states them (sections 3, 4 and 16), not read back
  from the header: storage classes, leading dimensions, the k-block and segment strides of the Gram operand, k_base / k_chunk, the
  slab stride, the blocked destination, the spans, the flops (compared as float.hex).
- What the launcher would refuse cannot come out of a form: M, N % 8, K % 16, k_chunk, step 2's mirrored pair, leading dimensions,
  and for every operand of a role launch  need <= span <= the buffer the engine allocates for it.
- The exchange pieces of a sharded build are whole groups of Gram K splits, and the splits tile the rank's p-range."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

GENERIC, CONG1, CONG2, GRAM = range(4)
KLIM_NONE, KLIM_BY_M, KLIM_BY_N, KLIM_BAND = range(4)
EPI_STORE, EPI_BLOCKED, EPI_SLAB = range(3)
TILE = 128
LINV, ASRC, TBUF, DST, SLAB = 0x10000000, 0x20000000000, 0x40000000000, 0x60000000000, 0x80000000000     # the driver's addresses
FIELDS = ("A B C A2 B2 lda2 ldb2 strideA2 strideB2 b_sky spanA spanB spanA2 spanB2 lda ldb ldc strideA strideB strideC M N K a_kmajor "
          "b_kmajor a_kblk b_kblk seg_rows seg_extra klimit lower_only tile_col_mask epilogue batch queue_global alpha beta role flops "
          "blk_row_stride blk_row0 nblk k_chunk k_base slab_stride needA needB needA2 needB2 accepted").split()
FLOATS = ("alpha", "beta", "flops")

NS, WORLDS, MS = (16, 128, 144, 384, 464, 2000), (1, 2, 3), (1, 24, 250)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_calls") / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "gemm_calls_driver.cpp")])
    return exe


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [row.split() for row in out.split("\n")[:-1]]


def parse(row):
    assert len(row) == len(FIELDS)
    return {k: (float.fromhex(v).hex() if k in FLOATS else int(v)) for k, v in zip(FIELDS, row)}


# ---- the rules, restated ---------------------------------------------------------------------------
def roundup(x, q):
    return (x + q - 1) // q * q


def ntiles(x):
    return (x + TILE - 1) // TILE


def sky_size(n16):
    """skyline storage: the 128-column panels from their diagonal block downwards, the last one w x w"""
    T = ntiles(n16)
    return sum(TILE * (n16 - TILE * t) for t in range(T - 1)) + (n16 - TILE * (T - 1)) ** 2


def layout(n, world, m):
    n16 = roundup(n, 16)
    nblk = n16 // 16
    npb = nblk * (nblk + 1) // 2 * 16
    Lr = roundup(-(-m // world) + 3, 8 if world == 1 else TILE)
    return dict(n=n, m=m, world=world, n16=n16, nblk=nblk, npb=npb, npb_loc=-(-npb // world), Lr=Lr, R=world * Lr, astride=sky_size(n16),
                npad=roundup(n, TILE), mloc=len(range(0, m, world)))


def operand_pad(ld):                       # doubles of slack behind a buffer whose rows are ld apart
    return (128 * max(16, ld) * 8 + 4096) // 8


PAD_DOUBLES = 8192


def zero_fields():
    return {k: ((0.0).hex() if k in FLOATS else 0) for k in FIELDS[:-5]}


def mask_share(NT, mask):
    """step 2 by tile: tile (tm, tn), tm >= tn, runs tn + 1 K blocks; the share of the mask's tile columns"""
    if not mask or NT > 64:
        return 1.0
    every = sum((NT - tn) * (tn + 1) for tn in range(NT))
    return sum((NT - tn) * (tn + 1) for tn in range(NT) if (mask >> tn) & 1) / every


def check(got, want, what):
    bad = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not bad, f"{what}: (got, expected) {bad}"
    assert got["accepted"] == 1, what
    assert got["M"] % 8 == 0 and got["N"] % 8 == 0 and got["K"] % 16 == 0, what
    if got["role"] != GENERIC:
        for op in ("A", "B", "A2", "B2"):
            if got[op]:
                assert 0 < got["need" + op] <= got["span" + op], (what, op, got["need" + op], got["span" + op])
        assert max(got[k] for k in ("lda", "ldb", "lda2", "ldb2")) <= 2 ** 20, what


def grid(driver):
    """(layout, plan Bc, plan nsplit) over the grid, the layout checked against the header's"""
    cases = [(n, w, m) for n in NS for w in WORLDS for m in MS]
    rows = run(driver, [f"LAYOUT {n} {w} {m}" for n, w, m in cases])
    out = []
    for (n, w, m), r in zip(cases, rows):
        L = layout(n, w, m)
        r = [int(v) for v in r]
        assert r[:7] == [L[k] for k in ("n16", "nblk", "npb", "npb_loc", "Lr", "R", "astride")], (n, w, m)
        assert r[9] == w * L["npb_loc"] * L["Lr"] * 16 and r[10] == operand_pad(L["n16"]) and r[11] == PAD_DOUBLES and r[12] == L["mloc"]
        out.append((L, r[7], r[8]))
    return out


# ---- tests -------------------------------------------------------------------------------------------
def test_congruence_forms(driver):
    lines, want = [], []
    for L, plan_bc, _ in grid(driver):
        n, n16, nn, ldl = L["n"], L["n16"], L["n16"] ** 2, L["npad"]
        n3 = (float(n) * n) * n
        rows_held = max(1, L["mloc"])                                     # matrices behind the resident rows
        afull = L["astride"] * rows_held + operand_pad(n16)               # what the engine allocates for it
        for Bc in sorted({1, 8, plan_bc}):
            t_buf = nn * Bc + operand_pad(n16)
            count = L["mloc"]
            for b0 in sorted({0, (max(count, 1) - 1) // Bc * Bc}):         # the first and the last batch of the range
                nb = max(1, min(Bc, count - b0))
                tag = f"{L['n']}/{L['world']}/{L['m']} Bc {Bc} b0 {b0}"
                lines.append(f"STEP1 {n} {L['world']} {L['m']} {ldl} {rows_held} {b0} {nb}")
                w = zero_fields()
                w.update(A=LINV, lda=ldl, B=ASRC + 8 * b0 * L["astride"], ldb=n16, b_kmajor=1, strideB=L["astride"], b_sky=1, C=TBUF, ldc=n16,
                         strideC=nn, M=n16, N=n16, K=n16, batch=nb, alpha=(1.0).hex(), klimit=KLIM_BAND, lower_only=1, epilogue=EPI_STORE,
                         role=CONG1, flops=(float(nb) * n3 / 3.0).hex(), spanA=ldl * ldl, spanB=afull - b0 * L["astride"])
                want.append((w, "step 1 " + tag, dict(spanA=ldl * ldl, spanB=afull - b0 * L["astride"])))
                for mask in (0, 0b0101):
                    row0 = 5 + b0
                    lines.append(f"STEP2 {n} {L['world']} {L['m']} {Bc} {ldl} {nb} {row0} {mask}")
                    w = zero_fields()
                    w.update(A=TBUF, lda=n16, strideA=nn, B=LINV, ldb=ldl, A2=LINV, lda2=ldl, B2=TBUF, ldb2=n16, strideB2=nn, C=DST, M=n16, N=n16,
                             K=n16, batch=nb, alpha=(1.0).hex(), klimit=KLIM_BY_N, lower_only=1, epilogue=EPI_BLOCKED, blk_row_stride=L["Lr"],
                             blk_row0=row0, nblk=L["nblk"], role=CONG2, tile_col_mask=mask, spanA=t_buf, spanB2=t_buf, spanB=ldl * ldl,
                             spanA2=ldl * ldl, flops=(float(nb) * n3 * 2.0 / 3.0 * mask_share(ntiles(n16), mask)).hex())
                    want.append((w, "step 2 " + tag, dict(spanA=t_buf, spanB2=t_buf, spanB=ldl * ldl, spanA2=ldl * ldl)))
        lines.append(f"IROW {n} {L['world']} {L['m']} {ldl} {L['mloc']}")
        w = zero_fields()
        w.update(A=LINV, lda=ldl, B=LINV, ldb=ldl, C=DST, M=n16, N=n16, K=n16, batch=1, alpha=(1.0).hex(), klimit=KLIM_BY_N, lower_only=1,
                 epilogue=EPI_BLOCKED, blk_row_stride=L["Lr"], blk_row0=L["mloc"], nblk=L["nblk"], role=GENERIC)
        want.append((w, f"I row {n}", {}))
    got = [parse(r) for r in run(driver, lines)]
    assert len(got) == len(want) > 500
    for g, (w, what, buffers) in zip(got, want):
        check(g, w, what)
        for k, cap in buffers.items():
            assert g[k] <= cap, (what, k)                                  # never more than the allocation
        if g["role"] == CONG2:                                             # the second pair mirrors the first
            assert (g["A2"], g["B2"], g["lda2"], g["ldb2"], g["strideA2"], g["strideB2"]) == (g["B"], g["A"], g["ldb"], g["lda"], g["strideB"], g["strideA"])
            assert g["lower_only"] and g["epilogue"] == EPI_BLOCKED and g["klimit"] == KLIM_BY_N and not g["a_kmajor"] and not g["b_kmajor"]


def split_counts(L, plan_nsplit):
    odd = next(s for s in range(3, 200) if L["npb_loc"] % s)              # a count that does not divide the rank's p-blocks
    return sorted({1, 8, plan_nsplit, odd})


def test_gram_forms(driver):
    lines, want = [], []
    for L, _, plan_nsplit in grid(driver):
        n, m, world, R = L["n"], L["m"], L["world"], L["R"]
        exch = world * L["npb_loc"] * L["Lr"] * 16 + PAD_DOUBLES           # an exchange buffer with its slack
        for nsplit in split_counts(L, plan_nsplit):
            chunk = -(-L["npb_loc"] // nsplit)
            z0, nz = (0, 1) if nsplit == 1 else (1, max(1, nsplit - 2))     # a proper sub-range of the splits
            for acc in (0, 1):
                lines.append(f"GRAM {n} {world} {m} {nsplit} {z0} {nz} {acc} {1 - acc}")
                rows = m + 3.0
                w = zero_fields()
                w.update(A=DST, B=DST, a_kmajor=1, b_kmajor=1, lda=16, ldb=16, a_kblk=L["Lr"] * 16, b_kblk=L["Lr"] * 16, C=SLAB, ldc=R, M=R, N=R,
                         K=L["npb_loc"] * 16, lower_only=1, epilogue=EPI_SLAB, batch=nz, k_chunk=chunk * 16, k_base=z0 * chunk * 16, slab_stride=R * R,
                         alpha=(1.0).hex(), beta=float(acc).hex(), role=GRAM, queue_global=1 - acc, spanA=exch, spanB=exch,
                         seg_rows=L["Lr"] if world > 1 else 0, seg_extra=(L["npb_loc"] - 1) * L["Lr"] * 16 if world > 1 else 0,
                         flops=(rows * (rows + 1.0) * 0.5 * (float(n) * (n + 1) * 0.5) * 2.0 / world * (nz / nsplit)).hex())
                want.append((w, f"Gram {n}/{world}/{m} nsplit {nsplit}"))
    got = [parse(r) for r in run(driver, lines)]
    assert len(got) == len(want) > 300
    for g, (w, what) in zip(got, want):
        check(g, w, what)
        assert g["k_chunk"] > 0 and g["k_chunk"] % 16 == 0, what


def test_gathered_and_lp_forms(driver):
    lines, want = [], []
    for n, world, m, nc, nz in ((144, 1, 24, 100, 3), (96, 2, 24, 2000, 8), (464, 1, 250, 33, 1)):
        L = layout(n, world, m)
        R, nc16 = L["R"], roundup(nc, 16)
        span = R * nc16 + ntiles(R) * TILE * 16 + PAD_DOUBLES               # the gather buffer (engine_build.h: signed_correction)
        for acc, alpha in ((0, -2.0), (1, 2.0)):
            lines.append(f"GATHERED {n} {world} {m} {nc} {nz} {alpha} {acc} {span}")
            w = zero_fields()
            w.update(A=ASRC, B=ASRC, a_kmajor=1, b_kmajor=1, lda=16, ldb=16, a_kblk=R * 16, b_kblk=R * 16, C=SLAB, ldc=R, M=R, N=R, K=nc16,
                     lower_only=1, epilogue=EPI_SLAB, batch=nz, k_chunk=-(-(nc16 // 16) // nz) * 16, slab_stride=R * R, alpha=alpha.hex(),
                     beta=float(acc).hex(), role=GRAM, queue_global=1, spanA=span, spanB=span, flops=(float(R) * (R + 1) * 0.5 * float(nc) * 2.0).hex())
            want.append((w, f"gathered {n} {nc}"))
    for m, ncol in ((40, 300), (250, 5000), (1, 7), (1000, 200000)):
        mpad = roundup(m, TILE)
        kc = min(roundup(ncol, 16), max(16, ((1 << 25) // mpad) // 16 * 16))   # columns per chunk (engine_lp.h)
        span = kc // 16 * mpad * 16 + PAD_DOUBLES                              # the dense buffer W
        for kv in sorted({min(kc, ncol), ncol % kc or kc}):                    # a full chunk and the last one
            lines.append(f"LP {ncol} 1 {m} {mpad} {kc} {kv} {mpad}")
            w = zero_fields()
            w.update(A=ASRC, B=ASRC, a_kmajor=1, b_kmajor=1, lda=16, ldb=16, a_kblk=mpad * 16, b_kblk=mpad * 16, C=SLAB, ldc=mpad, M=roundup(m, 16),
                     N=roundup(m, 16), K=roundup(kv, 16), lower_only=1, epilogue=EPI_STORE, batch=1, alpha=(1.0).hex(), beta=(1.0).hex(), role=GRAM,
                     spanA=span, spanB=span, flops=(float(m) * (m + 1) * float(kv)).hex())
            want.append((w, f"LP {m} x {ncol}"))
    got = [parse(r) for r in run(driver, lines)]
    for g, (w, what) in zip(got, want):
        check(g, w, what)


def test_plain_product(driver):
    """generic role, STORE epilogue; everything a site does not say is zero"""
    cases = [dict(M=144, N=32, K=144, alpha=1.0, beta=0.0, lda=256, a_kmajor=0, strideA=0, ldb=144, b_kmajor=1, strideB=0, ldc=144, klimit=KLIM_BY_M,
                  lower_only=0, batch=1, strideC=0),
             dict(M=256, N=256, K=128, alpha=-1.0, beta=1.0, lda=512, a_kmajor=0, strideA=0, ldb=512, b_kmajor=0, strideB=0, ldc=512, klimit=KLIM_NONE,
                  lower_only=1, batch=1, strideC=0),
             dict(M=128, N=128, K=128, alpha=-1.0, beta=0.0, lda=512, a_kmajor=1, strideA=131328, ldb=512, b_kmajor=1, strideB=131328, ldc=512,
                  klimit=KLIM_BY_M, lower_only=0, batch=2, strideC=131328)]
    keys = "M N K alpha beta lda a_kmajor strideA ldb b_kmajor strideB ldc klimit lower_only batch strideC".split()
    got = [parse(r) for r in run(driver, ["PLAIN 0 1 0 " + " ".join(str(c[k]) for k in keys) for c in cases])]
    for g, c in zip(got, cases):
        w = zero_fields()
        w.update({k: (v.hex() if k in FLOATS else v) for k, v in c.items()}, A=LINV, B=ASRC, C=DST, epilogue=EPI_STORE, role=GENERIC)
        check(g, w, "plain product")


def test_exchange_pieces_are_whole_groups_of_gram_splits(driver):
    lines, want = [], []
    for L, _, plan_nsplit in grid(driver):
        npb_loc = L["npb_loc"]
        for nsplit in split_counts(L, plan_nsplit):
            chunk = -(-npb_loc // nsplit)                                   # p-blocks per split: the one number both sides use
            lines.append(f"CHUNK {L['n']} {L['world']} {L['m']} {nsplit}")
            want.append([chunk])
            # the K ranges of the splits, cut at the rank's p-range, tile it without gap or overlap
            cuts = [(min(npb_loc, z * chunk), min(npb_loc, (z + 1) * chunk)) for z in range(nsplit)]
            assert cuts[0][0] == 0 and cuts[-1][1] == npb_loc and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
            for P in (p for p in range(1, nsplit + 1) if nsplit % p == 0):
                for k in range(P):
                    mine = cuts[k * nsplit // P:(k + 1) * nsplit // P]
                    lines.append(f"PIECE {L['n']} {L['world']} {L['m']} {nsplit} {k} {P}")
                    want.append([mine[0][0], mine[-1][1]])
    got = [[int(v) for v in r] for r in run(driver, lines)]
    assert len(got) > 1000 and got == want
