"""Writes tests/golden/gemm_geom_parent.json: what the GEMM launcher (csrc/gemm_f64.hip) says about a grid of launches -- the flops
their MFMA instructions execute (issued_mfma_flops, every role and tile subset) and how far each operand's unmasked tile loads
reach (the `need` of the launcher's span check, read from its own refusal when the caller vouches for nothing).  It is meant to be
run on the commit BEFORE those rules moved into csrc/gemm_geom.h and again on the tree, which must reproduce every integer.

The "host" section needs no device: a host-only program includes gemm_f64.hip, stands in for the allocator and the persistent
launcher, calls issued_mfma_flops directly and lets hdm_launch_gemm refuse.  The "device" section is written only where a device
and a built library are found: one Schur build per shape with kernel timing on, recording per role the algorithmic flops, the
issued flops and the launch count of HMiGetKernelTimingEx, and M itself (float.hex(), bit for bit).

    python tools/gemm_geom_fixture.py [--csrc DIR] [--no-device] [out.json]
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GENERIC, CONG1, CONG2, GRAM, CONG2D = range(5)          # HdmRole
KLIM_NONE, KLIM_BY_M, KLIM_BY_N, KLIM_BAND = range(4)   # HdmKLimit
EPI_STORE, EPI_BLOCKED, EPI_SLAB = range(3)             # HdmEpilogue
SIZES = (128, 144, 256, 336, 384, 464, 2000, 8256)      # M = N = K; 8256: more than 64 tile columns (the mask is ignored)
DEVICE_SHAPES = ((128, 24), (144, 24), (384, 24), (464, 24))
FIELDS = ("role", "M", "N", "K", "klimit", "lower_only", "colmask", "epilogue", "batch", "k_base", "k_chunk", "a_kmajor", "b_kmajor",
          "a_kblk", "b_kblk", "lda", "ldb", "lda2", "ldb2", "strideA", "strideB", "strideA2", "strideB2", "seg_rows", "seg_extra",
          "b_sky", "second")

DRIVER = r"""
#include "gemm_f64.hip"
#include <iostream>
#include <sstream>
#include <string>
// no device: nothing is allocated and nothing is launched
hipError_t hdm_malloc(void **p, size_t) { *p = nullptr; return hipErrorOutOfMemory; }
bool hdm_persist_supported(bool, bool, int, int) { return false; }
int hdm_launch_persist(bool, bool, int, int, dim3, dim3, hipStream_t, const HdmGemmDev &, int *) { return 1; }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned long long v[27];   // (a column mask may have bit 63 set; nothing here is negative)
        for (auto &x : v) if (!(in >> x)) return 2;
        HdmGemmArgs a = {};
        a.role = (int) v[0]; a.M = (int) v[1]; a.N = (int) v[2]; a.K = (int) v[3]; a.klimit = (int) v[4]; a.lower_only = (int) v[5];
        a.tile_col_mask = (unsigned long long) v[6]; a.epilogue = (int) v[7]; a.batch = (int) v[8]; a.k_base = (long) v[9]; a.k_chunk = (long) v[10];
        a.a_kmajor = (int) v[11]; a.b_kmajor = (int) v[12]; a.a_kblk = v[13]; a.b_kblk = v[14];
        a.lda = v[15]; a.ldb = v[16]; a.lda2 = v[17]; a.ldb2 = v[18];
        a.strideA = v[19]; a.strideB = v[20]; a.strideA2 = v[21]; a.strideB2 = v[22];
        a.seg_rows = v[23]; a.seg_extra = v[24]; a.b_sky = (int) v[25];
        a.nblk = a.N / 16; a.blk_row_stride = 8; a.alpha = 1.0;
        static double mem[2];
        a.A = mem; a.B = mem + 1; a.C = mem;
        if (v[26]) { a.A2 = a.B; a.B2 = a.A; }
        printf("ISSUED %.17g %.17g %.17g\n", issued_mfma_flops(a, 0), issued_mfma_flops(a, 1), issued_mfma_flops(a, 2));
        fflush(stdout);
        // the span check: every operand but one vouched for without bound, that one for nothing -- the refusal names its need
        if (a.role != HDM_ROLE_GENERIC)
            for (int op = 0; op < (v[26] ? 4 : 2); ++op) {
                HdmGemmArgs s = a;
                const long big = 1L << 62;
                s.spanA = op == 0 ? 0 : big; s.spanB = op == 1 ? 0 : big; s.spanA2 = op == 2 ? 0 : big; s.spanB2 = op == 3 ? 0 : big;
                if (hdm_launch_gemm(s, nullptr) != 1) return 3;
            }
        fprintf(stderr, "END\n");
        fflush(stderr);
    }
    return 0;
}
"""


def case(role, n, **kw):
    c = dict.fromkeys(FIELDS, 0)
    c.update(role=role, M=n, N=n, K=n, batch=1, lda=n, ldb=n, lda2=n, ldb2=n)
    c.update(kw)
    return c


def grid():
    """every tile class and every K rule: the three Schur roles as the engine launches them, step 2's two kernels, generic
    launches under each K limit; with and without a tile-column mask, batch 1 and 8, split-K with odd and even stage counts and a
    first split off zero, row segments and the skyline operand on and off"""
    out = []
    for n in SIZES:
        nn = n * n
        for batch in (1, 8):
            for sky in (0, 1):
                out.append(case(CONG1, n, klimit=KLIM_BAND, lower_only=1, epilogue=EPI_STORE, batch=batch, b_kmajor=1, b_sky=sky,
                                strideB=nn, ldb=n))
            for mask in (0, 0b0101, 0b0010, (1 << 63) | 1):
                step2 = dict(klimit=KLIM_BY_N, lower_only=1, epilogue=EPI_BLOCKED, batch=batch, colmask=mask, strideA=nn)
                out.append(case(CONG2, n, second=1, strideB2=nn, **step2))
                out.append(case(CONG2D, n, **step2))
            # Gram: K-major operands in [k block][row][16] storage; k_chunk 48 / 64: 3 / 4 stages per split
            for chunk in (48, 64):
                for base in (0, 32):
                    for seg in (0, 1):
                        out.append(case(GRAM, n, klimit=KLIM_NONE, lower_only=1, epilogue=EPI_SLAB, batch=batch, k_base=base,
                                        k_chunk=chunk, a_kmajor=1, b_kmajor=1, lda=16, ldb=16, a_kblk=16 * n, b_kblk=16 * n,
                                        seg_rows=128 * seg, seg_extra=4096 * seg))
        for klimit in (KLIM_NONE, KLIM_BY_M, KLIM_BY_N, KLIM_BAND):
            for lower in (0, 1):
                for second in (0, 1):
                    out.append(case(GENERIC, n, klimit=klimit, lower_only=lower, epilogue=EPI_STORE, batch=2, second=second,
                                    colmask=0b0110 * lower))
    return out


def build_driver(csrc, workdir):
    src, exe = os.path.join(workdir, "gemm_geom_parent.cpp"), os.path.join(workdir, "gemm_geom_parent")
    with open(src, "w") as f:
        f.write(DRIVER)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # the host side only (the kernels take minutes to compile and are never launched here); the code bundle the host object
    # registers at load time is then an empty one of our own
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", csrc, "-c", src, "-o", exe + ".o"])
    syms = subprocess.check_output(["nm", exe + ".o"], text=True)
    bundle = re.search(r"\bU (__hip_fatbin_\w+)", syms).group(1)
    with open(exe + "_bundle.c", "w") as f:
        f.write(f'const char {bundle}[32] __attribute__((aligned(4096))) = "__CLANG_OFFLOAD_BUNDLE__";\n')
    subprocess.check_call([hipcc, "-c", "-x", "c", exe + "_bundle.c", "-o", exe + "_bundle.o"])
    subprocess.check_call([hipcc, exe + ".o", exe + "_bundle.o", "-o", exe])
    return exe


def host_section(csrc):
    cases = grid()
    with tempfile.TemporaryDirectory() as d:
        exe = build_driver(csrc, d)
        text = "".join(" ".join(str(c[f]) for f in FIELDS) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    issued = [[int(float(x)) for x in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("ISSUED")]
    refusals = r.stderr.split("END\n")[:-1]
    assert len(issued) == len(cases) == len(refusals), (len(issued), len(cases), len(refusals))
    for c, iss, ref in zip(cases, issued, refusals):
        c["issued"] = iss
        c["need"] = {m.group(1): int(m.group(2)) for m in re.finditer(r"operand (\w+) needs (-?\d+) readable", ref)}
        assert len(c["need"]) == (0 if c["role"] == GENERIC else 4 if c["second"] else 2), ref
    return cases


def device_record(n, m):
    """one HKKTBuildUp of the synthetic dense block (congruence + Gram path) with kernel timing on: per role
    [flops, issued, launches] of HMiGetKernelTimingEx, and M (lower triangle), every double as float.hex()"""
    import ctypes as C
    import numpy as np
    from hdsdp_amd import api
    lib = api.load_library()
    cone = api.SDPCone.synthetic(n, m)
    try:
        cone.set_start(-200.0)
        assert cone.check_is_interior(0.9, 0.05 * np.sin(1.7 * np.arange(1, m + 1))) and cone.path == 0
        kkt = api.KKT(m, [cone])
        ms, fl, iss, ln = np.zeros(5), np.zeros(5), np.zeros(5), np.zeros(5, dtype=np.int64)
        dp = C.POINTER(C.c_double)
        lib.HMiGetKernelTimingEx(ms.ctypes.data_as(dp), fl.ctypes.data_as(dp), iss.ctypes.data_as(dp), ln.ctypes.data_as(C.POINTER(C.c_int64)))
        lib.HMiSetKernelTiming(1)
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        lib.HMiSetKernelTiming(0)
        lib.HMiGetKernelTimingEx(ms.ctypes.data_as(dp), fl.ctypes.data_as(dp), iss.ctypes.data_as(dp), ln.ctypes.data_as(C.POINTER(C.c_int64)))
        M = np.array(kkt.M, dtype=np.float64)          # C order: M[j, i] is element (row i, column j), valid where i >= j
        rec = {"m": m, "roles": [[float(fl[r]).hex(), float(iss[r]).hex(), int(ln[r])] for r in range(5)],
               "M": [float(M[j, i]).hex() for j in range(m) for i in range(j, m)]}
        kkt.destroy()
        return rec
    finally:
        cone.destroy()


def device_section():
    return {str(n): device_record(n, m) for n, m in DEVICE_SHAPES}


def main(argv):
    csrc = os.path.join(ROOT, "hdsdp_amd", "csrc")
    if "--csrc" in argv:
        csrc = argv.pop(argv.index("--csrc") + 1)
        argv.remove("--csrc")
    device = "--no-device" not in argv
    out = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "tests", "golden", "gemm_geom_parent.json"))
    res = {"fields": list(FIELDS), "host": host_section(csrc)}
    if device:
        import torch
        device = torch.cuda.is_available()
    if device:
        res["device"] = device_section()
    elif os.path.exists(out):                           # keep a device section recorded earlier
        with open(out) as f:
            old = json.load(f)
        if "device" in old:
            res["device"] = old["device"]
    with open(out, "w") as f:
        json.dump(res, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(res['host'])} launches" + (", device section" if "device" in res else ", no device section"))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)                                # (run as a script, the package is not on the path; an importer has it)
    main(sys.argv[1:])
