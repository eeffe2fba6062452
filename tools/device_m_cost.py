"""Step and build time with the host mirror of M on and off (the diagonal channel), one device.

A step is what the reference's driver does per Schur build: interior check, HKKTBuildUp, the bound cone on y through
HKKTBuildUpExtraCone (a stand-in that adds its diagonal through kktDiag[], as interface/hdsdp_conic_bound.c:201-249),
HKKTRegularize(1e-6), HKKTFactorize and three solves.  "build" is HKKTBuildUp + the extra cone alone (with the mirror on,
the copy of M to the host is part of it).  One JSON line per (n, m, mirror).
usage: tools/device_m_cost.py [n:m ...]        (default 2000:2000 2000:8000)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdsdp_amd import api  # noqa: E402

BUILD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int)


class HostCone(C.Structure):   # hdsdp_cone, interface/def_hdsdp_conic.h:60-100
    _fields_ = [("iCone", C.c_int), ("cone", C.c_int), ("usrData", C.c_void_p), ("coneData", C.c_void_p),
                ("slots", C.c_void_p * 30)]


def bound_stand_in(m, y, lo, up):
    """the bound cone's diagonal (1/(y-l))^2 + (1/(u-y))^2 added through kktDiag[] in one strided numpy pass"""
    add = (1.0 / (y - lo)) ** 2 + (1.0 / (up - y)) ** 2

    @BUILD_FN
    def build(cone_data, icone, kkt_ptr, type_kkt):
        if type_kkt == api.KKT_TYPE_CORRECTOR:
            return 0
        k = C.cast(kkt_ptr, C.POINTER(api.hdsdp_kkt)).contents
        p0 = C.cast(k.kktDiag[0], C.c_void_p).value
        stride = (C.cast(k.kktDiag[1], C.c_void_p).value - p0) // 8   # 1 (channel) or m + 1 (dense host matrix)
        buf = np.ctypeslib.as_array((C.c_double * ((m - 1) * stride + 1)).from_address(p0))
        buf[::stride] += add
        return 0
    cone = HostCone()
    cone.slots[11] = C.cast(build, C.c_void_p)
    cone._keep = build
    return cone


def measure(n, m, reps=5):
    lib = api.load_library()
    cone = api.SDPCone.synthetic(n, m)
    cone.set_start(-10.0 * n)
    y = np.zeros(m)
    b = cone.traces()
    host = bound_stand_in(m, y, -1.0, 1.0)
    hp = C.cast(C.pointer(host), C.c_void_p)
    out = []
    for mirror in (True, False):
        kkt = api.KKT(m, [cone], host_mirror=mirror)

        def build():
            kkt.build_up(api.KKT_TYPE_INFEASIBLE)
            assert lib.HKKTBuildUpExtraCone(kkt._k, hp, api.KKT_TYPE_INFEASIBLE) == 0

        def step():
            assert cone.check_is_interior(1.0, y)
            build()
            kkt.regularize(1e-6)
            kkt.factorize()
            e = kkt.export()
            return kkt.solve(b), kkt.solve(e["ASinv"]), kkt.solve(e["ASinvRdSinv"])
        first = step()
        t0 = time.perf_counter()
        for _ in range(reps):
            step()
        t_step = (time.perf_counter() - t0) / reps
        api.load_library().HMiDeviceSynchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            build()
        api.load_library().HMiDeviceSynchronize()
        t_build = (time.perf_counter() - t0) / reps
        h, d = kkt.matrix_traffic()
        calls = 2 * reps + 1
        out.append({"n": n, "m": m, "mirror": int(mirror), "step_ms": round(t_step * 1e3, 2), "build_ms": round(t_build * 1e3, 2),
                    "bytes_to_host_per_build": h // calls, "bytes_to_device_per_factorize": d // (reps + 1), "d1": first[0]})
        kkt.destroy()
    cone.destroy()
    same = np.array_equal(out[0]["d1"], out[1]["d1"])
    for o in out:
        o.pop("d1")
        o["solution_bit_identical"] = bool(same)
        print(json.dumps(o), flush=True)
    return out


if __name__ == "__main__":
    sizes = sys.argv[1:] or ["2000:2000", "2000:8000"]
    for s in sizes:
        n, m = (int(v) for v in s.split(":"))
        measure(n, m)
