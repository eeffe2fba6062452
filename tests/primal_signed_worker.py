"""child process of tests/test_gpu_primal_signed.py: one KKT_TYPE_PRIMAL build of a synthetic block on an in-process loopback
device group (or one device), its results and route written to an .npz; the environment switches are the parent's.
usage: primal_signed_worker.py n m world x.npy out.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from hdsdp_amd import api  # noqa: E402

n, m, world = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
X = np.load(sys.argv[4])
out = {}
if world > 1:
    api.set_devices([0] * world, shard_min_dim=32)
cone = api.SDPCone.synthetic(n, m)
try:
    out["shards"] = np.array([cone.shard_count()])
    Rd = -2.5 * n
    cone.set_start(Rd)
    assert cone.check_is_interior(1.0, 0.02 * np.sin(1.3 * np.arange(m) + 0.4))
    kkt = api.KKT(m, [cone])
    kkt.register_psdp([X])
    try:
        kkt.build_up(api.KKT_TYPE_PRIMAL)
        ex = kkt.export()
        out["M"] = kkt.M.copy()
        out["ASinv"], out["ASinvRdSinv"], out["TraceSinv"] = ex["ASinv"], ex["ASinvRdSinv"], np.array([ex["TraceSinv"]])
        out["ok"] = np.array([1])
    except api.HDSDPError:
        out["ok"] = np.array([0])
    r = cone.primal_route()
    out["route"] = np.array([r[0], r[1], r[2]] if r else [-1, 0, 0.0])
    kkt.destroy()
finally:
    cone.destroy()
np.savez(sys.argv[5], **out)
print("primal_signed_worker: done", file=sys.stderr, flush=True)
