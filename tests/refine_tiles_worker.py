"""child process of tests/test_gpu_refine_tiles.py: the arrow128 golden cones' sparse Schur operator in tile form under whatever
HDSDP_MI355X_REFINE / HDSDP_MI355X_REFINE_TILES the parent set (HKKTInit reads both); prints the operator's refinement state
before and after one solve as JSON"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from hdsdp_amd import api  # noqa: E402
from util import load_golden, y_of  # noqa: E402

g = load_golden("arrow128_A")
m = int(g["mb_dims"][1])
prob = api.read_sdpa(os.path.join(ROOT, "tests", "golden", "arrow128.dat-s"))
cones = [api.SDPCone.from_csc(blk["n"], m, blk["beg"], blk["idx"], blk["val"], iCone=k) for k, blk in enumerate(prob["blocks"])]
for cn in cones:
    cn.set_start(float(g["Rd"][0]))
    assert cn.check_is_interior(float(g["tau"][0]), y_of(g))
kkt = api.KKT(m, cones)
out = {"tile_form": kkt.tile_info() is not None, "switch": kkt.refine_tiles(), "before": kkt.refine_stats()}
kkt.build_up(api.KKT_TYPE_INFEASIBLE)
kkt.regularize(1e-3)
A = np.triu(kkt.M) + np.triu(kkt.M, 1).T
kkt.factorize()
b = np.sin(np.arange(m) + 1.0)
x = kkt.solve(b)
out["after"] = kkt.refine_stats()
out["residual"] = float(np.linalg.norm(A @ x - b) / np.linalg.norm(b))
out["cond"] = float(np.linalg.cond(A))
kkt.destroy()
for cn in cones:
    cn.destroy()
print("REFINE_TILES_WORKER_JSON " + json.dumps(out))
