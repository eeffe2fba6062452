"""child process of tests/test_gpu_refine.py: a small dense Schur operator under whatever HDSDP_MI355X_REFINE the parent set
(HKKTInit reads it); prints the operator's refinement state before and after one solve as JSON"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from hdsdp_amd import api  # noqa: E402

n = m = 32
cone = api.SDPCone.synthetic(n, m)
cone.set_start(-10.0 * n)
assert cone.check_is_interior(1.0, np.zeros(m))
kkt = api.KKT(m, [cone])
out = {"before": kkt.refine_stats()}
kkt.build_up(api.KKT_TYPE_INFEASIBLE)
A = np.triu(kkt.M) + np.triu(kkt.M, 1).T
kkt.factorize()
b = np.cos(np.arange(m) + 0.5)
x = kkt.solve(b)
out["after"] = kkt.refine_stats()
out["residual"] = float(np.linalg.norm(A @ x - b) / np.linalg.norm(b))
out["cond"] = float(np.linalg.cond(A))
kkt.destroy()
cone.destroy()
print("REFINE_WORKER_JSON " + json.dumps(out))
