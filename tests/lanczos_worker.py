"""child process of tests/test_gpu_lanczos_forms.py and tools/lanczos_fixture.py: three consecutive ratio tests (one fresh, two
warm-started) on five blocks, one per size class of the form rule (csrc/lanczos_rule.h: hdm_lz_form); the steps go out as
hexadecimal floats, one JSON line.  The HDM_LANCZOS_* switches of the environment decide which form runs."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from util import load_golden, y_of  # noqa: E402
from hdsdp_amd import api  # noqa: E402

# (name, n, m): a golden of the compiled reference where m is None, else the synthetic family at y = 0
BLOCKS = [("syn100", 100, None),      # resident
          ("n144", 144, 4),           # the first size past the resident form
          ("syn200", 200, None),
          ("n272", 272, 4),           # the first size on the 8-trip co-resident form
          ("n2064", 2064, 4)]         # the first size on the 16-trip form


def run_block(name, n, m):
    if m is None:
        g = load_golden(name)
        assert int(g["dims"][0]) == n
        cone = api.SDPCone.synthetic(n, int(g["dims"][1]))
        cone.set_start(float(g["Rd"][0]))
        assert cone.check_is_interior(float(g["tau"][0]), y_of(g))
        calls = [(float(g["rt_par" + t][0]), g["rt_dy" + t], float(g["rt_par" + t][1])) for t in ("1", "2", "2")]
    else:
        cone = api.SDPCone.synthetic(n, m)
        cone.set_start(-10.0 * n)
        assert cone.check_is_interior(1.0, np.zeros(m))
        calls = [(0.0, 40.0 * np.cos(0.7 * np.arange(m) + 0.2), 0.0)] * 3
    steps = [float(cone.ratio_test(*c)).hex() for c in calls]
    cone.destroy()
    return steps


if __name__ == "__main__":
    out = {name: run_block(name, n, m) for name, n, m in BLOCKS}
    print("LANCZOS_WORKER_JSON " + json.dumps(out), flush=True)
