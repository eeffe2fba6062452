"""writes tests/golden/lanczos_parent.json: the steps of tests/lanczos_worker.py under the six switch settings of
tests/test_gpu_lanczos_forms.py, as THIS build computes them on the GPU at hand.  Run it on a build of the parent commit
(or point it at one: --lib PATH/libhdsdp_mi355x.so) and commit the file with the change that must reproduce it.

    python tools/lanczos_fixture.py [--lib LIBRARY] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_lanczos_forms as forms  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="library to record (default: the tree's own build)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lanczos_parent.json"))
    a = ap.parse_args()
    steps = forms.run_settings({"HDSDP_MI355X_LIB": os.path.abspath(a.lib)} if a.lib else None)
    bad = [k for k, v in steps.items() if not isinstance(v, dict)]
    if bad or len(steps) != len(forms.SETTINGS):
        sys.exit("a child ended abnormally: %s" % {k: steps[k] for k in bad})
    with open(a.out, "w") as f:
        json.dump({"what": "ratio-test steps (hexadecimal floats) per switch setting and block, three consecutive tests each; "
                           "see tests/lanczos_worker.py", "steps": steps}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)
