"""Every form of the ratio test (csrc/lanczos_rule.h: hdm_lz_form) against what the parent commit computed on the same GPU:
tests/golden/lanczos_parent.json, written by tools/lanczos_fixture.py from a build of the parent.  Six settings of the
HDM_LANCZOS_* switches, which the library reads once per process: one child (tests/lanczos_worker.py) per setting, one after the
other, each under its own time limit, and none is started after one that ended abnormally.  In each child three consecutive
ratio tests (one fresh, two warm-started) on five blocks: n = 100 (resident), 144 (the first size past it), 200, 272 (the first on
the 8-trip co-resident form) and 2064 (the first on the 16-trip form).  Every step must equal the parent's bit for bit."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = [
    {},
    {"HDM_LANCZOS_WHOLE": "0"},
    {"HDM_LANCZOS_WHOLE": "0", "HDM_LANCZOS_FUSED": "0"},
    {"HDM_LANCZOS_WHOLE": "0", "HDM_LANCZOS_FUSED": "0", "HDM_LANCZOS_GROUP": "0"},
    {"HDM_LANCZOS_BIG": "0"},
    {"HDM_LANCZOS_BIG": "0", "HDM_LANCZOS_GROUP": "0"},
]


def setting_id(s):
    return ",".join(f"{k}={v}" for k, v in s.items()) or "defaults"


def run_settings(extra_env=None, timeout=120):
    """{setting id: {block: [three hex steps]}} up to the first child that ended abnormally; that one's entry is its output"""
    base = {k: v for k, v in os.environ.items() if not (k.startswith("HDM_") or k.startswith("HDSDP_MI355X_"))}
    base.update(extra_env or {})
    got = {}
    for s in SETTINGS:
        env = dict(base)
        env.update(s)
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "lanczos_worker.py")], capture_output=True, text=True, timeout=timeout, env=env)
        except subprocess.TimeoutExpired as e:
            got[setting_id(s)] = "timed out: " + str(e)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("LANCZOS_WORKER_JSON ")]
        if r.returncode != 0 or not line:
            got[setting_id(s)] = "exit %d: %s" % (r.returncode, (r.stdout + r.stderr)[-2000:])
            break
        got[setting_id(s)] = json.loads(line[-1][len("LANCZOS_WORKER_JSON "):])
    return got


@pytest.fixture(scope="module")
def runs():
    return run_settings()


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(HERE, "golden", "lanczos_parent.json")) as f:
        return json.load(f)["steps"]


@pytest.mark.parametrize("setting", SETTINGS, ids=[setting_id(s) for s in SETTINGS])
def test_every_form_gives_the_parents_steps_bit_for_bit(setting, runs, parent):
    sid = setting_id(setting)
    assert sid in runs, "not run: an earlier setting's child ended abnormally"
    assert isinstance(runs[sid], dict), runs[sid]
    assert sorted(runs[sid]) == sorted(parent[sid]) and len(parent[sid]) == 5
    for block, want in parent[sid].items():
        assert len(want) == 3
        assert runs[sid][block] == want, (sid, block, [float.fromhex(v) for v in runs[sid][block]], [float.fromhex(v) for v in want])
