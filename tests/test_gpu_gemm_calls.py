"""Every call site of the fp64 GEMM family after the call forms of csrc/gemm_calls.h, bit for bit against the commit before them:
tests/golden/gemm_calls_parent.json holds, per case, the per-role [flops, issued, launches] of HMiGetKernelTimingEx and the
results (every double as float.hex(), large arrays as the SHA-256 of their bytes) that commit gave; tools/gemm_calls_fixture.py
says what the cases are and records them.  The arguments of every launch are the same, so the bits are: no tolerance."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.gemm_calls_fixture import CASES, MAY_DIFFER, record  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "gemm_calls_parent.json")) as _f:
    WANT = json.load(_f)


def test_every_deterministic_case_is_in_the_fixture():
    assert set(CASES) - set(WANT) <= set(MAY_DIFFER) and set(WANT) <= set(CASES)


def differences(got, want, where=""):
    if isinstance(want, dict) and isinstance(got, dict) and set(got) == set(want):
        return [d for k in sorted(want) for d in differences(got[k], want[k], f"{where}/{k}")]
    if isinstance(want, list) and isinstance(got, list) and len(got) == len(want):
        return [d for i, (g, w) in enumerate(zip(got, want)) for d in differences(g, w, f"{where}[{i}]")]
    return [] if got == want else [f"{where}: {got!r}, the parent's {want!r}"]


@pytest.mark.parametrize("name", sorted(WANT))
def test_case_computes_and_reports_what_the_parent_commit_did(name):
    got = json.loads(json.dumps(record(name)))
    diff = differences(got, WANT[name])
    assert not diff, f"{name}: {len(diff)} differences, the first: {diff[:5]}"
