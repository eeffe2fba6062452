"""The rules and the host half of the ratio test (csrc/lanczos_rule.h, csrc/lanczos_host.h) without a device: the headers are
compiled alone with the host C++ compiler beside tests/lanczos_rule_driver.cpp.  Expected values are written here from the
rules as they are stated, not from what the code gives:

- constants: Krylov dimension 30, a check every min(3, 30 / 5) = 3 steps, warm-start weight 1e-3, residual threshold 1e-4, gap
  floor 1e-16, acceptance bounds 1e-3 and 0.5, single-workgroup forms up to n16 = 256, resident up to 128, co-resident for
  256 < n16 <= 4096 (8 trips up to 2048, 16 above) on min(256, CUs) workgroups of 16 columns at most, 32 chunks;
- the mailbox: no two ranges overlap, all inside 128 doubles, the group block holds three pairs, a count and the give-up word;
- the form rule:
      n16 <= 128          one launch, resident       } WHOLE=0: fused groups; and FUSED=0: queued
      128 < n16 <= 256    one launch, from global    }
      256 < n16 <= 2048   co-resident, 8 trips       } BIG=0, big_ok cleared, a shared device, no CU count, or
      2048 < n16 <= 4096  co-resident, 16 trips      }   ceil(n16 / min(256, CUs)) > 16: queued
      4096 < n16          queued
  and "queued" is "stepwise" under GROUP=0;
- a check is due after every third step and at a zero norm; a group runs up to the next check;
- the acceptance rule: gap = eig1 - eig2 - r2, floored at 1e-16 where not positive; gamma = min(r1, r1^2 / gap); accepted if
  gamma < 1e-3 or gamma + eig1 <= 0.5, with step 1 / (gamma + eig1), infinite where gamma + eig1 <= 0; else a zero norm is a
  failure, and anything else continues with the provisional step 1 / (gamma + eig1);
- the eigen-solvers against numpy.linalg.eigh within the textbook bound of tql2, 100 k eps |T|_2, values and residuals;
- the driver, over a backend of dense loops, against the compiled reference's rt_step1 / rt_step2 (fresh, then warm-started)
  to RATIO_TOL, and the two breakdown cases dS = -c I (step 1 / c) and dS = +c I (unbounded)."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from util import RATIO_TOL, load_golden, y_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

RESIDENT, GLOBAL, FUSED, GROUP8, GROUP16, QUEUED, STEPWISE = range(7)
ACCEPTED, CONTINUE, FAILED = range(3)
SWITCHES = ("HDM_LANCZOS_WHOLE", "HDM_LANCZOS_FUSED", "HDM_LANCZOS_GROUP", "HDM_LANCZOS_BIG")
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lanczos_rule") / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "lanczos_rule_driver.cpp")])
    return exe


def run(exe, lines, env=None):
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    base.update(env or {})
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, env=base).stdout
    return [row.split() for row in out.splitlines()]


def hx(v):
    return float(v).hex()


def fl(tokens):
    return [float.fromhex(t) for t in tokens]


# ---- constants and mailbox ------------------------------------------------------------------
def test_constants(driver):
    t = run(driver, ["CONST"])[0]
    assert [int(t[0]), int(t[1])] == [30, min(3, 30 // 5)]
    assert fl(t[2:7]) == [1e-3, 1e-4, 1e-16, 1e-3, 0.5]
    assert [int(v) for v in t[7:]] == [256, 128, 4096, 2048, 256, 16, 32]


def test_mailbox_ranges_are_disjoint_and_fit(driver):
    r1, r2, y1, carry, group, group_len, whole, whole_len, y2, size = (int(v) for v in run(driver, ["MAILBOX"])[0])
    assert size == 128 and whole_len == 3
    assert group_len >= 2 * 3 + 2                     # three (alpha, norm) pairs, the count, the give-up word
    ranges = sorted([(r1, 1), (r2, 1), (y1, 30), (carry, 1), (group, group_len), (whole, whole_len), (y2, 30)])
    assert ranges[0][0] >= 0
    for (a, la), (b, _) in zip(ranges, ranges[1:]):
        assert a + la <= b, (a, la, b)
    assert ranges[-1][0] + ranges[-1][1] <= size
    assert group + 2 * 8 + 2 > whole                  # (the block would NOT hold the eight steps the loop once allowed)


# ---- form rule ----------------------------------------------------------------------------
def expected_form(n16, whole, fused, group, big, big_ok, shared, cus):
    queued = QUEUED if group else STEPWISE
    if n16 <= 256:
        if whole:
            return RESIDENT if n16 <= 128 else GLOBAL
        return FUSED if fused else queued
    if n16 > 4096 or not big or not big_ok or shared or cus <= 0:
        return queued
    if -(-n16 // min(256, cus)) > 16:
        return queued
    return GROUP8 if n16 <= 2048 else GROUP16


def test_form_rule_for_every_combination(driver):
    combos = list(itertools.product((16, 128, 144, 256, 272, 2048, 2064, 4096, 4112), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (0, 1),
                                    (0, 64, 256)))
    assert len(combos) == 9 * 16 * 2 * 2 * 3
    rows = run(driver, ["FORM " + " ".join(str(v) for v in c) for c in combos])
    for c, row in zip(combos, rows):
        assert int(row[0]) == expected_form(*c), c
    # the table's rows with everything at its default, on a whole device and on a quarter of one
    got = {(n16, cus): int(run(driver, [f"FORM {n16} 1 1 1 1 1 0 {cus}"])[0][0]) for n16 in (16, 128, 144, 256, 272, 2048, 2064, 4096, 4112)
           for cus in (64, 256)}
    assert [got[n, 256] for n in (16, 128, 144, 256, 272, 2048, 2064, 4096, 4112)] == [RESIDENT, RESIDENT, GLOBAL, GLOBAL, GROUP8, GROUP8,
                                                                                       GROUP16, GROUP16, QUEUED]
    # 64 workgroups of 16 columns reach n16 = 1024: ceil(272 / 64) = 5, ceil(2048 / 64) = 32
    assert [got[n, 64] for n in (272, 2048, 2064, 4096)] == [GROUP8, QUEUED, QUEUED, QUEUED]
    assert [int(r[0]) for r in run(driver, ["FORM 1024 1 1 1 1 1 0 64", "FORM 1040 1 1 1 1 1 0 64", "FORM 1040 1 1 0 1 1 0 64"])] == \
        [GROUP8, QUEUED, STEPWISE]


def test_switches_are_read_once(driver):
    assert run(driver, ["SWITCHES"]) == [["1", "1", "1", "1"]]
    for k, name in enumerate(SWITCHES):
        want = ["1", "1", "1", "1"]
        assert run(driver, ["SWITCHES"], env={name: "1"}) == [want]
        want[k] = "0"
        assert run(driver, ["SWITCHES"], env={name: "0"}) == [want]
    rows = run(driver, ["SWITCHES"] + [f"SETENV {name} 0" for name in SWITCHES] + ["SWITCHES"])
    assert rows == [["1", "1", "1", "1"], ["1", "1", "1", "1"]]


# ---- predicates and acceptance rule ------------------------------------------------------------
def test_check_due_and_group_length(driver):
    rows = run(driver, [f"DUE {k} {hx(nrm)}" for k in range(30) for nrm in (1.0, 0.0)])
    for k in range(30):
        pos, zero = rows[2 * k], rows[2 * k + 1]
        assert int(pos[0]) == int(k in (2, 5, 8, 11, 14, 17, 20, 23, 26, 29)), k
        assert int(zero[0]) == 1, k
        assert int(pos[1]) == int(zero[1]) == 3 - k % 3, k       # steps up to and including the next check; 30 = 10 x 3
    # the two residuals: below the threshold, and at the last step whatever the estimate
    assert run(driver, [f"RESID {hx(np.nextafter(1e-4, 0.0))} 2", f"RESID {hx(1e-4)} 2", f"RESID {hx(1.0)} 28", f"RESID {hx(1.0)} 29"]) == \
        [["1"], ["0"], ["0"], ["1"]]


def accept(driver, eig1, eig2, r1, r2, nrm):
    t = run(driver, ["ACCEPT " + " ".join(hx(v) for v in (eig1, eig2, r1, r2, nrm))])[0]
    return int(t[0]), float.fromhex(t[1])


def test_acceptance_rule(driver):
    # a gap below the floor (eig1 - eig2 - r2 = -0.1): gamma = min(1e-9, 1e-18 / 1e-16 = 1e-2) = 1e-9 < 1e-3
    assert accept(driver, 1.0, 1.0, 1e-9, 0.1, 1.0) == (ACCEPTED, 1.0 / (1e-9 + 1.0))
    # ... and a gap of exactly zero is floored too: gamma = min(1e-10, 1e-20 / 1e-16 = 1e-4)
    assert accept(driver, 3.0, 2.0, 1e-10, 1.0, 1.0) == (ACCEPTED, 1.0 / (1e-10 + 3.0))
    # r1 above r1^2 / gap (r1 = 0.01 < gap = 1): gamma = 1e-4 < 1e-3
    assert accept(driver, 2.0, 1.0, 0.01, 0.0, 1.0) == (ACCEPTED, 1.0 / (0.01 * 0.01 / 1.0 + 2.0))
    # r1 below r1^2 / gap (r1 = 4 > gap = 1): gamma = 4, gamma + eig1 = 6: not accepted, provisional step
    assert accept(driver, 2.0, 1.0, 4.0, 0.0, 1.0) == (CONTINUE, 1.0 / 6.0)
    # ... where a zero norm is a failure
    assert accept(driver, 2.0, 1.0, 4.0, 0.0, 0.0)[0] == FAILED
    # gamma + eig1 at 0 (gap 0.25, r1 = 0.5: gamma = min(0.5, 1) = 0.5): accepted, unbounded; just above 0: a finite step
    assert accept(driver, -0.5, -0.75, 0.5, 0.0, 1.0) == (ACCEPTED, float("inf"))
    assert accept(driver, -1.5, -1.75, 0.5, 0.0, 1.0) == (ACCEPTED, float("inf"))
    assert accept(driver, -0.25, -0.5, 0.5, 0.0, 1.0) == (ACCEPTED, 4.0)
    # gamma + eig1 at 0.5: accepted; one step of 2^-40 above: not
    assert accept(driver, 0.0, -0.25, 0.5, 0.0, 1.0) == (ACCEPTED, 2.0)
    tiny = 2.0 ** -40
    assert accept(driver, tiny, tiny - 0.25, 0.5, 0.0, 1.0) == (CONTINUE, 1.0 / (0.5 + tiny))
    assert accept(driver, tiny, tiny - 0.25, 0.5, 0.0, 0.0)[0] == FAILED
    # a zero norm with an accepted pair is accepted
    assert accept(driver, 0.0, -0.25, 0.5, 0.0, 0.0) == (ACCEPTED, 2.0)
    assert accept(driver, 2.0, 1.0, 0.01, 0.0, 0.0) == (ACCEPTED, 1.0 / (1e-4 + 2.0))


# ---- eigen-solvers ----------------------------------------------------------------------------
def tridiagonals():
    rng = np.random.default_rng(11)
    yield "order 1", [1.5], []
    yield "order 2", [2.0, -1.0], [0.5]
    yield "order 3", [1.0, 2.0, 3.0], [0.25, -0.75]
    yield "order 30", list(rng.standard_normal(30)), list(rng.standard_normal(29))
    off = rng.standard_normal(29)
    off[14] = 0.0
    yield "order 30, a zero off-diagonal entry", list(rng.standard_normal(30)), list(off)
    yield "repeated eigenvalue 2 (and a zero off-diagonal entry)", [2.0, 1.0, 1.0], [0.0, 1.0]
    yield "a Lanczos matrix: large diagonal, decaying norms", list(3.0 + 0.1 * rng.standard_normal(30)), list(10.0 ** -np.linspace(0, 12, 29))


def dense(diag, off):
    T = np.diag(np.asarray(diag, dtype=float))
    for i, e in enumerate(off):
        T[i, i + 1] = T[i + 1, i] = e
    return T


@pytest.mark.parametrize("which", ["QL", "JACOBI"])
def test_eigen_solvers_against_numpy(driver, which):
    for name, diag, off in tridiagonals():
        k = len(diag)
        T = dense(diag, off)
        t = run(driver, [f"EIG {which} {k} " + " ".join(hx(v) for v in list(diag) + list(off))])[0]
        assert t[0] == "1", name
        vals = np.array(fl(t[1:1 + k]))
        Y = np.array(fl(t[1 + k:])).reshape(k, k).T             # columns = vectors
        bound = 100.0 * k * EPS * np.linalg.norm(T, 2)
        assert np.all(np.diff(vals) >= 0.0), name                # ascending
        assert np.max(np.abs(vals - np.linalg.eigh(T)[0])) <= bound, (name, which)
        for c in range(k):
            assert np.linalg.norm(T @ Y[:, c] - vals[c] * Y[:, c]) <= bound, (name, which, c)
            assert abs(np.linalg.norm(Y[:, c]) - 1.0) <= 100.0 * k * EPS, (name, which, c)


def test_ritz_pairs_and_their_sign(driver):
    for name, diag, off in tridiagonals():
        k = len(diag)
        T = dense(diag, off)
        t = fl(run(driver, [f"RITZ {k} " + " ".join(hx(v) for v in list(diag) + list(off))])[0])
        eig1, eig2, y1, y2 = t[0], t[1], np.array(t[2:2 + k]), np.array(t[2 + k:])
        want = np.linalg.eigh(T)[0]
        bound = 100.0 * k * EPS * np.linalg.norm(T, 2)
        assert abs(eig1 - want[-1]) <= bound and abs(eig2 - want[-2 if k > 1 else -1]) <= bound, name
        assert eig1 >= eig2
        for lam, y in ((eig1, y1), (eig2, y2)):
            assert np.linalg.norm(T @ y - lam * y) <= bound, name
            assert y[np.argmax(np.abs(y))] > 0.0, name           # the component of largest magnitude is positive
        if k == 1:
            assert list(y1) == [1.0] and list(y2) == [1.0] and eig1 == eig2 == diag[0]
    # a vector the QL iteration returns with its large component negative would be flipped: both signs of one matrix's
    # off-diagonal give the same first vector up to the sign of its second component, the first staying positive
    a = fl(run(driver, ["RITZ 2 " + " ".join(hx(v) for v in (2.0, 1.0, 0.5))])[0])
    b = fl(run(driver, ["RITZ 2 " + " ".join(hx(v) for v in (2.0, 1.0, -0.5))])[0])
    assert a[2] > 0.0 and b[2] > 0.0 and a[3] > 0.0 and b[3] < 0.0
    assert abs(a[2] - b[2]) <= 8 * EPS and abs(a[3] + b[3]) <= 8 * EPS


# ---- the driver, end to end ---------------------------------------------------------------------
def drive(driver, tmp_path, Linv, dS_list):
    """Linv, dS: symmetric / lower-triangular matrices as numpy sees them (element (i, j) at [i, j]); the file is column-major"""
    n = Linv.shape[0]
    path = str(tmp_path / "mats.bin")
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(Linv.T).tobytes())
        for dS in dS_list:
            f.write(np.ascontiguousarray(dS.T).tobytes())
    t = run(driver, [f"DRIVE {n} {path} {len(dS_list)}"])[0]
    return [(int(t[3 * q]), float.fromhex(t[3 * q + 1]), int(t[3 * q + 2])) for q in range(len(dS_list))]


GOLDENS = ["gpp100_A", "gpp100_B", "mix40_A", "mix40_B", "syn64", "syn96x40_B", "syn100", "syn200", "theta1_A", "theta1_B"]


@pytest.fixture(scope="module")
def oracle_py():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py as mod
    return mod


@pytest.mark.parametrize("name", GOLDENS)
def test_driver_against_the_compiled_reference(driver, tmp_path, oracle_py, name):
    g = load_golden(name)
    n, m = int(g["dims"][0]), int(g["dims"][1])
    if "csc_beg" in g:
        blk = oracle_py.Block(n, m, g["csc_beg"], g["csc_idx"], g["csc_val"])
    else:
        beg, idx, val, _ = oracle_py.synth_csc(n, m)
        blk = oracle_py.Block(n, m, beg, idx, val)
    try:
        Rd, tau = float(g["Rd"][0]), float(g["tau"][0])
        sym = lambda A: np.triu(A) + np.triu(A, 1).T   # noqa: E731  (column-major lower triangle = the C-order view's upper one)
        Lf, info = blk.factor(blk.assemble_S(tau, y_of(g), Rd))
        assert info == 0
        Linv = np.linalg.inv(np.triu(Lf).T)                        # L is the lower-triangular factor, S = L L^T
        dS = [sym(blk.assemble_S(float(g["rt_par" + t][0]), np.asarray(g["rt_dy" + t], dtype=np.float64), -float(g["rt_par" + t][1]) * Rd))
              for t in ("1", "2")]
    finally:
        blk.close()
    got = drive(driver, tmp_path, np.tril(Linv), dS)
    for (rc, step, steps), tag in zip(got, ("1", "2")):
        ref = float(g["rt_step" + tag][0])
        print(name, tag, "step %.17g reference %.17g rel %.2e after %d steps" % (step, ref, abs(step - ref) / abs(ref), steps))
        assert rc == 0
        assert abs(step - ref) <= RATIO_TOL * abs(ref), (name, tag, step, ref)
        assert steps in (2, 5, 8, 11, 14, 17, 20, 23, 26, 29, 30)   # a test ends at a check, or runs out of steps


def test_breakdown_cases(driver, tmp_path):
    n, c = 5, 2.0
    eye = np.eye(n)
    # Op = L^-1 (-dS) L^-T = c I: every vector is an eigenvector, the first step leaves nothing -- a zero norm, checked at
    # once -- or rounding noise, which a later zero norm or the check after the third step sees as a converged pair:
    # eig1 = c to a few ulps, gamma <= r1 <= a few n eps c, step = 1 / (gamma + eig1)
    (rc, step, steps), (rc2, step2, _) = drive(driver, tmp_path, eye, [-c * eye, -c * eye])
    assert rc == 0 and rc2 == 0 and 0 <= steps <= 2
    assert abs(step - 1.0 / c) <= 100 * n * EPS / c and abs(step2 - 1.0 / c) <= 100 * n * EPS / c
    # Op = -c I: S + alpha dS is positive definite for every alpha >= 0
    (rc, step, steps), (rc2, step2, _) = drive(driver, tmp_path, eye, [c * eye, c * eye])
    assert rc == 0 and rc2 == 0 and step == float("inf") and step2 == float("inf")
