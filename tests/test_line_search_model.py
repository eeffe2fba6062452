"""The host fp64 model of tests/line_search_model.py (T(tau, y, eye), log det, the exact largest step) against the pinned
oracle (oracle/oracle_py.py) on the same data, before any device number is compared with it (tests/test_gpu_line_search.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)
import oracle_py  # noqa: E402
import line_search_model as lm  # noqa: E402

ORACLE_STEP_FLOOR = lm.ORACLE_STEP_FLOOR


def _upper(S):
    return np.triu(S) + np.triu(S, 1).T      # oracle_py returns the column-major lower triangle, i.e. C-order upper


def test_csc_round_trip_and_the_oracles_generator():
    n, m = 23, 7
    beg, idx, val, _ = oracle_py.synth_csc(n, m)
    C, A = lm.from_csc(n, m, beg, idx, val)
    b2, i2, v2 = lm.to_csc([C] + list(A))
    C2, A2 = lm.from_csc(n, m, b2, i2, v2)
    assert np.array_equal(C, C2) and np.array_equal(A, A2)
    assert np.array_equal(A[3], oracle_py.synth_matrix(n, 3))


@pytest.mark.parametrize("n,m,seed", [(1, 2, 3), (17, 5, 4), (40, 9, 5)])
def test_model_matches_the_oracle(n, m, seed):
    rng = np.random.default_rng(seed)
    mats = [lm.random_sym(rng, n, 0.5) for _ in range(m + 1)]
    beg, idx, val = lm.to_csc(mats)
    C, A = lm.from_csc(n, m, beg, idx, val)
    blk = oracle_py.Block(n, m, beg, idx, val)
    try:
        y = 0.1 * rng.standard_normal(m)
        tau = 0.9
        base = lm.T(C, A, tau, y, 0.0)
        Rd = -(abs(float(np.linalg.eigvalsh(base)[0])) + 1.0)
        S = lm.T(C, A, tau, y, -Rd)
        So = _upper(blk.assemble_S(tau, y, Rd))
        scale = float(np.max(np.abs(S)))
        assert float(np.max(np.abs(S - So))) <= 1e-14 * scale
        Lf, info = blk.factor(blk.assemble_S(tau, y, Rd))
        assert info == 0 and lm.is_pd(S)
        assert abs(blk.logdet(Lf) - lm.logdet(S)) <= 1e-12 * max(1.0, abs(lm.logdet(S))) * n
        # the factor decides as the model does: far outside the cone
        _, info2 = blk.factor(blk.assemble_S(tau, y, -Rd))
        assert (info2 == 0) == lm.is_pd(lm.T(C, A, tau, y, Rd))
        if n > 1:
            dy = rng.standard_normal(m)
            for dtau, ada in ((0.0, 0.0), (-0.2, 0.5)):
                dS = lm.T(C, A, dtau, dy, ada * Rd)
                a = lm.alpha_star(S, dS)
                got = blk.ratio_test(Lf, dtau, dy, ada * Rd)
                assert np.isfinite(a)
                assert ORACLE_STEP_FLOOR * a <= got <= a * (1 + 1e-12), (got, a)
                assert not lm.is_pd(S + 1.001 * a * dS) and lm.is_pd(S + 0.999 * a * dS)
    finally:
        blk.close()


@pytest.mark.parametrize("n", [2, 16, 17, 129, 257])
def test_ratio_block_spectra_and_the_oracles_step(n):
    """the constructed directions have the exact steps the construction says; the oracle's step lies in
    [ORACLE_STEP_FLOOR alpha*, alpha*] on every one of them"""
    C, A = lm.ratio_block(n, 11 + n)
    mats = [C] + list(A)
    beg, idx, val = lm.to_csc(mats)
    C, A = lm.from_csc(n, 4, beg, idx, val)
    blk = oracle_py.Block(n, 4, beg, idx, val)
    try:
        S = lm.T(C, A, 1.0, np.zeros(4), 0.0)
        Lf, info = blk.factor(blk.assemble_S(1.0, np.zeros(4), 0.0))
        assert info == 0
        want = {"rank-one": 0.5, "near-degenerate pair": 1.0, "dS = -S": 1.0, "psd": np.inf}
        for dtau, dy, ada, name in lm.ratio_directions():
            dS = lm.T(C, A, dtau, dy, 0.0)
            a = lm.alpha_star(S, dS)
            if name in want:
                assert (a == want[name]) if want[name] == np.inf else abs(a - want[name]) <= 1e-12 * n, (name, a)
            got = blk.ratio_test(Lf, dtau, dy, 0.0)
            if np.isinf(a):
                assert got > 1e6, (name, got)
            else:
                assert ORACLE_STEP_FLOOR * a <= got <= a * (1 + 1e-12), (name, got, a)
    finally:
        blk.close()
