"""A Schur operator that comes up sparse with a banded pattern: a chain of fifty small blocks of the synthetic family, shared by
tests/test_gpu_parity.py (the envelope factorisation) and tests/test_gpu_pivoted.py (the same operator switched to the pivoted
solver)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

CHAIN_BLOCKS, CHAIN_M = 50, 408


def block_with_rows(n, m, keep):
    """a block of the synthetic family on which only the constraints in `keep` have data (CSC, column 0 = C)"""
    import oracle_py
    beg0, idx0, val0, _ = oracle_py.synth_csc(n, m)
    beg, idx, val = [0], [], []
    for col in range(m + 1):
        lo, hi = int(beg0[col]), int(beg0[col + 1])
        if col == 0 or (col - 1) in keep:
            idx += [int(v) for v in idx0[lo:hi]]; val += [float(v) for v in val0[lo:hi]]
        beg.append(len(idx))
    return np.array(beg, dtype=np.int32), np.array(idx, dtype=np.int32), np.array(val)


def banded_chain(scrambled, cones):
    """block b holds constraints 8b .. 8b+15 (m = 408), renumbered at random if `scrambled`; every block at an interior state.
    Appends the engine's cones to `cones` as they are made (the caller destroys them, also after a failure in here) and returns
    the oracle's block-by-block sum of M (C-order view of the column-major matrix: upper triangle valid)."""
    import oracle_py
    from hdsdp_amd import api
    m = CHAIN_M
    Rd, tau = -30.0, 1.0
    y = 0.02 * np.cos(np.arange(m) + 0.3)
    Mref = np.zeros((m, m))
    renum = np.random.default_rng(7).permutation(m) if scrambled else np.arange(m)
    for b in range(CHAIN_BLOCKS):
        n = 10 + (b % 3)
        keep = sorted(int(renum[k]) for k in range(8 * b, 8 * b + 16))
        beg, idx, val = block_with_rows(n, m, keep)
        blk = oracle_py.Block(n, m, beg, idx, val)
        Lf, info = blk.factor(blk.assemble_S(tau, y, Rd))
        assert info == 0
        Mref += blk.kkt_build(blk.inverse(Lf), Rd, 0)["M"]
        blk.close()
        c = api.SDPCone.from_csc(n, m, beg, idx, val, iCone=b)
        c.set_start(Rd)
        assert c.check_is_interior(tau, y)
        cones.append(c)
    return Mref
