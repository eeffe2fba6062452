"""Child process of tests/test_gpu_sparse_schur.py: the envelope cases of tests/sparse_schur_cases.py at one size through
HMiCholEnvelopeSolve, on the envelope and dense, in a process whose environment the parent chose (HDM_TRSV_FLOW is read once
per process).  Writes the solutions to an .npz: x_env_<k>, x_dense_<k> for the k-th case of the size.

    python sparse_schur_worker.py <n> <out.npz>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import sparse_schur_cases as sc  # noqa: E402


def main():
    from hdsdp_amd import api
    n, out = int(sys.argv[1]), sys.argv[2]
    res = {}
    for k, (family, nn, cond, grade) in enumerate(c for c in sc.env_cases() if c[1] == n):
        c = sc.env_case(family, nn, cond, grade)
        xe, _, info_e = api.chol_envelope_solve(c.A, c.first, c.b)
        xd, _, info_d = api.chol_envelope_solve(c.A, None, c.b)
        assert info_e == 0 and info_d == 0, (family, nn, cond, grade, info_e, info_d)
        res[f"x_env_{k}"], res[f"x_dense_{k}"] = xe, xd
    np.savez(out, **res)
    print("SPARSE_WORKER_OK", len(res) // 2)


if __name__ == "__main__":
    main()
