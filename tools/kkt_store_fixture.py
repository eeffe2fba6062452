"""Writes tests/golden/kkt_store_parent.json: what HKKTInit decides about a Schur operator's storage (sparse or dense, tile form
or dense device matrix, block envelope, reordering, where kktDiag points) and what one build, regularisation, factorisation and
solve move over the bus, for a grid of small operators under each of the five storage switches at 0 and 1.  It is meant to be run
on the commit BEFORE those rules moved into csrc/kkt_store.h and again on the tree, which must reproduce every integer exactly
and every fraction bit for bit (fractions are stored as float.hex()).  No device was free when that change was made, so the
file and the GPU test on it do not exist yet (profiles/kkt_store_refactor_mi355x.txt); run_setting(setting) is what such a test
compares, setting by setting.

    python tools/kkt_store_fixture.py [out.json]          every setting, one process each (three switches are read once per process)
    python tools/kkt_store_fixture.py --worker            the grid under this process's environment, as one JSON line on stdout
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SWITCHES = ("HDSDP_MI355X_SPARSE_KKT", "HDSDP_MI355X_KKT_TILES", "HDSDP_MI355X_KKT_ENVELOPE", "HDSDP_MI355X_KKT_RCM",
            "HDSDP_MI355X_DEVICE_M")
SETTINGS = ["default"] + [f"{s}={v}" for s in SWITCHES for v in (0, 1)]


def chain(m, width=16, stride=8, dense_row=False, seed=None):
    """constraint sets of a chain of small blocks: block b holds `width` consecutive constraints starting at stride * b (a band
    pattern), after constraint 0 if `dense_row` (an arrow: row 0 reaches every column), renumbered at random if `seed`"""
    first = 1 if dense_row else 0
    assert (m - first - width) % stride == 0
    renum = np.random.default_rng(seed).permutation(m) if seed is not None else np.arange(m)
    keeps = []
    for b in range((m - first - width) // stride + 1):
        rows = list(range(first + stride * b, first + stride * b + width)) + ([0] if dense_row else [])
        keeps.append(sorted(int(renum[k]) for k in rows))
    return keeps


# name -> (m, constraint sets per block, or None for one dense synthetic block)
OPERATORS = {
    "band": (408, chain(408)),                           # tests/test_gpu_parity.py: four 128-blocks, too few for the tile form
    "band_scrambled": (408, chain(408, seed=7)),
    "dense_block": (40, None),
    "dense_row": (297, chain(297, dense_row=True)),
    "band_tiles": (1032, chain(1032)),                   # nine 128-blocks: the band's tiles are under half of the triangle's
}


@functools.lru_cache(maxsize=None)
def synth(n, m):
    import oracle_py
    return oracle_py.synth_csc(n, m)[:3]


def block_csc(n, m, keep):
    """a block of the synthetic family on which only the constraints in `keep` have data (CSC, column 0 = C)"""
    beg0, idx0, val0 = synth(n, m)
    beg, idx, val = [0], [], []
    for col in range(m + 1):
        if col == 0 or (col - 1) in keep:
            idx.append(idx0[beg0[col]:beg0[col + 1]])
            val.append(val0[beg0[col]:beg0[col + 1]])
        beg.append(sum(len(v) for v in idx))
    return np.array(beg, dtype=np.int32), np.concatenate(idx).astype(np.int32), np.concatenate(val).astype(np.float64)


def record(name):
    from hdsdp_amd import api
    m, keeps = OPERATORS[name]
    Rd, tau = -30.0, 1.0
    y = 0.02 * np.cos(np.arange(m) + 0.3)
    cones = []
    try:
        if keeps is None:
            cones.append(api.SDPCone.synthetic(64, m))
            Rd, tau, y = -200.0, 0.9, 0.05 * np.sin(1.7 * np.arange(1, m + 1))
        else:
            for b, keep in enumerate(keeps):
                cones.append(api.SDPCone.from_csc(10 + (b % 3), m, *block_csc(10 + (b % 3), m, set(keep)), iCone=b))
        for c in cones:
            c.set_start(Rd)
            assert c.check_is_interior(tau, y), name
        kkt = api.KKT(m, cones)
        out = {"m": m, "is_sparse": int(kkt.is_sparse), "diag_target_at_init": kkt.diag_target()}
        permuted, fraction = kkt.envelope_info()
        out["envelope"] = [int(permuted), float(fraction).hex()]
        tiles = kkt.tile_info()
        out["tiles"] = None if tiles is None else [int(v) for v in tiles]
        out["nnz"] = int(kkt.csc()[0][m]) if kkt.is_sparse else None
        kkt.build_up(api.KKT_TYPE_INFEASIBLE)
        kkt.regularize(1e-6)
        kkt.factorize()
        x = kkt.solve(np.sin(np.arange(m) + 1.0))
        assert np.all(np.isfinite(x)), name
        out["diag_target"] = kkt.diag_target()
        out["traffic"] = [int(v) for v in kkt.matrix_traffic()]
        kkt.destroy()
        return out
    finally:
        for c in cones:
            c.destroy()


def run_setting(setting):
    """the grid in a fresh process whose environment holds `setting` (and none of the other switches)"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if setting != "default":
        k, v = setting.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], capture_output=True, text=True, timeout=300, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"{setting}: worker ended with {r.returncode}\n{r.stderr[-3000:]}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def main(out):
    res = {}
    for s in SETTINGS:
        res[s] = run_setting(s)
        print(s, "done", flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if "--worker" in sys.argv:
        print(json.dumps({name: record(name) for name in OPERATORS}, sort_keys=True))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "kkt_store_parent.json"))
