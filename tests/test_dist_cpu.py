"""world_size-2 (and 3) gloo tests on CPU of the N > 1 path: the sharding plan and the two collectives
(all-to-all transpose + all-reduce) reproduce the unsharded Schur quantities."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "dist_worker.py")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(mode, world, n, m, out, timeout=600):
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, WORKER, mode, str(n), str(m), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{outs[r][-3000:]}"


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_schur_choreography_gloo(world, tmp_path):
    n, m = 20, 7  # n not a multiple of 16, m not a multiple of world: ragged shards and padding
    out1 = str(tmp_path / "w1.npy")
    outw = str(tmp_path / "ww.npy")
    launch("numpy", 1, n, m, out1)
    launch("numpy", world, n, m, outw)
    assert np.allclose(np.load(out1), np.load(outw), rtol=1e-12, atol=1e-14)


def test_shard_plan_invariants():
    from hdsdp_amd.dist import ShardPlan
    for n, m, w in [(2000, 2000, 1), (2000, 2000, 8), (2000, 8000, 8), (50, 104, 2), (100, 101, 4), (17, 3, 2)]:
        p = ShardPlan(n, m, w)
        rs = p.rows_seg()
        assert sorted(rs[rs >= 0].tolist()) == list(range(m))          # every constraint exactly once
        assert (rs == -2).sum() == (rs == -3).sum() == (rs == -4).sum() == 1
        assert p.npb_loc * w >= p.npb and p.R == w * p.Lr
        assert sum(len(p.owned(r)) for r in range(w)) == m
        if w > 1:
            assert p.Lr % 128 == 0                                      # Gram tiles never straddle segments
        # balanced by construction: shard sizes differ by at most one row
        sizes = [len(p.owned(r)) for r in range(w)]
        assert max(sizes) - min(sizes) <= 1
    # transpose volume: each rank sends (w-1)/w of its rows' data -- 1/w of an all-gather
    p = ShardPlan(2000, 2000, 8)
    assert p.chunk * 8 * 7 < 0.15 * (p.npb * 16 * 2000 * 8)


PLAN_KNOBS = ("HDM_TCAP_GIB", "HDM_BC", "HDM_GRAM_KSTAGES", "HDM_NSPLIT", "HDM_SHARE_T_SLABS", "HDM_GRAM_QUEUE")


def test_work_plan_query_reproduces_the_parents_plan(monkeypatch):
    """the engine's work plan (csrc/work_plan.h through api.work_plan: host arithmetic, no GPU) against
    tests/golden/work_plan_parent.json -- what the Python re-derivation of the commit before work_plan.h said over a grid that
    reaches every branch (tools/work_plan_fixture.py): every integer of the layout, the batch size, the split and slab counts
    and every part's bytes, exactly"""
    import json
    from hdsdp_amd import api
    from hdsdp_amd.dist import ShardPlan
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    with open(os.path.join(HERE, "golden", "work_plan_parent.json")) as f:
        grid = json.load(f)
    seen = set()
    for e in grid:
        n, m, w, r = e["n"], e["m"], e["world"], e["rank"]
        seen.add((n, m, w, r))
        wp = api.work_plan(n, m, w, r)
        p = ShardPlan(n, m, w)
        for k, v in e["layout"].items():
            assert getattr(p, k) == v, (n, m, w, k)                       # the pure-Python layout (chunk included)
            assert k == "chunk" or wp[k] == v, (n, m, w, k)               # and the engine's
        assert wp["npb_loc"] * wp["Lr"] * 16 == e["layout"]["chunk"]
        assert wp["mloc"] == len(p.owned(r))
        assert (wp["Bc"], wp["nsplit"], wp["nslab"]) == (e["Bc"], e["nsplit"], e["nslab"]), (n, m, w, r, wp)
        assert wp["shared_ts"] == (w == 1) and wp["gram_queue_global"] == 1
        assert wp["t_bytes"] == e["Bc"] * p.n16 * p.n16 * 8 and wp["slab_bytes"] == e["nslab"] * p.R * p.R * 8
        assert wp["astride"] * wp["mloc"] * 8 == e["parts"]["A (A_L form, skyline)"]
        assert p.hbm_bytes(r) == e["parts"], (n, m, w, r)
    # the grid cannot quietly lose a branch: one device on both sides of the long-K cut, single-split shards, a sharded
    # block with as many slabs as splits and two with fewer, first and last rank
    by = {(e["n"], e["m"], e["world"], e["rank"]): e for e in grid}
    assert {(200, 200, 1, 0), (640, 900, 1, 0), (1000, 1000, 1, 0), (2000, 2000, 1, 0), (2000, 8000, 1, 0)} <= seen
    assert by[(200, 200, 1, 0)]["nsplit"] <= 64 < by[(640, 900, 1, 0)]["nsplit"]
    assert by[(2000, 8000, 1, 0)]["nslab"] < by[(2000, 8000, 1, 0)]["nsplit"]
    for n, m, w in [(100, 101, 4), (17, 3, 2), (640, 900, 2), (2000, 2000, 8), (2000, 8000, 8), (2000, 8000, 2)]:
        assert {(n, m, w, 0), (n, m, w, w - 1)} <= seen
    assert by[(100, 101, 4, 0)]["nsplit"] == by[(17, 3, 2, 1)]["nsplit"] == 1
    assert by[(2000, 2000, 8, 0)]["nslab"] == by[(2000, 2000, 8, 0)]["nsplit"] > 64
    for key in [(2000, 8000, 8, 0), (2000, 8000, 8, 7), (2000, 8000, 2, 0)]:
        assert by[key]["nslab"] < by[key]["nsplit"], key
    assert api.work_plan(2000, 8000, 8, 0)["nslab"] == 16 and api.work_plan(2000, 8000, 8, 0)["nsplit"] == 64


def test_work_plan_knobs_have_their_documented_effects():
    """the pure query under each setting tests/test_gpu_switches.py runs for the plan's six knobs, in a child process as
    there, at the worker's two tiled sizes and at n = 640, m = 900 (one device and two shards): a knob changes what the
    header's switch table says it changes, and nothing else"""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("switch_tests_plan", os.path.join(HERE, "test_gpu_switches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    settings = [s for s in mod.SETTINGS if set(s) <= set(PLAN_KNOBS)]
    assert set(k for s in settings for k in s) == set(PLAN_KNOBS)
    sizes = [(640, 24, 1), (2304, 6, 1), (640, 900, 1), (640, 900, 2)]
    code = ("import json, sys; sys.path.insert(0, %r); from hdsdp_amd import api; "
            "print('PLAN_JSON ' + json.dumps([api.work_plan(n, m, w, 0) for n, m, w in %r]))" % (os.path.dirname(HERE), sizes))

    def run(extra):
        env = {k: v for k, v in os.environ.items() if not (k.startswith("HDM_") or k.startswith("HDSDP_MI355X_"))}
        env.update(extra, HDSDP_MI355X_NO_TORCH="1")
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (extra, (r.stdout + r.stderr)[-2000:])
        line = [l for l in r.stdout.splitlines() if l.startswith("PLAN_JSON ")]
        return json.loads(line[-1][len("PLAN_JSON "):])

    default = run({})
    assert [d["shared_ts"] for d in default] == [1, 1, 1, 0] and all(d["gram_queue_global"] == 1 for d in default)
    for s in settings:
        got = run(s)
        for (n, m, w), d, g in zip(sizes, default, got):
            n16 = d["n16"]
            changed = {k for k in d if d[k] != g[k]}
            kb16 = d["npb_loc"] // 16
            if s == {"HDM_NSPLIT": "24"}:                  # 24 slabs where kblocks / 16 allows
                assert kb16 >= 24 and g["nslab"] == 24 and g["nsplit"] in (24, d["nsplit"]) and g["nsplit"] >= 24   # (the split count stays where the K-length rule set it)
                assert changed <= {"nslab", "nsplit", "slab_bytes"}
            elif s == {"HDM_GRAM_KSTAGES": "16", "HDM_NSPLIT": "8"}:
                assert g["nslab"] == 8
                if w == 1:                                  # one device: 16 stages per job, so more splits than slabs
                    assert g["nsplit"] == -(-d["npb_loc"] // 16) > g["nslab"]
                else:                                       # (not honoured on a sharded block; K is short here: splits = slabs)
                    assert d["npb_loc"] // 96 < 128 and g["nsplit"] == 8
                assert changed <= {"nslab", "nsplit", "slab_bytes"}
            elif s == {"HDM_SHARE_T_SLABS": "0"}:
                assert g["shared_ts"] == 0 and changed == ({"shared_ts"} if w == 1 else set())
            elif s == {"HDM_GRAM_QUEUE": "0"}:
                assert g["gram_queue_global"] == 0 and changed == {"gram_queue_global"}
            elif s == {"HDM_BC": "8"}:
                assert g["Bc"] == (8 if d["mloc"] >= 8 else d["mloc"]) and g["t_bytes"] == g["Bc"] * n16 * n16 * 8
                assert changed <= {"Bc", "t_bytes", "nslab", "nsplit", "slab_bytes"}
            elif s == {"HDM_TCAP_GIB": "1"}:
                assert g["t_bytes"] <= 1 << 30 and g["Bc"] <= d["Bc"]
                if m == 900:                                # 327 matrices of 640 x 640 fit 1 GiB: 900 rows in 3 x 300, 450 in 2 x 225
                    assert g["Bc"] == (300 if w == 1 else 225)
                assert changed <= {"Bc", "t_bytes", "nslab", "nsplit", "slab_bytes"}
            else:
                raise AssertionError("a setting of the plan's knobs without a documented effect here: %r" % (s,))


def test_config5_fits_the_hbm_of_eight_mi355x():
    """BASELINE configs[4] (n = 2000, m = 8000 over 8 GPUs): what one rank allocates, by the plan that mirrors the engine's
    allocation rules, against 288 GB of HBM3E per MI355X -- half of it; two ranks could not hold the problem"""
    from hdsdp_amd.dist import ShardPlan
    HBM = 288e9
    for rank in (0, 7):
        parts = ShardPlan(2000, 8000, 8).hbm_bytes(rank)
        assert parts["total"] < 0.6 * HBM, parts
        assert 0.52 * 1000 * 2000 * 2000 * 8 < parts["A (A_L form, skyline)"] < 0.55 * 1000 * 2000 * 2000 * 8
    one = ShardPlan(2000, 2000, 1).hbm_bytes(0)
    assert 90e9 < one["total"] < 110e9, one           # about 100 GB for the 32 GB problem
    assert ShardPlan(2000, 8000, 2).hbm_bytes(0)["total"] < HBM < ShardPlan(2000, 8000, 1).hbm_bytes(0)["total"] * 2
