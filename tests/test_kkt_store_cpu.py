"""The rules of the Schur operator's matrix store (csrc/kkt_store.h), without a device: the header is compiled alone with the host
C++ compiler beside tests/kkt_store_driver.cpp.  The expected values are written here from the rules as they are stated, not from
what the code gives:

- the load plan of HKKTFactorize, for every combination of form, mirror, permuted, indef, "M valid" and "channel folded":

    form  | mirror | requires | staging                                 | source        | load             | on pivot failure
    TILES | on     | --       | zero factor store, upload nnz, scatter  | --            | (done by staging)| fail
    TILES | off    | M valid  | fold channel if not folded              | --            | load_M           | fail
    CSC   | on     | --       | zero device M, upload nnz, scatter;     | device M      | device/permuted  | switch to pivoted
          |        |          | M becomes valid                         |               |                  |
    CSC   | off    | M valid  | fold channel if not folded              | device M      | device/permuted  | switch to pivoted
    DENSE | on     | --       | none                                    | host M, ld = m| load_host        | switch to pivoted
    DENSE | off    | M valid  | fold channel if not folded              | device M      | load_device      | switch to pivoted

  a permuted CSC gathers from device M first when the mirror is off; once switched to the pivoted solver (DENSE, CSC), load and
  Cholesky are replaced by the pivoted factorisation from the recorded source and staging still runs; an unmet requirement is a
  failure with no step; bytes up: 8 nnz for an uploaded CSC, 8 m^2 for the dense mirror, 8 m for a folded channel;
- the transitions, each followed by the plan it must change;
- the block envelope's cost against its definition in numpy, and the choice of an order (taken below 0.8 x the natural cost);
- the bounds of the reordering's eligibility (nnz <= 5e7, nnz < 0.15 m^2) and of the sparse-or-dense rule (0.3 m^2, an empty
  column, a column that does not start on the diagonal);
- the five switches: two read at every call, three once per process."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

DENSE, CSC, TILES = range(3)                                            # forms
ST_NONE, ST_FOLD, ST_CSC_TO_FACTOR, ST_CSC_TO_M = range(4)              # staging
SRC_NONE, SRC_HOST, SRC_DEVICE = range(3)                               # recorded source
LD_STAGED, LD_TILES, LD_HOST, LD_DEVICE, LD_PERMUTED, LD_PIVOTED = range(6)
FAIL, SWITCH = range(2)                                                 # on a pivot failure
LD_DEV = 512                                                            # the driver's stand-in device matrix
SWITCHES = ("HDSDP_MI355X_SPARSE_KKT", "HDSDP_MI355X_KKT_TILES", "HDSDP_MI355X_KKT_ENVELOPE", "HDSDP_MI355X_KKT_RCM",
            "HDSDP_MI355X_DEVICE_M")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kkt_store") / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "kkt_store_driver.cpp")])
    return exe


def run(exe, lines, env=None):
    """one fresh state per script; one row of numbers per query"""
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    base.update(env or {})
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, env=base).stdout
    return [row.split() for row in out.splitlines()]


def plan_row(t):
    return {"ok": int(t[0]), "stage": int(t[1]), "source": int(t[2]), "load": int(t[3]), "gather": int(t[4]), "on_pivot": int(t[5]),
            "matrix_bytes": int(t[6]), "channel_bytes": int(t[7])}


def state_row(t):
    return dict(zip(("form", "mirror", "permuted", "indef", "m_valid", "chan_folded", "source", "ld"), (int(v) for v in t)))


def reach(form, mirror, permuted, indef, m_valid, folded):
    """the transitions that bring a fresh state there"""
    lines = [f"INIT {form} {int(permuted)}", f"MIRROR {int(mirror)}"]
    if indef:
        lines.append("PIVOTED")
    if m_valid:
        lines.append("FINISH 0")
    if folded:
        lines.append("FOLDED")
    return lines


def combinations():
    for form in (DENSE, CSC, TILES):
        for mirror, permuted, indef, m_valid, folded in itertools.product((1, 0), repeat=5):
            if permuted and form != CSC:
                continue
            if indef and form == TILES:
                continue
            yield form, mirror, permuted, indef, m_valid, folded


def expected_plan(form, mirror, permuted, indef, m_valid, folded, m, nnz):
    """the table of this file's docstring, row by row"""
    if not mirror and not m_valid:
        return None
    fold = ST_NONE if folded else ST_FOLD
    p = {"ok": 1, "gather": 0, "matrix_bytes": 0, "channel_bytes": 0}
    if form == TILES:
        p.update(stage=ST_CSC_TO_FACTOR if mirror else fold, source=SRC_NONE, load=LD_STAGED if mirror else LD_TILES, on_pivot=FAIL)
    elif form == CSC:
        p.update(stage=ST_CSC_TO_M if mirror else fold, source=SRC_DEVICE, load=LD_PERMUTED if permuted else LD_DEVICE, on_pivot=SWITCH)
        p["gather"] = int(bool(permuted and not mirror))
    else:
        p.update(stage=ST_NONE if mirror else fold, source=SRC_HOST if mirror else SRC_DEVICE, load=LD_HOST if mirror else LD_DEVICE,
                 on_pivot=SWITCH)
    if indef:       # the pivoted factorisation replaces load and Cholesky: no gather, and its own failure is a failure
        p.update(load=LD_PIVOTED, gather=0, on_pivot=FAIL)
    if mirror and form != DENSE:
        p["matrix_bytes"] = 8 * nnz
    if mirror and form == DENSE:
        p["matrix_bytes"] = 8 * m * m
    if p["stage"] == ST_FOLD:
        p["channel_bytes"] = 8 * m
    return p


def test_load_plan_for_every_combination(driver):
    m, nnz = 408, 5003
    combos = list(combinations())
    assert len(combos) == 8 * (2 + 4 + 1)                # mirror, M valid, folded; DENSE: x indef; CSC: x permuted x indef
    for c in combos:
        form, mirror, permuted, indef, m_valid, folded = c
        rows = run(driver, reach(*c) + ["STATE", f"DO {m} {nnz}", "STATE"])
        before, got, after = state_row(rows[0]), plan_row(rows[1]), state_row(rows[2])
        assert before == {"form": form, "mirror": mirror, "permuted": permuted, "indef": indef, "m_valid": m_valid,
                          "chan_folded": folded, "source": SRC_NONE, "ld": 0}, c
        want = expected_plan(*c, m, nnz)
        if want is None:                                 # a requirement that is not met: "fail", no step, nothing committed
            assert got == {"ok": 0, "stage": ST_NONE, "source": SRC_NONE, "load": LD_STAGED, "gather": 0, "on_pivot": FAIL,
                           "matrix_bytes": 0, "channel_bytes": 0}, c
            assert after == before, c
            continue
        assert got == want, c
        # after the commit: a scattered CSC made M valid, a fold is not repeated, and the source is the table's
        want_after = dict(before)
        want_after["m_valid"] = int(m_valid or (form == CSC and mirror))
        want_after["chan_folded"] = int(folded or not mirror)
        want_after["source"] = want["source"]
        want_after["ld"] = {SRC_NONE: 0, SRC_HOST: m, SRC_DEVICE: LD_DEV}[want["source"]]
        assert after == want_after, c


def test_transitions_change_the_plan_they_must(driver):
    # mirror off: no factorisation before a build; a finished build makes M valid, with an unfolded channel
    rows = run(driver, [f"INIT {DENSE} 0", "MIRROR 0", "PLAN 10 0", "START 0", "PLAN 10 0", "FINISH 0", "DO 10 0", "PLAN 10 0",
                        "START 1", "FINISH 1", "PLAN 10 0", "START 0", "PLAN 10 0"])
    p = [plan_row(r) for r in rows]
    assert [q["ok"] for q in p] == [0, 0, 1, 1, 1, 1]
    assert p[2]["stage"] == ST_FOLD and p[2]["channel_bytes"] == 80       # the first factorisation after the build folds ...
    assert p[3]["stage"] == ST_NONE and p[3]["channel_bytes"] == 0        # ... the second does not
    assert p[4]["stage"] == ST_NONE                                       # a corrector build leaves both as they were
    assert p[5]["stage"] == ST_FOLD                                       # the next build starts an unfolded channel
    # a corrector build on a fresh operator does not make M valid
    rows = run(driver, [f"INIT {TILES} 0", "MIRROR 0", "START 1", "FINISH 1", "PLAN 10 0", "STATE"])
    assert plan_row(rows[0])["ok"] == 0 and state_row(rows[1])["m_valid"] == 0
    # the regulariser folded the channel: the factorisation does not fold again
    rows = run(driver, [f"INIT {CSC} 1", "MIRROR 0", "START 0", "FINISH 0", "FOLDED", "PLAN 10 7"])
    assert plan_row(rows[0])["stage"] == ST_NONE and plan_row(rows[0])["gather"] == 1
    # a mirror switch changes only what kkt_point_diag and the plan read
    rows = run(driver, [f"INIT {CSC} 1", "START 0", "FINISH 0", "STATE", "PLAN 10 7", "MIRROR 0", "STATE", "PLAN 10 7", "MIRROR 1", "STATE"])
    s0, s1, s2 = state_row(rows[0]), state_row(rows[2]), state_row(rows[4])
    assert s1 == dict(s0, mirror=0) and s2 == s0
    assert plan_row(rows[1])["stage"] == ST_CSC_TO_M and plan_row(rows[3])["stage"] == ST_FOLD
    # the host CSC scattered into the device matrix makes it valid: with the mirror switched off next, the plan holds
    rows = run(driver, [f"INIT {CSC} 0", "MIRROR 0", "PLAN 10 7", "MIRROR 1", "DO 10 7", "MIRROR 0", "PLAN 10 7", "STATE"])
    assert plan_row(rows[0])["ok"] == 0 and plan_row(rows[2])["ok"] == 1 and state_row(rows[3])["m_valid"] == 1
    rows = run(driver, [f"INIT {CSC} 0", "MIRROR 0", "SCATTERED", "PLAN 10 7"])
    assert plan_row(rows[0])["ok"] == 1
    # the fused small pass wrote M and its factor: M valid, the source is the device matrix with the pass's leading dimension
    rows = run(driver, [f"INIT {DENSE} 0", "START 0", "SMALL", "STATE"])
    assert state_row(rows[0]) == {"form": DENSE, "mirror": 1, "permuted": 0, "indef": 0, "m_valid": 1, "chan_folded": 0,
                                  "source": SRC_DEVICE, "ld": 128}
    # switched to the pivoted solver: stays switched, whatever is built or factored afterwards
    rows = run(driver, [f"INIT {DENSE} 0", "PLAN 10 0", "PIVOTED", "DO 10 0", "START 0", "FINISH 0", "PLAN 10 0", "STATE"])
    assert plan_row(rows[0])["load"] == LD_HOST and plan_row(rows[1])["load"] == LD_PIVOTED and plan_row(rows[2])["load"] == LD_PIVOTED
    assert plan_row(rows[1])["matrix_bytes"] == 800                        # (the pivoted solver's own load of the host matrix)
    assert state_row(rows[3])["indef"] == 1 and state_row(rows[3])["source"] == SRC_HOST and state_row(rows[3])["ld"] == 10
    # a host matrix handed to a linear system that is no operator's
    rows = run(driver, ["HOSTM", "STATE"])
    assert state_row(rows[0])["source"] == SRC_HOST and state_row(rows[0])["ld"] == 77
    # HKKTInit starts a fresh matrix and solver; the mirror keeps what it was told
    rows = run(driver, ["MIRROR 0", "PIVOTED", "FINISH 0", "FOLDED", "HOSTM", f"INIT {TILES} 0", "STATE"])
    assert state_row(rows[0]) == {"form": TILES, "mirror": 0, "permuted": 0, "indef": 0, "m_valid": 0, "chan_folded": 0,
                                  "source": SRC_NONE, "ld": 0}


# ---- envelope -------------------------------------------------------------------------------
def band_pattern(renum=None):
    """the chain of tests/test_gpu_parity.py::test_sparse_operator_with_a_banded_pattern_over_several_blocks_of_M: fifty blocks,
    block b holding constraints 8b .. 8b+15 (m = 408, four 128-blocks); the lower triangle's (row, column) pairs"""
    m = 408
    renum = np.arange(m) if renum is None else renum
    pairs = set()
    for b in range(50):
        keep = [int(renum[k]) for k in range(8 * b, 8 * b + 16)]
        pairs.update((max(i, j), min(i, j)) for i in keep for j in keep)
    assert max(r for r, _ in pairs) == m - 1
    return sorted(pairs, key=lambda rc: (rc[1], rc[0]))


def envelope_by_definition(pairs, nb, perm=None):
    """first[b]: the first 128-block column an entry of block row b lies in (the diagonal block at the latest); a block column k
    of the factor runs down to the last block row whose envelope reaches it, h blocks below the diagonal; its elimination costs
    one diagonal factorisation, h triangular solves and h (h + 1) / 2 updates"""
    rc = np.array(pairs)
    if perm is not None:
        rc = np.sort(np.asarray(perm)[rc], axis=1)[:, ::-1]
    br, bc = rc[:, 0] // 128, rc[:, 1] // 128
    first = [min([b] + list(bc[br == b])) for b in range(nb)]
    cost = 0.0
    for k in range(nb):
        h = max(b for b in range(k, nb) if first[b] <= k) - k
        cost += 1.0 + h + 0.5 * h * (h + 1.0)
    return cost, first


def envelope_cmd(pairs, nb, perm=None):
    flat = " ".join(f"{r} {c}" for r, c in pairs)
    tail = "" if perm is None else " " + " ".join(str(int(v)) for v in perm)
    return f"ENV {nb} {len(pairs)} {0 if perm is None else 1} {flat}{tail}"


def envelope_row(t):
    return float.fromhex(t[0]), [int(v) for v in t[1:]]


def test_envelope_cost_and_the_choice_of_an_order(driver):
    nb = 4
    band = band_pattern()
    want_nat = envelope_by_definition(band, nb)
    assert want_nat == (10.0, [0, 0, 1, 2])                    # three block columns one block tall, and the last diagonal block
    ident, rev = np.arange(408), np.arange(408)[::-1]
    rows = run(driver, [envelope_cmd(band, nb), envelope_cmd(band, nb, ident), envelope_cmd(band, nb, rev)])
    assert envelope_row(rows[0]) == want_nat and envelope_row(rows[1]) == want_nat
    assert envelope_row(rows[2]) == envelope_by_definition(band, nb, rev)
    # a band already: no candidate order is 0.2 cheaper, the natural order is kept
    for cand in (envelope_row(rows[1])[0], envelope_row(rows[2])[0]):
        assert not cand < 0.8 * want_nat[0]
        assert run(driver, [f"TAKEN {cand.hex()} {want_nat[0].hex()}"]) == [["0"]]
    # the same pattern renumbered by a fixed random permutation; the inverse renumbering as the candidate order
    renum = np.random.default_rng(7).permutation(408)
    inv = np.empty(408, dtype=int)
    inv[renum] = np.arange(408)
    scr = band_pattern(renum)
    rows = run(driver, [envelope_cmd(scr, nb), envelope_cmd(scr, nb, inv)])
    nat, cand = envelope_row(rows[0]), envelope_row(rows[1])
    assert nat == envelope_by_definition(scr, nb) and cand == envelope_by_definition(scr, nb, inv)
    assert cand == want_nat                                     # (the band again)
    assert cand[0] < 0.8 * nat[0]
    assert run(driver, [f"TAKEN {cand[0].hex()} {nat[0].hex()}"]) == [["1"]]
    # the rule's edge: strictly below 0.8 x the natural cost
    assert run(driver, [f"TAKEN {(0.8 * 20.0).hex()} {(20.0).hex()}", f"TAKEN {np.nextafter(0.8 * 20.0, 0.0).hex()} {(20.0).hex()}",
                        f"TAKEN inf {(20.0).hex()}"]) == [["0"], ["1"], ["0"]]


def test_reordering_is_looked_for_within_its_bounds(driver):
    # nnz <= 5e7 (m large enough that the fill bound is not the one that binds: 0.15 m^2 = 6e7)
    assert 0.15 * 20000.0 * 20000 > 50000001
    assert run(driver, ["RCMOK 50000000 20000", "RCMOK 50000001 20000"]) == [["1"], ["0"]]
    # nnz < 0.15 m^2
    m = 1000
    edge = 0.15 * float(m) * m
    assert edge == int(edge)
    at = int(edge)
    assert run(driver, [f"RCMOK {at - 1} {m}", f"RCMOK {at} {m}", f"RCMOK {at + 1} {m}"]) == [["1"], ["0"], ["0"]]


def test_sparse_or_dense(driver):
    m = 100
    edge = int(0.3 * float(m) * float(m))
    assert edge == 3000
    # a cone's symmetric nnz, or the pattern collected so far: dense from 0.3 m^2 on
    assert run(driver, [f"COUNT {edge - 1} {m}", f"COUNT {edge} {m}", f"COUNT {edge + 1} {m}"]) == [["1"], ["0"], ["0"]]
    cols = lambda beg, idx: "COLS %d %s %s" % (len(beg) - 1, " ".join(map(str, beg)), " ".join(map(str, idx)))  # noqa: E731
    assert run(driver, [cols([0, 2, 4, 5], [0, 2, 1, 2, 2]),          # every column starts on its diagonal
                        cols([0, 2, 2, 3], [0, 2, 2]),                # column 1 is empty
                        cols([0, 2, 3, 4], [0, 2, 2, 2]),             # column 1 starts below its diagonal
                        cols([0, 1, 2, 2], [0, 1])]) == [["1"], ["0"], ["0"], ["0"]]   # the last column is empty


def test_switches_and_when_they_are_read(driver):
    assert run(driver, ["SWITCHES"]) == [["1", "1", "1", "1", "0"]]
    for k, name in enumerate(SWITCHES[:4]):
        want = ["1", "1", "1", "1", "0"]
        assert run(driver, ["SWITCHES"], env={name: "1"}) == [want]
        want[k] = "0"
        assert run(driver, ["SWITCHES"], env={name: "0"}) == [want]
    assert run(driver, ["SWITCHES"], env={SWITCHES[4]: "1"}) == [["1", "1", "1", "1", "1"]]
    assert run(driver, ["SWITCHES"], env={SWITCHES[4]: "0"}) == [["1", "1", "1", "1", "0"]]
    assert run(driver, ["SWITCHES"], env={SWITCHES[4]: "2"}) == [["1", "1", "1", "1", "0"]]
    # SPARSE_KKT and DEVICE_M are read at every call, the other three once per process
    rows = run(driver, ["SWITCHES"] + [f"SETENV {name} 0" for name in SWITCHES[:4]] + [f"SETENV {SWITCHES[4]} 1", "SWITCHES",
                                                                                      f"SETENV {SWITCHES[0]} 1", "SWITCHES"])
    assert rows == [["1", "1", "1", "1", "0"], ["0", "1", "1", "1", "1"], ["1", "1", "1", "1", "1"]]
