"""The rule of a cone's constraint rows (csrc/row_store_rule.h), without a device: the header is compiled alone with the host C++
compiler beside tests/row_store_rule_driver.cpp.  The expected values are written here from the rule as DESIGN.md section 21
states it, not from what the code gives:

- resident needs  8 astride max(1, mloc)  +  exchange bytes  +  min(41 GiB, max(8 n16^2 min(rows, 1024), 64 R^2))  +  24 m^2 + 16 GiB
  and the rows are streamed iff that is MORE than what is free (one device) or than 0.97 x the capacity (a shard); figures that
  could not be read: not streamed; HDSDP_MI355X_STREAM_A set: that; no rows, or another path than congruence + Gram: never;
- a streamed batch holds hdm_even_out(mloc, max(1, HDM_BC)) rows;
- the sweep copy: HDSDP_MI355X_ZS=0 never, unset / 1 where a sweep costs something (4 mloc n (n + 1) >= 16 MiB) with a fill cap
  of 0.6, 2 or more at any size with a cap of 1.0; never without rows;
- the copy yields iff less is free than  min(32 GiB, 8 n16^2 rows) + exchange bytes + 41 GiB  -- never in the expanded form.

Every byte count is an integer below 2^53, so the doubles are exact and the comparisons can be asked at equality."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

GIB, MIB = 1 << 30, 1 << 20
RESIDENT, GENERATED, EXPANDED = range(3)
UNSET = (0, 0)
# (n, m): both sides of min(rows, 1024) (8000 / 64 rows), the 41 GiB cap (8 x 2400^2 x 1024 = 47.2e9 > 44.0e9), and the Gram
# term as the larger one (64 x 5008^2 against 8 x 64^2 x 1024)
SHAPES = [(2000, 8000), (2000, 64), (2400, 1100), (64, 5000)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("row_store_rule") / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "row_store_rule_driver.cpp")])
    return exe


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [row.split() for row in out.splitlines()]


FIELDS = ("n", "n16", "m", "mloc", "world", "astride", "R", "exch", "synthetic", "gemm")


def layout(exe, n, m, world=1, rank=0):
    return dict(zip(FIELDS, (int(t) for t in run(exe, [f"LAYOUT {n} {m} {world} {rank}"])[0])))


def fs(f):
    return " ".join(str(f[k]) for k in FIELDS)


def need(f):
    """the resident form's bytes, as the rule states them"""
    rows = max(1, f["mloc"])
    work = min(41 * GIB, max(8 * f["n16"] ** 2 * min(rows, 1024), 64 * f["R"] ** 2))
    return 8 * f["astride"] * rows + f["exch"] + work + 24 * f["m"] ** 2 + 16 * GIB


def want(f):
    """what must be free for the sweep copy to stay"""
    return min(32 * GIB, 8 * f["n16"] ** 2 * max(1, f["mloc"])) + f["exch"] + 41 * GIB


def stream(exe, f, free, total, known=1, env=UNSET):
    return run(exe, [f"STREAM {fs(f)} {known} {free} {total} {env[0]} {env[1]}"])[0][0] == "1"


def test_the_rule_header_compiles_alone(tmp_path):
    """no HIP call, no engine state: row_store_rule.h by itself is a translation unit"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "row_store_rule.h"\nint main() { return hdm_rows_batch(11, 4) == 4 ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


def test_the_constants_are_the_stated_ones(driver):
    c = [float.fromhex(t) for t in run(driver, ["CONSTANTS"])[0]]
    assert c == [41.0 * GIB, 16.0 * GIB, 32.0 * GIB, 0.97, 0.6]


@pytest.mark.parametrize("n,m", SHAPES)
def test_resident_need_term_for_term(driver, n, m):
    f = layout(driver, n, m)
    rows = max(1, f["mloc"])
    # the shape stands on the side of each clamp it is here for
    if (n, m) == (2000, 8000):
        assert rows > 1024 and 8 * f["n16"] ** 2 * 1024 < 41 * GIB
    if (n, m) == (2000, 64):
        assert rows < 1024
    if (n, m) == (2400, 1100):
        assert 8 * f["n16"] ** 2 * 1024 > 41 * GIB
    if (n, m) == (64, 5000):
        assert 64 * f["R"] ** 2 > 8 * f["n16"] ** 2 * 1024 and 64 * f["R"] ** 2 < 41 * GIB
    assert need(f) < 1 << 53
    assert float.fromhex(run(driver, [f"NEED {fs(f)}"])[0][0]) == float(need(f))


@pytest.mark.parametrize("n,m", SHAPES)
def test_one_device_compares_with_free_memory_strictly(driver, n, m):
    f = layout(driver, n, m)
    nd = need(f)
    for total in (nd // 2, 4 * nd):                       # (the capacity has no say on one device)
        assert stream(driver, f, nd, total) is False      # equal: it fits
        assert stream(driver, f, nd - MIB, total) is True
        assert stream(driver, f, nd + MIB, total) is False
        assert stream(driver, f, nd - 1, total) is True


@pytest.mark.parametrize("n,m", SHAPES)
def test_a_shard_compares_with_the_capacity_share(driver, n, m):
    """world = 2: against 0.97 x total, whatever is free.  The exchange bytes are a free term of the sum: they are moved (by
    less than 97 x 8 bytes) to make the need a multiple of 97, so that 0.97 x total can be the need exactly."""
    f = layout(driver, n, m, world=2, rank=0)
    assert f["world"] == 2 and f["mloc"] == (m + 1) // 2
    f["exch"] += (-need(f)) % 97
    nd = need(f)
    total = nd // 97 * 100
    assert nd % 97 == 0 and 0.97 * float(total) == float(nd)
    for free in (0, nd // 3, 16 * nd):
        assert stream(driver, f, free, total) is False
        assert stream(driver, f, free, total - 2 * MIB) is True        # 0.97 x 2 MiB: over one MiB below the need
        assert stream(driver, f, free, total + 2 * MIB) is False
    assert 0.97 * float(total - 100) == float(nd - 97)
    assert stream(driver, f, 0, total - 100) is True


def test_unknown_device_figures_do_not_stream(driver):
    f = layout(driver, 2000, 8000)
    assert stream(driver, f, 0, 0, known=1) is True
    assert stream(driver, f, 0, 0, known=0) is False
    f2 = layout(driver, 2000, 8000, world=2)
    assert stream(driver, f2, 0, 0, known=0) is False


def test_the_switch_overrides_both_ways(driver):
    f = layout(driver, 96, 50)
    nd = need(f)
    assert stream(driver, f, 4 * nd, 4 * nd) is False
    assert stream(driver, f, 4 * nd, 4 * nd, env=(1, 1)) is True
    assert stream(driver, f, 4 * nd, 4 * nd, env=(1, 7)) is True
    assert stream(driver, f, 0, 0) is True
    assert stream(driver, f, 0, 0, env=(1, 0)) is False
    assert stream(driver, f, 0, 0, known=0, env=(1, 1)) is True      # the switch needs no figures


def test_no_rows_never_stream(driver):
    f = layout(driver, 96, 50)
    f["mloc"] = 0
    assert stream(driver, f, 0, 0) is False
    assert stream(driver, f, 0, 0, env=(1, 1)) is False
    g = layout(driver, 96, 50)
    g["gemm"] = 0                                         # the rank-one and gather paths keep their rows resident
    assert stream(driver, g, 0, 0) is False
    assert stream(driver, g, 0, 0, env=(1, 1)) is False


def even_out(rows, bmax):
    launches = -(-rows // bmax)
    return -(-rows // launches)


@pytest.mark.parametrize("bc", [-3, 0, 1, 4, 24, 1024])
@pytest.mark.parametrize("mloc", [1, 11, 90, 1025])
def test_batch_rows(driver, mloc, bc):
    got, stated = (int(t) for t in run(driver, [f"BATCH {mloc} {bc}"])[0])
    assert got == stated == even_out(mloc, max(1, bc))
    assert 1 <= got <= max(1, bc) and -(-mloc // got) == -(-mloc // max(1, bc))     # no more launches than the clamp allows
    if (mloc, bc) == (11, 4):
        assert got == 4
    if (mloc, bc) == (1025, 1024):
        assert got == 513


def copy_rule(exe, f, has_rows=1, env=UNSET):
    b, cap = run(exe, [f"COPY {fs(f)} {has_rows} {env[0]} {env[1]}"])[0]
    return b == "1", float.fromhex(cap)


@pytest.mark.parametrize("n", [63, 260])
def test_sweep_copy_rule(driver, n):
    per_row = 4 * n * (n + 1)
    least = -(-(16 * MIB) // per_row)                     # the smallest mloc whose sweep costs something
    assert (least - 1) * per_row < 16 * MIB <= least * per_row
    assert run(driver, [f"COSTS {least} {n}", f"COSTS {least - 1} {n}"]) == [["1"], ["0"]]
    for mloc, costs in ((least, True), (least - 1, False)):
        f = layout(driver, n, mloc)
        assert f["mloc"] == mloc
        assert copy_rule(driver, f) == (costs, 0.6)                     # unset: by cost
        assert copy_rule(driver, f, env=(1, 1)) == (costs, 0.6)
        assert copy_rule(driver, f, env=(1, 0))[0] is False             # never
        assert copy_rule(driver, f, env=(1, 2)) == (True, 1.0)          # any size, any fill
        assert copy_rule(driver, f, env=(1, 3)) == (True, 1.0)
        for env in (UNSET, (1, 0), (1, 1), (1, 2), (1, 3)):
            assert copy_rule(driver, f, has_rows=0, env=env)[0] is False
            g = dict(f, mloc=0)
            assert copy_rule(driver, g, env=env)[0] is False


def yields(exe, form, in_use, f, free, known=1):
    return run(exe, [f"YIELDS {form} {in_use} {fs(f)} {known} {free}"])[0][0] == "1"


@pytest.mark.parametrize("n,m,term", [(2000, 2000, "cap"), (260, 90, "rows")])
def test_the_sweep_copy_yields_below_the_builders_bound(driver, n, m, term):
    f = layout(driver, n, m)
    rows_bytes = 8 * f["n16"] ** 2 * f["mloc"]
    assert (rows_bytes > 32 * GIB) == (term == "cap")     # each of the two terms of the min
    w = want(f)
    assert w == (32 * GIB if term == "cap" else rows_bytes) + f["exch"] + 41 * GIB
    for form in (RESIDENT, GENERATED):
        assert yields(driver, form, 1, f, w) is False     # equal: it stays
        assert yields(driver, form, 1, f, w - MIB) is True
        assert yields(driver, form, 1, f, w + MIB) is False
        assert yields(driver, form, 1, f, w - 1) is True
        assert yields(driver, form, 0, f, 0) is False     # no copy in use: nothing to yield
        assert yields(driver, form, 1, f, 0, known=0) is False
    for free in (0, w - MIB, w, w + MIB):                 # the only image of the data never goes
        assert yields(driver, EXPANDED, 1, f, free) is False
        assert yields(driver, EXPANDED, 0, f, free) is False
