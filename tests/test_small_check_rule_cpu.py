"""The rule of the one-launch interior check (csrc/small_check_rule.h), without a device: the header is compiled alone with the
host C++ compiler and asked at its edges.  The expected values are written here from the rule as DESIGN.md section 19 states it:

- the switch on, world == 1, constraint data resident, n16 <= 128;
- mloc * n16^2 <= 2^19 doubles for n16 <= 64 and <= 2^17 above;
- a factor object of one block with npad == 128;
- dynamic LDS of 8 * (128 * 129 + 128 + max(1, m)) bytes, at most 160 KB: m <= 3840 (never the binding bound: the data
  bound allows 2048 rows at most, at n16 = 16)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

DRIVER = r"""
#include "small_check_rule.h"
#include <cstdio>
int main() {
    int on, world, resident, n16, npad, nblk;
    long mloc;
    while (scanf("%d %d %d %d %ld %d %d", &on, &world, &resident, &n16, &mloc, &npad, &nblk) == 7) {
        HdmSmallCheckCone c;
        c.on = on != 0; c.world = world; c.resident = resident != 0; c.n16 = n16; c.mloc = mloc; c.fac_npad = npad; c.fac_nblk = nblk;
        printf("%d %d %d %ld\n", hdm_small_check_eligible(c) ? 1 : 0, hdm_small_check_block_ok(c) ? 1 : 0,
               hdm_small_check_factor_ok(npad, nblk) ? 1 : 0, hdm_small_check_lds_bytes(mloc));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("small_check_rule")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, str(src)])
    return exe


def ask(exe, on=1, world=1, resident=1, n16=16, mloc=1, npad=128, nblk=1):
    out = subprocess.run([exe], input=f"{on} {world} {resident} {n16} {mloc} {npad} {nblk}\n", capture_output=True, text=True, check=True).stdout
    e, b, f, lds = out.split()
    return {"eligible": e == "1", "block": b == "1", "factor": f == "1", "lds": int(lds)}


def test_the_rule_header_compiles_alone(tmp_path):
    """no HIP call, no engine state: small_check_rule.h by itself is a translation unit"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "small_check_rule.h"\nint main() { return hdm_small_check_factor_ok(128, 1) ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


@pytest.mark.parametrize("n16,bound,expect", [(64, 1 << 19, True), (80, 1 << 17, True), (128, 1 << 17, True), (144, 1 << 17, False)])
def test_dimension_edges(driver, n16, bound, expect):
    """n16 = 64 still has the 2^19 bound, 80 and 128 the 2^17 one, 144 is no small block whatever it owns"""
    assert ask(driver, n16=n16, mloc=1)["eligible"] is expect
    most = bound // (n16 * n16)
    assert ask(driver, n16=n16, mloc=most)["eligible"] is expect
    assert ask(driver, n16=n16, mloc=most + 1)["eligible"] is False
    if n16 == 64:       # what 80 may own is not what 64 may own: 2^17 / 64^2 = 32 rows would be the other bound
        assert most == 128 and ask(driver, n16=64, mloc=33)["eligible"] is True
    if n16 == 80:
        assert most == 20 and ask(driver, n16=80, mloc=21)["eligible"] is False


def test_data_bound_at_sixteen(driver):
    """mloc * n16^2 at 2^19 and at 2^19 + 256 for n16 = 16"""
    assert 2048 * 256 == 1 << 19
    assert ask(driver, n16=16, mloc=2048)["eligible"] is True
    assert ask(driver, n16=16, mloc=2049)["eligible"] is False


def test_data_bound_at_one_hundred_and_twenty_eight(driver):
    """mloc * n16^2 at 2^17 and at 2^17 + 128^2 for n16 = 128"""
    assert 8 * 128 * 128 == 1 << 17
    assert ask(driver, n16=128, mloc=8)["eligible"] is True
    assert ask(driver, n16=128, mloc=9)["eligible"] is False


def test_no_rows_is_a_block(driver):
    assert ask(driver, n16=16, mloc=0)["eligible"] is True
    assert ask(driver, n16=128, mloc=0)["eligible"] is True


def test_kind_conditions(driver):
    """switch off, two ranks, no resident data: the block's own part fails; a factor object of another shape: the factor's"""
    good = dict(n16=32, mloc=5)
    assert ask(driver, **good) == {"eligible": True, "block": True, "factor": True, "lds": 8 * (128 * 129 + 128 + 5)}
    for bad in (dict(on=0), dict(world=2), dict(resident=0)):
        r = ask(driver, **good, **bad)
        assert (r["eligible"], r["block"], r["factor"]) == (False, False, True), bad
    for bad in (dict(npad=256), dict(npad=64), dict(nblk=2), dict(npad=256, nblk=2), dict(npad=0, nblk=0)):
        r = ask(driver, **good, **bad)
        assert (r["eligible"], r["block"], r["factor"]) == (False, True, False), bad


def test_lds_bound(driver):
    """8 * (128 * 129 + 128 + max(1, m)) bytes against 160 KB: 3840 rows fit, 3841 do not; no row counts as one"""
    assert ask(driver, mloc=0)["lds"] == ask(driver, mloc=1)["lds"] == 8 * (128 * 129 + 128 + 1)
    assert ask(driver, mloc=3840)["lds"] == 160 * 1024
    assert ask(driver, mloc=3841)["lds"] == 160 * 1024 + 8
    # the data bound is the tighter one wherever n16 >= 16 (2048 rows at most), so the LDS bound is seen alone only below that:
    # n16 = 8 does not occur in the engine (n16 is a multiple of 16) but shows the LDS and the row bound of the launcher at work
    assert ask(driver, n16=8, mloc=3840)["block"] is True
    assert ask(driver, n16=8, mloc=3841)["block"] is False
    assert ask(driver, n16=8, mloc=4097)["block"] is False
