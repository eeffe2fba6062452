"""The one reader of the library's environment (csrc/env_switches.h), without a device: the header is compiled alone with the
host C++ compiler beside tests/env_switches_driver.cpp and run in child processes whose environment the test sets.  The
expected values are written here from the rules, not read back from the header:

- ON_UNLESS_ZERO: unset -> on; set -> atoi(text) != 0.  OFF_UNLESS_NONZERO: unset -> off; set -> atoi(text) != 0.
  INT: whether the variable is set, and atol(text).  STRING: the text.  atoi / atol: "", "abc" and "00" are 0; " 1" and "1x" are 1;
- ONCE: the first read in the process is kept whatever the environment says later; NOW: every read asks the environment;
- the list, the table of include/hdsdp_mi355x.h: the same names, each once, with the same default text."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hdsdp_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hdsdp_mi355x.h")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

# what atoi / atol make of the texts a user can set
TEXTS = {"": 0, "0": 0, "1": 1, "2": 2, "-1": -1, "abc": 0, " 1": 1, "1x": 1, "00": 0}
# the variables whose sites ask the environment at every call; every other one is read once per process
READ_NOW = {"LOCAL_RANK", "HDSDP_MI355X_GPUS", "HDSDP_MI355X_LOOPBACK", "HDSDP_MI355X_SHARD_MIN_N", "HDSDP_MI355X_TRANSPORT",
            "HDSDP_MI355X_A2A_PIECES", "HDSDP_MI355X_STAGED_A2A", "HDSDP_MI355X_FORCE_GEMM", "HDSDP_MI355X_FORCE_PATH",
            "HDSDP_MI355X_SPARSE_KKT", "HDSDP_MI355X_PRIMAL_SIGNED", "HDSDP_MI355X_DIRECT_ROWS", "HDSDP_MI355X_STREAM_A",
            "HDSDP_MI355X_DEVICE_M", "HDSDP_MI355X_REFINE", "HDSDP_MI355X_REFINE_TILES", "HDSDP_MI355X_PRELOAD",
            "HDSDP_MI355X_CALL_STATS", "HDM_TCAP_GIB", "HDM_BC", "HDM_NSPLIT", "HDM_GRAM_KSTAGES", "HDM_GRAM_QUEUE", "HDM_SHARE_T_SLABS"}


def build_driver(directory):
    exe = os.path.join(str(directory), "env_switches_driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-pthread", "-I", CSRC, "-o", exe, os.path.join(HERE, "env_switches_driver.cpp")])
    return exe


def run(exe, args, env):
    clean = {k: v for k, v in os.environ.items() if not (k.startswith("HDM_") or k.startswith("HDSDP_MI355X_") or k == "LOCAL_RANK")}
    clean.update(env)
    return subprocess.run([exe] + args, env=clean, capture_output=True, text=True, check=True).stdout.splitlines()


def driver_list(exe):
    """the list as the driver prints it: [(name, kind, read time, default text)]"""
    return [tuple(line.split("|")) for line in run(exe, ["LIST"], {})]


def header_table():
    """the public table: (its text, [(name, default text)]).  The table is column-aligned: names start in column 4, defaults in
    column 35, meanings in column 45; a default may go on in the same columns of the next line"""
    table = open(HEADER).read().split("environment switches")[1].split("utilities")[0]
    rows = []
    for line in table.splitlines():
        m = re.match(r"^ \*  ([A-Z][A-Z_0-9]+)\s", line)
        if m:
            assert line[4 + len(m.group(1)):35].strip() == "" and line[34] == " " and line[44:45] in ("", " "), "misaligned row: " + line
            rows.append([m.group(1), line[35:45].strip()])
        elif rows and line.startswith(" *") and line[2:35].strip() == "" and line[35:36].strip():
            rows[-1][1] += " " + line[35:45].strip()
    return table, [tuple(r) for r in rows]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("env_switches"))


def test_the_header_compiles_alone(tmp_path):
    """no HIP call, no engine state: env_switches.h by itself is a translation unit"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "env_switches.h"\nint main() { return hdm_env_table[ENV_ZS].kind == HdmEnvKind::INT ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


def test_the_list_is_the_public_table(driver):
    """both ways on name and default text, no name twice, the kinds are the four, and the read time of every variable is the one
    its site had before the list existed"""
    listed = driver_list(driver)
    names = [e[0] for e in listed]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    _, rows = header_table()
    assert len(set(r[0] for r in rows)) == len(rows)
    assert sorted((e[0], e[3]) for e in listed) == sorted(rows)
    assert set(e[1] for e in listed) == {"ON_UNLESS_ZERO", "OFF_UNLESS_NONZERO", "INT", "STRING"}
    assert [e[0] for e in listed if e[1] == "STRING"] == ["HDSDP_MI355X_TRANSPORT"]
    assert set(e[0] for e in listed if e[2] == "NOW") == READ_NOW and all(e[2] in ("ONCE", "NOW") for e in listed)
    assert not {"HDM_VAR", "HDM_CONG2_DIRECT", "HDM_DBG_SYNC", "HDM_GRAPHS"} & set(names)       # diagnostic builds only / retired


@pytest.mark.parametrize("text", [None] + list(TEXTS), ids=["unset"] + [repr(t) for t in TEXTS])
def test_every_kind_reads_what_its_rule_says(driver, text):
    names = ["HDM_DIAG_SWEEP", "HDM_POISON", "HDSDP_MI355X_ZS", "HDSDP_MI355X_TRANSPORT", "HDM_TCAP_GIB", "HDM_BC", "HDM_GRAM_KSTAGES",
             "HDM_NSPLIT", "HDM_SHARE_T_SLABS", "HDM_GRAM_QUEUE"]
    out = run(driver, ["READ"], {} if text is None else {n: text for n in names})
    if text is None:
        assert out == ["on_unless_zero 1", "off_unless_nonzero 0", "int 0 0", "string -", "knobs 32 1024 0 0 0 1 1"]
        return
    v = TEXTS[text]
    assert out[0] == "on_unless_zero %d" % (v != 0)
    assert out[1] == "off_unless_nonzero %d" % (v != 0)
    assert out[2] == "int 1 %d" % v
    assert out[3] == "string [%s]" % text
    # the work plan's knobs: a set HDM_GRAM_KSTAGES is at least 1, HDM_NSPLIT records that it was set, HDM_BC is taken as written
    assert out[4] == "knobs %d %d %d 1 %d %d %d" % (v, v, max(1, v), v, v != 0, v != 0)


def test_a_variable_read_once_keeps_its_first_reading_and_one_read_now_does_not(driver):
    """the driver reads, sets the four variables to another value in its own environment, and reads again"""
    first = {"HDSDP_MI355X_ZS": "3", "HDSDP_MI355X_REFINE": "3", "HDM_PERSIST": "0", "HDSDP_MI355X_SPARSE_KKT": "0"}
    #                                       ONCE int   NOW int   ONCE on / off, NOW on / off
    assert run(driver, ["WHEN", "1"], first) == ["1 3 1 3 0 0", "1 3 1 1 0 1"]
    assert run(driver, ["WHEN", "0"], {}) == ["0 0 0 0 1 1", "0 0 1 0 1 0"]      # "unset" is a first reading too


def test_concurrent_first_reads_agree(driver):
    for _ in range(5):
        assert run(driver, ["THREADS"], {"HDSDP_MI355X_AFFINE_S": "2"}) == ["2 2 2 2 2 2 2 2 2"]
