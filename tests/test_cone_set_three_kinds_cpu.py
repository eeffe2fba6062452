"""csrc/cone_set.h with a cone that carries THREE links, as the engine's cone does since the step set (check, ratio, step:
DESIGN.md sections 23 and 24): the rule is not written again for a third kind, so what tests/test_cone_set_cpu.py pins for two
kinds must hold for the third and between all three.  The header is compiled alone with the host C++ compiler and driven through
a script on stdin; the driver's world is sets A, B, C of three kinds (links `a`, `b`, `c`) and a second set C2 of the third kind,
cones 0..5, everything on the heap.  Expected values are written here from the rule:

- the third kind's adopt / forget / release work as the others', and no kind sees another: a set of kind c that is ON keeps
  its members from C2, and keeps nothing from A or B;
- forgetting one link leaves the cone's two other memberships alone; destroying the cone leaves all three sets with a null;
- releasing or destroying one set clears only its own kind's links;
- a set of the third kind that is OFF gives its members up to another of its kind, slot by slot."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdsdp_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

DRIVER = r"""
#include "cone_set.h"
#include <cstdio>
#include <cstring>
struct Cone { HdmConeLink<Cone> a, b, c; };
struct Set : HdmConeSet<Cone> { using HdmConeSet<Cone>::HdmConeSet; };
static const char *NAMES[4] = {"A", "B", "C", "C2"};
static Set *sets[4] = {};
static Cone *cones[6] = {};
static int set_no(const char *s) { for (int k = 0; k < 4; ++k) if (!strcmp(s, NAMES[k])) return k; return -1; }
static const char *set_name(const HdmConeSet<Cone> *s) { for (int k = 0; k < 4; ++k) if (s && s == sets[k]) return NAMES[k]; return s ? "?" : "-"; }
static int cone_no(const Cone *c) { for (int i = 0; i < 6; ++i) if (c && c == cones[i]) return i; return -1; }
static HdmConeLink<Cone> &link_of(Cone *c, char k) { return k == 'a' ? c->a : k == 'b' ? c->b : c->c; }
static void show() {
    for (int k = 0; k < 4; ++k) {
        const Set *s = sets[k];
        if (!s) continue;
        printf("%s on=%d count=%d members=", NAMES[k], s->on ? 1 : 0, s->count());
        for (size_t q = 0; q < s->members.size(); ++q) {
            if (q) printf(",");
            if (s->members[q]) printf("%d", cone_no(s->members[q])); else printf("-");
        }
        printf("\n");
    }
    for (int i = 0; i < 6; ++i)
        if (cones[i]) {
            printf("c%d", i);
            for (char k : {'a', 'b', 'c'}) printf(" %c=%s:%d", k, set_name(link_of(cones[i], k).set), link_of(cones[i], k).slot);
            printf(" active=%d%d%d\n", cones[i]->a.active() ? 1 : 0, cones[i]->b.active() ? 1 : 0, cones[i]->c.active() ? 1 : 0);
        }
}
int main() {
    char what[16], name[16];
    int i, v;
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "show")) { show(); continue; }
        if (!strcmp(what, "new")) { if (scanf("%d", &i) != 1 || cones[i]) return 2; cones[i] = new Cone(); continue; }
        if (!strcmp(what, "free")) { if (scanf("%d", &i) != 1 || !cones[i]) return 2; delete cones[i]; cones[i] = nullptr; continue; }
        if (!strcmp(what, "forget")) {        // forget i a|b|c
            if (scanf("%d %15s", &i, name) != 2 || !cones[i]) return 2;
            link_of(cones[i], name[0]).forget();
            continue;
        }
        if (scanf("%15s", name) != 1) return 2;
        const int k = set_no(name);
        if (k < 0) return 2;
        if (!strcmp(what, "mk")) { if (sets[k]) return 2; sets[k] = new Set(k == 0 ? &Cone::a : k == 1 ? &Cone::b : &Cone::c); continue; }
        if (!sets[k]) return 2;
        Set &s = *sets[k];
        if (!strcmp(what, "del")) { delete sets[k]; sets[k] = nullptr; }
        else if (!strcmp(what, "on")) { if (scanf("%d", &v) != 1) return 2; s.on = v != 0; }
        else if (!strcmp(what, "release")) s.release();
        else if (!strcmp(what, "adopt")) { if (scanf("%d", &i) != 1 || !cones[i]) return 2; printf("adopt %d\n", s.adopt(cones[i]) ? 1 : 0); }
        else return 2;
    }
    for (int k = 0; k < 4; ++k) delete sets[k];
    for (int q = 0; q < 6; ++q) delete cones[q];
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cone_set3")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, str(src)])
    return exe


def _run(exe, script):
    """the lines the script printed, as {first word: rest} -- the last `show` wins -- plus the adopt answers in order"""
    out = subprocess.run([exe], input=script + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    state, adopted = {}, []
    for line in out:
        key, _, rest = line.partition(" ")
        if key == "adopt":
            adopted.append(int(rest))
        else:
            state[key] = rest
    return state, adopted


# cones 0, 1, 2 in all three kinds of set (the third kind in another order), all three switched on
ALL = ("mk A mk B mk C new 0 new 1 new 2 adopt A 0 adopt A 1 adopt A 2 adopt B 0 adopt B 1 adopt B 2 "
       "adopt C 2 adopt C 0 adopt C 1 on A 1 on B 1 on C 1 ")


def test_three_links_compile_and_the_third_kind_adopts(driver):
    st, ad = _run(driver, ALL + "show")
    assert ad == [1] * 9
    assert st["C"] == "on=1 count=3 members=2,0,1"
    assert st["c0"] == "a=A:0 b=B:0 c=C:1 active=111"
    assert st["c1"] == "a=A:1 b=B:1 c=C:2 active=111"
    assert st["c2"] == "a=A:2 b=B:2 c=C:0 active=111"


def test_an_active_set_of_the_third_kind_keeps_its_members_from_its_own_kind_only(driver):
    st, ad = _run(driver, ALL + "mk C2 adopt C2 0 adopt C2 2 new 3 adopt C2 3 adopt C 0 show")
    assert ad[9:] == [0, 0, 1, 0]                                 # C is on: 0 and 2 stay; a free cone is taken; 0 is in C already
    assert st["C"] == "on=1 count=3 members=2,0,1" and st["C2"] == "on=0 count=1 members=3"
    assert st["c3"] == "a=-:-1 b=-:-1 c=C2:0 active=000"
    # A and B being on kept nothing from C at the start, and C being on keeps nothing from a new set of kind a once A is off
    st, ad = _run(driver, ALL.replace("on A 1 ", "") + "del B mk B adopt B 1 show")
    assert ad[-1] == 1 and st["B"] == "on=0 count=1 members=1"
    assert st["c1"] == "a=A:1 b=B:0 c=C:2 active=001"


def test_one_link_forgotten_leaves_the_other_two(driver):
    st, _ = _run(driver, ALL + "forget 0 c show")
    assert st["C"] == "on=1 count=2 members=2,-,1"
    assert st["A"] == "on=1 count=3 members=0,1,2" and st["B"] == "on=1 count=3 members=0,1,2"
    assert st["c0"] == "a=A:0 b=B:0 c=-:-1 active=110"
    st, _ = _run(driver, ALL + "forget 0 a forget 0 b show")
    assert st["c0"] == "a=-:-1 b=-:-1 c=C:1 active=001" and st["C"] == "on=1 count=3 members=2,0,1"


def test_a_destroyed_cone_leaves_a_null_in_all_three(driver):
    st, _ = _run(driver, ALL + "free 2 show")
    assert (st["A"], st["B"], st["C"]) == ("on=1 count=2 members=0,1,-", "on=1 count=2 members=0,1,-", "on=1 count=2 members=-,0,1")
    assert "c2" not in st and st["c1"] == "a=A:1 b=B:1 c=C:2 active=111"


def test_release_and_destruction_clear_one_kind(driver):
    for end in ("release C show", "del C show"):
        st, _ = _run(driver, ALL + end)
        assert st.get("C", "on=0 count=0 members=") == "on=0 count=0 members="
        for i in range(3):
            assert st[f"c{i}"] == f"a=A:{i} b=B:{i} c=-:-1 active=110"
    st, _ = _run(driver, ALL + "release A release B show")
    assert st["C"] == "on=1 count=3 members=2,0,1"
    assert st["c0"] == "a=-:-1 b=-:-1 c=C:1 active=001"


def test_an_inactive_set_of_the_third_kind_gives_its_members_up(driver):
    st, ad = _run(driver, ALL + "on C 0 mk C2 adopt C2 0 show")
    assert ad[-1] == 1
    assert st["C"] == "on=0 count=2 members=2,-,1" and st["C2"] == "on=0 count=1 members=0"
    assert st["c0"] == "a=A:0 b=B:0 c=C2:0 active=110"
    # the sets go first, then the cones: nothing dangles (the driver deletes whatever is left at exit)
    st, _ = _run(driver, ALL + "del A del C show del B")
    for i in range(3):
        assert st[f"c{i}"] == f"a=-:-1 b=B:{i} c=-:-1 active=010"
