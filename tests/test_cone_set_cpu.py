"""The membership rule of an operator's cone sets (csrc/cone_set.h), without a device: the header is compiled alone with the host
C++ compiler and driven through a script on stdin, with a cone that holds just its two links.  The expected values are written
here from the rule as DESIGN.md section 23 states it:

- adopt takes a cone in the order offered; one already in this set is not taken twice; one held by another set of the kind that
  is ON stays there; one held by a set that is OFF moves here, the old set's slot becomes null and its other slots do not move;
- forget (the cone is being destroyed) nulls the cone's slot and clears its link; count() skips the null;
- release clears every living member's link, empties the set and turns it off; a set's destruction releases;
- either side may be destroyed first; a cone is in at most one set of each KIND, and the kinds do not see each other;
- a launch's members stand at the front of the table in member order.

The driver's world: sets A and A2 of one kind (they use the cone's link `a`), set B of another (link `b`), cones 0..7; sets and
cones live on the heap, so that a build with -fsanitize=address,undefined sees a touch of anything freed
(profiles/cone_sets_refactor.txt)."""
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
struct Cone { HdmConeLink<Cone> a, b; };
struct Set : HdmConeSet<Cone> { using HdmConeSet<Cone>::HdmConeSet; };
static const char *NAMES[3] = {"A", "A2", "B"};
static Set *sets[3] = {nullptr, nullptr, nullptr};
static Cone *cones[8] = {};
static int set_no(const char *s) { for (int k = 0; k < 3; ++k) if (!strcmp(s, NAMES[k])) return k; return -1; }
static const char *set_name(const HdmConeSet<Cone> *s) { for (int k = 0; k < 3; ++k) if (s && s == sets[k]) return NAMES[k]; return s ? "?" : "-"; }
static int cone_no(const Cone *c) { for (int i = 0; i < 8; ++i) if (c && c == cones[i]) return i; return -1; }
static void show() {
    for (int k = 0; k < 3; ++k) {
        const Set *s = sets[k];
        if (!s) continue;
        long r[4];
        s->report(r);
        printf("%s on=%d count=%d members=", NAMES[k], s->on ? 1 : 0, s->count());
        for (size_t q = 0; q < s->members.size(); ++q) {
            if (q) printf(",");
            if (s->members[q]) printf("%d", cone_no(s->members[q])); else printf("-");
        }
        printf(" launched=");
        for (size_t q = 0; q < s->launched.size(); ++q) printf(q ? ",%d" : "%d", s->launched[q]);
        printf(" report=%ld,%ld,%ld,%ld left_out=%ld\n", r[0], r[1], r[2], r[3], s->last_left_out);
    }
    for (int i = 0; i < 8; ++i)
        if (cones[i]) printf("c%d a=%s:%d b=%s:%d active=%d%d\n", i, set_name(cones[i]->a.set), cones[i]->a.slot, set_name(cones[i]->b.set),
                             cones[i]->b.slot, cones[i]->a.active() ? 1 : 0, cones[i]->b.active() ? 1 : 0);
}
int main() {
    char what[16], name[16];
    int i, v;
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "show")) { show(); continue; }
        if (!strcmp(what, "new")) { if (scanf("%d", &i) != 1 || cones[i]) return 2; cones[i] = new Cone(); continue; }
        if (!strcmp(what, "free")) { if (scanf("%d", &i) != 1 || !cones[i]) return 2; delete cones[i]; cones[i] = nullptr; continue; }
        if (!strcmp(what, "forget")) {        // forget i a|b
            if (scanf("%d %15s", &i, name) != 2 || !cones[i]) return 2;
            (name[0] == 'a' ? cones[i]->a : cones[i]->b).forget();
            continue;
        }
        if (scanf("%15s", name) != 1) return 2;
        const int k = set_no(name);
        if (k < 0) return 2;
        if (!strcmp(what, "mk")) { if (sets[k]) return 2; sets[k] = new Set(k < 2 ? &Cone::a : &Cone::b); continue; }
        if (!sets[k]) return 2;
        Set &s = *sets[k];
        if (!strcmp(what, "del")) { delete sets[k]; sets[k] = nullptr; }
        else if (!strcmp(what, "on")) { if (scanf("%d", &v) != 1) return 2; s.on = v != 0; }
        else if (!strcmp(what, "release")) s.release();
        else if (!strcmp(what, "zero")) s.reset_counters();
        else if (!strcmp(what, "adopt")) { if (scanf("%d", &i) != 1 || !cones[i]) return 2; printf("adopt %d\n", s.adopt(cones[i]) ? 1 : 0); }
        else if (!strcmp(what, "launch")) {   // launch S i: every living member but cone i (-1: none left out), as the engine's loops go
            if (scanf("%d", &i) != 1) return 2;
            long left_out = 0;
            s.launch_begin();
            printf("places");
            for (size_t q = 0; q < s.members.size(); ++q) {
                Cone *c = s.members[q];
                if (!c) continue;
                if (cone_no(c) == i) { left_out += 1; continue; }
                printf(" %d@%d", cone_no(c), s.launch_take(q));
            }
            printf("\n");
            s.last_left_out = left_out;
            if (!s.launched.empty()) s.launch_made();
        } else return 2;
    }
    for (int k = 0; k < 3; ++k) delete sets[k];
    for (int q = 0; q < 8; ++q) delete cones[q];
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cone_set")
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


FOUR = "mk A new 0 new 1 new 2 new 3 adopt A 0 adopt A 1 adopt A 2 adopt A 3 "
FREE = "a=-:-1 b=-:-1 active=00"


def test_the_header_compiles_alone(tmp_path):
    """no HIP call, no engine state, no cone type of the engine's"""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "cone_set.h"\nstruct C { HdmConeLink<C> l; };\n'
                   "int main() { HdmConeSet<C> s(&C::l); C c; return (s.adopt(&c) && s.count() == 1 && c.l.slot == 0) ? 0 : 1; }\n")
    exe = str(tmp_path / "alone")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.run([exe]).returncode == 0


def test_four_cones_adopted_in_order(driver):
    st, ad = _run(driver, FOUR + "show")
    assert ad == [1, 1, 1, 1]
    assert st["A"] == "on=0 count=4 members=0,1,2,3 launched= report=4,0,0,0 left_out=0"
    for i in range(4):
        assert st[f"c{i}"] == f"a=A:{i} b=-:-1 active=00"
    st, _ = _run(driver, FOUR + "on A 1 show")
    assert st["c2"] == "a=A:2 b=-:-1 active=10"           # a member of a set whose switch is on


def test_the_same_cone_offered_twice(driver):
    st, ad = _run(driver, "mk A new 0 new 1 adopt A 0 adopt A 0 adopt A 1 adopt A 0 show")
    assert ad == [1, 0, 1, 0]
    assert st["A"].startswith("on=0 count=2 members=0,1 ")
    assert st["c0"] == "a=A:0 b=-:-1 active=00" and st["c1"] == "a=A:1 b=-:-1 active=00"


def test_a_member_is_forgotten(driver):
    st, _ = _run(driver, FOUR + "forget 1 a show")
    assert st["A"].startswith("on=0 count=3 members=0,-,2,3 ")
    assert st["c0"] == "a=A:0 b=-:-1 active=00"
    assert st["c1"] == FREE
    assert st["c2"] == "a=A:2 b=-:-1 active=00"
    assert st["c3"] == "a=A:3 b=-:-1 active=00"
    # forgotten twice, and destroyed afterwards: nothing more happens
    st2, _ = _run(driver, FOUR + "forget 1 a forget 1 a free 1 show")
    assert st2["A"] == st["A"] and "c1" not in st2


def test_an_active_set_keeps_its_members(driver):
    st, ad = _run(driver, FOUR + "on A 1 mk A2 adopt A2 0 adopt A2 1 adopt A2 2 adopt A2 3 show")
    assert ad == [1, 1, 1, 1, 0, 0, 0, 0]
    assert st["A"].startswith("on=1 count=4 members=0,1,2,3 ")
    assert st["A2"].startswith("on=0 count=0 members= ")
    for i in range(4):
        assert st[f"c{i}"] == f"a=A:{i} b=-:-1 active=10"


def test_an_inactive_set_gives_its_members_up(driver):
    """cone 1 has been destroyed; A2 takes the living ones in the order offered, A keeps its length and only nulls"""
    take = FOUR + "free 1 mk A2 adopt A2 3 adopt A2 0 adopt A2 2 "
    st, ad = _run(driver, take + "show")
    assert ad == [1, 1, 1, 1, 1, 1, 1]
    assert st["A"].startswith("on=0 count=0 members=-,-,-,- ")
    assert st["A2"].startswith("on=0 count=3 members=3,0,2 ")
    assert (st["c3"], st["c0"], st["c2"]) == ("a=A2:0 b=-:-1 active=00", "a=A2:1 b=-:-1 active=00", "a=A2:2 b=-:-1 active=00")
    # A's later release, and A's destruction, touch none of A2's members' links
    for end in ("release A show", "del A show"):
        st2, _ = _run(driver, take + "on A2 1 " + end)
        assert st2["A2"].startswith("on=1 count=3 members=3,0,2 ")
        assert (st2["c3"], st2["c0"], st2["c2"]) == ("a=A2:0 b=-:-1 active=10", "a=A2:1 b=-:-1 active=10", "a=A2:2 b=-:-1 active=10")
    # one cone moves while the others stay: the old set's other slots do not move
    st3, _ = _run(driver, FOUR + "mk A2 adopt A2 2 show")
    assert st3["A"].startswith("on=0 count=3 members=0,1,-,3 ")
    assert st3["c3"] == "a=A:3 b=-:-1 active=00" and st3["c2"] == "a=A2:0 b=-:-1 active=00"


def test_release(driver):
    st, _ = _run(driver, FOUR + "on A 1 launch A -1 free 2 release A show")
    assert st["A"] == "on=0 count=0 members= launched= report=0,1,4,4 left_out=0"     # (the counters are the caller's to reset)
    assert st["c0"] == FREE and st["c1"] == FREE and st["c3"] == FREE and "c2" not in st
    st, ad = _run(driver, FOUR + "on A 1 launch A -1 release A zero A adopt A 3 show")   # HKKTInit again
    assert ad[-1] == 1
    assert st["A"] == "on=0 count=1 members=3 launched= report=1,0,0,0 left_out=0"
    assert st["c3"] == "a=A:0 b=-:-1 active=00"


def test_the_set_is_destroyed_while_its_cones_live(driver):
    st, _ = _run(driver, FOUR + "on A 1 del A show free 0 free 1 free 2 free 3")
    assert "A" not in st
    for i in range(4):
        assert st[f"c{i}"] == FREE


def test_the_cones_are_destroyed_before_the_set(driver):
    st, _ = _run(driver, FOUR + "on A 1 forget 0 a free 0 free 1 free 2 forget 3 a free 3 show del A")
    assert st["A"].startswith("on=1 count=0 members=-,-,-,- ")
    assert [k for k in st if k.startswith("c")] == []


def test_a_member_of_two_kinds_of_set(driver):
    both = "mk A mk B new 0 new 1 new 2 adopt A 0 adopt A 1 adopt A 2 adopt B 2 adopt B 1 on A 1 "
    st, ad = _run(driver, both + "show")
    assert ad == [1, 1, 1, 1, 1]                              # B is another kind: A being on does not keep it from taking them
    assert st["c1"] == "a=A:1 b=B:1 active=10" and st["c2"] == "a=A:2 b=B:0 active=10" and st["c0"] == "a=A:0 b=-:-1 active=10"
    st, _ = _run(driver, both + "forget 1 a show")            # one link only
    assert st["A"].startswith("on=1 count=2 members=0,-,2 ") and st["B"].startswith("on=0 count=2 members=2,1 ")
    assert st["c1"] == "a=-:-1 b=B:1 active=00"
    st, _ = _run(driver, both + "free 1 show")                # the cone is destroyed: both sets lose it
    assert st["A"].startswith("on=1 count=2 members=0,-,2 ") and st["B"].startswith("on=0 count=1 members=2,- ")
    assert st["c2"] == "a=A:2 b=B:0 active=10"
    st, _ = _run(driver, both + "release B show")             # one set released: the other kind's links stay
    assert st["A"].startswith("on=1 count=3 members=0,1,2 ") and st["B"].startswith("on=0 count=0 members= ")
    assert st["c1"] == "a=A:1 b=-:-1 active=10" and st["c2"] == "a=A:2 b=-:-1 active=10"


def test_launched_members_stand_first_in_member_order(driver):
    """five members, the one in slot 3 destroyed, cone 1 left out of the launch: table places 0, 1, 2 hold slots 0, 2, 4"""
    out = subprocess.run([driver], input=FOUR + "new 4 adopt A 4 on A 1 free 3 launch A 1 show\n", capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert "places 0@0 2@1 4@2" in out
    st, _ = _run(driver, FOUR + "new 4 adopt A 4 on A 1 free 3 launch A 1 show")
    assert st["A"] == "on=1 count=4 members=0,1,2,-,4 launched=0,2,4 report=4,1,3,3 left_out=1"
    # a second launch takes everybody: the list starts again, the counters add up
    st, _ = _run(driver, FOUR + "new 4 adopt A 4 on A 1 free 3 launch A 1 launch A -1 show")
    assert st["A"] == "on=1 count=4 members=0,1,2,-,4 launched=0,1,2,4 report=4,2,4,7 left_out=0"
