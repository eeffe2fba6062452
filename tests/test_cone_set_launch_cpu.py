"""What an operator's question sets do with their members (csrc/cone_set.h: HdmQuestionSet), without a device: the header is
compiled alone with the host C++ compiler and driven through a script on stdin, with a fake kind whose "device" is a host
array, whose fire can be told to fail and can be told to leave chosen members' report words at "nothing reported".  The expected
values are written here from the protocol as DESIGN.md section 25 states it:

1. launch_begin, then the members in order, a null skipped;
2. the rule is asked again: a member it does not admit is neither launched nor counted, one that cannot be asked or is already
   served is left out and counted;
3. a taken member's table entry stands at its launch place, its report word says "nothing reported";
4. what the launch will overwrite is unknown from then on;
5. last_left_out is set; if nobody was taken there is no launch and no count, and the call returns 0;
6. a fire that fails returns nonzero before launch_made;
7. launch_made, then every launched member is committed unless its word still says "nothing reported".

The switch: fewer than two members stay off; a prepare or the tables failing frees everything through the free hook, prints the
kind's message once and returns 0; every turn empties the stored answers.  populate (HKKTInit) starts counters and answers from
zero and takes no member of another set of the kind that is ON (cone_set.h's rule, reached through the protocol).

The driver's world: sets A and A2 of the fake kind, cones 0..7 with id = number; a question is a non-negative int; a stored answer
is the question it serves (-1: none).  Sets, cones and the fake tables live on the heap, so that a build with
-fsanitize=address,undefined sees a touch of anything freed and anything not freed (profiles/question_sets_refactor.txt)."""
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
#include <cstring>
struct Cone { HdmConeLink<Cone> a; int id = 0; bool ok = true, can = true; };
struct Fake : HdmQuestionSet<Cone, Fake> {
    static constexpr const char *NO_MEMORY = "fake set: no memory for %s; the per-cone path stays\n";
    std::vector<int> ans, made;                 // per slot: the question the stored answer serves (-1: none); prepare made its piece
    int *table = nullptr, *words = nullptr;     // the "device": ids in launch order; one report word per slot
    int fires = 0, frees = 0, fail_fire = 0, fail_prep = -1, fail_tab = 0;
    bool mute[8] = {};
    Fake() : HdmQuestionSet<Cone, Fake>(&Cone::a) {}
    ~Fake() { free_launch(); }
    bool eligible(const Cone *c) const { return c->ok; }
    void empty() { ans.assign(members.size(), -1); }
    void free_launch() { delete[] table; delete[] words; table = words = nullptr; made.assign(members.size(), 0); frees += 1; }
    const char *prepare(size_t k, Cone *) { if ((int) k == fail_prep) return "a member's piece"; made[k] = 1; return nullptr; }
    const char *alloc_tables() {
        if (fail_tab) return "the table";
        table = new int[members.size()]; words = new int[members.size()];
        for (size_t k = 0; k < members.size(); ++k) table[k] = words[k] = -9;
        return nullptr;
    }
    HdmSetSort sort(size_t, Cone *c, const int &) { return !c->ok ? HDM_SET_NOT_NOW : c->can ? HDM_SET_TAKE : HDM_SET_LEFT_OUT; }
    bool serves(size_t k, Cone *, const int &q) { return ans[k] == q; }
    void fill(int place, size_t k, Cone *c, const int &) { table[place] = c->id; words[k] = -1; ans[k] = -1; }
    int fire(int nl, const int &q) {
        fires += 1;
        if (fail_fire) return 1;
        for (int p = 0; p < nl; ++p) if (!mute[table[p]]) words[launched[(size_t) p]] = 100 * q + table[p];
        return 0;
    }
    void commit(int, size_t k, Cone *c, const int &q) { if (words[k] < 0) return; ans[k] = q; printf("commit %d=%d\n", c->id, words[k]); }
};
static const char *NAMES[2] = {"A", "A2"};
static Fake *sets[2] = {nullptr, nullptr};
static Cone *cones[8] = {};
static int cone_no(const Cone *c) { for (int i = 0; i < 8; ++i) if (c && c == cones[i]) return i; return -1; }
static void show() {
    for (int s = 0; s < 2; ++s) {
        Fake *f = sets[s];
        if (!f) continue;
        long r[6];
        f->report(r);
        printf("%s on=%d members=", NAMES[s], f->on ? 1 : 0);
        for (size_t k = 0; k < f->members.size(); ++k) { if (k) printf(","); if (f->members[k]) printf("%d", cone_no(f->members[k])); else printf("-"); }
        printf(" launched=");
        for (size_t k = 0; k < f->launched.size(); ++k) printf(k ? ",%d" : "%d", f->launched[k]);
        printf(" report=%ld,%ld,%ld,%ld,%ld,%ld fires=%d ans=", r[0], r[1], r[2], r[3], r[4], r[5], f->fires);
        for (size_t k = 0; k < f->ans.size(); ++k) printf(k ? ",%d" : "%d", f->ans[k]);
        int made = 0;
        for (int m : f->made) made += m;
        printf(" made=%d tables=%d table=", made, f->table ? 1 : 0);
        for (size_t k = 0; f->table && k < f->launched.size(); ++k) printf(k ? ",%d" : "%d", f->table[k]);
        printf("\n");
    }
}
int main() {
    char what[16], name[16];
    int i, v;
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "show")) { show(); continue; }
        if (!strcmp(what, "new")) { if (scanf("%d", &i) != 1 || cones[i]) return 2; cones[i] = new Cone(); cones[i]->id = i; continue; }
        if (!strcmp(what, "free")) { if (scanf("%d", &i) != 1 || !cones[i]) return 2; delete cones[i]; cones[i] = nullptr; continue; }
        if (!strcmp(what, "inel")) { if (scanf("%d", &i) != 1 || !cones[i]) return 2; cones[i]->ok = false; continue; }
        if (!strcmp(what, "cannot")) { if (scanf("%d", &i) != 1 || !cones[i]) return 2; cones[i]->can = false; continue; }
        if (scanf("%15s", name) != 1) return 2;
        const int s = !strcmp(name, "A") ? 0 : !strcmp(name, "A2") ? 1 : -1;
        if (s < 0) return 2;
        if (!strcmp(what, "mk")) { if (sets[s]) return 2; sets[s] = new Fake(); continue; }
        if (!sets[s]) return 2;
        Fake &f = *sets[s];
        if (!strcmp(what, "del")) { delete sets[s]; sets[s] = nullptr; continue; }
        if (scanf("%d", &v) != 1) return 2;
        if (!strcmp(what, "pop")) f.populate(v, [&](int q) { return cones[q]; });       // HKKTInit over cones 0..v-1 (nullptr: no such cone)
        else if (!strcmp(what, "turn")) { const int k = f.turn(v); printf("turn %d\n", k); }
        else if (!strcmp(what, "failfire")) f.fail_fire = v;
        else if (!strcmp(what, "failprep")) f.fail_prep = v;
        else if (!strcmp(what, "failtab")) f.fail_tab = v;
        else if (!strcmp(what, "mute")) f.mute[v] = true;
        else if (!strcmp(what, "serve")) { if (scanf("%d", &i) != 1) return 2; f.ans[(size_t) cones[v]->a.slot] = i; }     // serve S cone q
        else if (!strcmp(what, "launch")) { const int r = f.launch(v); printf("launch %d\n", r); }
        else if (!strcmp(what, "answer")) {                                               // answer S cone q
            if (scanf("%d", &i) != 1) return 2;
            const bool r = f.answer((size_t) cones[v]->a.slot, cones[v], i);
            printf("answer %d\n", r ? 1 : 0);
        } else return 2;
    }
    for (int s = 0; s < 2; ++s) delete sets[s];
    for (int q = 0; q < 8; ++q) delete cones[q];
    return 0;
}
"""

FIVE = "mk A new 0 new 1 new 2 new 3 new 4 pop A 5 turn A 1 "


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cone_set_launch")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    return exe


def _run(exe, script):
    """({set name: its last `show` line as {key: value}}, the other lines in order, stderr)"""
    r = subprocess.run([exe], input=script + "\n", capture_output=True, text=True, check=True)
    state, events = {}, []
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key in ("A", "A2"):
            state[key] = dict(kv.split("=", 1) for kv in rest.split(" "))
        else:
            events.append(line)
    return state, events, r.stderr


def test_the_table_is_compact_in_launch_order(driver):
    """members {0..4}, member 1 served, member 3's cone destroyed: places 0, 1, 2 hold 0, 2, 4"""
    st, ev, _ = _run(driver, FIVE + "serve A 1 7 free 3 launch A 7 show")
    a = st["A"]
    assert ev == ["turn 5", "commit 0=700", "commit 2=702", "commit 4=704", "launch 0"]
    assert a["members"] == "0,1,2,-,4" and a["launched"] == "0,2,4" and a["table"] == "0,2,4"
    assert a["report"] == "4,1,3,3,0,1"          # living members; launches, last_cones, total_cones; from the store; last_left_out
    assert a["ans"] == "7,7,7,-1,7" and a["fires"] == "1"
    # a member that cannot be asked is left out and counted; one the rule no longer admits is neither launched nor counted
    st, ev, _ = _run(driver, FIVE + "cannot 1 inel 2 launch A 7 show")
    assert st["A"]["launched"] == "0,3,4" and st["A"]["table"] == "0,3,4" and st["A"]["report"] == "5,1,3,3,0,1"
    assert st["A"]["ans"] == "7,-1,-1,7,7"
    # a second launch: the list starts again, total_cones adds up, what was just answered is served and left out
    st, _, _ = _run(driver, FIVE + "serve A 1 7 free 3 launch A 7 launch A 8 show")
    assert st["A"]["launched"] == "0,1,2,4" and st["A"]["report"] == "4,2,4,7,0,0" and st["A"]["ans"] == "8,8,8,-1,8"


def test_nobody_to_launch(driver):
    script = FIVE + "launch A 7 launch A 7 show"
    st, ev, _ = _run(driver, script)
    assert ev[-1] == "launch 0" and [e for e in ev if e.startswith("commit")] == [f"commit {i}={700 + i}" for i in range(5)]
    assert st["A"]["fires"] == "1" and st["A"]["launched"] == ""
    assert st["A"]["report"] == "5,1,5,5,0,5"    # launches and the counts of the last real launch stand; everybody was left out


def test_fire_fails(driver):
    st, ev, _ = _run(driver, FIVE + "serve A 1 6 failfire A 1 launch A 7 show")
    assert ev == ["turn 5", "launch 1"]
    assert st["A"]["fires"] == "1" and st["A"]["report"] == "5,0,0,0,0,0"       # launch_made is not counted
    assert st["A"]["ans"] == "-1,-1,-1,-1,-1"                                  # no member's answer is valid afterwards
    st, ev, _ = _run(driver, FIVE + "failfire A 1 launch A 7 failfire A 0 launch A 7 show")
    assert ev[1] == "launch 1" and ev[-1] == "launch 0"
    assert st["A"]["launched"] == "0,1,2,3,4" and st["A"]["report"] == "5,1,5,5,0,0" and st["A"]["ans"] == "7,7,7,7,7"
    # the member that asked gets no answer from a failed launch
    st, ev, _ = _run(driver, FIVE + "failfire A 1 answer A 2 7 show")
    assert ev[-1] == "answer 0" and st["A"]["report"] == "5,0,0,0,0,0"


def test_a_member_the_launch_did_not_report_for(driver):
    st, ev, _ = _run(driver, FIVE + "mute A 2 launch A 7 show")
    assert ev == ["turn 5", "commit 0=700", "commit 1=701", "commit 3=703", "commit 4=704", "launch 0"]
    assert st["A"]["ans"] == "7,7,-1,7,7" and st["A"]["report"] == "5,1,5,5,0,0"
    # its own question fails after the one launch; the others' are then answered from the store
    st, ev, _ = _run(driver, FIVE + "mute A 2 answer A 2 7 answer A 0 7 answer A 4 7 show")
    assert [e for e in ev if e.startswith("answer")] == ["answer 0", "answer 1", "answer 1"]
    assert st["A"]["fires"] == "1" and st["A"]["report"] == "5,1,5,5,2,0"


def test_answer_launches_once_for_all(driver):
    st, ev, _ = _run(driver, FIVE + "answer A 3 7 answer A 0 7 answer A 3 8 show")
    assert [e for e in ev if e.startswith("answer")] == ["answer 1", "answer 1", "answer 1"]
    assert st["A"]["fires"] == "2" and st["A"]["report"] == "5,2,5,10,1,0" and st["A"]["ans"] == "8,8,8,8,8"


def test_a_cone_destroyed_between_two_launches(driver):
    st, ev, _ = _run(driver, FIVE + "launch A 7 free 2 launch A 8 show")
    assert ev[-5:] == ["commit 0=800", "commit 1=801", "commit 3=803", "commit 4=804", "launch 0"]
    assert st["A"]["members"] == "0,1,-,3,4" and st["A"]["launched"] == "0,1,3,4" and st["A"]["table"] == "0,1,3,4"
    assert st["A"]["report"] == "4,2,4,9,0,0" and st["A"]["ans"] == "8,8,7,8,8"


def test_the_switch(driver):
    # fewer than two members: 0, and the set stays off
    st, ev, err = _run(driver, "mk A new 0 new 1 inel 1 pop A 2 turn A 1 show")
    assert ev == ["turn 0"] and st["A"]["on"] == "0" and st["A"]["members"] == "0" and st["A"]["tables"] == "0" and err == ""
    st, ev, _ = _run(driver, "mk A new 0 new 1 pop A 2 free 1 turn A 1 show")
    assert ev == ["turn 0"] and st["A"]["on"] == "0"
    # on: every living member prepared, the tables made
    st, ev, err = _run(driver, FIVE.replace("turn", "free 3 turn") + "show")
    assert ev == ["turn 4"] and st["A"]["on"] == "1" and st["A"]["made"] == "4" and st["A"]["tables"] == "1" and err == ""
    # prepare fails for the member in slot 2: what slots 0 and 1 made is freed, one message, 0, off
    st, ev, err = _run(driver, "mk A new 0 new 1 new 2 new 3 new 4 pop A 5 failprep A 2 turn A 1 show")
    assert ev == ["turn 0"] and st["A"]["on"] == "0" and st["A"]["made"] == "0" and st["A"]["tables"] == "0"
    assert err == "fake set: no memory for a member's piece; the per-cone path stays\n"
    st, ev, err = _run(driver, "mk A new 0 new 1 new 2 pop A 3 failtab A 1 turn A 1 show")
    assert ev == ["turn 0"] and st["A"]["on"] == "0" and st["A"]["made"] == "0"
    assert err == "fake set: no memory for the table; the per-cone path stays\n"
    # off, then on again: every stored answer is emptied, and so is the count of answers from the store; the launch counters stay
    st, ev, _ = _run(driver, FIVE + "launch A 7 answer A 0 7 turn A 0 show turn A 1 show")
    assert ev[-2:] == ["turn 0", "turn 5"]
    assert st["A"]["on"] == "1" and st["A"]["ans"] == "-1,-1,-1,-1,-1" and st["A"]["report"] == "5,1,5,5,0,0"
    st, _, _ = _run(driver, FIVE + "launch A 7 turn A 0 show")
    assert st["A"]["on"] == "0" and st["A"]["ans"] == "-1,-1,-1,-1,-1" and st["A"]["tables"] == "0" and st["A"]["made"] == "0"


def test_populate_twice(driver):
    st, ev, _ = _run(driver, FIVE + "launch A 7 answer A 0 7 pop A 5 show")
    a = st["A"]
    assert a["on"] == "0" and a["members"] == "0,1,2,3,4" and a["launched"] == "" and a["report"] == "5,0,0,0,0,0"
    assert a["ans"] == "-1,-1,-1,-1,-1" and a["tables"] == "0" and a["made"] == "0"
    # members held by another set of the kind that is ON are not taken; an ineligible cone and a missing one neither
    st, _, _ = _run(driver, FIVE + "mk A2 new 5 new 7 inel 7 pop A2 8 show")
    assert st["A"]["members"] == "0,1,2,3,4" and st["A"]["on"] == "1"
    assert st["A2"]["members"] == "5" and st["A2"]["ans"] == "-1"
    # ... and those of one that is OFF move
    st, _, _ = _run(driver, FIVE + "turn A 0 mk A2 pop A2 3 show")
    assert st["A"]["members"] == "-,-,-,3,4" and st["A2"]["members"] == "0,1,2"


def test_either_side_destroyed_first(driver):
    _run(driver, FIVE + "launch A 7 del A free 0 free 1 show")
    _run(driver, FIVE + "launch A 7 free 0 free 1 free 2 free 3 free 4 launch A 8 del A show")
