// cone_set.h -- membership of cones in an operator's sets (the check set, the ratio set), stated once.  Pure host code: no HIP
// call, no engine state, no cone type of its own (tests/test_cone_set_cpu.py compiles it alone).  DESIGN.md section 23.
// What a set ASKS is the set's business; this is what a set is on the member side.  A cone carries one link per KIND of set; a set
// names its members and the link of a cone that its kind uses.  Neither owns the other, either may be destroyed first, and
// nothing outside this header assigns a link:
//   adopt    takes a cone the caller found eligible.  One already here is not taken twice; one held by another set of the kind
//            that is ON stays there; one held by a set that is OFF moves here (the old set's slot becomes nullptr).
//   forget   (the link's, and its destructor: the cone is being destroyed) nulls the cone's slot and clears the link.
//   release  (the operator is initialised again or cleared; the set's destructor) clears every living member's link, empties
//            the set and turns it off.
// A launch puts the members it takes at the front of the set's table, in member order: launch_begin, launch_take, launch_made.
// What a set DOES with its members -- populate, switch, launch, answer -- is HdmQuestionSet's, below, stated once for every kind
// (tests/test_cone_set_launch_cpu.py); a kind supplies its rule, its table entry and its commit.
#pragma once
#include <cstddef>
#include <cstdio>
#include <vector>

template <class Cone> struct HdmConeSet;

// a cone's place in a set of one kind; not owned
template <class Cone> struct HdmConeLink {
    HdmConeSet<Cone> *set = nullptr;
    int slot = -1;
    HdmConeLink() = default;
    HdmConeLink(const HdmConeLink &) = delete;
    HdmConeLink &operator=(const HdmConeLink &) = delete;
    bool active() const { return set && set->on; }     // a member of a set whose switch is on
    void forget() {
        if (!set) return;
        if (slot >= 0 && slot < (int) set->members.size()) {
            Cone *&m = set->members[(size_t) slot];
            if (m && &(m->*(set->which)) == this) m = nullptr;
        }
        set = nullptr; slot = -1;
    }
    ~HdmConeLink() { forget(); }
};

template <class Cone> struct HdmConeSet {
    typedef HdmConeLink<Cone> Cone::*Which;
    const Which which;                     // the link of a cone that sets of this kind use
    bool on = false;                       // the set's switch
    std::vector<Cone *> members;           // in the order adopted; nullptr: destroyed since (not owned)
    std::vector<int> launched;             // slots of the members in the launch being made: entry t is at place t of the table
    // launches, members in the last one, members launched in all, members left out of the last launch
    long launches = 0, last_cones = 0, total_cones = 0, last_left_out = 0;

    explicit HdmConeSet(Which w) : which(w) {}
    HdmConeSet(const HdmConeSet &) = delete;
    ~HdmConeSet() { release(); }

    int count() const { int k = 0; for (const Cone *c : members) k += c ? 1 : 0; return k; }
    bool adopt(Cone *c) {
        HdmConeLink<Cone> &l = c->*which;
        if (l.set == this) return false;                       // (the same cone named twice)
        if (l.set) {
            if (l.set->on) return false;
            l.forget();
        }
        l.set = this; l.slot = (int) members.size();
        members.push_back(c);
        return true;
    }
    void release() {                       // the members are free again (for another operator's set)
        for (Cone *c : members) if (c) { (c->*which).set = nullptr; (c->*which).slot = -1; }
        members.clear(); launched.clear();
        on = false;
    }
    void reset_counters() { launches = last_cones = total_cones = last_left_out = 0; }
    // what the operator's Get call reports first: living members and the three launch counters
    void report(long out[4]) const { out[0] = count(); out[1] = launches; out[2] = last_cones; out[3] = total_cones; }

    void launch_begin() { launched.clear(); }
    int launch_take(size_t slot) { launched.push_back((int) slot); return (int) launched.size() - 1; }   // its place in the table
    void launch_made() { const long nl = (long) launched.size(); launches += 1; last_cones = nl; total_cones += nl; }
};

// What a kind says of a member when a question is put to the set: not a member now (the rule, asked again, does not admit it: it
// is left to its own path and not counted), left out (it cannot be asked: its own call fails as it would alone), or take.
enum HdmSetSort { HDM_SET_NOT_NOW = 0, HDM_SET_LEFT_OUT, HDM_SET_TAKE };

// A set that answers a question of type Q put to one member for all members in one launch.  The protocol -- the loops, the
// counters, the order of events -- is here; Kind (the derived struct, known at compile time) supplies, with k a member's slot:
//   NO_MEMORY                 the switch's message, with one %s for what could not be made
//   eligible(cone)            populate: the kind's membership rule
//   empty()                   every stored answer and every per-member record back to "nothing", one per slot
//   free_launch()             free what only a launch needs (tables, staging blocks)
//   prepare(k, cone)          switch: make what a launch needs of this member; nullptr, or what could not be made
//   alloc_tables()            switch: the tables, after every prepare; nullptr, or what could not be made
//   sort(k, cone, q)          launch: HdmSetSort, but for "already served", which is serves'
//   serves(k, cone, q)        does the member's stored answer serve q?  (It may gather q to where the launch reads it.)
//   fill(place, k, cone, q)   the table entry at `place`, "nothing reported" into the member's report word, and what the launch
//                             will overwrite marked unknown
//   fire(nl, q)               the launches of the first nl table entries and the synchronisation; nonzero: not made or not finished
//   commit(place, k, cone, q) after a launch that finished: a member whose word still says "nothing reported" keeps an empty
//                             answer, every other member's answer is stored
template <class Cone, class Kind> struct HdmQuestionSet : HdmConeSet<Cone> {
    typedef HdmConeSet<Cone> Base;
    long from_store = 0;                   // members' questions answered from what was stored, since the switch went on
    explicit HdmQuestionSet(typename Base::Which w) : Base(w) {}
    Kind &kind() { return static_cast<Kind &>(*this); }
    void release() { Base::release(); kind().free_launch(); from_store = 0; kind().empty(); }

    // HKKTInit: membership only.  find(i): the i-th cone of the operator as a Cone, or nullptr
    template <class Find> void populate(int n, Find find) {
        release();
        kind().reset_counters();            // (a kind with counters of its own since HKKTInit shadows it)
        for (int i = 0; i < n; ++i)
            if (Cone *c = find(i)) { if (kind().eligible(c)) this->adopt(c); }
        kind().empty();
    }
    // the switch: returns the number of members (0: off, or fewer than two members).  Turning it on makes everything a launch needs.
    int turn(int on_) {
        this->on = false;
        kind().free_launch();
        from_store = 0; kind().empty();
        const int n = this->count();
        if (!on_ || n < 2) return 0;
        const char *lacks = nullptr;
        for (size_t k = 0; k < this->members.size() && !lacks; ++k)
            if (Cone *c = this->members[k]) lacks = kind().prepare(k, c);
        if (!lacks) lacks = kind().alloc_tables();
        if (lacks) {
            kind().free_launch();
            fprintf(stderr, Kind::NO_MEMORY, lacks);
            return 0;
        }
        this->on = true;
        return n;
    }
    // One launch for every member that can be asked q and is not served already.  Nonzero: the launch could not be made or did
    // not finish -- no member's answer is valid then (fill has emptied them), and launch_made is not counted.
    template <class Q> int launch(const Q &q) {
        this->launch_begin();
        long left_out = 0;
        for (size_t k = 0; k < this->members.size(); ++k) {
            Cone *c = this->members[k];
            if (!c) continue;
            const HdmSetSort s = kind().sort(k, c, q);
            if (s == HDM_SET_NOT_NOW) continue;
            if (s == HDM_SET_LEFT_OUT || kind().serves(k, c, q)) { left_out += 1; continue; }
            kind().fill(this->launch_take(k), k, c, q);
        }
        this->last_left_out = left_out;
        const int nl = (int) this->launched.size();
        if (nl == 0) return 0;
        if (kind().fire(nl, q)) return 1;
        this->launch_made();
        for (int place = 0; place < nl; ++place) {
            const size_t k = (size_t) this->launched[(size_t) place];
            kind().commit(place, k, this->members[k], q);
        }
        return 0;
    }
    // the member in slot k is asked q: true when its stored answer serves q, from the store or after one launch
    template <class Q> bool answer(size_t k, Cone *c, const Q &q) {
        if (kind().serves(k, c, q)) { from_store += 1; return true; }
        return launch(q) == 0 && kind().serves(k, c, q);
    }
    // what the operator's Get call reports: Base::report, then answers from the store and members left out of the last launch
    void report(long out[6]) const { Base::report(out); out[4] = from_store; out[5] = this->last_left_out; }
};
