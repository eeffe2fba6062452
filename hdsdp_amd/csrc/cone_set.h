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
#pragma once
#include <cstddef>
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
