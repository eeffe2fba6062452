// driver of tests/test_refine_rule_cpu.py: csrc/refine_rule.h and csrc/kkt_store.h compiled alone with the host compiler.  Reads one
// command per line from stdin and prints one line per query; fractions travel as C hex floats, so nothing is rounded on the way.
//   CLAMP k                     -> the step cap HMiLinsysSetRefine(k) leaves
//   TOL relTol absTol rhsNorm   -> tol
//   LOOP cap tol n2_0 n2_1 ...  one refined solve fed the squared residual norms in order (first the unrefined solve's)
//                               -> status keep steps solves resid0 resid consumed   (consumed: norms the loop asked for)
//   the state's transitions, as tests/kkt_store_driver.cpp names them:
//   INIT form permuted | START c | FINISH c | FOLDED | SCATTERED | SMALL | PIVOTED | HOSTM | MIRROR on | DO   (plan, then commit)
//   REFINE k                    "refinement was switched"
//   SOURCE                      -> matrix why_none permute pivoted wants_copy cap   (matrix 0 = none, 1 = device M, 2 = the copy)
#include "kkt_store.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

static const double hostM[1] = {0.0}, devM[1] = {0.0};

int main() {
    HdmKktState st;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        if (!(in >> cmd)) continue;
        std::vector<double> v;
        while (in >> tok) v.push_back(strtod(tok.c_str(), nullptr));
        if (cmd == "CLAMP") printf("%d\n", hdm_refine_clamp((int) v.at(0)));
        else if (cmd == "TOL") printf("%a\n", hdm_refine_tol(v.at(0), v.at(1), v.at(2)));
        else if (cmd == "LOOP") {
            HdmRefineLoop loop((int) v.at(0), v.at(1));
            size_t k = 2;
            bool more = loop.first(v.at(k++));
            while (more) more = loop.next(v.at(k++));
            printf("%d %d %d %d %a %a %d\n", (int) loop.status, (int) loop.keep, loop.steps, loop.solves, loop.resid0, loop.resid, (int) k - 2);
        }
        else if (cmd == "INIT") st.storage_decided((HdmKktForm) (int) v.at(0), v.at(1) != 0.0);
        else if (cmd == "START") st.build_started(v.at(0) != 0.0);
        else if (cmd == "FINISH") st.build_finished(v.at(0) != 0.0);
        else if (cmd == "FOLDED") st.channel_folded();
        else if (cmd == "SCATTERED") st.csc_scattered();
        else if (cmd == "SMALL") st.small_pass_done(devM, 128);
        else if (cmd == "PIVOTED") st.switched_to_pivoted();
        else if (cmd == "HOSTM") st.host_matrix_given(hostM, 77);
        else if (cmd == "MIRROR") st.mirror_switched(v.at(0) != 0.0);
        else if (cmd == "REFINE") st.refine_set((int) v.at(0));
        else if (cmd == "DO") {
            const HdmKktLoadPlan p = hdm_kkt_load_plan(st);
            if (p.ok) st.commit(p, hostM, 408, devM, 512);
        }
        else if (cmd == "SOURCE") {
            const HdmRefineSource s = hdm_kkt_refine_source(st);
            printf("%d %d %d %d %d %d\n", (int) s.matrix, (int) s.why_none, (int) s.permute, (int) s.pivoted, (int) st.refine_wants_copy(), st.refine());
        }
        else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
