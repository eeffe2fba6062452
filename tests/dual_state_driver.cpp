// driver of tests/test_dual_state_cpu.py: csrc/dual_state.h compiled alone with the host compiler.  Reads one command per line
// from stdin and prints one line per query; numbers travel as C hex floats, so nothing is rounded on the way.
//   S | D | ADV  tau eye y...   transitions "S assembled at", "dS assembled at", "S advanced to"
//   OVER | DATA | STALE         "S written by someone else", "the data changed", "factor stale"
//   FAC r                       "S factored with result r"
//   FACAT tau eye y...          -> held psd          (S_factored_at)
//   PLAN | DO  target mode world tau eye y...        (DO: the plan, then commit; target 0 = S, 1 = checker, 2 = dS)
//                               -> action alpha delta counter tracked line_missed off_line worst worst_at
//   MODE mloc n                 -> hdm_dual_mode
//   MISS target mode world tau eye y...   -> the HDSDP_MI355X_AFFINE_DEBUG line of that request
#include "dual_state.h"
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

int main() {
    HdmDualState st;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        if (!(in >> cmd)) continue;
        int target = 0, mode = 0, world = 1;
        if (cmd == "PLAN" || cmd == "DO" || cmd == "MISS") in >> target >> mode >> world;
        std::vector<double> v;
        while (in >> tok) v.push_back(strtod(tok.c_str(), nullptr));
        HdmDualPoint p;
        if (v.size() >= 2) { p.tau = v[0]; p.eye = v[1]; p.y = v.data() + 2; p.ny = (int) v.size() - 2; }
        if (cmd == "S") st.S_assembled_at(p);
        else if (cmd == "D") st.dS_assembled_at(p);
        else if (cmd == "ADV") st.S_advanced_to(p);
        else if (cmd == "OVER") st.S_overwritten();
        else if (cmd == "DATA") st.data_changed();
        else if (cmd == "STALE") st.factor_stale();
        else if (cmd == "FAC") st.S_factored((int) v.at(0));
        else if (cmd == "FACAT") { int psd = -1; const bool held = st.S_factored_at(p, &psd); printf("%d %d\n", held ? 1 : 0, psd); }
        else if (cmd == "MODE") printf("%d\n", hdm_dual_mode((long) v.at(0), (long) v.at(1)));
        else if (cmd == "PLAN" || cmd == "DO" || cmd == "MISS") {
            const HdmDualPlan r = hdm_dual_plan(st, p, (HdmDualTarget) target, mode, world);
            if (cmd == "MISS") { hdm_dual_print_miss(stdout, st, p, (HdmDualTarget) target, r); continue; }
            printf("%d %a %a %d %d %d %d %a %d\n", (int) r.action, r.alpha, r.delta, (int) r.counter, r.tracked ? 1 : 0, r.line_missed ? 1 : 0,
                   r.off_line, r.worst, r.worst_at);
            if (cmd == "DO") st.commit(r, p, (HdmDualTarget) target);
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
