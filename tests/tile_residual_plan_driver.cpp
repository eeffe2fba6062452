// driver of tests/test_tile_residual_plan_cpu.py: csrc/tile_residual_plan.h and csrc/kkt_store.h compiled alone with the host compiler.
// One command per line on stdin:
//   PLAN m nb | bptr (nb + 1 numbers) | brow (bptr[nb] numbers)   three lines -> the plan:
//        N njobs nslots nrb
//        J tile qi qj rblk cblk slot_direct slot_trans diag       one per job, in order
//        P slot_ptr ...                                           nrb + 1 numbers
//        U slot_use ...                                           one per slot
//   the state's transitions as tests/refine_rule_driver.cpp names them, and
//   TILESW on                   "the tile form's switch was set"
//   SOURCE                      -> matrix why_none permute pivoted wants_copy wants_tile_copy cap tiles_switch
#include "kkt_store.h"
#include "tile_residual_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

static const double hostM[1] = {0.0}, devM[1] = {0.0};

static std::vector<int> numbers(const std::string &line) {
    std::istringstream in(line);
    std::vector<int> v;
    int k;
    while (in >> k) v.push_back(k);
    return v;
}

int main() {
    HdmKktState st;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        std::vector<double> v;
        double d;
        while (in >> d) v.push_back(d);
        if (cmd == "PLAN") {
            std::string l1, l2;
            if (!std::getline(std::cin, l1) || !std::getline(std::cin, l2)) return 3;
            const int m = (int) v.at(0), nb = (int) v.at(1);
            const std::vector<int> bptr = numbers(l1), brow = numbers(l2);
            if ((int) bptr.size() != nb + 1 || (int) brow.size() != bptr.back()) return 4;
            const HdmTileResPlan p = hdm_tile_residual_plan(m, nb, bptr.data(), brow.data());
            printf("N %d %d %d\n", (int) p.jobs.size(), p.nslots(), p.nrb);
            for (const HdmTileResJob &j : p.jobs)
                printf("J %d %d %d %d %d %d %d %d\n", j.tile, j.qi, j.qj, j.rblk, j.cblk, j.slot_direct, j.slot_trans, j.diag);
            printf("P");
            for (int s : p.slot_ptr) printf(" %d", s);
            printf("\nU");
            for (int s : p.slot_use) printf(" %d", s);
            printf("\n");
        }
        else if (cmd == "INIT") st.storage_decided((HdmKktForm) (int) v.at(0), v.at(1) != 0.0);
        else if (cmd == "START") st.build_started(v.at(0) != 0.0);
        else if (cmd == "FINISH") st.build_finished(v.at(0) != 0.0);
        else if (cmd == "FOLDED") st.channel_folded();
        else if (cmd == "MIRROR") st.mirror_switched(v.at(0) != 0.0);
        else if (cmd == "REFINE") st.refine_set((int) v.at(0));
        else if (cmd == "TILESW") st.refine_tiles_set(v.at(0) != 0.0);
        else if (cmd == "DO") {
            const HdmKktLoadPlan p = hdm_kkt_load_plan(st);
            if (p.ok) st.commit(p, hostM, 408, devM, 512);
        }
        else if (cmd == "SOURCE") {
            const HdmRefineSource s = hdm_kkt_refine_source(st);
            printf("%d %d %d %d %d %d %d %d\n", (int) s.matrix, (int) s.why_none, (int) s.permute, (int) s.pivoted, (int) st.refine_wants_copy(),
                   (int) st.refine_wants_tile_copy(), st.refine(), (int) st.refine_tiles());
        }
        else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
