// driver of tests/test_kkt_store_cpu.py: csrc/kkt_store.h compiled alone with the host compiler.  Reads one command per line from
// stdin and prints one line per query; fractions travel as C hex floats, so nothing is rounded on the way.
//   INIT form permuted          "HKKTInit decided the storage" (form 0 = DENSE, 1 = CSC, 2 = TILES)
//   START c | FINISH c          "a build started / finished" (c = 1: a corrector build)
//   FOLDED | SCATTERED | SMALL | PIVOTED | HOSTM     the transitions of those names (SMALL, HOSTM: with the driver's own matrices)
//   MIRROR on                   "the mirror was switched"
//   STATE                       -> form mirror permuted indef m_valid chan_folded source ld   (source 0 = none, 1 = host, 2 = device)
//   PLAN m nnz | DO m nnz       -> ok stage source load gather on_pivot matrix_bytes channel_bytes   (DO: the plan, then commit)
//   ENV nb nnz useperm  r c ... [perm ...]   -> cost first[0] .. first[nb-1]
//   RCMOK nnz m | TAKEN cost_rcm cost_nat | COUNT count m   -> 0 / 1
//   COLS m  beg[0..m] idx...    -> 0 / 1
//   SETENV name value | SWITCHES   -> sparse tiles envelope rcm device_m
#include "kkt_store.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

static const double hostM[1] = {0.0}, devM[1] = {0.0};   // stand-ins for the operator's host and device matrices
static const long LD_DEV = 512;

int main() {
    HdmKktState st;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        if (!(in >> cmd)) continue;
        if (cmd == "SETENV") { std::string k, v; in >> k >> v; setenv(k.c_str(), v.c_str(), 1); continue; }
        std::vector<double> v;
        while (in >> tok) v.push_back(strtod(tok.c_str(), nullptr));
        if (cmd == "INIT") st.storage_decided((HdmKktForm) (int) v.at(0), v.at(1) != 0.0);
        else if (cmd == "START") st.build_started(v.at(0) != 0.0);
        else if (cmd == "FINISH") st.build_finished(v.at(0) != 0.0);
        else if (cmd == "FOLDED") st.channel_folded();
        else if (cmd == "SCATTERED") st.csc_scattered();
        else if (cmd == "SMALL") st.small_pass_done(devM, 128);
        else if (cmd == "PIVOTED") st.switched_to_pivoted();
        else if (cmd == "HOSTM") st.host_matrix_given(hostM, 77);
        else if (cmd == "MIRROR") st.mirror_switched(v.at(0) != 0.0);
        else if (cmd == "STATE")
            printf("%d %d %d %d %d %d %d %ld\n", (int) st.form(), (int) st.mirror(), (int) st.permuted(), (int) st.indef(), (int) st.m_valid(),
                   (int) st.chan_folded(), st.src_host() == hostM ? 1 : st.src_dev() == devM ? 2 : 0, st.src_ld());
        else if (cmd == "PLAN" || cmd == "DO") {
            const long m = (long) v.at(0), nnz = (long) v.at(1);
            const HdmKktLoadPlan p = hdm_kkt_load_plan(st);
            printf("%d %d %d %d %d %d %lld %lld\n", (int) p.ok, (int) p.stage, (int) p.source, (int) p.load, (int) p.gather, (int) p.on_pivot,
                   (long long) p.matrix_bytes(m, nnz), (long long) p.channel_bytes(m));
            if (cmd == "DO" && p.ok) st.commit(p, hostM, m, devM, LD_DEV);
        } else if (cmd == "ENV") {
            const int nb = (int) v.at(0);
            const size_t nnz = (size_t) v.at(1);
            const bool useperm = v.at(2) != 0.0;
            std::vector<int> rows(nnz), cols(nnz), perm;
            for (size_t q = 0; q < nnz; ++q) { rows[q] = (int) v.at(3 + 2 * q); cols[q] = (int) v.at(4 + 2 * q); }
            for (size_t i = 3 + 2 * nnz; i < v.size(); ++i) perm.push_back((int) v[i]);
            const HdmKktEnvelope e = hdm_kkt_envelope(rows.data(), cols.data(), nnz, nb, useperm ? perm.data() : nullptr);
            printf("%a", e.cost);
            for (int b = 0; b < nb; ++b) printf(" %d", e.first[b]);
            printf("\n");
        } else if (cmd == "RCMOK") printf("%d\n", (int) hdm_kkt_rcm_eligible((int64_t) v.at(0), (int) v.at(1)));
        else if (cmd == "TAKEN") printf("%d\n", (int) hdm_kkt_rcm_taken(v.at(0), v.at(1)));
        else if (cmd == "COUNT") printf("%d\n", (int) hdm_kkt_count_is_sparse((int64_t) v.at(0), (int) v.at(1)));
        else if (cmd == "COLS") {
            const int m = (int) v.at(0);
            std::vector<int> beg, idx;
            for (int i = 0; i <= m; ++i) beg.push_back((int) v.at(1 + i));
            for (size_t i = 2 + m; i < v.size(); ++i) idx.push_back((int) v[i]);
            printf("%d\n", (int) hdm_kkt_columns_are_sparse(m, beg.data(), idx.data()));
        } else if (cmd == "SWITCHES") {
            const HdmKktSwitches s = hdm_kkt_switches();
            printf("%d %d %d %d %d\n", (int) s.sparse, (int) s.tiles, (int) s.envelope, (int) s.rcm, (int) s.device_m);
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
