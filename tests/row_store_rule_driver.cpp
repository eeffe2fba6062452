// driver of tests/test_row_store_rule_cpu.py: csrc/row_store_rule.h compiled alone with the host compiler.  Reads one command per
// line from stdin and prints one line per command; all arguments are integers, doubles travel back as C hex floats.
//   FACTS = n n16 m mloc world astride R exch_bytes synthetic gemm_path      (HdmRowFacts, field by field)
//   LAYOUT n m world rank                    -> the FACTS the engine's layout gives a dense block (mloc = rows of `rank`)
//   NEED FACTS                               -> hdm_rows_resident_need
//   STREAM FACTS known free total set value  -> hdm_rows_stream (set value: HDSDP_MI355X_STREAM_A as read)
//   BATCH mloc bc_max                        -> hdm_rows_batch  hdm_even_out(mloc, max(1, bc_max))
//   COSTS mloc n                             -> hdm_sweep_costs
//   COPY FACTS has_rows set value            -> build max_fill  (set value: HDSDP_MI355X_ZS as read)
//   YIELDS form in_use FACTS known free      -> hdm_sweep_copy_yields (form 0 = RESIDENT, 1 = GENERATED, 2 = EXPANDED)
//   CONSTANTS                                -> work cap, Schur slack, intermediates cap (bytes), capacity share, fill cap
#include "row_store_rule.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static HdmRowFacts facts(const std::vector<long long> &v, size_t at) {
    HdmRowFacts f;
    f.n = (int) v.at(at); f.n16 = (int) v.at(at + 1); f.m = (long) v.at(at + 2); f.mloc = (long) v.at(at + 3); f.world = (int) v.at(at + 4);
    f.astride = (long) v.at(at + 5); f.R = (long) v.at(at + 6); f.exch_bytes = (size_t) v.at(at + 7);
    f.synthetic = v.at(at + 8) != 0; f.gemm_path = v.at(at + 9) != 0;
    return f;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        if (!(in >> cmd)) continue;
        std::vector<long long> v;
        while (in >> tok) v.push_back(strtoll(tok.c_str(), nullptr, 10));
        if (cmd == "LAYOUT") {
            const int n = (int) v.at(0), m = (int) v.at(1), world = (int) v.at(2), rank = (int) v.at(3);
            const HdmRowFacts f = hdm_row_facts(hdm_layout(n, world, (m + world - 1) / world), n, m, hdm_rows_of_rank(m, world, rank), false, true);
            printf("%d %d %ld %ld %d %ld %ld %zu %d %d\n", f.n, f.n16, f.m, f.mloc, f.world, f.astride, f.R, f.exch_bytes, (int) f.synthetic, (int) f.gemm_path);
        } else if (cmd == "NEED") printf("%a\n", hdm_rows_resident_need(facts(v, 0)));
        else if (cmd == "STREAM") {
            HdmDeviceFacts d;
            d.known = v.at(10) != 0; d.free_bytes = (size_t) v.at(11); d.total_bytes = (size_t) v.at(12);
            printf("%d\n", (int) hdm_rows_stream(facts(v, 0), d, HdmEnvInt{v.at(13) != 0, (long) v.at(14)}));
        } else if (cmd == "BATCH") printf("%ld %ld\n", hdm_rows_batch((long) v.at(0), (long) v.at(1)), hdm_even_out((long) v.at(0), std::max(1L, (long) v.at(1))));
        else if (cmd == "COSTS") printf("%d\n", (int) hdm_sweep_costs((long) v.at(0), (long) v.at(1)));
        else if (cmd == "COPY") {
            const HdmSweepCopyRule r = hdm_sweep_copy_rule(facts(v, 0), v.at(10) != 0, HdmEnvInt{v.at(11) != 0, (long) v.at(12)});
            printf("%d %a\n", (int) r.build, r.max_fill);
        } else if (cmd == "YIELDS") {
            HdmDeviceFacts d;
            d.known = v.at(12) != 0; d.free_bytes = (size_t) v.at(13);
            printf("%d\n", (int) hdm_sweep_copy_yields((HdmRowForm) (int) v.at(0), v.at(1) != 0, facts(v, 2), d));
        } else if (cmd == "CONSTANTS")
            printf("%a %a %a %a %a\n", HDM_ROWS_WORK_CAP_BYTES, HDM_ROWS_SCHUR_SLACK_BYTES, HDM_ROWS_T_CAP_BYTES, HDM_ROWS_CAPACITY_SHARE, HDM_SWEEP_COPY_MAX_FILL);
        else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
