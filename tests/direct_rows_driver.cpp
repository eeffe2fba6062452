// driver of tests/test_direct_rows_cpu.py: csrc/direct_rows.h compiled alone with the host compiler.  Reads one command per line
// from stdin and prints one line per query; fractions travel as C hex floats, so nothing is rounded on the way.
//   RULE world synthetic streamed natural_path force_gemm force_path n n16 sw     -> on kmax
//   KMAX n16                                                                      -> hdm_direct_kmax(n16) HDM_DR_MIN_N
//   NTERMS type stored kmax                                                       -> terms the row would take (0: congruence row)
//   PART on kmax table_bytes type stored type stored ...                          -> nCongruence nDirect nRankOne nterms order...
//   DECODE pk n                                                                   -> row col
//   TERMS type n sign slot pk val pk val ...                                      -> c x y  c x y ...
//   VALUE type n sign pk val ... | u_0 .. u_{n-1} | Linv (n x n, column-major)    -> the n x n transformed row, column-major
#include "direct_rows.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

static_assert(hdm_direct_rule(1, false, false, 0, false, false, 4096, 4096, 3).kmax == 3, "usable in constant expressions");
static_assert(hdm_direct_nterms(HDM_DR_DSR1, 100000, 1) == 1 && hdm_direct_nterms(HDM_DR_DENSE, 2, 8) == 0, "class rules");

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        if (!(in >> cmd)) continue;
        std::vector<std::string> w;
        while (in >> tok) w.push_back(tok);
        auto I = [&](size_t k) { return strtol(w.at(k).c_str(), nullptr, 10); };
        auto D = [&](size_t k) { return strtod(w.at(k).c_str(), nullptr); };
        if (cmd == "RULE") {
            const HdmDirectRule r = hdm_direct_rule((int) I(0), I(1) != 0, I(2) != 0, (int) I(3), I(4) != 0, I(5) != 0, (int) I(6), (int) I(7), (int) I(8));
            printf("%d %d", (int) r.on, r.kmax);
        } else if (cmd == "KMAX") {
            printf("%d %d", hdm_direct_kmax((int) I(0)), HDM_DR_MIN_N);
        } else if (cmd == "NTERMS") {
            printf("%ld", hdm_direct_nterms((int) I(0), I(1), (int) I(2)));
        } else if (cmd == "PART") {
            std::vector<int> type;
            std::vector<long> stored;
            for (size_t k = 3; k + 1 < w.size(); k += 2) { type.push_back((int) I(k)); stored.push_back(I(k + 1)); }
            const HdmDirectPlan p = hdm_direct_partition(type, stored, HdmDirectRule{I(0) != 0, (int) I(1)}, I(2));
            printf("%d %d %d %ld", p.nCongruence, p.nDirect, p.nRankOne, p.nterms);
            for (int i : p.order) printf(" %d", i);
        } else if (cmd == "DECODE") {
            int r = 0, c = 0;
            hdm_packed_decode(I(0), (int) I(1), &r, &c);
            printf("%d %d", r, c);
        } else if (cmd == "TERMS" || cmd == "VALUE") {
            const int type = (int) I(0), n = (int) I(1);
            const double sign = D(2);
            size_t k = cmd == "TERMS" ? 4 : 3;
            std::vector<int> idx;
            std::vector<double> val;
            for (; k + 1 < w.size() && w[k] != "|"; k += 2) { idx.push_back((int) I(k)); val.push_back(D(k + 1)); }
            std::vector<HdmDirectTerm> t;
            hdm_direct_terms(type, n, idx, val, sign, cmd == "TERMS" ? (int) I(3) : 0, t);
            if (cmd == "TERMS") {
                for (const HdmDirectTerm &e : t) printf("%a %d %d ", e.c, e.x, e.y);
            } else {
                std::vector<double> U, L;
                for (k += 1; w.at(k) != "|"; ++k) U.push_back(D(k));
                for (k += 1; k < w.size(); ++k) L.push_back(D(k));
                if ((int) U.size() != n || (long) L.size() != (long) n * n) { printf("bad"); }
                else
                    for (int j = 0; j < n; ++j)
                        for (int i = 0; i < n; ++i) printf("%a ", hdm_direct_value(t.data(), (long) t.size(), L.data(), n, U.data(), n, i, j));
            }
        } else {
            printf("?");
        }
        printf("\n");
    }
    return 0;
}
