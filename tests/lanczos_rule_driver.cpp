// Driver of tests/test_lanczos_rule_cpu.py: csrc/lanczos_rule.h and csrc/lanczos_host.h compiled alone with the host compiler.
// One command per line on stdin, one row of numbers per command on stdout; doubles travel as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "lanczos_host.h"

static double rd(std::istream &in) { std::string s; in >> s; return strtod(s.c_str(), nullptr); }
static void put(double v) { printf(" %a", v); }

// the three operations of hdm_lz_drive over dense loops: Op x = Linv (-dS (Linv^T x)), Linv lower triangular, column-major
struct DenseBackend {
    int n; const double *Linv, *dS;
    int nComputed = 0;
    std::vector<double> V, warm, rnd, t1, t2, w;
    DenseBackend(int n_, const double *L, const double *D) : n(n_), Linv(L), dS(D), V((size_t) n_ * (LZ_MD + 1)), warm(n_, 0.0), rnd(n_),
                                                             t1(n_), t2(n_), w(n_) { hdm_lanczos_start_vector(n, rnd.data()); }
    void op(const double *x, double *out) {
        for (int j = 0; j < n; ++j) { double s = 0.0; for (int i = j; i < n; ++i) s += Linv[i + (size_t) j * n] * x[i]; t1[j] = s; }
        for (int j = 0; j < n; ++j) { double s = 0.0; for (int i = 0; i < n; ++i) s += dS[i + (size_t) j * n] * t1[i]; t2[j] = -s; }
        for (int i = 0; i < n; ++i) { double s = 0.0; for (int j = 0; j <= i; ++j) s += Linv[i + (size_t) j * n] * t2[j]; out[i] = s; }
    }
    int start() {
        std::fill(V.begin(), V.end(), 0.0);
        double s = 0.0;
        for (int i = 0; i < n; ++i) { V[i] = nComputed == 0 ? rnd[i] : warm[i] + LZ_WARM_WEIGHT * rnd[i]; s += V[i] * V[i]; }
        const double nr = sqrt(s), inv = nr > 0.0 ? 1.0 / nr : 0.0;
        for (int i = 0; i < n; ++i) V[i] *= inv;
        return 0;
    }
    int steps(int k, int g, double hprev, double *pairs) {
        for (int q = 0; q < g; ++q, ++k) {
            const double *vk = &V[(size_t) k * n];
            op(vk, w.data());
            if (k > 0) for (int i = 0; i < n; ++i) w[i] -= hprev * V[(size_t) (k - 1) * n + i];
            double dt = 0.0;
            for (int i = 0; i < n; ++i) dt += w[i] * vk[i];
            const double alp = -dt;
            double s = 0.0;
            for (int i = 0; i < n; ++i) { w[i] += alp * vk[i]; s += w[i] * w[i]; }
            const double nrm = sqrt(s);
            pairs[2 * q] = alp; pairs[2 * q + 1] = nrm;
            if (!(nrm > 0.0)) break;
            for (int i = 0; i < n; ++i) V[(size_t) (k + 1) * n + i] = w[i] / nrm;
            hprev = nrm;
        }
        return 0;
    }
    double resid(int kp, const double *y, double eig1, bool keep) {
        std::vector<double> z(n, 0.0), oz(n);
        for (int c = 0; c < kp; ++c) for (int i = 0; i < n; ++i) z[i] += V[(size_t) c * n + i] * y[c];
        op(z.data(), oz.data());
        if (keep) warm = oz;
        double s = 0.0;
        for (int i = 0; i < n; ++i) { const double d = oz[i] - eig1 * z[i]; s += d * d; }
        return sqrt(s);
    }
    int residuals(int kp, const double *y1, const double *y2, double eig1, double *r1, double *r2) {
        *r1 = resid(kp, y1, eig1, true);
        *r2 = resid(kp, y2, eig1, false);
        return 0;
    }
};

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "CONST") {
            printf("%d %d %a %a %a %a %a %d %d %d %d %d %d %d", LZ_MD, LZ_CHECK_FREQ, LZ_WARM_WEIGHT, LZ_RESID_TOL, LZ_GAP_FLOOR, LZ_ACCEPT_GAM,
                   LZ_ACCEPT_SUM, LZ_FUSED_MAX, LZ_RESIDENT_MAX, LZ_BIG_MAX, LZ_BIG_TRIPS8_MAX, LZG_WG, LZG_COLS, LZ_NCHUNK);
        } else if (cmd == "MAILBOX") {
            printf("%d %d %d %d %d %d %d %d %d %d", LZ_MB_R1, LZ_MB_R2, LZ_MB_Y1, LZ_MB_CARRY, LZ_MB_GROUP, LZ_MB_GROUP_LEN, LZ_MB_WHOLE, LZ_MB_WHOLE_LEN,
                   LZ_MB_Y2, LZ_MB_SIZE);
        } else if (cmd == "SWITCHES") {
            const HdmLzSwitches &s = hdm_lz_switches();
            printf("%d %d %d %d", (int) s.whole, (int) s.fused, (int) s.group, (int) s.big);
        } else if (cmd == "SETENV") {
            std::string k, v;
            in >> k >> v;
            setenv(k.c_str(), v.c_str(), 1);
            continue;
        } else if (cmd == "FORM") {           // n16 whole fused group big big_ok shared cus
            int n16, w, f, g, b, ok, sh, cus;
            in >> n16 >> w >> f >> g >> b >> ok >> sh >> cus;
            printf("%d", (int) hdm_lz_form(n16, HdmLzSwitches{w != 0, f != 0, g != 0, b != 0}, ok != 0, sh != 0, cus));
        } else if (cmd == "DUE") {            // k nrm -> check due, group length
            int k;
            in >> k;
            const double nrm = rd(in);
            printf("%d %d", (int) hdm_lz_check_due(k, nrm), hdm_lz_group_len(k));
        } else if (cmd == "RESID") {          // resiVal k
            const double r = rd(in);
            int k;
            in >> k;
            printf("%d", (int) hdm_lz_residuals_due(r, k));
        } else if (cmd == "ACCEPT") {         // eig1 eig2 r1 r2 nrm -> verdict step
            const double e1 = rd(in), e2 = rd(in), r1 = rd(in), r2 = rd(in), nrm = rd(in);
            const HdmLzAccept a = hdm_lz_accept(e1, e2, r1, r2, nrm);
            printf("%d", a.verdict);
            put(a.step);
        } else if (cmd == "EIG" || cmd == "RITZ") {   // EIG QL|JACOBI k diag.. off.. -> ok, k values, k x k vectors (by column)
            std::string which;
            if (cmd == "EIG") in >> which;
            int k;
            in >> k;
            std::vector<double> dg(k), of(k > 1 ? k - 1 : 0);
            for (double &v : dg) v = rd(in);
            for (double &v : of) v = rd(in);
            if (cmd == "RITZ") {              // -> eig1 eig2 y1.. y2..
                HdmLzRitz R;
                hdm_lz_ritz(k, dg.data(), of.data(), &R);
                put(R.eig1); put(R.eig2);
                for (double v : R.y1) put(v);
                for (double v : R.y2) put(v);
            } else {
                std::vector<double> U((size_t) k * k, 0.0), d, Y;
                for (int i = 0; i < k; ++i) U[(size_t) i * k + i] = dg[i];
                for (int i = 0; i + 1 < k; ++i) U[(size_t) i * k + i + 1] = U[(size_t) (i + 1) * k + i] = of[i];
                bool ok = true;
                if (which == "QL") ok = tridiag_eig(k, U, d, Y);
                else jacobi_eig(k, U, d, Y);
                printf("%d", (int) ok);
                if (ok) { for (double v : d) put(v); for (double v : Y) put(v); }
            }
        } else if (cmd == "DRIVE") {          // n file tests: file = Linv, then one dS per test, n x n doubles each, column-major -> per test: rc step steps
            int n, tests;
            std::string path;
            in >> n >> path >> tests;
            std::vector<double> L((size_t) n * n), D((size_t) n * n * tests);
            FILE *f = fopen(path.c_str(), "rb");
            if (!f || fread(L.data(), sizeof(double), L.size(), f) != L.size() || fread(D.data(), sizeof(double), D.size(), f) != D.size()) return 2;
            fclose(f);
            DenseBackend be(n, L.data(), D.data());
            for (int t = 0; t < tests; ++t) {     // consecutive tests on one object: the second and later ones warm-start
                be.dS = D.data() + (size_t) t * n * n;
                double step = 0.0;
                int steps = -1;
                const int rc = hdm_lz_drive(be, &step, &steps);
                if (rc == 0) be.nComputed += 1;
                printf("%s%d", t ? " " : "", rc);
                put(step);
                printf(" %d", steps);
            }
        } else {
            return 3;
        }
        printf("\n");
    }
    return 0;
}
