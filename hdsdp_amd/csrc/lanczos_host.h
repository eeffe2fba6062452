// lanczos_host.h -- the host half of the ratio test (lanczos.hip), plain C++: the reference's start vector, the two small
// symmetric eigen-solvers, the choice of the two Ritz pairs, and the loop of HLanczosSolve (linalg/hdsdp_lanczos.c:161-292)
// written once over a backend that owns the vectors.  No HIP: tests/test_lanczos_rule_cpu.py runs it over dense loops.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "lanczos_rule.h"

// ---- glibc random_r TYPE_3 (r[i] = r[i-3] + r[i-31]), as srand(seed) / rand() use it -------------------------------
struct HdmGlibcRand {
    int f, b;   // front / rear indices of the 31-word state
    int32_t st[31];
    void seed(unsigned int s) {
        if (s == 0) s = 1;
        st[0] = (int32_t) s;
        long word = (int32_t) s;
        for (int i = 1; i < 31; ++i) {
            long hi = word / 127773, lo = word % 127773;
            word = 16807 * lo - 2836 * hi;
            if (word < 0) word += 2147483647;
            st[i] = (int32_t) word;
        }
        f = 3; b = 0;
        for (int i = 0; i < 310; ++i) (void) next();
    }
    int next() {
        uint32_t v = (uint32_t) st[f] + (uint32_t) st[b];
        st[f] = (int32_t) v;
        int out = (int) (v >> 1);
        if (++f >= 31) f = 0;
        if (++b >= 31) b = 0;
        return out;
    }
};

// HLanczosIPrepare's vector (glibc srand/rand stream reproduced without touching libc state)
inline void hdm_lanczos_start_vector(int n, double *p) {
    // HLanczosIPrepare (hdsdp_lanczos.c:33-42): srand(n); per entry srand(rand()); sqrt(sqrt(rand() % 1627)) * (rand() % 2 - 0.5)
    // (the reference re-seeds the one libc generator inside the loop, so a single generator object follows it)
    HdmGlibcRand g;
    g.seed((unsigned int) n);
    for (int i = 0; i < n; ++i) {
        g.seed((unsigned int) g.next());
        const int a = g.next() % 1627;
        const int b = g.next() % 2;
        p[i] = sqrt(sqrt((double) a)) * ((double) b - 0.5);
    }
}

// cyclic Jacobi for a small dense symmetric matrix (column-major k x k); eigenvalues ascending in d, vectors in Y
inline void jacobi_eig(int k, std::vector<double> A, std::vector<double> &d, std::vector<double> &Y) {
    Y.assign((size_t) k * k, 0.0);
    for (int i = 0; i < k; ++i) Y[(size_t) i * k + i] = 1.0;
    auto a = [&](int i, int j) -> double & { return A[(size_t) j * k + i]; };
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < k; ++p)
            for (int q = p + 1; q < k; ++q) off += a(p, q) * a(p, q);
        if (off < 1e-300) break;
        for (int p = 0; p < k; ++p)
            for (int q = p + 1; q < k; ++q) {
                const double apq = a(p, q);
                if (fabs(apq) < 1e-300) continue;
                const double theta = (a(q, q) - a(p, p)) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int r = 0; r < k; ++r) {
                    const double arp = a(r, p), arq = a(r, q);
                    a(r, p) = c * arp - s * arq;
                    a(r, q) = s * arp + c * arq;
                }
                for (int r = 0; r < k; ++r) {
                    const double apr = a(p, r), aqr = a(q, r);
                    a(p, r) = c * apr - s * aqr;
                    a(q, r) = s * apr + c * aqr;
                }
                for (int r = 0; r < k; ++r) {
                    const double yrp = Y[(size_t) p * k + r], yrq = Y[(size_t) q * k + r];
                    Y[(size_t) p * k + r] = c * yrp - s * yrq;
                    Y[(size_t) q * k + r] = s * yrp + c * yrq;
                }
            }
    }
    d.resize(k);
    for (int i = 0; i < k; ++i) d[i] = a(i, i);
    // ascending selection sort of (value, vector)
    for (int i = 0; i < k; ++i) {
        int mn = i;
        for (int j = i + 1; j < k; ++j) if (d[j] < d[mn]) mn = j;
        if (mn != i) {
            std::swap(d[i], d[mn]);
            for (int r = 0; r < k; ++r) std::swap(Y[(size_t) i * k + r], Y[(size_t) mn * k + r]);
        }
    }
}

// The Ritz matrix of a Lanczos run is TRIDIAGONAL: implicit QL with Wilkinson shifts (the EISPACK tql2 recurrence) instead of the
// cyclic Jacobi above, which took 1.1 ms at k = 30 and 3.7 ms over the ten checks of a 30-step test on a host core -- three
// times the device time of those steps once they ran in one launch per group.  U: the symmetric k x k matrix (column-major; only
// its diagonal and first subdiagonal are read).  Eigenvalues ascending in d, vectors in the columns of Y.  Returns false if an
// eigenvalue does not converge in 60 sweeps (the caller then takes the Jacobi route).
inline bool tridiag_eig(int k, const std::vector<double> &U, std::vector<double> &d, std::vector<double> &Y) {
    std::vector<double> e(k, 0.0);
    d.resize(k);
    for (int i = 0; i < k; ++i) d[i] = U[(size_t) i * k + i];
    for (int i = 0; i + 1 < k; ++i) e[i] = U[(size_t) i * k + i + 1];       // T(i + 1, i)
    Y.assign((size_t) k * k, 0.0);
    for (int i = 0; i < k; ++i) Y[(size_t) i * k + i] = 1.0;
    for (int l = 0; l < k; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < k - 1; ++m) {
                const double dd = fabs(d[m]) + fabs(d[m + 1]);
                if (fabs(e[m]) + dd == dd) break;
            }
            if (m != l) {
                if (iter++ == 60) return false;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = hypot(g, 1.0);
                g = d[m] - d[l] + e[l] / (g + copysign(r, g));
                double sn = 1.0, cs = 1.0, p = 0.0;
                int i;
                for (i = m - 1; i >= l; --i) {
                    double f = sn * e[i];
                    const double b = cs * e[i];
                    e[i + 1] = (r = hypot(f, g));
                    if (r == 0.0) { d[i + 1] -= p; e[m] = 0.0; break; }
                    sn = f / r; cs = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * sn + 2.0 * cs * b;
                    d[i + 1] = g + (p = sn * r);
                    g = cs * r - b;
                    double *yi = &Y[(size_t) i * k], *yi1 = &Y[(size_t) (i + 1) * k];
                    for (int q = 0; q < k; ++q) {
                        f = yi1[q];
                        yi1[q] = sn * yi[q] + cs * f;
                        yi[q] = cs * yi[q] - sn * f;
                    }
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p; e[l] = g; e[m] = 0.0;
            }
        } while (m != l);
    }
    for (int i = 0; i < k; ++i) {                 // ascending selection sort of (value, vector)
        int mn = i;
        for (int j = i + 1; j < k; ++j) if (d[j] < d[mn]) mn = j;
        if (mn != i) {
            std::swap(d[i], d[mn]);
            for (int r = 0; r < k; ++r) std::swap(Y[(size_t) i * k + r], Y[(size_t) mn * k + r]);
        }
    }
    return true;
}

// The two largest Ritz pairs of the leading kp x kp tridiagonal matrix (diag: kp entries, off: the kp - 1 beside them): QL,
// Jacobi if QL does not converge.  Sign convention: the component of largest magnitude is positive -- what LAPACK's
// tridiagonal eigenvector routines return (dstein scales that way, dstemr's twisted factorisation puts a positive 1 at the
// twist index) and what the one-launch kernel applies.  The sign of y1 matters: the NEXT ratio test is warm-started from
// Op (V y1) + 1e-3 x the pseudo-random vector (:166-181).  kp = 1: the second pair is the first.
struct HdmLzRitz { double eig1, eig2; std::vector<double> y1, y2; };
inline void hdm_lz_ritz(int kp, const double *diag, const double *off, HdmLzRitz *out) {
    std::vector<double> U((size_t) kp * kp, 0.0), d, Y;
    for (int i = 0; i < kp; ++i) U[(size_t) i * kp + i] = diag[i];
    for (int i = 0; i + 1 < kp; ++i) U[(size_t) i * kp + i + 1] = U[(size_t) (i + 1) * kp + i] = off[i];
    if (!tridiag_eig(kp, U, d, Y)) jacobi_eig(kp, U, d, Y);
    const int c1 = kp - 1, c2 = kp > 1 ? kp - 2 : kp - 1;
    for (int col : {c1, c2}) {
        double *yc = &Y[(size_t) col * kp], big = 0.0;
        for (int r = 0; r < kp; ++r) if (fabs(yc[r]) > fabs(big)) big = yc[r];
        if (big < 0.0) for (int r = 0; r < kp; ++r) yc[r] = -yc[r];
    }
    out->eig1 = d[c1]; out->eig2 = d[c2];
    out->y1.assign(Y.begin() + (size_t) c1 * kp, Y.begin() + (size_t) (c1 + 1) * kp);
    out->y2.assign(Y.begin() + (size_t) c2 * kp, Y.begin() + (size_t) (c2 + 1) * kp);
}

// HLanczosSolve's loop.  The backend owns the vectors and supplies three operations, each returning 0 or an error that
// ends the test and is handed back as it is:
//   start()                                          the start vector (fresh, or warm), normalised, as basis vector 0
//   steps(k, g, hprev, pairs)                        Lanczos steps k .. k + g - 1, hprev = the norm of step k - 1 (0 at
//                                                    k = 0); pairs: (alpha, norm) per step.  A zero norm ends the test at
//                                                    its step: what follows it in `pairs` is not looked at
//   residuals(kp, y1, y2, eig1, &r1, &r2)            z = V[:, 0..kp) y: r1 = |Op z1 - eig1 z1|, r2 = |Op z2 - eig1 z2|,
//                                                    and Op z1 becomes the next test's warm start
// step: the largest alpha with S + alpha dS >= 0 (INFINITY if unbounded); steps: Lanczos steps taken.
template <class Backend>
int hdm_lz_drive(Backend &be, double *step_out, int *steps_out) {
    double diag[LZ_MD + 1] = {0.0}, off[LZ_MD + 1] = {0.0};     // the tridiagonal matrix: -alpha_k, and norm_k beside it
    double pairs[2 * LZ_CHECK_FREQ] = {0.0};
    if (int rc = be.start()) return rc;
    HdmLzRitz R;
    double step = 0.0;
    int k = 0, k0 = 0, g = 0;
    for (k = 0; k < LZ_MD; ++k) {
        if (k >= k0 + g) {
            k0 = k; g = hdm_lz_group_len(k);
            if (int rc = be.steps(k, g, k > 0 ? off[k - 1] : 0.0, pairs)) return rc;
        }
        const double alp = pairs[2 * (k - k0)], nrm = pairs[2 * (k - k0) + 1];
        diag[k] = -alp;
        off[k] = nrm > 0.0 ? nrm : 0.0;
        if (!hdm_lz_check_due(k, nrm)) continue;
        const int kp = k + 1;
        hdm_lz_ritz(kp, diag, off, &R);
        if (!hdm_lz_residuals_due(fabs(off[k] * R.y1[k]), k)) continue;
        double r1 = 0.0, r2 = 0.0;
        if (int rc = be.residuals(kp, R.y1.data(), R.y2.data(), R.eig1, &r1, &r2)) return rc;
        const HdmLzAccept a = hdm_lz_accept(R.eig1, R.eig2, r1, r2, nrm);
        if (a.verdict == LZ_FAILED) return 1;
        step = a.step;
        if (a.verdict == LZ_ACCEPTED) break;
    }
    if (step_out) *step_out = step;
    if (steps_out) *steps_out = k;
    return 0;
}
