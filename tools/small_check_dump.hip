// small_check_dump.hip -- what hdm_small_check_kernel writes for a fixed list of shapes, as one binary file.
// A stand-alone program around csrc/small.hip (nothing of the engine): seeded data, one hdm_small_check launch per case, and the
// dual matrix S, the factor L, its inverse W, info and log det of every case appended to the output file.  Built against two
// trees it shows whether a change of small.hip moved the existing kernel's results: `cmp` of the two files.
// (profiles/grouped_check_refactor.txt was made this way.)
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I hdsdp_amd/csrc tools/small_check_dump.hip hdsdp_amd/csrc/small.hip \
//         hdsdp_amd/csrc/alloc.cpp -x hip -o small_check_dump
//   ./small_check_dump out.bin
#include "small.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd() {                                  // splitmix64 -> (-1, 1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double) (z >> 11) / (double) (1ull << 52) - 1.0;
}

struct Case { int n, m; double tau, eye, diag; };      // diag: C = noise + diag I (a negative one makes S indefinite)

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s out.bin\n", argv[0]); return 2; }
    const Case cases[] = {{1, 3, 1.0, 0.0, 4.0},   {15, 6, 1.0, 0.1, 4.0},  {16, 6, 0.9, 0.0, 4.0},  {17, 20, 1.0, -0.3, 4.0}, {63, 5, 1.1, 0.0, 4.0},
                          {64, 128, 1.0, 0.2, 4.0}, {65, 4, 1.0, 0.0, 4.0},  {127, 8, 0.7, 0.05, 4.0}, {128, 8, 1.0, 0.0, 4.0},  {5, 0, 1.0, 0.0, 4.0},
                          {12, 1, 1.0, 0.0, 4.0},  {16, 2048, 1.0, 0.0, 4.0}, {33, 7, 1.0, 0.0, -0.5}, {128, 3, 1.0, 0.0, -0.5}};
    FILE *f = fopen(argv[1], "wb");
    if (!f) { perror(argv[1]); return 2; }
    hipStream_t s;
    CK(hipStreamCreate(&s));
    double *L = nullptr, *W = nullptr;
    const size_t pp = (size_t) SMALL_P * SMALL_P;
    CK(hipMalloc((void **) &L, sizeof(double) * pp));
    CK(hipMalloc((void **) &W, sizeof(double) * pp));
    std::vector<double> hL(pp), hW(pp);
    for (const Case &c : cases) {
        const int n16 = (c.n + 15) / 16 * 16;
        const size_t n2 = (size_t) n16 * n16;
        std::vector<double> A(n2 * (size_t) (c.m > 0 ? c.m : 1), 0.0), C(n2, 0.0), y((size_t) c.m + 4, 0.0), S(n2, 0.0);
        for (int q = 0; q < c.m; ++q)                  // A_L form: strict lower + half diagonal; every third matrix dense
            for (int j = 0; j < c.n; ++j)
                for (int i = j; i < c.n; ++i) {
                    const double v = rnd(), keep = rnd();
                    if (q % 3 == 0 || keep > 0.4) A[(size_t) q * n2 + i + (size_t) j * n16] = (i == j) ? 0.5 * v : v;
                }
        for (int j = 0; j < c.n; ++j)
            for (int i = j; i < c.n; ++i) {
                const double v = 0.1 * rnd() + (i == j ? c.diag : 0.0);
                C[i + (size_t) j * n16] = v; C[j + (size_t) i * n16] = v;
            }
        for (int q = 0; q < c.m; ++q) y[(size_t) q] = 0.02 * rnd() / (c.m > 64 ? 16.0 : 1.0);
        double *dA, *dC, *dS, *yo;
        CK(hipMalloc((void **) &dA, sizeof(double) * A.size()));
        CK(hipMalloc((void **) &dC, sizeof(double) * n2));
        CK(hipMalloc((void **) &dS, sizeof(double) * n2));
        CK(hipHostMalloc((void **) &yo, sizeof(double) * y.size(), hipHostMallocMapped));
        CK(hipMemcpy(dA, A.data(), sizeof(double) * A.size(), hipMemcpyHostToDevice));
        CK(hipMemcpy(dC, C.data(), sizeof(double) * n2, hipMemcpyHostToDevice));
        CK(hipMemset(dS, 0, sizeof(double) * n2));
        CK(hipMemset(L, 0, sizeof(double) * pp));
        CK(hipMemset(W, 0, sizeof(double) * pp));
        for (size_t q = 0; q < y.size(); ++q) yo[q] = y[q];
        yo[c.m] = -1.0;
        double *yd = nullptr;
        CK(hipHostGetDevicePointer((void **) &yd, yo, 0));
        HdmSmallCheckArgs a = {};
        a.n = c.n; a.n16 = n16; a.m = c.m; a.A = dA; a.astride = (long) n2; a.C = dC; a.y = yd; a.tau = c.tau; a.eye = c.eye;
        a.Sout = dS; a.L = L; a.W = W; a.out = yd + c.m;
        if (hdm_small_check(a, s)) { fprintf(stderr, "n %d m %d: the launcher refused\n", c.n, c.m); return 1; }
        CK(hipStreamSynchronize(s));
        CK(hipMemcpy(S.data(), dS, sizeof(double) * n2, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hL.data(), L, sizeof(double) * pp, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hW.data(), W, sizeof(double) * pp, hipMemcpyDeviceToHost));
        const double rep[2] = {yo[c.m], yo[c.m + 1]};
        fwrite(S.data(), sizeof(double), n2, f); fwrite(hL.data(), sizeof(double), pp, f); fwrite(hW.data(), sizeof(double), pp, f);
        fwrite(rep, sizeof(double), 2, f);
        printf("n %3d n16 %3d m %4d tau %.2f eye %+.2f: info %3d logdet %.17g\n", c.n, n16, c.m, c.tau, c.eye, (int) rep[0], rep[1]);
        CK(hipFree(dA)); CK(hipFree(dC)); CK(hipFree(dS)); CK(hipHostFree(yo));
    }
    fclose(f);
    CK(hipFree(L)); CK(hipFree(W));
    CK(hipStreamDestroy(s));
    return 0;
}
