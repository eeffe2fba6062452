// direct_rows.h -- low-rank rows of a block on the congruence + Gram path, written into the transformed-row buffer without
// the congruence: which rows qualify, in what order the block's rows then stand, the terms a row is
// the sum of, the value of a transformed row at one matrix position, and when the form is on.
//   A = sigma a a'                        ->  L^-1 A L^-T = sigma u u',  u = L^-1 a
//   A = sum_e v_e (e_p e_q' + e_q e_p')   ->  L^-1 A L^-T = sum_e v_e (w_p w_q' + w_q w_p'),  w_p = column p of L^-1
// Pure arithmetic: no HIP header, no allocation on the device, no environment.  Under hipcc the term formula is
// __host__ __device__ (the writer kernel, schur.hip, sums with it); tests/test_direct_rows_cpu.py compiles this header alone
// with the host compiler.
#pragma once
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define HDM_DR_HD __host__ __device__ __attribute__((always_inline))
#else
#define HDM_DR_HD
#endif

// (the classes of coeff.h: MiCoeffType, restated so that this header stands alone; engine.hip holds the two to each other)
enum { HDM_DR_ZERO = 0, HDM_DR_SPARSE = 1, HDM_DR_DENSE = 2, HDM_DR_SPR1 = 3, HDM_DR_DSR1 = 4 };
enum { HDM_DR_PATH_GEMM = 0 };

// ---- the cutoffs (measured: profiles/direct_rows_timing.jsonl, tools/direct_rows_timing.py) ---------------------------
// kmax(n16): the largest measured term count k whose per-row writer time is at most HALF the congruence's per-row time at that
// size; between the measured sizes the smaller neighbour's figure holds.  The floor: the smallest measured n at which the build of
// the mixed case is not slower with the form than without by more than the run-to-run spread (at 128 the two tie to 0.3 %).
constexpr int HDM_DR_MIN_N = 256;
constexpr long HDM_DR_TABLE_BYTES = 1L << 30;   // the term table stops growing here: later rows stay congruence rows
HDM_DR_HD constexpr int hdm_direct_kmax(int n16) { return n16 >= 2000 ? 64 : 32; }   // measured: 32 at 256 and 1024, 64 at 2000

// ---- when the form is on ----------------------------------------------------------------------------------------------
// sw: HDSDP_MI355X_DIRECT_ROWS as read at cone creation -- negative: unset; 0: off; k > 0: on whatever the size, kmax = k.
struct HdmDirectRule { bool on; int kmax; };
HDM_DR_HD constexpr HdmDirectRule hdm_direct_rule(int world, bool synthetic, bool streamed, int natural_path, bool force_gemm,
                                                  bool force_path, int n, int n16, int sw) {
    if (world != 1 || synthetic || streamed || natural_path != HDM_DR_PATH_GEMM || force_gemm || force_path || sw == 0)
        return {false, 0};
    if (sw > 0) return {true, sw};
    if (n < HDM_DR_MIN_N) return {false, 0};
    return {true, hdm_direct_kmax(n16)};
}

// ---- the terms ----------------------------------------------------------------------------------------------------------
// The value of a term at (r, s) is c (x_r y_s + y_r x_s).  x, y >= 0: columns x, y of L^-1; x = y = -1 - j: column j of
// U = L^-1 [a_j], the transformed factors of the block's rank-one direct rows.
//   off-diagonal entry (p, q), value v:  c = v,        x = w_p, y = w_q
//   diagonal entry (p, p), value v:      c = v / 2,    x = y = w_p
//   rank-one row sigma a a':             c = sigma / 2, x = y = u
struct HdmDirectTerm { double c; int x, y; };
static_assert(sizeof(HdmDirectTerm) == 16, "the term table's 1 GiB cap counts 16 bytes per term");

// packed index of the lower triangle, column by column (coeff.h) -> (row, column)
inline void hdm_packed_decode(long pk, int n, int *row, int *col) {
    int j = 0;
    long start = 0;
    while (pk >= start + (n - j)) { start += n - j; ++j; }
    *col = j;
    *row = j + (int) (pk - start);
}
HDM_DR_HD constexpr bool hdm_direct_is_r1(int type) { return type == HDM_DR_SPR1 || type == HDM_DR_DSR1; }
// terms the row would take (0: a congruence row whatever kmax is)
HDM_DR_HD constexpr long hdm_direct_nterms(int type, long stored, int kmax) {
    return hdm_direct_is_r1(type) ? 1 : (type == HDM_DR_SPARSE && stored >= 1 && stored <= kmax) ? stored : 0;
}
// the terms of one row, appended in ascending order of packed index (idx is sorted: coeff.h); r1_slot: the row's column of U
inline void hdm_direct_terms(int type, int n, const std::vector<int> &idx, const std::vector<double> &val, double sign, int r1_slot,
                             std::vector<HdmDirectTerm> &out) {
    if (hdm_direct_is_r1(type)) { out.push_back({0.5 * sign, -1 - r1_slot, -1 - r1_slot}); return; }
    for (size_t e = 0; e < idx.size(); ++e) {
        int p = 0, q = 0;
        hdm_packed_decode(idx[e], n, &p, &q);
        if (p == q) out.push_back({0.5 * val[e], p, p});
        else out.push_back({val[e], p, q});
    }
}

// entry i of a term's vector: column v of Linv (leading dimension ldl), or column -1 - v of U (leading dimension ldu)
HDM_DR_HD inline double hdm_direct_vec(int v, long i, const double *Linv, long ldl, const double *U, long ldu) {
    return v >= 0 ? Linv[i + (long) v * ldl] : U[i + (long) (-1 - v) * ldu];
}
// One multiply-add form, the same wherever a row is summed (host reference, writer kernel): acc + c (x_r y_s + y_r x_s) as two
// fused multiply-adds around one product, so that two builds -- and the host and the device -- round alike.
HDM_DR_HD inline double hdm_direct_fma(double acc, double c, double xr, double ys, double yr, double xs) {
    return __builtin_fma(c, __builtin_fma(xr, ys, yr * xs), acc);
}
// the transformed row at matrix position (i, j): its terms in table order
HDM_DR_HD inline double hdm_direct_value(const HdmDirectTerm *t, long nt, const double *Linv, long ldl, const double *U, long ldu,
                                         long i, long j) {
    double acc = 0.0;
    for (long e = 0; e < nt; ++e)
        acc = hdm_direct_fma(acc, t[e].c, hdm_direct_vec(t[e].x, i, Linv, ldl, U, ldu), hdm_direct_vec(t[e].y, j, Linv, ldl, U, ldu),
                             hdm_direct_vec(t[e].y, i, Linv, ldl, U, ldu), hdm_direct_vec(t[e].x, j, Linv, ldl, U, ldu));
    return acc;
}

// ---- the partition and the row order --------------------------------------------------------------------------------------
// rows: the block's constraints in ascending global order, class and stored entries each (zero rows are skipped: one GPU leaves
// them out of the device data).  order: congruence rows first, ascending, then direct rows, ascending.  A row whose terms would
// take the table past `table_bytes` stays a congruence row (the row, not the block).
struct HdmDirectPlan {
    std::vector<int> order;       // global rows in local order
    int nCongruence = 0, nDirect = 0, nRankOne = 0;
    long nterms = 0;
};
inline HdmDirectPlan hdm_direct_partition(const std::vector<int> &type, const std::vector<long> &stored, HdmDirectRule rule,
                                          long table_bytes = HDM_DR_TABLE_BYTES) {
    HdmDirectPlan p;
    std::vector<int> direct;
    for (size_t i = 0; i < type.size(); ++i) {
        if (type[i] == HDM_DR_ZERO) continue;
        const long k = rule.on ? hdm_direct_nterms(type[i], stored[i], rule.kmax) : 0;
        if (k > 0 && (p.nterms + k) * (long) sizeof(HdmDirectTerm) <= table_bytes) {
            direct.push_back((int) i);
            p.nterms += k;
            p.nRankOne += hdm_direct_is_r1(type[i]) ? 1 : 0;
        } else p.order.push_back((int) i);
    }
    p.nCongruence = (int) p.order.size();
    p.nDirect = (int) direct.size();
    p.order.insert(p.order.end(), direct.begin(), direct.end());
    return p;
}
