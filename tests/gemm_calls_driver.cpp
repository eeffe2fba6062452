// Driver of tests/test_gemm_calls_cpu.py: csrc/gemm_calls.h alone, with the host compiler.  One request per line of stdin; every
// form's answer is one line: the fields of its HdmGemmArgs in the struct's order (pointers as integers, doubles as hex floats),
// then, for each of the operands A, B, A2, B2, how far the launch's unmasked tile loads reach (gemm_geom.h: hdm_operand_need, as
// the launcher asks it; -1 for an operand that is absent) and whether the launcher's argument checks pass.
#include "gemm_calls.h"
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

// the operands live at fixed made-up addresses: only their differences are looked at
static const double *LINV = (const double *) (uintptr_t) 0x10000000ULL;
static const double *ASRC = (const double *) (uintptr_t) 0x20000000000ULL;
static double *TBUF = (double *) (uintptr_t) 0x40000000000ULL;
static double *DST = (double *) (uintptr_t) 0x60000000000ULL;
static double *SLAB = (double *) (uintptr_t) 0x80000000000ULL;

// the launcher's adapter and checks (gemm_f64.hip: tile_geom, hdm_launch_gemm), restated on gemm_geom.h's functions
static HdmTileGeom tile_geom(const HdmGemmArgs &a) {
    return {a.M, a.N, a.K, a.klimit, a.lower_only, a.tile_col_mask, a.role, a.epilogue == HDM_EPI_SLAB, a.batch, a.k_base, a.k_chunk,
            ((a.role == HDM_ROLE_CONG2 || a.role == HDM_ROLE_GENERIC) && a.A2) ? 2 : 1};
}
static int launcher_accepts(const HdmGemmArgs &a) {
    if ((a.M % 8) || (a.N % 8) || (a.K % HDM_BK)) return 0;
    if (a.epilogue == HDM_EPI_SLAB && (a.k_chunk <= 0 || a.k_chunk % HDM_BK)) return 0;
    if (a.role == HDM_ROLE_CONG2) {
        const bool mirrored = a.A2 == a.B && a.B2 == a.A && a.lda2 == a.ldb && a.ldb2 == a.lda && a.strideA2 == a.strideB && a.strideB2 == a.strideA;
        if (!mirrored || !a.lower_only || a.epilogue != HDM_EPI_BLOCKED || a.klimit != HDM_KLIM_BY_N || a.M != a.N || a.a_kmajor || a.b_kmajor) return 0;
    }
    if (a.role != HDM_ROLE_GENERIC) {
        const long lds[4] = {a.lda, a.ldb, a.A2 ? a.lda2 : 0, a.B2 ? a.ldb2 : 0};
        for (long ld : lds) if (ld < 0 || ld > (1L << 20)) return 0;
    }
    return 1;
}
static void dump(const HdmGemmArgs &a) {
    auto p = [](const void *q) { return (unsigned long long) (uintptr_t) q; };
    printf("%llu %llu %llu %llu %llu %ld %ld %ld %ld %d %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %d %d %d %d %d %ld %ld %ld %ld %d %d %llu %d %d %d %a %a %d %a "
           "%ld %ld %d %ld %ld %ld",
           p(a.A), p(a.B), p(a.C), p(a.A2), p(a.B2), a.lda2, a.ldb2, a.strideA2, a.strideB2, a.b_sky, a.spanA, a.spanB, a.spanA2, a.spanB2, a.lda,
           a.ldb, a.ldc, a.strideA, a.strideB, a.strideC, a.M, a.N, a.K, a.a_kmajor, a.b_kmajor, a.a_kblk, a.b_kblk, a.seg_rows, a.seg_extra, a.klimit,
           a.lower_only, a.tile_col_mask, a.epilogue, a.batch, a.queue_global, a.alpha, a.beta, a.role, a.flops, a.blk_row_stride, a.blk_row0, a.nblk,
           a.k_chunk, a.k_base, a.slab_stride);
    const HdmTileGeom gm = tile_geom(a);
    struct { const double *q; bool km; long ld, kblk, stride; int rows; } ops[4] = {
        {a.A, a.a_kmajor != 0, a.lda, a.a_kblk, a.strideA, a.M}, {a.B, a.b_kmajor != 0, a.ldb, a.b_kblk, a.strideB, a.N},
        {a.A2, a.a_kmajor != 0, a.lda2, (long) HDM_BK, a.strideA2, a.M}, {a.B2, a.b_kmajor != 0, a.ldb2, (long) HDM_BK, a.strideB2, a.N}};
    for (auto &o : ops)
        printf(" %ld", o.q ? hdm_operand_need(gm, o.km, o.ld, o.kblk, o.stride, o.rows, a.seg_rows, a.seg_extra, o.q == a.B && a.b_sky) : -1L);
    printf(" %d\n", launcher_accepts(a));
}

int main() {
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> cmd;
        int n = 0, world = 1, m = 0;
        in >> n >> world >> m;
        const HdmLayout L = hdm_layout(n, world, (m + world - 1) / world);
        if (cmd == "LAYOUT") {
            const HdmWorkPlan p = hdm_work_plan(L, hdm_rows_of_rank(m, world, 0), false, 0, HdmKnobs());
            printf("%d %d %ld %ld %d %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", L.n16, L.nblk, L.npb, L.npb_loc, L.Lr, L.R, L.astride, p.Bc, p.nsplit,
                   (long) hdm_exchange_doubles(L), (long) (hdm_operand_pad(L.n16) / 8), (long) HDM_OPERAND_PAD_DOUBLES, hdm_rows_of_rank(m, world, 0), p.nslab);
        } else if (cmd == "STEP1") {
            long ldl, src_rows, b0; int nb;
            in >> ldl >> src_rows >> b0 >> nb;
            dump(hdm_cong_step1(L, n, LINV, ldl, ASRC, src_rows, b0, nb, TBUF));
        } else if (cmd == "STEP2") {
            long Bc, ldl, row0; int nb; unsigned long long mask;
            in >> Bc >> ldl >> nb >> row0 >> mask;
            dump(hdm_cong_step2(L, n, Bc, LINV, ldl, TBUF, nb, DST, row0, mask));
        } else if (cmd == "IROW") {
            long ldl, row0;
            in >> ldl >> row0;
            dump(hdm_cong_irow(L, LINV, ldl, DST, row0));
        } else if (cmd == "GRAM") {
            long nsplit; int z0, nz, acc, qg;
            in >> nsplit >> z0 >> nz >> acc >> qg;
            dump(hdm_gram_splits(L, n, m, nsplit, z0, nz, DST, SLAB, acc != 0, qg != 0));
        } else if (cmd == "GATHERED") {
            long nc, span; int nz, acc; double alpha;
            in >> nc >> nz >> alpha >> acc >> span;
            dump(hdm_gram_gathered(L.R, nc, hdm_roundup(nc, 16), nz, alpha, acc != 0, ASRC, span, SLAB, true));
        } else if (cmd == "LP") {   // n: columns of the LP cone, m: its rows
            int kc, kv, mpad; long ldm;
            in >> mpad >> kc >> kv >> ldm;
            dump(hdm_gram_lp(m, (int) hdm_roundup(m, 16), mpad, kc, kv, (int) hdm_roundup(kv, 16), ASRC, SLAB, ldm));
        } else if (cmd == "PLAIN") {
            int M, N, K, ak, bk, klimit, lower, batch; long lda, ldb, ldc, sa, sb, sc; double alpha, beta;
            in >> M >> N >> K >> alpha >> beta >> lda >> ak >> sa >> ldb >> bk >> sb >> ldc >> klimit >> lower >> batch >> sc;
            dump(hdm_gemm_product(DST, ldc, M, N, K, alpha, hdm_operand(LINV, lda, ak, sa), hdm_operand(ASRC, ldb, bk, sb), beta,
                                  hdm_klimit(klimit).lower(lower).batched(batch, sc)));
        } else if (cmd == "CHUNK") {
            long nsplit;
            in >> nsplit;
            printf("%ld\n", hdm_gram_chunk(L, nsplit));
        } else if (cmd == "PIECE") {
            long nsplit, lo, hi; int k, P;
            in >> nsplit >> k >> P;
            hdm_piece_range(L, nsplit, k, P, &lo, &hi);
            printf("%ld %ld\n", lo, hi);
        } else {
            return 2;
        }
    }
    return 0;
}
