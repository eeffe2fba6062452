// driver of tests/test_gemm_geom_cpu.py: csrc/gemm_geom.h compiled alone with the host compiler.  Reads one command per line from
// stdin and prints one line per query; fractions travel as C hex floats, so nothing is rounded on the way.
//   GEOM M N K klimit lower_only colmask role slab batch k_base k_chunk npass      the launch the next queries are about
//   LIST subset                 -> tm tn tm tn ...            (launch order)
//   LAUNCH subset               -> MFMA instructions of the launch's tiles (one batch entry; split-K: all splits)
//   TILE tm tn z                -> selected kbeg kend kind rv RV mfmas
//   NEED kmajor ld kblk stride rows seg_rows seg_extra sky    -> elements the operand's unmasked loads reach
//   RULES x                     -> hdm_ntiles(x) hdm_cell_rows(x) weight(NONE) weight(BY_M) weight(BY_N) weight(BAND) of tile (x, 1)
//   MASK mask NT                -> the mask the launch honours
//   TABLES                      -> MFMAs of the four triangular K blocks (step 2 last, P + P^T last, step 1 first, step 1 last), of a full one
//   DIAGSHARE M N mask | MASKSHARE NT mask                    -> the share
//   BLK nblk                    -> for every bj <= bi < nblk: sub col_of(sub); then one line "start(0) .. start(nblk - 1)"
//   PBLOCK q nblk               -> sub bi bj col
#include "gemm_geom.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

static_assert(hdm_block_mfmas(HDM_LIVE_CONG2_LAST) == 1280 && HDM_KBLOCK_MFMAS == 2048, "usable in constant expressions");

int main() {
    HdmTileGeom g = {};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        if (!(in >> cmd)) continue;
        std::vector<unsigned long long> v;
        while (in >> tok) v.push_back(strtoull(tok.c_str(), nullptr, 10));
        if (cmd == "GEOM") {
            g = {(int) v.at(0), (int) v.at(1), (int) v.at(2), (int) v.at(3), (int) v.at(4), v.at(5), (int) v.at(6), (int) v.at(7), (int) v.at(8),
                 (long) v.at(9), (long) v.at(10), (int) v.at(11)};
            continue;
        }
        if (cmd == "LIST") {
            for (const HdmTile &t : hdm_tile_list(g, (int) v.at(0))) printf("%d %d ", t.tm, t.tn);
        } else if (cmd == "LAUNCH") {
            printf("%ld", hdm_launch_mfmas(g, (int) v.at(0)));
        } else if (cmd == "TILE") {
            const int tm = (int) v.at(0), tn = (int) v.at(1), z = (int) v.at(2);
            const HdmKRange r = hdm_tile_krange(g, tm, tn, z);
            const HdmTileClass c = hdm_tile_class(g, tm, tn);
            printf("%d %ld %ld %d %d %d %ld", (int) hdm_tile_selected(g, tm, tn), r.kbeg, r.kend, (int) c.kind, c.rv, c.RV, hdm_tile_mfmas(g, tm, tn, z));
        } else if (cmd == "NEED") {
            printf("%ld", hdm_operand_need(g, v.at(0) != 0, (long) v.at(1), (long) v.at(2), (long) v.at(3), (int) v.at(4), (long) v.at(5),
                                           (long) v.at(6), v.at(7) != 0));
        } else if (cmd == "RULES") {
            const int x = (int) v.at(0);
            printf("%d %d %ld %ld %ld %ld", hdm_ntiles(x), hdm_cell_rows(x), hdm_tile_weight(HDM_KLIM_NONE, x, 1), hdm_tile_weight(HDM_KLIM_BY_M, x, 1),
                   hdm_tile_weight(HDM_KLIM_BY_N, x, 1), hdm_tile_weight(HDM_KLIM_BAND, x, 1));
        } else if (cmd == "MASK") {
            printf("%llu", hdm_colmask_effective(v.at(0), (int) v.at(1)));
        } else if (cmd == "TABLES") {
            printf("%ld %ld %ld %ld %ld", hdm_block_mfmas(HDM_LIVE_CONG2_LAST), hdm_block_mfmas(HDM_LIVE_CONG2D_LAST),
                   hdm_block_mfmas(HDM_LIVE_CONG1_FIRST), hdm_block_mfmas(HDM_LIVE_CONG1_LAST), HDM_KBLOCK_MFMAS);
        } else if (cmd == "DIAGSHARE") {
            printf("%a", hdm_cong2_diag_share((int) v.at(0), (int) v.at(1), v.at(2)));
        } else if (cmd == "MASKSHARE") {
            printf("%a", hdm_cong2_mask_share((int) v.at(0), v.at(1)));
        } else if (cmd == "BLK") {
            const int nblk = (int) v.at(0);
            for (int bj = 0; bj < nblk; ++bj)
                for (int bi = bj; bi < nblk; ++bi) printf("%ld %d ", hdm_blk_sub(bi, bj, nblk), hdm_blk_col_of(hdm_blk_sub(bi, bj, nblk), nblk));
            printf("\n");
            for (int bj = 0; bj < nblk; ++bj) printf("%ld ", hdm_blk_col_start(bj, nblk));
        } else if (cmd == "PBLOCK") {
            const HdmPBlock p = hdm_pblock_decode((long) v.at(0), (int) v.at(1));
            printf("%ld %d %d %ld", p.sub, p.bi, p.bj, p.col);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        printf("\n");
    }
    return 0;
}
