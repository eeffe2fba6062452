// Host driver of tests/test_gemm_layouts_cpu.py: the indices of the three storage formats as the engine's headers state them,
// written to stdout as raw int64 values.  argv: n16 world maxloc kstep.
//   [0]                      hdm_sky_size(n16)
//   n16 * n16                hdm_sky_off(i, j, n16) in row-major (i, j) order, -1 where i < 128 * (j / 128)
//   nblk * nblk              hdm_blk_sub(bi, bj, nblk), -1 above the diagonal
//   npb * 4                  hdm_pblock_decode(q, nblk): sub, bi, bj, col
//   7                        the layout: n16 nblk npb npb_loc Lr R astride
//   R * npb_loc * (k % 16 in 0, kstep, ..)   the Gram operand's element offset as SStager<true>::init (gemm_tile.h) adds it up
//                            from the fields hdm_gram_splits fills: tile row x0 = 128 (i / 128), lane row i - x0
#include "gemm_calls.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const int n16 = atoi(argv[1]), world = atoi(argv[2]), maxloc = atoi(argv[3]), kstep = atoi(argv[4]);
    std::vector<int64_t> out;
    out.push_back(hdm_sky_size(n16));
    for (int i = 0; i < n16; ++i)
        for (int j = 0; j < n16; ++j) out.push_back(i >= 128 * (j / 128) ? hdm_sky_off(i, j, n16) : -1);
    const HdmLayout L = hdm_layout(n16, world, maxloc);
    for (int bi = 0; bi < L.nblk; ++bi)
        for (int bj = 0; bj < L.nblk; ++bj) out.push_back(bi >= bj ? hdm_blk_sub(bi, bj, L.nblk) : -1);
    for (long q = 0; q < L.npb; ++q) {
        const HdmPBlock p = hdm_pblock_decode(q, L.nblk);
        out.push_back(p.sub); out.push_back(p.bi); out.push_back(p.bj); out.push_back(p.col);
    }
    const int64_t lay[7] = {L.n16, L.nblk, L.npb, L.npb_loc, L.Lr, L.R, L.astride};
    out.insert(out.end(), lay, lay + 7);
    const HdmGemmArgs a = hdm_gram_splits(L, n16, maxloc, 1, 0, 1, nullptr, nullptr, false, true);
    for (long i = 0; i < L.R; ++i) {
        const long x0 = i / HDM_TILE * HDM_TILE;
        const long segoff = a.seg_rows ? (x0 / a.seg_rows) * a.seg_extra : 0;
        for (long kt = 0; kt < L.npb_loc; ++kt)
            for (int k = 0; k < 16; k += kstep) out.push_back(segoff + kt * a.a_kblk + (x0 + (i - x0)) * a.lda + k);
    }
    return fwrite(out.data(), sizeof(int64_t), out.size(), stdout) == out.size() ? 0 : 1;
}
