// grouped_plan.h -- the plan of the grouped Schur build: which SDP cones of an operator are built together
// in a fixed number of launches, how their rows are cut into jobs, and who contributes to which entry of M and of the m-vectors.
// Pure host arithmetic on integers: no HIP call, no engine state, no I/O -- HKKTInit keeps what this header says in the
// operator's private state (engine_grouped.h), the kernels of small.hip read it from the device, and HMiGroupedPlanQuery hands
// the same numbers to callers without a device.
#pragma once
#include "gemm_geom.h"
#include <algorithm>
#include <cstdint>
#include <vector>

// ---- the rule ---------------------------------------------------------------------------------
#define HDM_GROUPED_MAX_N 64              /* block dimension: four n16 x n16 images of a job fit 160 KB of LDS */
#define HDM_GROUPED_MAX_DATA (1L << 19)   /* mloc * n16 * n16: cone_small_check's bound for n16 <= 64 */
#define HDM_GROUPED_JOB_ROWS 8            /* owned rows per job (one workgroup) */
#define HDM_GROUPED_MIN_CONES 2           /* fewer eligible cones: the per-cone slots, as without the switch */

// One cone of the operator as the rule sees it.  `kind_ok`: an engine SDP cone on one device (world == 1), not synthetic, not
// streamed, its A_L forms resident -- what only the engine can say; the dimension and data bounds are checked here.
// rows: global constraint numbers of the owned rows in the cone's LOCAL order (distinct; ascending unless it has direct rows).
struct HdmGroupedCone {
    int n = 0, mloc = 0;
    const int *rows = nullptr;
    bool kind_ok = false;
};
static inline int hdm_grouped_n16(int n) { return (n + 15) / 16 * 16; }
static inline bool hdm_grouped_eligible(const HdmGroupedCone &c) {
    if (!c.kind_ok || c.n < 1 || c.n > HDM_GROUPED_MAX_N || c.mloc < 0) return false;
    const long n16 = hdm_grouped_n16(c.n);
    return (long) c.mloc * n16 * n16 <= HDM_GROUPED_MAX_DATA;
}

// ---- the plan ---------------------------------------------------------------------------------
struct HdmGroupedJob { int slot, q0, q1, first; };   // grouped cone (slot), its local rows [q0, q1), 1: the cone's first job (scalars)

// local lower Gram of a cone with mloc rows, packed by columns: entry (p, q), p >= q (LOCAL rows)
HDM_HD inline long hdm_grouped_gidx(int p, int q, int mloc) { return (long) q * mloc - (long) q * (q - 1) / 2 + (p - q); }
static inline long hdm_grouped_gsize(int mloc) { return (long) mloc * (mloc + 1) / 2; }

struct HdmGroupedPlan {
    std::vector<int> cones;       // the grouped cones (positions in the operator's cones[]), ascending; empty: the pass is not used
    std::vector<int> slot_of;     // per cone of the operator: its slot, or -1
    std::vector<HdmGroupedJob> jobs;
    // staging: per slot, offsets (in doubles) of X = S^-1 (n16 x n16), the packed local Gram, the local vectors (3 x mloc, then 4 scalars)
    std::vector<long> xoff, goff, voff;
    long x_doubles = 0, g_doubles = 0, v_doubles = 0;
    // contributor lists, CSR: destination e of M is (m_row[e], m_col[e]), row >= col, its contributors m_slot / m_idx[m_ptr[e] ..
    // m_ptr[e + 1]) -- slot and packed local Gram index -- in ascending cone order; destination r of the vectors is row v_row[r],
    // its contributors v_slot / v_idx (local row), in ascending cone order.  Destinations ascend column by column / row by row.
    std::vector<int> m_row, m_col, m_slot, m_idx, v_row, v_slot, v_idx;
    std::vector<long> m_ptr, v_ptr;
    bool used() const { return !cones.empty(); }
};

static inline HdmGroupedPlan hdm_grouped_plan(int nRow, const std::vector<HdmGroupedCone> &cs) {
    HdmGroupedPlan p;
    p.slot_of.assign(cs.size(), -1);
    p.m_ptr.assign(1, 0L);
    p.v_ptr.assign(1, 0L);
    std::vector<int> el;
    for (size_t k = 0; k < cs.size(); ++k)
        if (hdm_grouped_eligible(cs[k])) el.push_back((int) k);
    if ((int) el.size() < HDM_GROUPED_MIN_CONES) return p;
    p.cones = el;
    struct Contrib { int64_t key; int slot, idx; };
    std::vector<Contrib> mc, vc;
    for (size_t s = 0; s < el.size(); ++s) {
        const HdmGroupedCone &c = cs[(size_t) el[s]];
        const long n16 = hdm_grouped_n16(c.n);
        p.slot_of[(size_t) el[s]] = (int) s;
        p.xoff.push_back(p.x_doubles); p.x_doubles += n16 * n16;
        p.goff.push_back(p.g_doubles); p.g_doubles += std::max(1L, hdm_grouped_gsize(c.mloc));
        p.voff.push_back(p.v_doubles); p.v_doubles += 3L * c.mloc + 4;
        // a cone that no constraint touches still has one job: the objective's scalars
        for (int q0 = 0, first = 1; first || q0 < c.mloc; q0 += HDM_GROUPED_JOB_ROWS, first = 0)
            p.jobs.push_back({(int) s, q0, std::min(c.mloc, q0 + HDM_GROUPED_JOB_ROWS), first});
        for (int q = 0; q < c.mloc; ++q) {
            vc.push_back({(int64_t) c.rows[q], (int) s, q});
            for (int pp = q; pp < c.mloc; ++pp) {
                const int r = std::max(c.rows[pp], c.rows[q]), col = std::min(c.rows[pp], c.rows[q]);
                mc.push_back({(int64_t) col * nRow + r, (int) s, (int) hdm_grouped_gidx(pp, q, c.mloc)});
            }
        }
    }
    // stable: contributors of one destination stay in the order they were listed, which is ascending cone order
    auto by_key = [](const Contrib &a, const Contrib &b) { return a.key < b.key; };
    std::stable_sort(mc.begin(), mc.end(), by_key);
    std::stable_sort(vc.begin(), vc.end(), by_key);
    for (size_t e = 0; e < mc.size(); ++e) {
        if (e == 0 || mc[e].key != mc[e - 1].key) {
            if (e) p.m_ptr.push_back((long) e);
            p.m_row.push_back((int) (mc[e].key % nRow)); p.m_col.push_back((int) (mc[e].key / nRow));
        }
        p.m_slot.push_back(mc[e].slot); p.m_idx.push_back(mc[e].idx);
    }
    if (!mc.empty()) p.m_ptr.push_back((long) mc.size());
    for (size_t e = 0; e < vc.size(); ++e) {
        if (e == 0 || vc[e].key != vc[e - 1].key) {
            if (e) p.v_ptr.push_back((long) e);
            p.v_row.push_back((int) vc[e].key);
        }
        p.v_slot.push_back(vc[e].slot); p.v_idx.push_back(vc[e].idx);
    }
    if (!vc.empty()) p.v_ptr.push_back((long) vc.size());
    return p;
}
