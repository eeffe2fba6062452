// small_check_rule.h -- which blocks the one-launch interior check (small.hip: hdm_small_check_kernel) answers, as one rule.
// Pure host arithmetic: no HIP call, no engine state.  cone_small_check (engine_cone.h) asks it per call, the check set of an
// operator (engine_check_set.h) asks it per cone at HKKTInit: a cone is a member of a set exactly when its own one-launch check
// would have run.  tests/test_small_check_rule_cpu.py compiles this header alone.
//
// A single workgroup walks the block's resident constraint data: up to 1 MB of it in general (mloc n16^2 <= 2^17 doubles), 4 MB
// (2^19) for blocks of dimension <= 64, where the call-by-call assembly's few workgroups are latency-bound themselves (theta1:
// 0.45 ms per check).  The factor object must be one 128-block, whose Dinv is the triangular inverse the kernel writes.
#pragma once
#include <cstddef>

constexpr int HDM_SMALL_CHECK_P = 128;                      // padded dimension of the register sweep (small.h: SMALL_P)
constexpr long HDM_SMALL_CHECK_DATA_LOW = 1L << 19;         // doubles of resident constraint data, n16 <= 64
constexpr long HDM_SMALL_CHECK_DATA_HIGH = 1L << 17;        // ... 64 < n16 <= 128
constexpr int HDM_SMALL_CHECK_ROWS_MAX = 4096;              // the launcher's bound on the rows of one block
constexpr long HDM_SMALL_CHECK_LDS_MAX = 160L * 1024;       // dynamic LDS a workgroup may ask for (gfx950: 160 KB per CU)

// dynamic LDS of a check of a block with m resident rows: S as 128 x 129, 128 deferred scale factors, the multipliers
static inline long hdm_small_check_lds_bytes(long m) {
    return (long) sizeof(double) * ((long) HDM_SMALL_CHECK_P * (HDM_SMALL_CHECK_P + 1) + HDM_SMALL_CHECK_P + (m > 1 ? m : 1));
}

struct HdmSmallCheckCone {
    bool on = true;            // HDSDP_MI355X_SMALL_CHECK
    int world = 1;             // ranks the block's rows are dealt over
    bool resident = false;     // the A_L forms of the owned rows are in device memory
    int n16 = 0;               // block dimension rounded up to 16
    long mloc = 0;             // rows owned
    int fac_npad = 0, fac_nblk = 0;   // the factor object the launch would write (HdmChol::npad, ::nblk)
};

// the block's own part: everything but the factor object (which depends on the buffer asked for)
static inline bool hdm_small_check_block_ok(const HdmSmallCheckCone &c) {
    if (!c.on || c.world != 1 || !c.resident || c.n16 > HDM_SMALL_CHECK_P) return false;
    const long doubles = c.mloc * c.n16 * c.n16;
    if (doubles > ((c.n16 <= 64) ? HDM_SMALL_CHECK_DATA_LOW : HDM_SMALL_CHECK_DATA_HIGH)) return false;
    return c.mloc <= HDM_SMALL_CHECK_ROWS_MAX && hdm_small_check_lds_bytes(c.mloc) <= HDM_SMALL_CHECK_LDS_MAX;
}
static inline bool hdm_small_check_factor_ok(int npad, int nblk) { return npad == HDM_SMALL_CHECK_P && nblk == 1; }

static inline bool hdm_small_check_eligible(const HdmSmallCheckCone &c) {
    return hdm_small_check_block_ok(c) && hdm_small_check_factor_ok(c.fac_npad, c.fac_nblk);
}
