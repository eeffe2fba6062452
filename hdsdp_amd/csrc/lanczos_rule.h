// lanczos_rule.h -- the rules of the ratio test (lanczos.hip), stated once for the host driver (lanczos_host.h), the one-launch
// kernel and the launcher: the constants of HLanczosSolve (linalg/hdsdp_lanczos.c:161-292), when a Ritz check is due, how
// many steps lie before the next one, the acceptance rule, the layout of the host/device mailbox, and which of the forms runs.
// Pure arithmetic: no HIP header, no allocation.  Under hipcc the predicates and the acceptance rule are __host__ __device__;
// the switches are host only.  tests/test_lanczos_rule_cpu.py compiles this header alone with the host compiler.
#pragma once
#include "env_switches.h"
#include <cmath>
#include <cstdlib>

#if defined(__HIPCC__)
#define HDM_LZ_HD __host__ __device__ __attribute__((always_inline))
#else
#define HDM_LZ_HD
#endif

// ---- constants ------------------------------------------------------------------------------
constexpr int LZ_MD = 30;                  // Krylov dimension (hdsdp_conic_sdp.c:1393)
constexpr int LZ_CHECK_FREQ = (LZ_MD / 5 > 3) ? 3 : LZ_MD / 5;   // a Ritz check every third step (hdsdp_lanczos.c:187-189)
static_assert(LZ_CHECK_FREQ >= 1, "the check frequency is md / 5: the Krylov dimension is 5 at least");
constexpr double LZ_WARM_WEIGHT = 1e-03;   // warm start = previous Ritz image + this x the pseudo-random vector (:166-181)
constexpr double LZ_RESID_TOL = 1e-04;     // |beta_k y1[k]| below this: the two residuals are taken (:247)
constexpr double LZ_GAP_FLOOR = 1e-16;     // gamma's denominator when eig1 - eig2 - r2 <= 0 (:268)
constexpr double LZ_ACCEPT_GAM = 1e-03;    // accepted if gamma < this ...
constexpr double LZ_ACCEPT_SUM = 0.5;      // ... or gamma + eig1 <= this (:272)
constexpr int LZ_FUSED_MAX = 256;          // n16 up to which a single workgroup runs whole steps (vectors in LDS)
constexpr int LZ_RESIDENT_MAX = 128;       // n16 up to which both packed triangles fit in LDS beside them
constexpr int LZ_BIG_MAX = 4096;           // n16 up to which the co-resident form runs (16 trips of 256 rows)
constexpr int LZ_BIG_TRIPS8_MAX = 2048;    // 8 trips up to here, 16 above
constexpr int LZG_WG = 256;                // its workgroups: one per CU, this many at most ...
constexpr int LZG_COLS = 16;               // ... each owning this many columns at most
constexpr int LZ_NCHUNK = 32;              // column chunks of the launch-per-product form's last product (summed in chunk order)

// ---- when a check is due, and the steps up to it ----------------------------------------------
// (hdsdp_lanczos.c:221: `k > md - 1` never holds inside the loop -- the reference's clause, kept as it stands)
HDM_LZ_HD inline bool hdm_lz_check_due(int k, double nrm) { return (k + 1) % LZ_CHECK_FREQ == 0 || k > LZ_MD - 1 || nrm == 0.0; }
// steps from step k up to and including the next check (a zero norm ends a group early, as it ends the reference's loop)
HDM_LZ_HD inline int hdm_lz_group_len(int k) {
    const int to_check = LZ_CHECK_FREQ - k % LZ_CHECK_FREQ, left = LZ_MD - k;
    return to_check < left ? to_check : left;
}
// the Ritz pair is looked at closely -- two operator applications -- once its estimate is small, and at the last step (:247)
HDM_LZ_HD inline bool hdm_lz_residuals_due(double resiVal, int k) { return resiVal < LZ_RESID_TOL || k >= LZ_MD - 1; }

// ---- the acceptance rule (hdsdp_lanczos.c:262-284) ------------------------------------------------
// r1 = |Op z1 - eig1 z1|, r2 = |Op z2 - eig1 z2| (eig1 in both, as the reference has it), nrm = the step's norm.
// gamma = min(r1, r1^2 / max(eig1 - eig2 - r2, floor)); the step is 1 / (gamma + eig1), infinite where that is not positive.
enum HdmLzVerdict { LZ_ACCEPTED = 0, LZ_CONTINUE = 1, LZ_FAILED = 2 };   // CONTINUE: `step` is provisional; FAILED: a zero norm without acceptance, no step
struct HdmLzAccept { int verdict; double step; };
HDM_LZ_HD inline HdmLzAccept hdm_lz_accept(double eig1, double eig2, double r1, double r2, double nrm) {
    const double resiDiff = eig1 - eig2 - r2;
    double gam = (resiDiff > 0) ? resiDiff : LZ_GAP_FLOOR;
    const double sq = r1 * r1 / gam;
    gam = r1 < sq ? r1 : sq;
    if (gam < LZ_ACCEPT_GAM || gam + eig1 <= LZ_ACCEPT_SUM) return {LZ_ACCEPTED, (gam + eig1 <= 0.0) ? INFINITY : 1.0 / (gam + eig1)};
    if (nrm == 0.0) return {LZ_FAILED, 0.0};
    return {LZ_CONTINUE, 1.0 / (gam + eig1)};
}

// ---- the mailbox: LZ_MB_SIZE doubles of mapped pinned memory between host and device --------------------
enum HdmLzMailbox {
    LZ_MB_R1 = 2, LZ_MB_R2 = 3,   // the two residual norms
    LZ_MB_Y1 = 8,                 // coefficients of the first Ritz vector, LZ_MD at most
    LZ_MB_CARRY = 43,             // launch-per-product form: the norm carried into a group's first step
    LZ_MB_GROUP = 44,             // a group of g steps: g (alpha, norm) pairs, the number of steps done, the give-up word
    LZ_MB_WHOLE = 60,             // one-launch form: step, Lanczos steps done, status
    LZ_MB_SAFE = 63,              // grouped form: the safeguard's word (0, or the first non-positive pivot + 1), behind the three
    LZ_MB_Y2 = 64,                // coefficients of the second Ritz vector
    LZ_MB_SIZE = 128
};
constexpr int LZ_MB_GROUP_LEN = 2 * LZ_CHECK_FREQ + 2, LZ_MB_WHOLE_LEN = 3;
static_assert(LZ_MB_R1 + 1 <= LZ_MB_R2 && LZ_MB_R2 + 1 <= LZ_MB_Y1 && LZ_MB_Y1 + LZ_MD <= LZ_MB_CARRY && LZ_MB_CARRY + 1 <= LZ_MB_GROUP,
              "mailbox ranges overlap");
static_assert(LZ_MB_GROUP + LZ_MB_GROUP_LEN <= LZ_MB_WHOLE, "a group of steps (the check frequency at most) must fit the mailbox's group block");
static_assert(LZ_MB_WHOLE + LZ_MB_WHOLE_LEN == LZ_MB_SAFE && LZ_MB_SAFE + 1 <= LZ_MB_Y2, "the safeguard's word follows the one-launch form's three");
static_assert(LZ_MB_WHOLE + LZ_MB_WHOLE_LEN <= LZ_MB_Y2 && LZ_MB_Y2 + LZ_MD <= LZ_MB_SIZE, "mailbox ranges overlap");

// ---- which form runs ------------------------------------------------------------------------
// HDM_LANCZOS_WHOLE / _FUSED / _GROUP / _BIG = 0 switch a form off (A/B, tests/test_gpu_switches.py; read time: env_switches.h).
struct HdmLzSwitches { bool whole, fused, group, big; };
static inline const HdmLzSwitches &hdm_lz_switches() {
    static const HdmLzSwitches sw = {hdm_env_on<ENV_LANCZOS_WHOLE>(), hdm_env_on<ENV_LANCZOS_FUSED>(), hdm_env_on<ENV_LANCZOS_GROUP>(),
                                     hdm_env_on<ENV_LANCZOS_BIG>()};
    return sw;
}

enum HdmLzForm {
    LZ_FORM_WHOLE_RESIDENT = 0,   // the whole test in one single-workgroup launch, both matrices packed into LDS
    LZ_FORM_WHOLE_GLOBAL = 1,     // the same, matrices read from global memory
    LZ_FORM_FUSED = 2,            // a group of steps per single-workgroup launch, Ritz checks on the host
    LZ_FORM_GROUP8 = 3,           // a group of steps per launch of co-resident workgroups, 8 trips of 256 rows
    LZ_FORM_GROUP16 = 4,          // the same, 16 trips
    LZ_FORM_QUEUED = 5,           // a launch per product, the steps of a group queued behind one synchronisation
    LZ_FORM_STEPWISE = 6          // a launch per product, one synchronisation per step
};
constexpr int hdm_lz_group_wgs(int cus) { return cus < LZG_WG ? cus : LZG_WG; }
//   n16            | runs                                       | unless
//   <= 128         | WHOLE_RESIDENT                             | WHOLE=0: FUSED; and FUSED=0: QUEUED
//   129 .. 256     | WHOLE_GLOBAL                               | WHOLE=0: FUSED; and FUSED=0: QUEUED
//   257 .. 2048    | GROUP8                                     | BIG=0, a wait of this object ran out (big_ok), the device is
//   2049 .. 4096   | GROUP16                                    |   shared with another engine, no CU count, or more than 16
//                  |                                            |   columns per workgroup (n16 > 16 min(256, cus)): QUEUED
//   > 4096         | QUEUED                                     |
//   and QUEUED is STEPWISE under GROUP=0.  WHOLE and FUSED mean nothing above 256, BIG nothing up to it.
inline HdmLzForm hdm_lz_form(int n16, const HdmLzSwitches &sw, bool big_ok, bool shared_device, int cus) {
    if (n16 <= LZ_FUSED_MAX) {
        if (sw.whole) return n16 <= LZ_RESIDENT_MAX ? LZ_FORM_WHOLE_RESIDENT : LZ_FORM_WHOLE_GLOBAL;
        if (sw.fused) return LZ_FORM_FUSED;
    } else if (sw.big && big_ok && !shared_device && n16 <= LZ_BIG_MAX) {
        const int wg = hdm_lz_group_wgs(cus);
        if (wg > 0 && (n16 + wg - 1) / wg <= LZG_COLS) return n16 <= LZ_BIG_TRIPS8_MAX ? LZ_FORM_GROUP8 : LZ_FORM_GROUP16;
    }
    return sw.group ? LZ_FORM_QUEUED : LZ_FORM_STEPWISE;
}
