// env_switches.h -- every environment variable the library reads, stated once: name, kind, read time, and the default as the
// table of include/hdsdp_mi355x.h prints it (tests/test_env_switches_cpu.py and tests/test_abi_cpu.py hold that table to this
// list).  A reader takes an HdmEnvId, not a string: a name that is not in the list cannot be read, and asking a variable for
// another kind than its own does not compile.  Pure host code: no HIP call, no engine state.
// Kinds (the text goes through atoi / atol: "", "abc" and "00" are 0; " 1" and "1x" are 1):
//   ON_UNLESS_ZERO      hdm_env_on:      unset -> true;  set -> atoi(text) != 0
//   OFF_UNLESS_NONZERO  hdm_env_on:      unset -> false; set -> atoi(text) != 0
//   INT                 hdm_env_int:     whether the variable is set, and atol(text); a threshold or clamp (DEVICE_M == 1,
//                                        REFINE > 0, A2A_PIECES >= 1, ...) is part of the variable's meaning and stays at its site
//   STRING              hdm_env_string:  the text itself, nullptr when unset
// Read times:
//   ONCE  the first read by anyone in the process is kept: a later read is the guard check of a function-local static (no
//         getenv, no lock, no allocation), and concurrent first reads are safe
//   NOW   every read asks the environment (tests set these in-process, the work plan's knobs between cones)
#pragma once
#include <cstdlib>
enum class HdmEnvKind { ON_UNLESS_ZERO, OFF_UNLESS_NONZERO, INT, STRING };
enum class HdmEnvWhen { ONCE, NOW };
//    identifier           variable                        kind                read  default
#define HDM_ENV_LIST_PRODUCT(X) \
    X(LOCAL_RANK,          "LOCAL_RANK",                   INT,                NOW,  "0") \
    X(GPUS,                "HDSDP_MI355X_GPUS",            INT,                NOW,  "1") \
    X(LOOPBACK,            "HDSDP_MI355X_LOOPBACK",        OFF_UNLESS_NONZERO, NOW,  "0") \
    X(SHARD_MIN_N,         "HDSDP_MI355X_SHARD_MIN_N",     INT,                NOW,  "512") \
    X(TRANSPORT,           "HDSDP_MI355X_TRANSPORT",       STRING,             NOW,  "copy") \
    X(A2A_PIECES,          "HDSDP_MI355X_A2A_PIECES",      INT,                NOW,  "8") \
    X(STAGED_A2A,          "HDSDP_MI355X_STAGED_A2A",      ON_UNLESS_ZERO,     NOW,  "1") \
    X(FORCE_GEMM,          "HDSDP_MI355X_FORCE_GEMM",      OFF_UNLESS_NONZERO, NOW,  "0") \
    X(FORCE_PATH,          "HDSDP_MI355X_FORCE_PATH",      INT,                NOW,  "-") \
    X(SPARSE_KKT,          "HDSDP_MI355X_SPARSE_KKT",      ON_UNLESS_ZERO,     NOW,  "1") \
    X(KKT_ENVELOPE,        "HDSDP_MI355X_KKT_ENVELOPE",    ON_UNLESS_ZERO,     ONCE, "1") \
    X(KKT_RCM,             "HDSDP_MI355X_KKT_RCM",         ON_UNLESS_ZERO,     ONCE, "1") \
    X(KKT_TILES,           "HDSDP_MI355X_KKT_TILES",       ON_UNLESS_ZERO,     ONCE, "1") \
    X(AFFINE_S,            "HDSDP_MI355X_AFFINE_S",        INT,                ONCE, "by cost") \
    X(SMALL_CHECK,         "HDSDP_MI355X_SMALL_CHECK",     ON_UNLESS_ZERO,     ONCE, "1") \
    X(ZS,                  "HDSDP_MI355X_ZS",              INT,                ONCE, "by cost") \
    X(PRIMAL_SIGNED,       "HDSDP_MI355X_PRIMAL_SIGNED",   ON_UNLESS_ZERO,     NOW,  "1") \
    X(DIRECT_ROWS,         "HDSDP_MI355X_DIRECT_ROWS",     INT,                NOW,  "by size") \
    X(STREAM_A,            "HDSDP_MI355X_STREAM_A",        INT,                NOW,  "by memory") \
    X(DEVICE_M,            "HDSDP_MI355X_DEVICE_M",        INT,                NOW,  "0") \
    X(GROUPED_BUILD,       "HDSDP_MI355X_GROUPED_BUILD",   OFF_UNLESS_NONZERO, ONCE, "0") \
    X(GROUPED_CHECK,       "HDSDP_MI355X_GROUPED_CHECK",   OFF_UNLESS_NONZERO, ONCE, "0") \
    X(GROUPED_RATIO,       "HDSDP_MI355X_GROUPED_RATIO",   OFF_UNLESS_NONZERO, ONCE, "0") \
    X(GRATIO_CHECKER,      "HDSDP_MI355X_GRATIO_CHECKER",  OFF_UNLESS_NONZERO, ONCE, "0") \
    X(GRATIO_REST,         "HDSDP_MI355X_GRATIO_REST",     OFF_UNLESS_NONZERO, ONCE, "0") \
    X(GROUPED_STEP,        "HDSDP_MI355X_GROUPED_STEP",    OFF_UNLESS_NONZERO, ONCE, "0") \
    X(REFINE,              "HDSDP_MI355X_REFINE",          INT,                NOW,  "0") \
    X(REFINE_TILES,        "HDSDP_MI355X_REFINE_TILES",    INT,                NOW,  "0") \
    X(TCAP_GIB,            "HDM_TCAP_GIB",                 INT,                NOW,  "32") \
    X(BC,                  "HDM_BC",                       INT,                NOW,  "1024") \
    X(NSPLIT,              "HDM_NSPLIT",                   INT,                NOW,  "by size") \
    X(GRAM_KSTAGES,        "HDM_GRAM_KSTAGES",             INT,                NOW,  "by size") \
    X(GRAM_QUEUE,          "HDM_GRAM_QUEUE",               ON_UNLESS_ZERO,     NOW,  "1") \
    X(SHARE_T_SLABS,       "HDM_SHARE_T_SLABS",            ON_UNLESS_ZERO,     NOW,  "1") \
    X(HOST_THREADS,        "HDSDP_MI355X_HOST_THREADS",    INT,                ONCE, "min(16, cores)") \
    X(PERSIST,             "HDM_PERSIST",                  ON_UNLESS_ZERO,     ONCE, "1") \
    X(PERSIST_RESERVE_CUS, "HDM_PERSIST_RESERVE_CUS",      INT,                ONCE, "0 / 8") \
    X(DIAG_SWEEP,          "HDM_DIAG_SWEEP",               ON_UNLESS_ZERO,     ONCE, "1") \
    X(CHOL_K128,           "HDM_CHOL_K128",                ON_UNLESS_ZERO,     ONCE, "1") \
    X(TRSV_FLOW,           "HDM_TRSV_FLOW",                ON_UNLESS_ZERO,     ONCE, "1") \
    X(TRSV_FLOW_FAIL_ONCE, "HDM_TRSV_FLOW_FAIL_ONCE",      OFF_UNLESS_NONZERO, ONCE, "0") \
    X(SYM_COMBINE_SKY,     "HDM_SYM_COMBINE_SKY",          ON_UNLESS_ZERO,     ONCE, "1") \
    X(LANCZOS_WHOLE,       "HDM_LANCZOS_WHOLE",            ON_UNLESS_ZERO,     ONCE, "1") \
    X(LANCZOS_FUSED,       "HDM_LANCZOS_FUSED",            ON_UNLESS_ZERO,     ONCE, "1") \
    X(LANCZOS_GROUP,       "HDM_LANCZOS_GROUP",            ON_UNLESS_ZERO,     ONCE, "1") \
    X(LANCZOS_BIG,         "HDM_LANCZOS_BIG",              ON_UNLESS_ZERO,     ONCE, "1") \
    X(PRELOAD,             "HDSDP_MI355X_PRELOAD",         ON_UNLESS_ZERO,     NOW,  "1") \
    X(CALL_STATS,          "HDSDP_MI355X_CALL_STATS",      OFF_UNLESS_NONZERO, NOW,  "0") \
    X(TRACE,               "HDSDP_MI355X_TRACE",           OFF_UNLESS_NONZERO, ONCE, "0") \
    X(RATIO_DEBUG,         "HDSDP_MI355X_RATIO_DEBUG",     INT,                ONCE, "0") \
    X(AFFINE_DEBUG,        "HDSDP_MI355X_AFFINE_DEBUG",    OFF_UNLESS_NONZERO, ONCE, "0") \
    X(POISON,              "HDM_POISON",                   OFF_UNLESS_NONZERO, ONCE, "0")
#ifdef HDM_DIAGNOSTICS   // three more, for stamped kernels and timing ablations: in the product they do not exist
#define HDM_ENV_LIST_DIAGNOSTIC(X) \
    X(VAR,                 "HDM_VAR",                      INT,                ONCE, "-") \
    X(CONG2_DIRECT,        "HDM_CONG2_DIRECT",             OFF_UNLESS_NONZERO, ONCE, "0") \
    X(DBG_SYNC,            "HDM_DBG_SYNC",                 INT,                NOW,  "-")
#else
#define HDM_ENV_LIST_DIAGNOSTIC(X)
#endif
#define HDM_ENV_LIST(X) HDM_ENV_LIST_PRODUCT(X) HDM_ENV_LIST_DIAGNOSTIC(X)

#define HDM_ENV_ID(id, name, kind, when, dflt) ENV_##id,
#define HDM_ENV_ENTRY(id, name, kind, when, dflt) {name, HdmEnvKind::kind, HdmEnvWhen::when, dflt},
enum HdmEnvId { HDM_ENV_LIST(HDM_ENV_ID) ENV_COUNT };
struct HdmEnvEntry { const char *name; HdmEnvKind kind; HdmEnvWhen when; const char *dflt; };
inline constexpr HdmEnvEntry hdm_env_table[] = {HDM_ENV_LIST(HDM_ENV_ENTRY)};

struct HdmEnvInt { bool set; long value; int value_or(int unset) const { return set ? (int) value : unset; } };   // value: 0 when unset

template <HdmEnvId ID> inline bool hdm_env_on() {
    constexpr HdmEnvKind K = hdm_env_table[ID].kind;
    static_assert(K == HdmEnvKind::ON_UNLESS_ZERO || K == HdmEnvKind::OFF_UNLESS_NONZERO, "not an on / off switch");
    const auto read = [] { const char *e = getenv(hdm_env_table[ID].name); return e ? atoi(e) != 0 : K == HdmEnvKind::ON_UNLESS_ZERO; };
    if constexpr (hdm_env_table[ID].when == HdmEnvWhen::ONCE) { static const bool on = read(); return on; } else return read();
}
template <HdmEnvId ID> inline HdmEnvInt hdm_env_int() {
    static_assert(hdm_env_table[ID].kind == HdmEnvKind::INT, "not an integer variable");
    const auto read = [] { const char *e = getenv(hdm_env_table[ID].name); return HdmEnvInt{e != nullptr, e ? atol(e) : 0L}; };
    if constexpr (hdm_env_table[ID].when == HdmEnvWhen::ONCE) { static const HdmEnvInt v = read(); return v; } else return read();
}
template <HdmEnvId ID> inline const char *hdm_env_string() {
    static_assert(hdm_env_table[ID].kind == HdmEnvKind::STRING && hdm_env_table[ID].when == HdmEnvWhen::NOW, "not a string variable");
    return getenv(hdm_env_table[ID].name);
}
