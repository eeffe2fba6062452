// driver of tests/test_env_switches_cpu.py: csrc/env_switches.h (and csrc/work_plan.h for the knobs) compiled alone with the host
// compiler.  The test sets the child's environment; the command is argv[1]:
//   LIST     one line per entry of the list: name|kind|read time|default
//   READ     one representative variable per kind, then the work plan's knobs, as the environment states them:
//            on_unless_zero (HDM_DIAG_SWEEP), off_unless_nonzero (HDM_POISON), int set value (HDSDP_MI355X_ZS),
//            string (HDSDP_MI355X_TRANSPORT: [text], or - when unset), knobs tcap bc kstages nsplit_set nsplit share_t_slabs gram_queue
//   WHEN v   reads a ONCE and a NOW variable of the integer kind (HDSDP_MI355X_ZS, HDSDP_MI355X_REFINE) and of the on / off kind
//            (HDM_PERSIST, HDSDP_MI355X_SPARSE_KKT), sets all four to v, reads them again: first readings, then second readings
//   THREADS  eight threads released together read HDSDP_MI355X_AFFINE_S (ONCE) for the first time; then the variable is set to 7
//            and read once more: the nine values
#include "work_plan.h"
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

static const char *kind_name(HdmEnvKind k) {
    switch (k) {
        case HdmEnvKind::ON_UNLESS_ZERO: return "ON_UNLESS_ZERO";
        case HdmEnvKind::OFF_UNLESS_NONZERO: return "OFF_UNLESS_NONZERO";
        case HdmEnvKind::INT: return "INT";
        default: return "STRING";
    }
}

static void print_when() {
    const HdmEnvInt once = hdm_env_int<ENV_ZS>(), now = hdm_env_int<ENV_REFINE>();
    printf("%d %ld %d %ld %d %d\n", (int) once.set, once.value, (int) now.set, now.value, (int) hdm_env_on<ENV_PERSIST>(),
           (int) hdm_env_on<ENV_SPARSE_KKT>());
}

int main(int argc, char **argv) {
    const char *cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "LIST")) {
        static_assert(sizeof(hdm_env_table) / sizeof(hdm_env_table[0]) == ENV_COUNT, "one table entry per identifier");
        for (int i = 0; i < ENV_COUNT; ++i) {
            const HdmEnvEntry &e = hdm_env_table[i];
            printf("%s|%s|%s|%s\n", e.name, kind_name(e.kind), e.when == HdmEnvWhen::ONCE ? "ONCE" : "NOW", e.dflt);
        }
    } else if (!strcmp(cmd, "READ")) {
        printf("on_unless_zero %d\n", (int) hdm_env_on<ENV_DIAG_SWEEP>());
        printf("off_unless_nonzero %d\n", (int) hdm_env_on<ENV_POISON>());
        const HdmEnvInt z = hdm_env_int<ENV_ZS>();
        printf("int %d %ld\n", (int) z.set, z.value);
        const char *t = hdm_env_string<ENV_TRANSPORT>();
        if (t) printf("string [%s]\n", t);
        else printf("string -\n");
        const HdmKnobs k = hdm_knobs_from_env();
        printf("knobs %ld %ld %ld %d %ld %d %d\n", k.tcap_gib, k.bc_max, k.gram_kstages, (int) k.nsplit_set, k.nsplit, (int) k.share_t_slabs,
               (int) k.gram_queue_global);
    } else if (!strcmp(cmd, "WHEN") && argc > 2) {
        print_when();
        for (const char *name : {"HDSDP_MI355X_ZS", "HDSDP_MI355X_REFINE", "HDM_PERSIST", "HDSDP_MI355X_SPARSE_KKT"}) setenv(name, argv[2], 1);
        print_when();
    } else if (!strcmp(cmd, "THREADS")) {
        std::atomic<int> waiting{0};
        long got[8];
        std::vector<std::thread> th;
        for (int i = 0; i < 8; ++i)
            th.emplace_back([&, i] {
                waiting.fetch_add(1);
                while (waiting.load() < 8) {}
                got[i] = hdm_env_int<ENV_AFFINE_S>().value;
            });
        for (std::thread &t : th) t.join();
        for (long v : got) printf("%ld ", v);
        setenv("HDSDP_MI355X_AFFINE_S", "7", 1);
        printf("%ld\n", hdm_env_int<ENV_AFFINE_S>().value);
    } else return 2;
    return 0;
}
