// dust_host_main.cpp — a stand-alone program over the host side of the lit particles that needs no device
// (relativitypathtracer_amd/csrc/rpt_dust_host.hpp: the flags' validation, the launch's refusals as predicates and the choice of the splat
// kernel), for tests/test_dust_host.py, which builds it plain and with -fsanitize=address,undefined and runs it.
// TEST INFRASTRUCTURE ONLY.  Prints "ok <checks>" and returns 0, or the first failed check and 1.
#include <cstdio>
#include <string>

#include "../../relativitypathtracer_amd/csrc/rpt_dust_host.hpp"

static int checks = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        checks++;                                                       \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static bool has(const std::string &s, const char *words) { return s.find(words) != std::string::npos; }

int main() {
    static_assert(RPT_PARTICLES_LIT == 1 && RPT_PARTICLES_SHADOWED == 2 && RPT_PARTICLES_AMBIENT == 4, "the three bits");
    const int L = RPT_PARTICLES_LIT, S = RPT_PARTICLES_SHADOWED, A = RPT_PARTICLES_AMBIENT;
    // ---- the setter: every value of the three bits, and every unknown bit
    for (int flags = 0; flags < 8; flags++) {
        const bool good = flags == 0 || (flags & L);
        CHECK(rptl::lighting_fault(flags).empty() == good);
    }
    CHECK(has(rptl::lighting_fault(S), "RPT_PARTICLES_SHADOWED needs RPT_PARTICLES_LIT"));
    CHECK(has(rptl::lighting_fault(S | A), "RPT_PARTICLES_SHADOWED needs RPT_PARTICLES_LIT"));
    CHECK(has(rptl::lighting_fault(A), "RPT_PARTICLES_AMBIENT needs RPT_PARTICLES_LIT"));
    for (int bit = 3; bit < 32; bit++) {
        const int unknown = (int)(1u << bit);
        CHECK(has(rptl::lighting_fault(unknown), "unknown flag bits"));
        CHECK(has(rptl::lighting_fault(unknown | L), "unknown flag bits"));
        CHECK(has(rptl::lighting_fault(unknown | L | S | A), "unknown flag bits"));
    }
    CHECK(has(rptl::lighting_fault(-1), "unknown flag bits"));
    // ---- the launch: nothing of its own while the pass is not lit
    for (int thermal : {0, 5})
        for (bool layout : {false, true}) {
            CHECK(rptl::launch_fault(0, thermal, layout).code == RPT_OK);
            CHECK(rptl::launch_fault(0, thermal, layout).message.empty());
        }
    for (int flags : {L, L | S, L | A, L | S | A}) {
        // temperatures are the caller's argument: RPT_ERR_ARG, whatever the layout
        CHECK(rptl::launch_fault(flags, 1, true).code == RPT_ERR_ARG && has(rptl::launch_fault(flags, 1, true).message, "temperatures"));
        CHECK(rptl::launch_fault(flags, 4096, false).code == RPT_ERR_ARG && has(rptl::launch_fault(flags, 4096, false).message, "temperatures"));
        CHECK(rptl::launch_fault(flags, 0, true).code == RPT_OK && rptl::launch_fault(flags, 0, true).message.empty());
        // the missing layout is the scene's state: RPT_ERR_STATE, for a shadowed pass only
        const rptl::LaunchFault f = rptl::launch_fault(flags, 0, false);
        CHECK((f.code == RPT_OK) == !(flags & S) && f.message.empty() == !(flags & S));
        if (flags & S) CHECK(f.code == RPT_ERR_STATE && has(f.message, "no derived layout"));
    }
    // ---- the kernel: off means 1130 (1132 with temperatures), interval 0 too (rule D0); 1134; 1135 / 1136 by the windows
    for (bool windows : {false, true}) {
        CHECK(rptl::splat_kernel(0, -1, 0, windows) == 1130);
        CHECK(rptl::splat_kernel(0, -1, 9, windows) == 1132);
        CHECK(rptl::splat_kernel(0, 0, 0, windows) == 1130);
        for (int flags : {L, L | S, L | A, L | S | A}) CHECK(rptl::splat_kernel(flags, 0, 0, windows) == 1130);
        CHECK(rptl::splat_kernel(L, -1, 0, windows) == 1134);
        CHECK(rptl::splat_kernel(L | A, -1, 0, windows) == 1134);
        CHECK(rptl::splat_kernel(L | S, -1, 0, windows) == (windows ? 1136 : 1135));
        CHECK(rptl::splat_kernel(L | S | A, -1, 0, windows) == (windows ? 1136 : 1135));
    }
    std::printf("ok %d\n", checks);
    return 0;
}
