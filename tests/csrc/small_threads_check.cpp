// small_threads_check.cpp -- host table of factor_small_threads (csrc/mf_launch_plan.hpp) for tests/test_small_threads_rule.py,
// which builds it with plain g++ (the launch plan is host-only code).  Usage: small_threads_check CU [CU ...]
// One line per (class, compute units, forced, count): "cls cu forced count threads lds".
#include <cstdio>
#include <cstdlib>

#include "../../multigridbarrier.jl_amd/csrc/mf_launch_plan.hpp"

int main(int argc, char** argv) {
    using namespace mgbhip;
    static const int classes[] = {16, 32, 48, 64, 88, 128};
    static const int forced[] = {0, 256, 512, 1024, 300};
    for (int a = 1; a < argc; ++a) {
        const int cu = atoi(argv[a]);
        for (int cls : classes)
            for (int f : forced) {
                const int top = 10 * (cu > 0 ? cu : 1) + 2;      // past every threshold: a compute unit holds at most 6 fronts
                for (int count = 1; count <= top; ++count) {
                    MfLaunch L{};
                    L.first = 0; L.count = count; L.cls = cls; L.max_m = cls; L.max_k = cls - 1;
                    printf("%d %d %d %d %d %zu\n", cls, cu, f, count, factor_small_threads(L, cu, f), factor_small_lds(cls));
                }
            }
    }
    return 0;
}
