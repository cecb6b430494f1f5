// bwd_split_check.cpp -- host check of the launch rule of the column-split backward sweep (csrc/mf_launch_plan.hpp:
// bwd_inv_split, bwd_split_stride, bwd_split_scratch).  Stand-alone: the rule at each of its edges, the scratch sizes on
// hand-built launch lists, and every "count max_k max_m S" quadruple given on the command line (tests/backward_split_cases.py
// pins S per launch of its cases).  Built with plain g++ and -fsanitize=address,undefined by
// tests/test_backward_split_cases.py; prints OK.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../multigridbarrier.jl_amd/csrc/mf_analysis.hpp"
#include "../../multigridbarrier.jl_amd/csrc/mf_launch_plan.hpp"

using namespace mgbhip;

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

void expect(int32_t count, int32_t max_k, int32_t max_m, int want) {
    const int got = bwd_inv_split(count, max_k, max_m);
    CHECK(got == want, "bwd_inv_split(%d, %d, %d) = %d, expected %d", count, max_k, max_m, got, want);
}

MfLaunch big(int32_t first, int32_t count, int32_t max_m, int32_t max_k, bool inv) {
    MfLaunch L{};
    L.first = first; L.count = count; L.cls = 0; L.max_m = max_m; L.max_k = max_k; L.inv = inv;
    return L;
}

}  // namespace

int main(int argc, char** argv) {
    // ---- the rule at its edges: S = min(16, 256 / count, ceil(max_k / 64)), 1 for a thin boundary
    // count (max_k = 4096 so that the column term is at the cap: 64 columns per workgroup would allow 64)
    expect(1, 4096, 5000, 16);
    expect(16, 4096, 5000, 16);          // 256 / 16 = 16
    expect(17, 4096, 5000, 15);          // 256 / 17 = 15
    expect(128, 4096, 5000, 2);
    expect(129, 4096, 5000, 1);
    expect(256, 4096, 5000, 1);
    expect(257, 4096, 5000, 1);          // 256 / 257 = 0: never below 1
    expect(0, 4096, 5000, 1);
    // pivot columns: one workgroup per started 64
    expect(1, 1, 200, 1);
    expect(1, 64, 200, 1);
    expect(1, 65, 200, 2);
    expect(1, 128, 400, 2);
    expect(1, 129, 400, 3);
    expect(1, 960, 2000, 15);
    expect(1, 961, 2000, 16);
    expect(1, 1025, 2000, 16);           // the cap
    expect(2, 255, 767, 4);              // the two-front level of fem2d_P2 at L = 9
    // boundary rows (max_m - max_k): up to 8 the fronts take one thread per column and the launch stays unsplit
    expect(1, 255, 255 + 1, 1);
    expect(1, 255, 255 + 8, 1);
    expect(1, 255, 255 + 9, 4);
    expect(4, 511, 511 + 8, 1);
    expect(4, 511, 511 + 9, 8);
    CHECK(BWD_THIN_BOUNDARY == 8 && BWD_SPLIT_MAX == 16 && BWD_SPLIT_COLS == 64 && BWD_SPLIT_CUS == 256, "constants of the rule");

    // ---- scratch: stride even and >= max_k; sizes = the largest split launch, unsplit / LDS / non-inverse launches do not count
    for (int32_t k = 1; k < 70; ++k) {
        const int32_t s = bwd_split_stride(k);
        CHECK(s >= k && s % 2 == 0 && s <= k + 1, "stride(%d) = %d", k, s);
    }
    {
        LevelLaunches solves(5);
        MfLaunch lds{};
        lds.first = 0; lds.count = 4000; lds.cls = 64; lds.max_m = 60; lds.max_k = 30;
        solves[0].push_back(lds);
        solves[0].push_back(big(4000, 300, 400, 200, true));        // 300 fronts: S = 1
        solves[1].push_back(big(4300, 40, 700, 255, true));         // S = 4: 40 counters, 40 * 256 doubles
        solves[2].push_back(big(4340, 3, 2000, 1001, true));        // S = 16: 3 counters, 3 * 1002 doubles
        solves[2].push_back(big(4343, 90, 3000, 2001, false));      // substitution kernels: no split
        solves[3].push_back(big(4433, 1, 512, 511, true));          // the root: border row only
        MfLaunch empty = big(4434, 0, 0, 0, true);
        solves[4].push_back(empty);
        int64_t need[2] = {-1, -1};
        bwd_split_scratch(solves, need);
        CHECK(need[0] == 40, "counters %lld", (long long)need[0]);
        CHECK(need[1] == 40 * 256, "doubles %lld", (long long)need[1]);
        solves[1].clear();
        bwd_split_scratch(solves, need);
        CHECK(need[0] == 3 && need[1] == 3 * 1002, "counters %lld doubles %lld", (long long)need[0], (long long)need[1]);
        solves[2].clear();
        bwd_split_scratch(solves, need);
        CHECK(need[0] == 0 && need[1] == 0, "no split launch: %lld %lld", (long long)need[0], (long long)need[1]);
        // every front of a split launch has its counter and its k products inside the allocation
        LevelLaunches one(1);
        one[0].push_back(big(0, 5, 264, 226, true));
        bwd_split_scratch(one, need);
        CHECK(need[0] >= 5 && need[1] >= (int64_t)4 * bwd_split_stride(226) + 226, "five fronts: %lld %lld", (long long)need[0], (long long)need[1]);
    }
    // ---- the environment switch
    {
        unsetenv("MGBHIP_BWD_SPLIT");
        CHECK(MfSwitches::from_env().bwd_split, "default: on");
        setenv("MGBHIP_BWD_SPLIT", "0", 1);
        CHECK(!MfSwitches::from_env().bwd_split, "MGBHIP_BWD_SPLIT=0: off");
        setenv("MGBHIP_BWD_SPLIT", "1", 1);
        CHECK(MfSwitches::from_env().bwd_split, "MGBHIP_BWD_SPLIT=1: on");
        unsetenv("MGBHIP_BWD_SPLIT");
    }
    // ---- the launches the cases pin
    CHECK((argc - 1) % 4 == 0, "arguments come in fours");
    int given = 0;
    for (int i = 1; i + 3 < argc; i += 4, ++given) expect(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]));
    if (g_failures) {
        fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    printf("%d pinned launches\nOK\n", given);
    return 0;
}
