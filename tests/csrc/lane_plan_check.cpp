// lane_plan_check.cpp -- host table of quad_decide and face_decide (csrc/quad_layout.hpp, csrc/faces_layout.hpp) for
// tests/test_lane_plan_host.py, which builds it with plain g++ (the layout headers are host-only code).
// One line per shape and count, every plan field:
//   "Q d e p Q N threads S G chunk tables_lds reduce_threads groups grid lds"
//   "F d p Qf F sides nfaces threads S G chunk tables_lds reduce_threads groups grid lds"
#include <cstdio>

#include "../../multigridbarrier.jl_amd/csrc/faces_layout.hpp"
#include "../../multigridbarrier.jl_amd/csrc/quad_layout.hpp"

template <class Plan>
static void fields(const Plan& P) {
    printf(" %d %d %d %d %d %d %lld %lld %zu\n", P.threads, P.S, P.G, P.chunk, P.tables_lds, P.reduce_threads, P.groups, P.grid, P.lds);
}

int main() {
    using namespace mgbhip;
    static const int de[][2] = {{1, 1}, {1, 2}, {1, 3}, {2, 2}, {2, 3}, {3, 3}};
    static const int ps[] = {1, 2, 3, 4, 6, 8, 9, 13, 14, 26, 27, 28, 64, 100, 120, 121, 125, 216, 729, 1000, 1389, 1390, 1500, 2600, 5000};
    static const int Qs[] = {1, 2, 3, 4, 7, 8, 9, 27, 64, 100, 128, 129, 255, 256, 257, 343, 512, 1000};
    static const int Qfs[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 25, 36, 64, 100, 101, 256, 300};
    static const int Fs[] = {3, 4, 6};
    static const long long counts[] = {0, 1, 31, 32, 33, 255, 256, 257, 32LL * 2047, 32LL * 2047 + 1, 32LL * 3000};
    for (const auto& s : de)
        for (int p : ps)
            for (int Q : Qs)
                for (long long N : counts) {
                    printf("Q %d %d %d %d %lld", s[0], s[1], p, Q, N);
                    fields(quad_decide(s[0], s[1], p, Q, N));
                }
    for (int d = 2; d <= 3; ++d)
        for (int p : ps)
            for (int Qf : Qfs)
                for (int F : Fs)
                    for (int sides = 1; sides <= 2; ++sides)
                        for (long long n : counts) {
                            printf("F %d %d %d %d %d %lld", d, p, Qf, F, sides, n);
                            fields(face_decide(d, p, Qf, F, sides, n));
                        }
    return 0;
}
