// elem_layout_check.cpp -- host check of the element kernels' LDS layout and dispatch decision (csrc/elem_layout.hpp).  Stand-alone: the sizes
// the layout gives every launch against the six formulas the launchers and the staging decision carried before the layout
// existed, written out here as the expected values.  Built with plain g++ by tests/test_elem_layout_host.py; prints OK.
#include <cstddef>
#include <cstdio>
#include <initializer_list>

#include "../../multigridbarrier.jl_amd/csrc/elem_layout.hpp"

using namespace mgbhip;

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

int group(int p) {
    int g = 1;
    while (g < p) g <<= 1;
    return g < 2 ? 2 : g;
}

// ---- the six formulas, as written before ------------------------------------------------------------------------------
size_t old_elem_lds_bytes(int p, int nu, int nD, int nstage, int mode) {
    const int G = group(p);
    const int EPB = 256 / G;
    size_t d = 256 * (size_t)nu + (size_t)nstage * EPB * p * p;
    if (mode == MODE_F1 || mode == MODE_F01) d += 256 * (size_t)nD;
    if (mode == MODE_F2) d += 256 * (size_t)(nD * (nD + 1) / 2);
    if (d < 256) d = 256;
    return d * sizeof(double);
}
size_t old_f2_fast_lds(int PN, int nu, int NY, int nstage) {          // try_f2_fast and launch_elem_f2_condense
    const int G = group(PN);
    const int EPB = 256 / G;
    return (256 * (size_t)nu + (size_t)nstage * EPB * PN * PN + (size_t)EPB * (NY * (NY + 1) / 2) * G) * sizeof(double);
}
size_t old_f01_fast_lds(int PN, int nu, int NY, int nstage) {
    const int G = group(PN);
    const int EPB = 256 / G;
    size_t lds = (256 * (size_t)nu + (size_t)nstage * EPB * PN * PN + (size_t)EPB * NY * G) * sizeof(double);
    if (lds < 256 * sizeof(double)) lds = 256 * sizeof(double);
    return lds;
}
size_t old_wide_lds_bytes(int p, int nu, int nD, int nstage, int mode) {
    const int G = group(p);
    const int threads = (mode == MODE_F2) ? 128 : 256;
    const int EPB = threads / G;
    size_t d = (size_t)threads * nu + (size_t)nstage * EPB * p * p;
    if (mode == MODE_F1 || mode == MODE_F01) d += (size_t)threads * nD;
    if (mode == MODE_F2) d += (size_t)threads * (nD * (nD + 1) / 2);
    if (d < 256) d = 256;
    return d * sizeof(double);
}
bool old_stage_decision(int p, int nu, int nD, int nstage_before, bool wide) {       // problem.cpp, non-dense
    const int G = group(p);
    const int EPB = 256 / G;
    size_t bytes = (size_t)(nstage_before + 1) * EPB * p * p * sizeof(double);
    size_t f2_total = bytes + 256 * sizeof(double) * (size_t)(nu + nD * (nD + 1) / 2);
    if (wide) f2_total = old_wide_lds_bytes(p, nu, nD, nstage_before + 1, MODE_F2);
    return bytes <= 64 * 1024 && f2_total <= 150 * 1024;
}

// ---- the dispatch, as launch_elem / try_fast / launch_elem_f2_condense / launch_elem_generic decided it before elem_decide ----
const int old_fast[8][2] = {{4, 7}, {3, 2}, {5, 8}, {4, 6}, {7, 7}, {6, 2}, {8, 8}, {7, 6}};
ElemPlan old_dispatch(int p, int nu, int nD, int nstage, bool wide, bool all_staged, bool default_sig, int mode, bool condensing,
                      long long N) {
    if (p > 64) return ElemPlan{ELEM_DENSE, 0, 0, 0, 0, 0, 0, 0};
    const int G = group(p);
    if (wide) {
        const int threads = (mode == MODE_F2) ? 128 : 256;
        const int EPB = threads / G;
        return ElemPlan{ELEM_WIDE, 0, 0, threads, G, EPB, (N + EPB - 1) / EPB, old_wide_lds_bytes(p, nu, nD, nstage, mode)};
    }
    const int EPB = 256 / G;
    const long long grid = (N + EPB - 1) / EPB;
    if (condensing && mode == MODE_F2 && nD == 4 && p == 7 && nu == 2 && nstage == 2 && default_sig && all_staged)
        return ElemPlan{ELEM_CONDENSE, 4, 7, 256, G, EPB, grid, old_f2_fast_lds(7, nu, 4, nstage)};
    if (mode == MODE_F2 || mode == MODE_F01)
        for (const auto& f : old_fast) {
            if (nD != f[0] || p != f[1] || !all_staged) continue;
            const size_t lds = (mode == MODE_F2) ? old_f2_fast_lds(p, nu, nD, nstage) : old_f01_fast_lds(p, nu, nD, nstage);
            if (lds > 160 * 1024) continue;
            return ElemPlan{default_sig ? ELEM_FAST_DEFAULT : ELEM_FAST_RUNTIME, nD, p, 256, G, EPB, grid, lds};
        }
    return ElemPlan{ELEM_GENERIC, nD, 0, 256, G, EPB, grid, old_elem_lds_bytes(p, nu, nD, nstage, mode)};
}
bool same(const ElemPlan& a, const ElemPlan& b) {
    return a.kind == b.kind && a.NY == b.NY && a.P == b.P && a.threads == b.threads && a.G == b.G && a.EPB == b.EPB && a.grid == b.grid &&
           a.lds == b.lds;
}

}  // namespace

int main() {
    const int ps[] = {1, 2, 3, 6, 7, 8, 27, 64}, nus[] = {1, 2, 4}, nDs[] = {1, 3, 4, 7, 10, 11, 13}, nstages[] = {0, 1, 2, 3};
    const int modes[] = {MODE_F0, MODE_F1, MODE_F2, MODE_NODE_F, MODE_NODE_SLACK, MODE_F01};
    long checked = 0;
    for (int p : ps) {
        CHECK(elem_group(p) == group(p), "p=%d", p);
        for (int nu : nus)
            for (int nD : nDs)
                for (int nstage : nstages) {
                    for (int mode : modes) {
                        // narrow generic launch: 256 threads
                        CHECK(elem_threads(false, mode) == 256, "mode=%d", mode);
                        CHECK(elem_lds_bytes(256, p, nu, nD, nstage, mode) == old_elem_lds_bytes(p, nu, nD, nstage, mode),
                              "narrow p=%d nu=%d nD=%d nstage=%d mode=%d", p, nu, nD, nstage, mode);
                        // wide launch: 128 threads for MODE_F2, 256 otherwise
                        const int wt = elem_threads(true, mode);
                        CHECK(wt == (mode == MODE_F2 ? 128 : 256), "mode=%d", mode);
                        CHECK(elem_lds_bytes(wt, p, nu, nD, nstage, mode) == old_wide_lds_bytes(p, nu, nD, nstage, mode),
                              "wide p=%d nu=%d nD=%d nstage=%d mode=%d", p, nu, nD, nstage, mode);
                        checked += 2;
                    }
                    // fast kernels and the condensing f2 (256 threads)
                    CHECK(elem_lds_bytes(256, p, nu, nD, nstage, MODE_F2) == old_f2_fast_lds(p, nu, nD, nstage),
                          "f2 fast p=%d nu=%d nD=%d nstage=%d", p, nu, nD, nstage);
                    CHECK(elem_lds_bytes(256, p, nu, nD, nstage, MODE_F01) == old_f01_fast_lds(p, nu, nD, nstage),
                          "f01 fast p=%d nu=%d nD=%d nstage=%d", p, nu, nD, nstage);
                    // staging decision with nstage operators already staged, both paths
                    for (int wide = 0; wide < 2; ++wide)
                        CHECK(elem_stage_fits(p, nu, nD, nstage + 1, wide != 0) == old_stage_decision(p, nu, nD, nstage, wide != 0),
                              "staging p=%d nu=%d nD=%d nstage=%d wide=%d", p, nu, nD, nstage, wide);
                    checked += 4;
                }
    }
    // the dispatch decision over the whole grid: every p up to the dense gate, every nD, both paths, every flag
    long decided = 0;
    int kinds_seen = 0;
    for (int p = 1; p <= 66; ++p)
        for (int nu = 1; nu <= 4; ++nu)
            for (int nD = 1; nD <= 13; ++nD)
                for (int nstage = 0; nstage <= 6; ++nstage)
                    for (int flags = 0; flags < 16; ++flags) {
                        const bool wide = (flags & 1) || nD > 10, all_staged = flags & 2, default_sig = flags & 4, condensing = flags & 8;
                        for (int mode : modes)
                            for (long long N : {1LL, 31LL, 32LL, 33LL, 129LL, 70000LL}) {
                                const ElemPlan got = elem_decide(p, nu, nD, nstage, wide, p > 64, all_staged, default_sig, mode, condensing, N);
                                const ElemPlan want = old_dispatch(p, nu, nD, nstage, wide, all_staged, default_sig, mode, condensing, N);
                                CHECK(same(got, want), "dispatch p=%d nu=%d nD=%d nstage=%d flags=%d mode=%d N=%lld: kind %d/%d NY %d/%d lds %zu/%zu",
                                      p, nu, nD, nstage, flags, mode, N, got.kind, want.kind, got.NY, want.NY, got.lds, want.lds);
                                if (got.kind != ELEM_DENSE) CHECK(got.EPB * got.G == got.threads && got.grid * got.EPB >= N && (got.grid - 1) * got.EPB < N,
                                                                  "grid covers N: p=%d mode=%d N=%lld", p, mode, N);
                                kinds_seen |= 1 << got.kind;
                                ++decided;
                            }
                    }
    CHECK(kinds_seen == 0x3f, "every kernel kind is reached: %x", kinds_seen);
    for (int i = 0; i < ELEM_FAST_COUNT; ++i) {
        CHECK(ELEM_FAST_TABLE[i][0] == old_fast[i][0] && ELEM_FAST_TABLE[i][1] == old_fast[i][1], "fast table entry %d", i);
        CHECK(elem_fast_index(ELEM_FAST_TABLE[i][0], ELEM_FAST_TABLE[i][1]) == i, "fast index %d", i);
    }
    CHECK(elem_fast_index(4, 8) == -1 && elem_fast_index(3, 7) == -1, "pairs outside the table");
    checked += decided;

    // the kernels' own offsets: opL behind zl, YL behind opL
    CHECK(elem_lds_z(256, 2) == 512 && elem_lds_z((size_t)128, 4) == 512, "z region");
    CHECK(elem_lds_ops(2, 32, 49) == 3136, "operator region");

    // staging decision on three shapes, operator by operator as problem.cpp walks the D table
    struct Shape { const char* name; int p, nu, nD, nops; bool wide; };
    const Shape shapes[] = {{"fem2d_P2 with bubble", 7, 2, 4, 2, false}, {"fem3d Q1", 8, 2, 5, 3, false},
                            {"phase-I image of 2-D p_harmonic (wide)", 7, 4, 11, 2, true}};
    for (const Shape& s : shapes)
        for (int staged = 0; staged < 6; ++staged) {
            const bool fits = elem_stage_fits(s.p, s.nu, s.nD, staged + 1, s.wide);
            CHECK(fits == old_stage_decision(s.p, s.nu, s.nD, staged, s.wide), "%s staged=%d", s.name, staged);
            if (staged < s.nops) CHECK(fits, "%s: operator %d must be staged", s.name, staged);
        }
    if (g_failures) {
        fprintf(stderr, "%d failures\n", g_failures);
        return 1;
    }
    printf("%ld sizes checked\nOK\n", checked);
    return 0;
}
