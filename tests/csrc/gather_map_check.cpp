// gather_map_check.cpp -- host check of the static gather maps of mf_big_gather (csrc/mf_launch_plan.hpp: build_gather_maps).
// Stand-alone: mf_analyze on a few block-arrow patterns, the launch classification, the maps -- and every map entry against
// a brute-force inversion of the children's relative index lists, every record against the plan.  Built with plain g++ and
// -fsanitize=address,undefined by tests/test_gather_map_host.py; prints OK.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../../multigridbarrier.jl_amd/csrc/mf_analysis.hpp"
#include "../../multigridbarrier.jl_amd/csrc/mf_launch_plan.hpp"

using namespace mgbhip;

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// A pattern as a union of cliques (tests/solver_gate_cases.py: Builder).
struct Builder {
    int32_t n = 0;
    std::vector<std::vector<int32_t>> cliques;
    std::vector<int32_t> cols(int32_t count) {
        std::vector<int32_t> out;
        for (int32_t i = 0; i < count; ++i) out.push_back(n++);
        return out;
    }
    void clique(std::vector<int32_t> a, const std::vector<int32_t>& b) {
        a.insert(a.end(), b.begin(), b.end());
        cliques.push_back(a);
    }
    // cliques of ks[i] unknowns under a shared separator of s unknowns; returns the separator
    std::vector<int32_t> arrow(const std::vector<int32_t>& ks, int32_t s) {
        const std::vector<int32_t> sep = cols(s);
        for (int32_t k : ks) clique(cols(k), sep);
        return sep;
    }
    void csr(std::vector<int32_t>& rowptr, std::vector<int32_t>& colidx) const {
        std::vector<std::set<int32_t>> adj((size_t)n);
        for (auto& c : cliques)
            for (int32_t u : c)
                for (int32_t v : c) adj[(size_t)u].insert(v);
        rowptr.assign(1, 0);
        colidx.clear();
        for (auto& a : adj) {
            colidx.insert(colidx.end(), a.begin(), a.end());
            rowptr.push_back((int32_t)colidx.size());
        }
    }
};

struct Seen {
    int fronts = 0;
    bool eight_children = false, unequal_children = false, partial_reach = false;
};

void check_pattern(const char* name, const Builder& b, Seen& seen) {
    std::vector<int32_t> rowptr, colidx;
    b.csr(rowptr, colidx);
    MfPlan plan;
    MfOptions opt;
    opt.border = true;
    mf_analyze(b.n, rowptr.data(), colidx.data(), opt, plan);
    MfSwitches sw = MfSwitches::from_env();
    LevelLaunches levels = classify_launches(plan, 128, true, sw);
    std::vector<GatherRec> recs;
    std::vector<int32_t> gmap;
    build_gather_maps(plan, levels, recs, gmap);

    int64_t nrec = 0, nmap = 0;
    int fronts_here = 0;
    for (auto& lev : levels)
        for (auto& L : lev) {
            if (L.count == 0 || big_assembly_kind(L) != MF_ASM_GATHER) {
                CHECK(L.grec_first == -1, "%s: a launch without gather assembly has record %d", name, L.grec_first);
                continue;
            }
            CHECK(L.grec_first == nrec, "%s: launch at front %d starts at record %d, expected %lld", name, L.first, L.grec_first, (long long)nrec);
            for (int32_t q = L.first; q < L.first + L.count; ++q, ++nrec) {
                const Front& f = plan.fronts[q];
                CHECK(nrec < (int64_t)recs.size(), "%s: front %d has no record", name, q);
                if (nrec >= (int64_t)recs.size()) return;
                const GatherRec& R = recs[(size_t)nrec];
                CHECK(f.nchild >= 0 && f.nchild <= GATHER_MAX_CHILD, "%s: front %d has %d children", name, q, f.nchild);
                CHECK(R.map_off == nmap, "%s: front %d map offset %lld, expected %lld", name, q, (long long)R.map_off, (long long)nmap);
                CHECK(R.map_off + (int64_t)f.nchild * f.m <= (int64_t)gmap.size(), "%s: front %d maps past the end", name, q);
                if (R.map_off + (int64_t)f.nchild * f.m > (int64_t)gmap.size()) return;
                std::set<int32_t> sizes;
                for (int32_t c = 0; c < GATHER_MAX_CHILD; ++c) {
                    if (c >= f.nchild) {
                        CHECK(R.base[c] == 0 && R.ld[c] == 0 && R.bs[c] == 0, "%s: front %d unused child slot %d is not zero", name, q, c);
                        continue;
                    }
                    const Front& ch = plan.fronts[plan.children[f.child_off + c]];
                    const int32_t bs = ch.m - ch.k;
                    CHECK(R.base[c] == ch.F_off + (int64_t)ch.k * ch.m + ch.k, "%s: front %d child %d base", name, q, c);
                    CHECK(R.ld[c] == ch.m, "%s: front %d child %d leading dimension", name, q, c);
                    CHECK(R.bs[c] == bs, "%s: front %d child %d block size", name, q, c);
                    CHECK(R.base[c] + (int64_t)(bs - 1) * ch.m + bs <= plan.arena_doubles, "%s: front %d child %d block leaves the arena", name, q, c);
                    sizes.insert(bs);
                    // brute force: the position of front row r in the child's list, by a search of the list for every r
                    const int32_t* rel = plan.rel.data() + ch.rel_off;
                    const int32_t* mp = gmap.data() + R.map_off + (int64_t)c * f.m;
                    int32_t reached = 0;
                    for (int32_t r = 0; r < f.m; ++r) {
                        int32_t pos = -1, hits = 0;
                        for (int32_t j = 0; j < bs; ++j)
                            if (rel[j] == r) { pos = j; ++hits; }
                        CHECK(hits <= 1, "%s: front %d child %d lists row %d %d times", name, q, c, r, hits);
                        CHECK(mp[r] == pos, "%s: front %d child %d row %d: map %d, list %d", name, q, c, r, mp[r], pos);
                        reached += pos >= 0;
                    }
                    CHECK(reached == bs, "%s: front %d child %d reaches %d rows of %d", name, q, c, reached, bs);
                    if (bs > 0 && rel[0] > 0) seen.partial_reach = true;
                }
                nmap += (int64_t)f.nchild * f.m;
                ++fronts_here;
                if (f.nchild == GATHER_MAX_CHILD) seen.eight_children = true;
                if (sizes.size() > 1) seen.unequal_children = true;
            }
        }
    CHECK(nrec == (int64_t)recs.size(), "%s: %lld records for %lld fronts", name, (long long)recs.size(), (long long)nrec);
    CHECK(nmap == (int64_t)gmap.size(), "%s: %lld map entries, expected %lld", name, (long long)gmap.size(), (long long)nmap);
    CHECK(fronts_here > 0, "%s: no front with gather assembly", name);
    seen.fronts += fronts_here;
    printf("%s: n = %d, %d fronts, %d with gather maps, %lld map entries\n", name, b.n, (int)plan.fronts.size(), fronts_here, (long long)gmap.size());
}

}  // namespace

int main() {
    Seen seen;
    {   // two block arrows of nine cliques: each root front (m = 129) has eight children
        Builder b;
        for (int rep = 0; rep < 2; ++rep) b.arrow(std::vector<int32_t>(9, 100), 28);
        check_pattern("eight children", b, seen);
    }
    {   // small cliques hung on five separator unknowns beside the large ones: children of unequal update blocks
        Builder b;
        const std::vector<int32_t> sep = b.arrow({100, 100}, 28);
        for (int i = 0; i < 8; ++i) b.clique(b.cols(1), std::vector<int32_t>(sep.begin(), sep.begin() + 5));
        check_pattern("unequal children", b, seen);
    }
    {   // a separator of several pivot blocks whose children reach only its last rows, cliques of different sizes
        Builder b;
        b.arrow({100, 60, 75, 90}, 300);
        check_pattern("wide separator", b, seen);
    }
    {   // columns per workgroup: the launches of the L = 9 fine level of fem2d_P2 (count, max_m), and the forced values
        auto ct_of = [](int32_t count, int32_t max_m, int forced) {
            MfLaunch L{};
            L.count = count;
            L.max_m = max_m;
            return big_gather_ct(L, forced);
        };
        CHECK(ct_of(256, 168, 0) == 32 && ct_of(128, 232, 0) == 32, "levels of 256 and 128 fronts take 32 columns");
        CHECK(ct_of(64, 328, 0) == 16 && ct_of(32, 456, 0) == 16, "levels of 64 and 32 fronts take 16 columns");
        CHECK(ct_of(16, 648, 0) == 8 && ct_of(1, 1280, 0) == 8 && ct_of(2, 129, 0) == 8, "levels of few fronts take 8 columns");
        CHECK(ct_of(1, 129, 16) == 16 && ct_of(1, 129, 32) == 32 && ct_of(256, 168, 8) == 8, "a forced value holds");
        CHECK(ct_of(256, 168, 7) == 32 && ct_of(1, 129, 64) == 8, "any other forced value is ignored");
    }
    CHECK(seen.eight_children, "no gather front with %d children was built", GATHER_MAX_CHILD);
    CHECK(seen.unequal_children, "no gather front with children of unequal update blocks was built");
    CHECK(seen.partial_reach, "no child that reaches only some rows of its parent was built");
    if (g_failures) {
        fprintf(stderr, "%d failures\n", g_failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
