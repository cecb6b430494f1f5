// assembly_plan_check.cpp -- host check of the assembly-plan builder (csrc/assembly_plan.hpp) against brute force written
// differently: the pattern as a std::set of (row, col) pairs, the contribution lists as every (row, col, src) emitted in the
// documented order and then std::stable_sort-ed by (row, col), the slab layout as a running counter over the blocks, the
// panels as sub-blocks of a dense R.  The gate decisions are held to the literals of tests/gate_cases.py.  Stand-alone: built
// with plain g++ and -fsanitize=address,undefined by tests/test_assembly_plan_host.py; prints OK.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

#include "../../multigridbarrier.jl_amd/csrc/assembly_plan.hpp"

using namespace mgbhip;

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// R of one level, written row by row: row(a, node) = a * n + node, entries (column, value) in the order given.
struct Problem {
    const char* name;
    int p, nu;
    int64_t NE, m;
    uint32_t state_id_mask = 0;
    std::vector<std::vector<std::pair<int32_t, double>>> rows;
    std::vector<int32_t> ptr, col;
    std::vector<double> val;
    Problem(const char* nm, int p_, int nu_, int64_t NE_, int64_t m_) : name(nm), p(p_), nu(nu_), NE(NE_), m(m_), rows((size_t)(nu_ * NE_ * p_)) {}
    int64_t n() const { return NE * p; }
    void set(int a, int64_t node, std::vector<std::pair<int32_t, double>> entries) { rows[(size_t)(a * n() + node)] = std::move(entries); }
    bool identity_state(int a) const { return (state_id_mask >> a) & 1u; }
    // running counter over blocks (a <= b, row-major), elements, then the block's entries: p diagonal entries where both
    // states are identity-only on a selection level, p x p column-major otherwise
    int32_t diag_mask(bool selection) const {
        int32_t mask = 0;
        int blk = 0;
        for (int a = 0; a < nu; ++a)
            for (int b = a; b < nu; ++b, ++blk)
                if (selection && identity_state(a) && identity_state(b)) mask |= 1 << blk;
        return mask;
    }
    PlanShape shape(bool selection) {
        ptr.assign(1, 0); col.clear(); val.clear();
        for (auto& r : rows) {
            for (auto& cv : r) { col.push_back(cv.first); val.push_back(cv.second); }
            ptr.push_back((int32_t)col.size());
        }
        return PlanShape{NE, n(), m, p, nu, (int64_t)rows.size(), ptr.data(), col.data(), val.data(), (int64_t)col.size(), state_id_mask,
                         diag_mask(selection)};
    }
};

using Triple = std::tuple<int32_t, int32_t, int64_t>;      // (row, col, src)

// slab index of Hel_ab[i, j] of element e on a selection level, from the layout written out entry by entry
std::map<std::tuple<int, int, int64_t, int, int>, int64_t> slab_table(const Problem& P) {
    std::map<std::tuple<int, int, int64_t, int, int>, int64_t> T;
    int64_t next = 0;
    for (int a = 0; a < P.nu; ++a)
        for (int b = a; b < P.nu; ++b) {
            const bool diag = P.identity_state(a) && P.identity_state(b);
            for (int64_t e = 0; e < P.NE; ++e) {
                if (diag) {
                    for (int i = 0; i < P.p; ++i) T[{a, b, e, i, i}] = next++;
                } else {
                    for (int j = 0; j < P.p; ++j)
                        for (int i = 0; i < P.p; ++i) T[{a, b, e, i, j}] = next++;
                }
            }
        }
    return T;
}

// every contribution in the documented order; selection: element, then (state a, node i), then (state b, node j)
std::vector<Triple> brute_selection(const Problem& P) {
    const auto T = slab_table(P);
    std::vector<Triple> out;
    const int w = P.nu * P.p;
    for (int64_t e = 0; e < P.NE; ++e)
        for (int I = 0; I < w; ++I)
            for (int J = 0; J < w; ++J) {
                const int a = I / P.p, i = I % P.p, b = J / P.p, j = J % P.p;
                const auto& ri = P.rows[(size_t)(a * P.n() + e * P.p + i)];
                const auto& rj = P.rows[(size_t)(b * P.n() + e * P.p + j)];
                if (ri.empty() || rj.empty()) continue;
                if (P.identity_state(a) && P.identity_state(b) && i != j) continue;     // structural zero of a diagonal block
                const int64_t src = a <= b ? T.at({a, b, e, i, j}) : T.at({b, a, e, j, i});    // the lower blocks are the transposes
                out.emplace_back(ri[0].first, rj[0].first, src);
            }
    return out;
}

// general: element, then gj outer, gi inner over the concatenated per-state sorted column sets; src counts the blocks' entries
std::vector<Triple> brute_general(const Problem& P, std::vector<std::vector<int32_t>>* cols_of = nullptr) {
    std::vector<Triple> out;
    int64_t next = 0;
    for (int64_t e = 0; e < P.NE; ++e) {
        std::vector<int32_t> cols;
        for (int a = 0; a < P.nu; ++a) {
            std::set<int32_t> s;
            for (int r = 0; r < P.p; ++r)
                for (auto& cv : P.rows[(size_t)(a * P.n() + e * P.p + r)]) s.insert(cv.first);
            cols.insert(cols.end(), s.begin(), s.end());
            if (cols_of) cols_of->push_back(std::vector<int32_t>(s.begin(), s.end()));
        }
        for (size_t gj = 0; gj < cols.size(); ++gj)
            for (size_t gi = 0; gi < cols.size(); ++gi) out.emplace_back(cols[gi], cols[gj], next++);
    }
    return out;
}

struct Built {
    ElementColumns C;
    std::vector<int32_t> ptr, col;
    HostLists lists;
};

// element_columns + host_pattern + host_lists against the brute-force triples
Built check_against(Problem& P, bool selection, const std::vector<Triple>& emitted) {
    const PlanShape S = P.shape(selection);
    Built B;
    B.C = element_columns(S);
    CHECK(B.C.selection == selection, "%s: selection %d", P.name, (int)B.C.selection);
    host_pattern(S, B.C, B.ptr, B.col);
    std::set<std::pair<int32_t, int32_t>> pat;
    for (auto& t : emitted) pat.insert({std::get<0>(t), std::get<1>(t)});
    {
        std::vector<char> touched((size_t)P.m, 0);
        for (auto& rc : pat) touched[(size_t)rc.first] = 1;
        for (int64_t i = 0; i < P.m; ++i)
            if (!touched[(size_t)i]) pat.insert({(int32_t)i, (int32_t)i});     // untouched unknown: its diagonal slot
    }
    CHECK((int64_t)B.ptr.size() == P.m + 1 && B.ptr[0] == 0 && B.ptr.back() == (int32_t)B.col.size(), "%s: row pointers", P.name);
    CHECK(B.col.size() == pat.size(), "%s: nnz %zu, brute force %zu", P.name, B.col.size(), pat.size());
    if (B.col.size() == pat.size() && (int64_t)B.ptr.size() == P.m + 1) {
        size_t q = 0;
        for (auto& rc : pat) {      // the set iterates in CSR order
            CHECK(B.col[q] == rc.second && B.ptr[rc.first] <= (int32_t)q && (int32_t)q < B.ptr[rc.first + 1], "%s: pattern entry %zu", P.name, q);
            ++q;
        }
    }
    for (auto& rc : pat) CHECK(pat.count({rc.second, rc.first}) == 1, "%s: pattern not symmetric at (%d, %d)", P.name, rc.first, rc.second);
    B.lists = host_lists(S, B.C, B.ptr, B.col);
    std::vector<Triple> sorted = emitted;
    std::stable_sort(sorted.begin(), sorted.end(), [](const Triple& x, const Triple& y) {
        return std::make_pair(std::get<0>(x), std::get<1>(x)) < std::make_pair(std::get<0>(y), std::get<1>(y));
    });
    CHECK(B.lists.total == (int64_t)sorted.size() && B.lists.cidx.size() == sorted.size(), "%s: %lld summands, brute force %zu", P.name,
          (long long)B.lists.total, sorted.size());
    CHECK(B.lists.cptr.size() == B.col.size() + 1 && B.lists.cptr[0] == 0 && B.lists.cptr.back() == (int32_t)sorted.size(), "%s: list pointers",
          P.name);
    if (B.lists.cidx.size() == sorted.size() && B.lists.cptr.size() == pat.size() + 1) {
        size_t q = 0, t = 0;
        for (auto& rc : pat) {
            size_t len = 0;
            while (t + len < sorted.size() && std::get<0>(sorted[t + len]) == rc.first && std::get<1>(sorted[t + len]) == rc.second) ++len;
            CHECK(B.lists.cptr[q] == (int32_t)t && B.lists.cptr[q + 1] == (int32_t)(t + len), "%s: list of (%d, %d) has length %d, brute force %zu", P.name,
                  rc.first, rc.second, B.lists.cptr[q + 1] - B.lists.cptr[q], len);
            for (size_t k = 0; k < len; ++k)
                CHECK((int64_t)B.lists.cidx[t + k] == std::get<2>(sorted[t + k]), "%s: summand %zu of (%d, %d): %d, brute force %lld", P.name, k, rc.first,
                      rc.second, B.lists.cidx[t + k], (long long)std::get<2>(sorted[t + k]));
            t += len;
            ++q;
        }
    }
    CHECK(B.lists.long_lists == (!B.col.empty() && B.lists.total / (int64_t)B.col.size() > 48), "%s: long_lists", P.name);
    return B;
}

int32_t position(const Built& B, int32_t row, int32_t c) {       // CSR position of (row, c) or -1
    for (int32_t q = B.ptr[row]; q < B.ptr[row + 1]; ++q)
        if (B.col[q] == c) return q;
    return -1;
}
std::vector<int32_t> list_of(const Built& B, int32_t row, int32_t c) {
    const int32_t q = position(B, row, c);
    if (q < 0) return {};
    return std::vector<int32_t>(B.lists.cidx.begin() + B.lists.cptr[q], B.lists.cidx.begin() + B.lists.cptr[q + 1]);
}

// -- selection, p = 2, nu = 2, N = 3: fem1d.  u: Dirichlet ends (nodes 0 and 5) have empty rows, the interior vertices are
//    columns 0 and 1; s: one column per broken node (2 .. 7); column 8 is touched by no element.
void selection_fem1d() {
    Problem P("selection fem1d", 2, 2, 3, 9);
    P.set(0, 1, {{0, 1.0}}); P.set(0, 2, {{0, 1.0}});
    P.set(0, 3, {{1, 1.0}}); P.set(0, 4, {{1, 1.0}});
    for (int node = 0; node < 6; ++node) P.set(1, node, {{2 + node, 1.0}});
    const Built B = check_against(P, true, brute_selection(P));
    CHECK(B.C.cmax == 2 && B.C.ctmax == 4, "cmax %d ctmax %lld", B.C.cmax, (long long)B.C.ctmax);
    CHECK(B.ptr[9] - B.ptr[8] == 1 && B.col[B.ptr[8]] == 8, "the untouched column keeps its diagonal slot");
    CHECK(B.lists.cptr[B.ptr[8] + 1] == B.lists.cptr[B.ptr[8]], "... with an empty list");
    // column 0 is node 1 of element 0 and node 0 of element 1: Hel_uu[1, 1] of element 0 (slab 0 * 4 + 1 * 2 + 1 = 3), then
    // Hel_uu[0, 0] of element 1 (slab 1 * 4 = 4)
    CHECK((list_of(B, 0, 0) == std::vector<int32_t>{3, 4}), "list of (0, 0) in element order");
    CHECK(position(B, 0, 1) >= 0 && list_of(B, 0, 1) == std::vector<int32_t>{4 + 1 * 2 + 0}, "(0, 1): Hel_uu[0, 1] of element 1");
}

// -- selection, nu = 3, states 1 and 2 identity-only: their three blocks are diagonal and stored compactly.  p = 2, N = 2;
//    u: node 0 -> column 0, nodes 1 and 2 -> column 1, node 3 Dirichlet; states 1 / 2: columns 2 .. 5 / 6 .. 9.
//    Layout: blocks (0,0), (0,1), (0,2) of N p p = 8 doubles at 0, 8, 16; (1,1), (1,2), (2,2) of N p = 4 at 24, 28, 32.
void selection_identity_states() {
    Problem P("selection identity states", 2, 3, 2, 10);
    P.state_id_mask = 0b110;
    P.set(0, 0, {{0, 1.0}}); P.set(0, 1, {{1, 1.0}}); P.set(0, 2, {{1, 1.0}});
    for (int node = 0; node < 4; ++node) { P.set(1, node, {{2 + node, 1.0}}); P.set(2, node, {{6 + node, 1.0}}); }
    CHECK(P.diag_mask(true) == 0b111000, "diag mask %d", P.diag_mask(true));
    const Built B = check_against(P, true, brute_selection(P));
    CHECK(position(B, 2, 3) < 0 && position(B, 3, 2) < 0, "off-diagonal slot of an identity block (1, 1) is absent");
    CHECK(position(B, 2, 7) < 0 && position(B, 7, 2) < 0, "off-diagonal slot of an identity block (1, 2) is absent");
    CHECK((list_of(B, 2, 6) == std::vector<int32_t>{28}), "compact block (1, 2), element 0, node 0: sel_off + e p + i");
    CHECK((list_of(B, 5, 9) == std::vector<int32_t>{28 + 1 * 2 + 1}), "compact block (1, 2), element 1, node 1");
    CHECK((list_of(B, 6, 2) == std::vector<int32_t>{28}), "a > b reads the transposed slot");
    CHECK((list_of(B, 1, 2) == std::vector<int32_t>{8 + (0 * 2 + 0) * 2 + 1}), "(u node 1, s node 0) of element 0: Hel_01[1, 0]");
    CHECK((list_of(B, 2, 1) == std::vector<int32_t>{8 + (0 * 2 + 0) * 2 + 1}), "a > b: Hel_10[0, 1] = Hel_01[1, 0]");
    CHECK((list_of(B, 0, 3) == std::vector<int32_t>{8 + (0 * 2 + 1) * 2 + 0}), "Hel_01[0, 1] of element 0");
}

// -- general, p = 2, nu = 2, N = 4, m = 6.  Element 2 has no u column; column 5 is touched by nobody; node 3 of state s also
//    reaches the u column 2 (element 1 holds column 2 in both states: four summands of (2, 2) from one element); node 6 of
//    state u has two entries in column 2 (summed in the panel).
Problem general_problem() {
    Problem P("general", 2, 2, 4, 6);
    P.set(0, 0, {{0, 0.5}, {1, 0.25}}); P.set(0, 1, {{1, 0.75}});
    P.set(0, 2, {{1, 0.5}, {2, 0.5}}); P.set(0, 3, {{2, 1.0}});
    P.set(0, 6, {{2, 0.3}, {2, 0.2}}); P.set(0, 7, {{0, 0.6}});
    P.set(1, 0, {{3, 0.9}}); P.set(1, 1, {{3, 0.8}});
    P.set(1, 2, {{3, 0.7}, {4, 0.1}}); P.set(1, 3, {{2, 0.05}, {4, 0.6}});
    P.set(1, 4, {{4, 0.5}}); P.set(1, 5, {{4, 0.4}});
    P.set(1, 6, {{3, 0.35}}); P.set(1, 7, {{4, 0.45}});
    return P;
}

void general_level() {
    Problem P = general_problem();
    std::vector<std::vector<int32_t>> cols_of;
    const std::vector<Triple> emitted = brute_general(P, &cols_of);
    const Built B = check_against(P, false, emitted);
    const ElementColumns& C = B.C;
    // column sets
    CHECK(C.ecol_ptr.size() == cols_of.size() + 1, "ecol_ptr size");
    int64_t slab = 0, ctmax = 1;
    int32_t cmax = 1;
    for (int64_t e = 0; e < P.NE; ++e) {
        int64_t ct = 0;
        for (int a = 0; a < P.nu; ++a) {
            const size_t k = (size_t)(e * P.nu + a);
            const std::vector<int32_t> got(C.ecols.begin() + C.ecol_ptr[k], C.ecols.begin() + C.ecol_ptr[k + 1]);
            CHECK(got == cols_of[k], "column set of element %lld state %d", (long long)e, a);
            ct += (int64_t)cols_of[k].size();
            cmax = std::max(cmax, (int32_t)cols_of[k].size());
        }
        CHECK(C.eoff[(size_t)e] == slab, "eoff[%lld]", (long long)e);
        slab += ct * ct;
        ctmax = std::max(ctmax, ct);
    }
    CHECK(C.ecol_ptr[2 * 2 + 1] == C.ecol_ptr[2 * 2], "element 2 has an empty u column set");
    CHECK(C.eoff[(size_t)P.NE] == slab && C.slab_est == slab && C.ctmax == ctmax && C.cmax == cmax, "slab %lld ctmax %lld cmax %d",
          (long long)C.slab_est, (long long)C.ctmax, C.cmax);
    CHECK(B.ptr[6] - B.ptr[5] == 1 && B.col[B.ptr[5]] == 5, "the untouched column keeps its diagonal slot");
    // the lists are a permutation of the slab, each in ascending slab order (element, then gj outer, gi inner)
    std::vector<int32_t> seen((size_t)slab, 0);
    for (int32_t s : B.lists.cidx)
        if (s >= 0 && s < slab) seen[(size_t)s]++;
    CHECK(B.lists.total == slab && std::all_of(seen.begin(), seen.end(), [](int32_t c) { return c == 1; }), "lists are a permutation of the slab");
    for (size_t q = 0; q + 1 < B.lists.cptr.size(); ++q)
        for (int32_t t = B.lists.cptr[q] + 1; t < B.lists.cptr[q + 1]; ++t) CHECK(B.lists.cidx[t - 1] < B.lists.cidx[t], "list %zu not in slab order", q);
    // element 1 has the columns [1, 2 | 2, 3, 4] at eoff 9: (2, 2) gets (gi, gj) = (1, 1), (2, 1), (1, 2), (2, 2) from it,
    // then (0, 0) from element 3 ([0, 2 | 3, 4] at 9 + 25 + 1 = 35: gi = gj = 1)
    CHECK((list_of(B, 2, 2) == std::vector<int32_t>{9 + 1 + 5 * 1, 9 + 2 + 5 * 1, 9 + 1 + 5 * 2, 9 + 2 + 5 * 2, 35 + 1 + 4 * 1}), "list of (2, 2)");
    // panels against the dense R
    std::vector<double> Rd((size_t)(P.rows.size() * P.m), 0.0);
    for (size_t r = 0; r < P.rows.size(); ++r)
        for (auto& cv : P.rows[r]) Rd[r * (size_t)P.m + (size_t)cv.first] += cv.second;
    const std::vector<double> panels = element_panels(P.shape(false), C);
    CHECK(panels.size() == (size_t)P.p * C.ecols.size(), "panel doubles");
    for (int64_t e = 0; e < P.NE && panels.size() == (size_t)P.p * C.ecols.size(); ++e)
        for (int a = 0; a < P.nu; ++a) {
            const int32_t o = C.ecol_ptr[(size_t)(e * P.nu + a)], c = C.ecol_ptr[(size_t)(e * P.nu + a) + 1] - o;
            for (int32_t ia = 0; ia < c; ++ia)
                for (int r = 0; r < P.p; ++r)
                    CHECK(panels[(size_t)P.p * o + r + (size_t)P.p * ia] == Rd[(size_t)(a * P.n() + e * P.p + r) * (size_t)P.m + (size_t)C.ecols[o + ia]],
                          "panel (%lld, %d)[%d, %d]", (long long)e, a, r, ia);
        }
    {
        const int32_t o = C.ecol_ptr[3 * 2 + 0];      // element 3, state u: columns [0, 2]; node 6 has 0.3 + 0.2 in column 2
        CHECK(panels[(size_t)P.p * o + 0 + (size_t)P.p * 1] == 0.3 + 0.2, "entries of one row in one column are summed");
    }
    // upper positions of this pattern
    for (int row_major = 0; row_major < 2; ++row_major) {
        const std::vector<int32_t> up = upper_positions(B.ptr, B.col, P.m, row_major != 0);
        std::set<int32_t> want;
        std::vector<std::pair<int32_t, int32_t>> rc(B.col.size());
        for (int64_t i = 0; i < P.m; ++i)
            for (int32_t q = B.ptr[i]; q < B.ptr[i + 1]; ++q) {
                rc[(size_t)q] = {(int32_t)i, B.col[q]};
                if (B.col[q] >= i) want.insert(q);
            }
        CHECK(std::set<int32_t>(up.begin(), up.end()) == want && up.size() == want.size(), "upper positions (row_major %d) are not the upper triangle", row_major);
        for (size_t k = 1; k < up.size(); ++k) {
            if (row_major) CHECK(up[k - 1] < up[k], "row-major order at %zu", k);
            else CHECK(std::make_pair(rc[up[k - 1]].second, rc[up[k - 1]].first) < std::make_pair(rc[up[k]].second, rc[up[k]].first), "(col, row) order at %zu", k);
        }
    }
}

// -- m = 0 and m = 1
void tiny_levels() {
    {
        Problem P("m0", 2, 2, 2, 0);          // no unknown: every row empty
        const Built B = check_against(P, true, brute_selection(P));
        CHECK(B.ptr == std::vector<int32_t>{0} && B.col.empty() && B.lists.cptr == std::vector<int32_t>{0} && B.lists.total == 0, "m = 0");
        CHECK(B.C.ecols.empty() && B.C.cmax == 1 && B.C.ctmax == 1 && B.C.slab_est == 0, "m = 0: column sets");
        CHECK(element_panels(P.shape(true), B.C).empty() && upper_positions(B.ptr, B.col, 0, false).empty(), "m = 0: panels, upper positions");
        CHECK(!decide_accumulate(2, 2, 2, 0, false, 1, 0).acc, "m = 0 never accumulates");
        std::vector<int32_t> ptr, col;
        dense_pattern(0, ptr, col);
        CHECK(ptr == std::vector<int32_t>{0} && col.empty(), "dense pattern of m = 0");
    }
    {
        Problem P("m1 untouched", 2, 2, 2, 1);
        const Built B = check_against(P, true, brute_selection(P));
        CHECK((B.ptr == std::vector<int32_t>{0, 1}) && B.col == std::vector<int32_t>{0} && B.lists.total == 0, "m = 1, no entry of R");
    }
    {
        Problem P("m1 selection", 2, 2, 2, 1);
        for (int a = 0; a < 2; ++a)
            for (int node = 0; node < 4; ++node) P.set(a, node, {{0, 1.0}});
        const Built B = check_against(P, true, brute_selection(P));
        CHECK(B.col.size() == 1 && B.lists.total == 2 * 16, "m = 1 selection: %lld summands", (long long)B.lists.total);
    }
    {
        Problem P("m1 general", 2, 2, 2, 1);
        for (int a = 0; a < 2; ++a)
            for (int node = 0; node < 4; ++node) P.set(a, node, {{0, 0.5}});
        const Built B = check_against(P, false, brute_general(P));
        CHECK(B.col.size() == 1 && B.lists.total == 2 * 4 && B.C.slab_est == 8, "m = 1 general: %lld summands", (long long)B.lists.total);
        CHECK((upper_positions(B.ptr, B.col, 1, false) == std::vector<int32_t>{0}), "m = 1: upper positions");
    }
    {
        std::vector<int32_t> ptr, col;
        dense_pattern(3, ptr, col);
        CHECK((ptr == std::vector<int32_t>{0, 3, 6, 9}) && (col == std::vector<int32_t>{0, 1, 2, 0, 1, 2, 0, 1, 2}), "dense pattern of m = 3");
        // row-major CSR positions 0 1 2 / 4 5 / 8; column-major: (0,0) (0,1) (1,1) (0,2) (1,2) (2,2)
        CHECK((upper_positions(ptr, col, 3, true) == std::vector<int32_t>{0, 1, 2, 4, 5, 8}), "dense upper positions, row-major");
        CHECK((upper_positions(ptr, col, 3, false) == std::vector<int32_t>{0, 1, 4, 2, 5, 8}), "dense upper positions, column-major");
    }
}

// -- the gates.  Scalar shapes (NE, m, ctmax, slab_est) of the levels of tests/gate_cases.py (fem1d: p = 2, nu = 2), expected
//    decisions from its literals: `acc` and `acc_split` of the level's `expect`, nsplit = 5 at m384 from the case's comment.
void gates() {
    struct Row { const char* name; int64_t NE, m, ctmax, slab_est; bool acc; int split; };
    const Row rows[] = {
        {"proj_small/m2", 64, 2, 2, 256, true, 1},            // slab_est 256 >= 16 mt = 48
        {"proj_small/m16", 64, 16, 4, 548, false, 1},         // slab_est < 16 mt = 2176
        {"proj_small/m17", 64, 17, 12, 7588, true, 1},        // slab_est >= 16 mt = 2448
        {"proj_wide/m384", 8, 384, 49, 19111, false, 5},      // nsplit = 5 > 4
        {"proj_wide/m385", 8, 385, 196, 304202, false, 0},    // m > 384
        {"acc_ne_max/m2", 65536, 2, 2, 262144, true, 1},      // NE = 65536 still accumulates
        {"gather_two_stage/m4", 65600, 4, 2, 213200, false, 1},   // NE > 65536 does not
        {"prolong_rows/rows65", 300, 80, 68, 560458, true, 1},
    };
    for (const Row& r : rows) {
        const AccumulateDecision A = decide_accumulate(2, 2, r.NE, r.m, false, r.ctmax, r.slab_est);
        CHECK(A.acc == r.acc, "%s: acc %d", r.name, (int)A.acc);
        if (r.split) CHECK(A.split == r.split, "%s: split %d", r.name, A.split);
        CHECK(A.tri == r.m * (r.m + 1) / 2 && (int64_t)A.chunk * A.split >= A.tri && A.waves >= 8, "%s: chunks cover the triangle", r.name);
        CHECK(!decide_accumulate(2, 2, r.NE, r.m, true, r.ctmax, r.slab_est).acc, "%s: a selection level never accumulates", r.name);
    }
    // two-stage gather: mean list length above 2048 (integer mean, as `mean > 2048` of gate_cases.restated_plan)
    {
        const std::vector<int32_t> at{0, 2048}, above{0, 2049};
        const GatherChunks a = decide_gather_chunks(at.data(), 1), b = decide_gather_chunks(above.data(), 1);
        CHECK(a.gather_chunk == 0 && a.gather_nchunk == 0, "mean 2048: one-stage gather");
        CHECK(b.gather_chunk == 1024 && b.gather_nchunk == 3, "mean 2049: chunks of 1024, %d x %d", b.gather_nchunk, b.gather_chunk);
        // gather_two_stage/m4: the slack list of 65 600 = 64 x 1025 summands beside three u lists: gather_chunk=1025, gather_nchunk=64
        const std::vector<int32_t> two{0, 65600, 65600 + 16401, 65600 + 16401 + 16399, 65600 + 16401 + 16399 + 16400};
        const GatherChunks c = decide_gather_chunks(two.data(), 4);
        CHECK(c.gather_chunk == 1025 && c.gather_nchunk == 64, "maxlen 64 x 1025: %d x %d", c.gather_nchunk, c.gather_chunk);
        CHECK(decide_gather_chunks(at.data(), 0).gather_nchunk == 0, "no entry, no chunks");
    }
}

}  // namespace

int main() {
    selection_fem1d();
    selection_identity_states();
    general_level();
    tiny_levels();
    gates();
    if (g_failures) {
        fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
