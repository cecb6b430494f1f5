// mf_launch_plan.hpp -- the launch plan of the numeric multifrontal LDL': which kernel every front of a symbolic plan goes to.
// Pure host C++ (no HIP), like mf_analysis.hpp: mf_numeric.hip includes it for MfSolver::analyze() / factor(), and the CPU
// checker build (oracle/csrc/mf_host.cpp) runs the same classification without a device, so that a test can pin, per launch,
// the kernel a hand-built pattern must get (tests/solver_gate_cases.py).
//
// The shape predicates of the launchers live here too (assembly kind, block-0 kind, backward variant): the launch code in
// mf_small.hpp / mf_big_inv.hpp / mf_big_assemble.hpp / mf_numeric.hip and the read-only report launch_rows() call the same
// functions.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_util.hpp"     // env_on
#include "mf_block_roles.hpp"
#include "mf_analysis.hpp"

namespace mgbhip {

struct MfLaunch {          // one kernel launch: a contiguous range of fronts of one size class
    int32_t first, count;
    int32_t cls;           // LDS working size (0 = large-front multi-workgroup path)
    int32_t max_m, max_k;  // largest front / pivot block in the range
    int32_t max_child = 0; // most children of a front in the range
    bool tiny = false;     // leaf fronts with m <= 16: 16-lanes-per-front kernels
    bool wave = false;     // m <= 48 and only small children: one wave per front (mf_factor_wave), packed LDS triangle
    bool inv = false;      // large fronts on the inverse-based path (W_j = L_jj^{-1} in the arena, pivots in dvec)
    bool iface = false;    // the interface front of a domain-decomposed system, alone in its launch: assembled, summed
                           // over ranks (MfSolver::iface_reduce), then factored redundantly on every rank
    int32_t grec_first = -1;   // gather launches: record of the launch's first front in the static gather maps (build_gather_maps)
};

constexpr int BIG_INV_MAX_M = 7000;     // work vectors of the single-workgroup solves stay in LDS
constexpr int GATHER_MAX_CHILD = 8;     // children whose index tables mf_big_gather keeps in LDS
constexpr int BIG_DIAG0_MIN_COUNT = 24; // fronts of a launch from which block 0 gets a launch of its own (mf_big_diag0)

// Environment switches of the launch plan (tools/README.md, switch table), read in one place by analyze().
struct MfSwitches {
    bool no_geo;            // MGBHIP_NO_GEO=1: no coordinates for the ordering (BFS level-set bisection)
    bool old_big;           // MGBHIP_OLD_BIG=1: substitution kernels for every large front
    bool merge_groups;      // off with MGBHIP_NO_MERGE_GROUPS=1
    bool packed_leaves;     // off with MGBHIP_NO_PACKED_LEAVES=1
    bool wave_small;        // off with MGBHIP_NO_WAVE_SMALL=1
    // Size gates of the two fastest kernel families (A/B switches of tests/test_gpu_solver.py).  Round 2 kept both off
    // systems of < 1024 unknowns after two creeping solves failed with them.  Round 3: all kernel selections are
    // equally backward stable on graded matrices (2.9e-13 componentwise) and the 27-problem sweep agrees with the
    // oracle without any gate (the 37-unknown case that motivated the wave gate: 5356 vs 5355 iterations), so the
    // one-wave kernel is ungated.  The inverse-based large-front path keeps its gate: without it config 4's phase I
    // (fem3d L=6, 9 000 iterations hugging the wall on a 145-unknown level) ends in "Initial centering failed" --
    // applying W = L_jj^{-1} is only forward stable in cond(L_jj), and such systems gain nothing from it.
    int64_t inv_min_n;      // MGBHIP_INV_MIN_N, default 1024
    int64_t wave_min_n;     // MGBHIP_WAVE_MIN_N, default 0
    bool gather_lds_maps;   // MGBHIP_GATHER_LDS_MAPS=1: mf_big_gather builds its index tables in LDS at every launch (the kernel
                            // before the static gather maps; the reference of tests/test_gpu_gather_maps.py)
    int gather_ct;          // MGBHIP_GATHER_CT=8/16/32: destination columns per workgroup of every mf_big_gather launch on the
                            // static maps (default 0: big_gather_ct chooses per launch)
    bool bwd_split;         // off with MGBHIP_BWD_SPLIT=0: one workgroup per front in every backward launch of the inverse-based
                            // path (bwd_inv_split; the reference of tests/test_gpu_backward_launches.py)
    int small_threads;      // MGBHIP_SMALL_THREADS=256/512/1024: that many threads per front in every mf_factor_small launch of a
                            // class > 32 (default 0: factor_small_threads chooses per launch; tests/test_gpu_small_threads.py)
    bool border_launches;   // MGBHIP_BORDER_LAUNCHES=1: a carried factorization and its sweep launch the 1 x 1 border front too
                            // (MfSolver::skips_border; the reference of tests/test_gpu_border_skip.py)
    int step_roles;         // MGBHIP_CHAIN_ORDER=legacy: the grids of mf_big_step and mf_big_gather in the layout ROLES_LEGACY (the chain
    int gather_roles;       // workgroup of a front dispatched after its tiles) instead of ROLES_CHAIN_FIRST (mf_block_roles.hpp); `step`
                            // / `gather`: chain-first in that kernel only (the per-kernel A/B of profiles/chain_order_ab.txt); unset or
                            // any other value: chain-first in both, the shipped configuration.  The same
                            // kernels and arithmetic either way; the reference of tests/test_gpu_chain_order.py
    static MfSwitches from_env() {
        auto num = [](const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; };
        const char* co = getenv("MGBHIP_CHAIN_ORDER");
        const std::string order = co ? co : "";
        const int step = (order == "legacy" || order == "gather") ? ROLES_LEGACY : ROLES_CHAIN_FIRST;
        const int gather = (order == "legacy" || order == "step") ? ROLES_LEGACY : ROLES_CHAIN_FIRST;
        return {env_on("MGBHIP_NO_GEO"), env_on("MGBHIP_OLD_BIG"), !env_on("MGBHIP_NO_MERGE_GROUPS"), !env_on("MGBHIP_NO_PACKED_LEAVES"),
                !env_on("MGBHIP_NO_WAVE_SMALL"), num("MGBHIP_INV_MIN_N", 1024), num("MGBHIP_WAVE_MIN_N", 0),
                env_on("MGBHIP_GATHER_LDS_MAPS"), (int)num("MGBHIP_GATHER_CT", 0), num("MGBHIP_BWD_SPLIT", 1) != 0,
                (int)num("MGBHIP_SMALL_THREADS", 0), env_on("MGBHIP_BORDER_LAUNCHES"), step, gather};
    }
};

using LevelLaunches = std::vector<std::vector<MfLaunch>>;

inline MfLaunch launch_of_range(const MfPlan& plan, MfLaunch L, int32_t first, int32_t count) {     // L's flags over [first, first + count)
    L.first = first; L.count = count;
    L.max_m = 0; L.max_k = 0; L.max_child = 0;
    for (int32_t t = first; t < first + count; ++t) {
        L.max_m = std::max(L.max_m, plan.fronts[t].m);
        L.max_k = std::max(L.max_k, plan.fronts[t].k);
        L.max_child = std::max(L.max_child, plan.fronts[t].nchild);
    }
    return L;
}

// Launches of one level are independent but share a stream: a straggler group (4 fronts of the next
// smaller class, 60 LDS-sized fronts beside 196 large ones) costs a full, latency-bound launch of
// 20-30 us.  Fold small groups into their neighbour:
//   (1) LDS-class fronts of a level whose bulk is on the large-front path join that path (it handles any m);
//   (2) an LDS class with few fronts joins the next larger LDS class of the level.
// Fronts are sorted by m inside a level, so a merge just extends the neighbour's range downwards.
inline void merge_straggler_groups(const MfPlan& plan, std::vector<MfLaunch>& G) {
    auto absorb = [&](size_t into, size_t from) {        // from == into - 1
        MfLaunch& A = G[into];
        const MfLaunch& B = G[from];
        A.first = B.first;
        A.count += B.count;
        A.max_k = std::max(A.max_k, B.max_k);
        A.max_child = std::max(A.max_child, B.max_child);
        G.erase(G.begin() + (long)from);
    };
    if (G.size() >= 2 && G.back().cls == 0 && G.back().inv) {
        int64_t lds_count = 0;
        bool ok = true;
        for (size_t g = 0; g + 1 < G.size(); ++g) { lds_count += G[g].count; ok = ok && !G[g].tiny && plan.fronts[G[g].first].m > 32; }
        if (ok && lds_count <= G.back().count)
            while (G.size() >= 2) absorb(G.size() - 1, G.size() - 2);
    }
    for (size_t g = 0; g + 1 < G.size();) {
        const bool next_lds = G[g + 1].cls != 0;
        if (next_lds && !G[g].tiny && (G[g].count < 256 || 4 * (int64_t)G[g].count < G[g + 1].count)) absorb(g + 1, g);
        else ++g;
    }
}

// The interface front gets a launch of its own on the large-front path (assemble / reduce / factor are separate
// kernels there, whatever its size): the launch that holds it is split around it.
inline void split_interface_front(const MfPlan& plan, LevelLaunches& levels, bool inv_allowed) {
    const int32_t q = plan.iface_front;
    for (auto& G : levels) {
        for (size_t g = 0; g < G.size(); ++g) {
            const MfLaunch L = G[g];
            if (q < L.first || q >= L.first + L.count) continue;
            std::vector<MfLaunch> out;
            if (q > L.first) out.push_back(launch_of_range(plan, L, L.first, q - L.first));
            MfLaunch I = launch_of_range(plan, L, q, 1);
            I.cls = 0; I.tiny = false; I.wave = false; I.iface = true;
            I.inv = (I.max_m <= BIG_INV_MAX_M && inv_allowed);
            out.push_back(I);
            if (q + 1 < L.first + L.count) out.push_back(launch_of_range(plan, L, q + 1, L.first + L.count - q - 1));
            G.erase(G.begin() + (long)g);
            G.insert(G.begin() + (long)g, out.begin(), out.end());
            break;
        }
    }
}

// Launches of fronts with m <= 48 whose children are all small (update block <= 8 x 8: the element leaves under a
// level-1 front, or no children) go to the one-wave-per-front kernel mf_factor_wave; with large children the
// 256-thread kernel's extend-add is faster and the launch stays there.
inline bool only_small_children(const MfPlan& plan, const MfLaunch& L) {
    for (int32_t q = L.first; q < L.first + L.count; ++q) {
        const Front& f = plan.fronts[q];
        for (int32_t c = 0; c < f.nchild; ++c) {
            const Front& ch = plan.fronts[plan.children[f.child_off + c]];
            if ((ch.m - ch.k) * (ch.m - ch.k) > 64) return false;
        }
    }
    return true;
}

// The factorization's launches, per tree level and leaves first: a function of the plan, the LDS cap, whether the
// inverse-based solves got their LDS (inv_ok) and the switches -- no device call.
inline LevelLaunches classify_launches(const MfPlan& plan, int32_t lds_cap, bool inv_ok, const MfSwitches& sw) {
    static const int32_t classes[] = {16, 32, 48, 64, 88, 128};
    const bool inv_allowed = inv_ok && !sw.old_big && plan.n >= sw.inv_min_n;
    const int32_t nlev = (int32_t)plan.level_ptr.size() - 1;
    LevelLaunches levels(nlev);
    for (int32_t l = 0; l < nlev; ++l) {
        int32_t i = plan.level_ptr[l];
        const int32_t end = plan.level_ptr[l + 1];
        while (i < end) {
            const int32_t m = plan.fronts[i].m;
            int32_t cls = 0;
            for (int32_t c : classes)
                if (m <= c && c <= lds_cap) { cls = c; break; }
            int32_t j = i;
            if (cls) {
                while (j < end && plan.fronts[j].m <= cls) ++j;
            } else {
                j = end;   // sorted by m: everything left in the level is large
            }
            MfLaunch L = launch_of_range(plan, MfLaunch{}, i, j - i);
            L.cls = cls;
            L.max_m = plan.fronts[j - 1].m;
            L.tiny = (l == 0 && cls == 16);     // leaves with m <= 16: 16 lanes per front
            L.inv = (cls == 0 && L.max_m <= BIG_INV_MAX_M && inv_allowed);
            levels[l].push_back(L);
            i = j;
        }
        if (sw.merge_groups) merge_straggler_groups(plan, levels[l]);
    }
    if (plan.iface_front >= 0) split_interface_front(plan, levels, inv_allowed);
    for (auto& lev : levels)
        for (auto& L : lev)
            L.wave = !L.tiny && L.cls && L.cls <= 48 && sw.wave_small && plan.n >= sw.wave_min_n && only_small_children(plan, L);
    return levels;
}

// the wave-per-front solve kernels do not depend on the LDS class: one launch per level
inline LevelLaunches merge_level_solves(const LevelLaunches& levels) {
    LevelLaunches solves(levels.size());
    for (size_t l = 0; l < levels.size(); ++l) {
        MfLaunch S{};
        for (auto& L : levels[l]) {
            if (!L.cls || L.tiny) { solves[l].push_back(L); continue; }
            if (S.count == 0) S = L;
            else {
                S.count += L.count;
                S.max_m = std::max(S.max_m, L.max_m);
                S.max_k = std::max(S.max_k, L.max_k);
            }
        }
        if (S.count) solves[l].insert(solves[l].begin(), S);
    }
    return solves;
}

// fronts of the large-front launches
inline std::vector<char> fronts_on_big_path(const MfPlan& plan, const LevelLaunches& levels) {
    std::vector<char> on_big_path(plan.fronts.size(), 0);
    for (auto& lev : levels)
        for (auto& L : lev)
            if (!L.cls)
                for (int32_t q = L.first; q < L.first + L.count; ++q) on_big_path[q] = 1;
    return on_big_path;
}

// Leaf fronts (m <= 16, the 16-lanes-per-front kernels) as packed lower triangles: m(m+1)/2 contiguous doubles
// instead of m*m, read back by their parents' extend-add and by the sweeps.  Only when every parent is an LDS
// front (the large-front assembly kernels read square children).  Whether the leaves of this plan can be packed.
inline bool leaf_fronts_packable(const MfPlan& plan, const LevelLaunches& levels, const std::vector<char>& on_big_path) {
    bool any = false;
    for (auto& lev : levels)
        for (auto& L : lev)
            if (L.tiny)
                for (int32_t q = L.first; q < L.first + L.count; ++q) {
                    const int32_t par = plan.fronts[q].parent;
                    if (par >= 0 && on_big_path[par]) return false;
                    any = true;
                }
    return any;
}

// ---- shape predicates of the launchers ------------------------------------------------------------------------
enum MfAssembly : int32_t { MF_ASM_NONE = 0, MF_ASM_GATHER = 1, MF_ASM_COLS = 2 };
enum MfBlock0 : int32_t { MF_B0_NA = 0, MF_B0_GATHER = 1, MF_B0_DIAG0 = 2, MF_B0_STEP0 = 3 };
enum MfBackward : int32_t { MF_BWD_NA = 0, MF_BWD_K8 = 1, MF_BWD_K16 = 2, MF_BWD_GENERAL = 3 };

// mf_big_gather: for every child the position of each front row in the child's update block
inline size_t big_gather_lds(const MfLaunch& L) { return (size_t)L.max_child * (size_t)L.max_m * sizeof(int32_t); }
// Assembly of the fronts of a large-front launch: the gathering kernel when it applies (few children, index table
// within 40 KB), the column-tiled one otherwise.  LDS fronts assemble inside their factorization kernel.
inline MfAssembly big_assembly_kind(const MfLaunch& L) {
    if (L.cls) return MF_ASM_NONE;
    if (L.max_child < 1 || L.max_child > GATHER_MAX_CHILD || big_gather_lds(L) > 40 * 1024) return MF_ASM_COLS;
    return MF_ASM_GATHER;
}
// Block 0 of the pivot chain on the inverse-based path (`inv`: L.inv and the solver is not in robust mode): an extra
// workgroup of the gather launch when that kernel applies; otherwise once per front up front (many fronts, or the
// interface front, whose sum over ranks is only complete after the assembly) or inside every tile of step 0 (few fronts).
inline MfBlock0 big_block0_kind(const MfLaunch& L, bool inv) {
    if (L.cls || !inv) return MF_B0_NA;
    if (!L.iface && big_assembly_kind(L) == MF_ASM_GATHER) return MF_B0_GATHER;
    return (L.iface || L.count >= BIG_DIAG0_MIN_COUNT) ? MF_B0_DIAG0 : MF_B0_STEP0;
}
// Backward sweep of an LDS launch: the register-resident variants for max_k <= 8 / <= 16, 0 = the general one
// (a 32-column variant holds 143 registers and loses more to occupancy on the 8192-front level than it gains)
inline int backward_small_kmax(const MfLaunch& L) { return L.max_k <= 8 ? 8 : (L.max_k <= 16 ? 16 : 0); }

// ---- threads per front of mf_factor_small ---------------------------------------------------------------------------
// Dynamic LDS of one workgroup: the front (a packed triangle for the classes >= 88) + the 8-column scaled panel.  The
// kernel's static arrays (child descriptors, one child's relative indices, pivot reciprocals) add SMALL_STATIC_LDS.
inline size_t factor_small_lds(int cls) {
    return (size_t)((cls >= 88 ? cls * (cls + 1) / 2 : cls * cls) + 8 * cls) * sizeof(double);
}
constexpr int SMALL_STATIC_LDS = 2112;
constexpr int CU_LDS_BYTES = 160 * 1024;    // LDS of a gfx950 compute unit
constexpr int SMALL_FILL_WAVES = 24;        // waves of one launch on a compute unit up to which wider workgroups won (below)
// One workgroup per front, and nothing in the kernel's arithmetic depends on its size: the fill, the extend-add, the update
// tiles and the write-back are dealt out to however many threads there are, in the same per-entry order.  256 threads are
// right for a launch that fills the device.  One that does not leaves the compute units' wave slots empty, and the same
// fronts finish sooner with more threads each.  A compute unit has per_cu workgroups of the launch at a time: ceil(count /
// compute units), and at most what the class's LDS lets it hold (class 128: two; a larger launch runs in rounds of that
// many).  The rule takes the widest of 256 / 512 / 1024 threads that keeps per_cu * threads / 64 <= SMALL_FILL_WAVES:
//   per_cu 1 (count <= 256 on the MI355X): 1024    2 and 3: 512    4 and more: 256
// which is, launch by launch, what three alternating passes over every LDS launch of the fem2d_P2 L = 9 ladder chose
// (profiles/small_threads_ab.txt: 1024 threads lose from per_cu = 2 on, 512 from per_cu = 4 on, by up to a factor of two;
// class 128 gains from 512 threads at 512 fronts, one round, and at 620, two).  `forced`: MGBHIP_SMALL_THREADS.  Classes
// <= 32 keep 64 / 128 threads.  The panel solve takes one row per thread, so a launch needs threads >= m - 1: 64 / 128 /
// 256 cover the classes 16 / 32 / 128 (static_assert below, MGB_REQUIRE in launch_factor_small).
inline int factor_small_threads(const MfLaunch& L, int compute_units, int forced = 0) {
    if (L.cls <= 16) return 64;
    if (L.cls <= 32) return 128;
    if (forced == 256 || forced == 512 || forced == 1024) return forced;
    const int64_t cu = std::max(compute_units, 1);
    const int64_t fit = std::max<int64_t>(1, CU_LDS_BYTES / (int64_t)(factor_small_lds(L.cls) + SMALL_STATIC_LDS));
    const int64_t per_cu = std::min(fit, ((int64_t)L.count + cu - 1) / cu);
    int threads = 256;
    while (threads < 1024 && per_cu * (2 * threads / 64) <= SMALL_FILL_WAVES) threads *= 2;
    return threads;
}
static_assert(16 - 1 <= 64 && 32 - 1 <= 128 && 128 - 1 <= 256, "mf_factor_small solves one panel row per thread");

// Destination columns per workgroup of mf_big_gather on the static maps: 8 (two per wave), doubled up to 32 while the launch
// keeps at least GATHER_MIN_WGS column workgroups.  A workgroup's fixed cost -- descriptor, map rows into LDS, two
// barriers, the tail of matrix entries -- is then shared by more columns; below that count the launch no longer fills the
// device (256 compute units, four resident workgroups each) and wider workgroups only lengthen it.  `forced`:
// MGBHIP_GATHER_CT.  Measured at L = 9 (profiles/gather_maps_ab.txt).
constexpr int GATHER_MIN_WGS = 768;
inline int big_gather_ct(const MfLaunch& L, int forced) {
    if (forced == 8 || forced == 16 || forced == 32) return forced;
    int ct = 8;
    while (ct < 32 && (int64_t)L.count * ((L.max_m + 2 * ct - 1) / (2 * ct)) >= GATHER_MIN_WGS) ct *= 2;
    return ct;
}

// Workgroups per front of a backward launch on the inverse-based path (mf_bwd_inv_split, mf_big_inv.hpp): the boundary
// product G[q] = sum_r A[r, q] x[r] of a front needs nothing of its own launch, so on levels of few fronts -- where one
// workgroup per front leaves most of the 256 compute units idle -- its pivot columns are dealt out to S workgroups; the
// last one to finish goes on with the block recurrence.  A pure function of the launch: as many workgroups as the device
// has compute units for (BWD_SPLIT_CUS / count), at least BWD_SPLIT_COLS columns each (one 4-column group per wave of a
// 1024-thread workgroup), BWD_SPLIT_MAX at most.  1 = one workgroup per front (mf_bwd_inv): also for launches whose
// fronts have a thin boundary (m - k <= BWD_THIN_BOUNDARY: one thread per column, the root front's border row).
constexpr int BWD_SPLIT_MAX = 16;
constexpr int BWD_SPLIT_CUS = 256;
constexpr int BWD_SPLIT_COLS = 64;
constexpr int BWD_THIN_BOUNDARY = 8;
inline int bwd_inv_split(int32_t count, int32_t max_k, int32_t max_m) {
    if (count < 1 || max_m - max_k <= BWD_THIN_BOUNDARY) return 1;
    return std::max(1, std::min({BWD_SPLIT_MAX, BWD_SPLIT_CUS / count, (max_k + BWD_SPLIT_COLS - 1) / BWD_SPLIT_COLS}));
}
// doubles of boundary-product scratch per front of a split launch
inline int32_t bwd_split_stride(int32_t max_k) { return (max_k + 1) & ~1; }
// What the split launches of a sweep need: per-front arrival counters (out[0]) and doubles of scratch (out[1]).  Launches
// of a sweep run one after the other, so all of them share one allocation, sized by the largest.
inline void bwd_split_scratch(const LevelLaunches& solves, int64_t out[2]) {
    out[0] = out[1] = 0;
    for (auto& lev : solves)
        for (auto& L : lev) {
            if (L.count == 0 || L.cls || !L.inv || bwd_inv_split(L.count, L.max_k, L.max_m) == 1) continue;
            out[0] = std::max<int64_t>(out[0], L.count);
            out[1] = std::max<int64_t>(out[1], (int64_t)L.count * bwd_split_stride(L.max_k));
        }
}

// ---- static gather maps of mf_big_gather ---------------------------------------------------------------------------
// What the gathering assembly needs of a front's children is a function of the symbolic plan alone, so analyze() lays it
// out once.  For every front of a launch whose assembly kind is MF_ASM_GATHER:
//   gmap[map_off + ch * m + r]   position of front row r in the update block of child ch, or -1 (the inverse of the
//                                child's relative index list: the table the kernel used to rebuild in LDS at every launch);
//   one GatherRec                where the maps start and, per child, where its update block starts in the arena
//                                (F_off + k m + k), its leading dimension m and its size m - k.
// Records are numbered in launch order; MfLaunch::grec_first is the record of a launch's first front, the others follow.
struct GatherRec {
    int64_t map_off;
    int64_t base[GATHER_MAX_CHILD];
    int32_t ld[GATHER_MAX_CHILD];
    int32_t bs[GATHER_MAX_CHILD];
};

inline void build_gather_maps(const MfPlan& plan, LevelLaunches& levels, std::vector<GatherRec>& recs, std::vector<int32_t>& gmap) {
    recs.clear();
    gmap.clear();
    for (auto& lev : levels)
        for (auto& L : lev) {
            L.grec_first = -1;
            if (L.count == 0 || big_assembly_kind(L) != MF_ASM_GATHER) continue;
            L.grec_first = (int32_t)recs.size();
            for (int32_t q = L.first; q < L.first + L.count; ++q) {
                const Front& f = plan.fronts[q];
                GatherRec R{};
                R.map_off = (int64_t)gmap.size();
                gmap.resize(gmap.size() + (size_t)f.nchild * (size_t)f.m, -1);
                for (int32_t c = 0; c < f.nchild; ++c) {            // f.nchild <= L.max_child <= GATHER_MAX_CHILD
                    const Front& ch = plan.fronts[plan.children[f.child_off + c]];
                    R.base[c] = ch.F_off + (int64_t)ch.k * ch.m + ch.k;
                    R.ld[c] = ch.m;
                    R.bs[c] = ch.m - ch.k;
                    int32_t* mp = gmap.data() + R.map_off + (int64_t)c * f.m;
                    for (int32_t j = 0; j < ch.m - ch.k; ++j) mp[plan.rel[ch.rel_off + j]] = j;
                }
                recs.push_back(R);
            }
        }
}

// ---- read-only report (mgbhip_solver_launches; mf_host_launches of the CPU checker build) ------------------------
// One row of MF_LAUNCH_ROW int32 per factorization launch, leaves first:
//   [0] tree level  [1] first  [2] count  [3] cls  [4] max_m  [5] max_k  [6] max_child
//   [7] tiny  [8] wave  [9] inv (as factor() runs it)  [10] iface  [11] fronts stored as packed triangles
//   [12] MfAssembly  [13] MfBlock0  [14] MfBackward of the level's LDS sweep  [15] 0
// Returns the number of launches; writes at most cap rows.
constexpr int MF_LAUNCH_ROW = 16;
inline int64_t launch_rows(const LevelLaunches& levels, const LevelLaunches& solves, bool leaf_packed, bool robust,
                           int32_t* out, int64_t cap) {
    int64_t n = 0;
    for (size_t l = 0; l < levels.size(); ++l) {
        int32_t bwd = 0;
        for (auto& S : solves[l])
            if (S.cls && !S.tiny) { const int km = backward_small_kmax(S); bwd = km == 8 ? MF_BWD_K8 : (km == 16 ? MF_BWD_K16 : MF_BWD_GENERAL); }
        for (auto& L : levels[l]) {
            if (n < cap && out) {
                const bool inv = L.inv && !robust;
                int32_t* r = out + n * MF_LAUNCH_ROW;
                r[0] = (int32_t)l; r[1] = L.first; r[2] = L.count; r[3] = L.cls; r[4] = L.max_m; r[5] = L.max_k; r[6] = L.max_child;
                r[7] = L.tiny; r[8] = L.wave; r[9] = inv; r[10] = L.iface; r[11] = L.tiny && leaf_packed;
                r[12] = big_assembly_kind(L); r[13] = big_block0_kind(L, inv); r[14] = (L.cls && !L.tiny) ? bwd : (int32_t)MF_BWD_NA; r[15] = 0;
            }
            ++n;
        }
    }
    return n;
}

}  // namespace mgbhip
