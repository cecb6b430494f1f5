// mf_numeric.hip -- numeric phase of the multifrontal LDL' factorization on gfx950: the MfSolver methods.
//
// `solve(symmetric(H), g)` in the reference is CHOLMOD's Cholesky with an LDL' fallback when
// H is not numerically positive definite (Julia's `\` for Symmetric sparse matrices,
// src/utils.jl:142-145).  One square-root-free LDL' (fixed ordering, no pivoting -- like
// CHOLMOD's) covers both: for SPD input it is the Cholesky factor column-scaled, for a
// numerically indefinite H it still returns the direction the reference would get, and the
// Newton loop's lambda^2 <= 0 test (src/newton.jl:257-271) decides.  Only an exactly zero or
// non-finite pivot is an error.
//
// The kernels and their host launchers live in the family headers, all part of this one translation unit
// (mf_device.hpp says why): mf_small.hpp (fronts factored out of LDS, m <= lds_cap), mf_big_subst.hpp and
// mf_big_inv.hpp (the two generations of multi-workgroup kernels for larger fronts), mf_big_assemble.hpp (the assembly
// of those fronts, shared by both generations).  Here: analyze() turns the
// symbolic plan into per-level launch lists (the classification itself is host-only code in mf_launch_plan.hpp, shared with
// the CPU checker build), factor() / forward_pass() / backward_pass() walk them.
#include <hip/hip_runtime.h>

#include <cstdio>

#include <algorithm>
#include <cstdlib>

#include "../../include/mgbhip.h"
#include "mf_solver.hpp"
#include "mf_device.hpp"
#include "mf_small.hpp"
#include "mf_big_subst.hpp"
#include "mf_big_inv.hpp"
#include "mf_big_assemble.hpp"

namespace mgbhip {

namespace {

// dynamic LDS above 64 KB needs an explicit opt-in: each bound is the kernel's own size function at its cap
int32_t query_lds_cap() {          // largest front class of mf_factor_small; the 64 KB classes if the opt-in is refused
    if (hipFuncSetAttribute((const void*)mf_factor_small<8, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)factor_small_lds(128)) == hipSuccess)
        return 128;
    (void)hipGetLastError();
    return 88;
}
bool query_inv_optin() {           // the single-workgroup solves of the inverse-based path at BIG_INV_MAX_M (148 960 B of the 160 KB)
    if (hipFuncSetAttribute((const void*)mf_fwd_inv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwd_inv_lds(BIG_INV_MAX_M)) == hipSuccess &&
        hipFuncSetAttribute((const void*)mf_bwd_inv, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)bwd_inv_lds(BIG_INV_MAX_M, BIG_INV_MAX_M)) == hipSuccess &&
        hipFuncSetAttribute((const void*)mf_bwd_inv_split, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)bwd_inv_lds(BIG_INV_MAX_M, BIG_INV_MAX_M)) == hipSuccess)
        return true;
    (void)hipGetLastError();
    return false;
}

// update-vector gather lists of the large fronts (forward solve): for every local index the entries of
// the children's update vectors that land on it, in child order (the summation order of the extend-add)
void build_gather_lists(const MfPlan& plan, const std::vector<char>& on_big_path, std::vector<FrontDev>& fd,
                        std::vector<int64_t>& ug_ptr, std::vector<int64_t>& ug_src) {
    for (int32_t i = 0; i < (int32_t)plan.fronts.size(); ++i) {
        const Front& f = plan.fronts[i];
        if (!on_big_path[i]) continue;
        fd[i].ug_off = (int64_t)ug_ptr.size();
        std::vector<int32_t> cnt((size_t)f.m + 1, 0);
        for (int32_t c = 0; c < f.nchild; ++c) {
            const Front& ch = plan.fronts[plan.children[f.child_off + c]];
            for (int32_t j = 0; j < ch.m - ch.k; ++j) cnt[plan.rel[ch.rel_off + j] + 1]++;
        }
        const int64_t base = (int64_t)ug_src.size();
        std::vector<int64_t> pos((size_t)f.m + 1);
        pos[0] = base;
        for (int32_t j = 0; j < f.m; ++j) pos[j + 1] = pos[j] + cnt[j + 1];
        ug_ptr.insert(ug_ptr.end(), pos.begin(), pos.end());
        ug_src.resize((size_t)pos[f.m]);
        std::vector<int64_t> fill(pos.begin(), pos.end() - 1);
        for (int32_t c = 0; c < f.nchild; ++c) {
            const Front& ch = plan.fronts[plan.children[f.child_off + c]];
            for (int32_t j = 0; j < ch.m - ch.k; ++j) ug_src[(size_t)fill[plan.rel[ch.rel_off + j]]++] = ch.u_off + j;
        }
    }
    if (ug_ptr.empty()) ug_ptr.push_back(0);
    if (ug_src.empty()) ug_src.push_back(0);
}

// Leaf fronts as packed lower triangles where the plan allows it (leaf_fronts_packable, mf_launch_plan.hpp): marks them
// in the device descriptors.  Returns whether any front was packed.
bool pack_leaf_fronts(const MfPlan& plan, const LevelLaunches& levels, const std::vector<char>& on_big_path,
                      std::vector<FrontDev>& fd) {
    if (!leaf_fronts_packable(plan, levels, on_big_path)) return false;
    for (auto& lev : levels)
        for (auto& L : lev)
            if (L.tiny)
                for (int32_t q = L.first; q < L.first + L.count; ++q) fd[q].packed = 1;
    return true;
}

// a_dst for the kernels that keep the front as a packed LDS triangle.  Leaf fronts with m <= 16 (mf_factor_tiny)
// scatter A with column stride 16: 136 LDS doubles per front instead of 256, which doubles the resident workgroups
// of that kernel; mf_factor_wave packs with stride 32 or 48; the packed classes of mf_factor_small (>= 88) with the
// front's own m.
std::vector<int32_t> remap_a_dst(const MfPlan& plan, const LevelLaunches& levels) {
    std::vector<int32_t> ad(plan.a_dst);
    for (auto& lev : levels)
        for (auto& L : lev) {
            const int stride = L.tiny ? 16 : (L.wave ? (L.cls <= 32 ? 32 : 48) : 0);
            const bool lds_front = L.cls >= 88 && !stride;
            if (!stride && !lds_front) continue;
            for (int32_t q = L.first; q < L.first + L.count; ++q) {
                const Front& f = plan.fronts[q];
                const int32_t sd = lds_front ? f.m : stride;
                for (int32_t t = 0; t < f.a_cnt; ++t) {
                    const int32_t d = plan.a_dst[f.a_off + t], lu = d % f.m, lv = d / f.m;      // row lu >= column lv
                    ad[f.a_off + t] = lv * sd - lv * (lv - 1) / 2 + (lu - lv);
                }
            }
        }
    return ad;
}

void dump_plan(const MfPlan& plan, const LevelLaunches& levels) {          // MGBHIP_DEBUG >= 2
    fprintf(stderr, "[mgbhip] solver plan: n=%lld fronts=%d levels=%d arena=%.1f MB\n", (long long)plan.n, (int)plan.fronts.size(),
            (int)levels.size(), plan.arena_doubles * 8e-6);
    for (size_t l = 0; l < levels.size(); ++l)
        for (auto& L : levels[l]) {
            double sm = 0, sk = 0, fl = 0;
            for (int32_t q = L.first; q < L.first + L.count; ++q) {
                const Front& f = plan.fronts[q];
                sm += f.m; sk += f.k;
                for (int c = 0; c < f.k; ++c) fl += (double)(f.m - c) * (f.m - c);
            }
            fprintf(stderr, "[mgbhip]   level %2d cls %3d count %7d max_m %4d max_k %4d avg_m %6.1f avg_k %6.1f Mflop %8.2f\n",
                    (int)l, L.cls, L.count, L.max_m, L.max_k, sm / L.count, sk / L.count, fl * 1e-6);
        }
}

// per-tree-level stage timers (MGBHIP_LEVEL_TIMING=1): "fac_lvNN", "fwd_lvNN", "bwd_lvNN"
StageTimers g_dummy_timers;
struct LevelScope {
    char nm[32];
    StageScope scope;
    static StageTimers& timers_or_dummy(StageTimers* t) {
        static const bool on = env_on("MGBHIP_LEVEL_TIMING");
        return (t && on) ? *t : g_dummy_timers;
    }
    LevelScope(StageTimers* t, const char* sweep, int level)
        : scope(timers_or_dummy(t), (snprintf(nm, sizeof(nm), "%s_lv%02d", sweep, level), nm)) {}
};

}  // namespace

// plan arrays that no later step of analyze() changes, and the work buffers sized by the plan
void MfSolver::upload_plan(hipStream_t st) {
    d_front_idx.upload(plan.front_idx, st);
    d_children.upload(plan.children, st);
    d_rel.upload(plan.rel, st);
    d_a_src.upload(plan.a_src, st);
    d_a_colptr.upload(plan.a_colptr, st);
    d_arena.alloc((size_t)std::max<int64_t>(plan.arena_doubles, 1));
    d_uvec.alloc((size_t)std::max<int64_t>(plan.uvec_doubles, 1));
    d_y.alloc((size_t)plan.n + 1);            // + the border unknown
    y_zero = y_border_one = status_zero = leaf_zero = false;
    d_bx.alloc((size_t)plan.n + 1);
    d_xx.alloc((size_t)plan.n + 1);
    {
        const double one = 1.0;
        d_one.upload(&one, 1, st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
    }
    d_tbig.alloc(plan.front_idx.size() ? plan.front_idx.size() : 1);
    d_tsol.alloc(plan.front_idx.size() ? plan.front_idx.size() : 1);
    d_dvec.alloc(plan.front_idx.size() ? plan.front_idx.size() : 1);
    d_status.alloc(2);           // [0] factorization, [1] leaf pivots of a condensing f2
    d_status.zero(st);
}

void MfSolver::analyze(int64_t n, const int32_t* rowptr, const int32_t* colidx, hipStream_t st,
                       const double* coords, int dim, bool protect_peeled, const int32_t* top, int64_t ntop) {
    const MfSwitches sw = MfSwitches::from_env();
    MfOptions opt;
    opt.protect_peeled = protect_peeled;
    opt.top = top;
    opt.ntop = ntop;
    opt.border = true;          // every system is factored bordered (mf_analysis.hpp): the Newton solve needs no forward sweep
    mf_analyze(n, rowptr, colidx, opt, plan, sw.no_geo ? nullptr : coords, dim);
    const int32_t nf = (int32_t)plan.fronts.size();
    std::vector<FrontDev> fd(nf);
    for (int32_t i = 0; i < nf; ++i) {
        const Front& f = plan.fronts[i];
        fd[i] = FrontDev{f.k, f.m, f.nchild, f.a_cnt, f.F_off, f.idx_off, f.u_off, f.child_off, f.rel_off, f.a_off, f.acol_off, -1, 0, 0};
    }
    upload_plan(st);

    lds_cap = query_lds_cap();
    // the inverse-based large-front path needs the > 64 KB dynamic LDS opt-in for its single-workgroup solves
    const bool inv_ok = !sw.old_big && query_inv_optin();
    level_launches = classify_launches(plan, lds_cap, inv_ok, sw);
    level_solves = merge_level_solves(level_launches);
    uses_inv = false;
    const std::vector<char> on_big_path = fronts_on_big_path(plan, level_launches);
    int32_t max_big = 1;
    for (auto& lev : level_launches)
        for (auto& L : lev) {
            uses_inv = uses_inv || L.inv;
            if (!L.cls) max_big = std::max(max_big, L.count);
        }
    d_dscr.alloc((size_t)max_big * 2 * NB * NB);
    {   // split backward launches (bwd_inv_split): per-front boundary products and arrival counters, shared by all launches
        int64_t need[2] = {0, 0};
        if (sw.bwd_split) bwd_split_scratch(level_solves, need);
        if (need[0] == 0) { d_bwd_g.release(); d_bwd_cnt.release(); }
        else {
            d_bwd_g.alloc((size_t)need[1]);
            d_bwd_cnt.alloc((size_t)need[0]);
            d_bwd_cnt.zero(st);
        }
    }

    std::vector<int64_t> ug_ptr, ug_src;
    build_gather_lists(plan, on_big_path, fd, ug_ptr, ug_src);
    leaf_packed = sw.packed_leaves && pack_leaf_fronts(plan, level_launches, on_big_path, fd);
    d_ug_ptr.upload(ug_ptr, st);
    d_ug_src.upload(ug_src, st);
    // static gather maps of mf_big_gather: the children's inverted index lists and update-block addresses, once per plan
    std::vector<GatherRec> grec;
    std::vector<int32_t> gmap;
    if (!sw.gather_lds_maps) build_gather_maps(plan, level_launches, grec, gmap);
    gather_ct = sw.gather_ct;
    small_threads = sw.small_threads;
    {   // compute units of the device in use: factor_small_threads sets a launch's workgroups against them
        int dev = 0, cus = 0;
        MGB_HIP_CHECK(hipGetDevice(&dev));
        MGB_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        compute_units = std::max(cus, 1);
    }
    border_launches = sw.border_launches;
    step_roles = sw.step_roles;
    gather_roles = sw.gather_roles;
    {   // the border unknown's own root front (mf_analyze: above every other root, so alone on the last level)
        const int32_t nlev = (int32_t)plan.level_ptr.size() - 1;
        border_alone = false;
        if (plan.border && nlev >= 2 && plan.level_ptr[nlev] - plan.level_ptr[nlev - 1] == 1) {
            const Front& f = plan.fronts[plan.level_ptr[nlev - 1]];
            border_alone = f.m == 1 && f.k == 1 && plan.front_idx[f.idx_off] == (int32_t)plan.n;
        }
    }
    border_skipped = false;
    carried_x = nullptr;
    if (grec.empty()) { d_grec.release(); d_gmap.release(); }
    else { d_grec.upload(grec, st); d_gmap.upload(gmap, st); }
    d_fronts.upload(fd, st);
    h_fronts = fd;
    h_a_dst = remap_a_dst(plan, level_launches);
    d_a_dst.upload(h_a_dst, st);
    if (debug_level() >= 2) dump_plan(plan, level_launches);
    analyzed = true;
    MGB_HIP_CHECK(hipStreamSynchronize(st));   // host staging vectors go out of scope
}

void MfSolver::set_direct_map(const int32_t* value_map, int64_t nnz, int64_t tail_base, hipStream_t st) {
    std::vector<int32_t> as(plan.a_src.size());
    for (size_t t = 0; t < as.size(); ++t) {
        const int64_t src = plan.a_src[t];
        const int64_t v = src < nnz ? (int64_t)value_map[src] : tail_base + (src - nnz);
        MGB_REQUIRE(v < (int64_t)INT32_MAX, "direct value index exceeds 32 bits");
        as[t] = (int32_t)v;
    }
    d_a_src_direct.upload(as, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

bool MfSolver::skips_border() const {
    return analyzed && border_alone && !border_launches && !robust && plan.iface_front < 0;
}

void MfSolver::factor(const double* d_values, hipStream_t st, StageTimers* timers, bool direct, bool condensed, double* carried_x_np1) {
    MGB_REQUIRE(!direct || d_a_src_direct.n > 0, "MfSolver::factor: no direct value map");
    MGB_REQUIRE(!condensed || (direct && condensed_ok), "MfSolver::factor: condensed leaves are not enabled");
    MGB_REQUIRE(analyzed, "MfSolver::factor before analyze");
    // condensed: the leaf fronts were written by the element kernel (kernels.hpp, launch_elem_f2_condense); the other
    // fronts take only their border entries from the value array -- every element contribution reaches them through
    // the leaves' update blocks
    const FactorArgs a{condensed ? d_fronts_c.p : d_fronts.p, d_children.p, d_rel.p,
                       condensed ? d_a_src_c.p : (direct ? d_a_src_direct.p : d_a_src.p), condensed ? d_a_dst_c.p : d_a_dst.p,
                       condensed ? d_a_colptr_c.p : d_a_colptr.p, d_values, d_arena.p, d_dscr.p, d_dvec.p, d_status.p, st,
                       d_grec.n ? d_grec.p : nullptr, d_gmap.p, gather_ct, small_threads, compute_units, step_roles, gather_roles};
    if (timers) timers->begin("factor");
    factored_inv = !robust;
    // The border front's pivot -1 - lambda^2 is read by nobody on the carried path (the Newton loop forms lambda^2 = <g, n>
    // itself, and a non-finite pivot there means a non-finite lambda^2, which it reports): no launch for it.
    border_skipped = carried_x_np1 != nullptr && skips_border();
    carried_x = border_skipped ? carried_x_np1 : nullptr;
    const int border_level = (int)level_launches.size() - 1;
    if (!status_zero) MGB_HIP_CHECK(hipMemsetAsync(d_status.p, 0, sizeof(int32_t), st));      // [1], the leaf flag of a condensing f2, stays
    status_zero = false;
    factored_condensed = condensed;
    int lvno = -1;
    for (auto& lev : level_launches) {
        if (border_skipped && lvno + 1 == border_level) break;
        LevelScope lvscope(timers, "fac", ++lvno);
        for (auto& L : lev) {
            if (L.count == 0) continue;
            if (condensed && lvno == 0) continue;          // written by the element kernel
            if (L.tiny) launch_factor_tiny(a, L);
            else if (L.wave && L.cls <= 32) launch_factor_wave<32>(a, L);
            else if (L.wave) launch_factor_wave<48>(a, L);
            else if (L.cls) launch_factor_small(a, L);
            else {
                // Large fronts: assemble, then the pivot chain of the generation in use.  On the inverse-based path block 0
                // of every front is factored by an extra workgroup of the gather launch when that kernel applies;
                // otherwise once per front up front (many fronts) or inside every tile of step 0 (few fronts).
                const bool inv = L.inv && !robust;
                const MfBlock0 b0 = big_block0_kind(L, inv);       // never the gather workgroup for the interface front
                MGB_REQUIRE(!L.iface || (bool)iface_reduce, "MfSolver: interface front without a reduction hook");
                launch_big_assemble(a, L, b0 == MF_B0_GATHER);
                if (L.iface) {
                    // this rank's contribution is assembled: sum over ranks, then factor the complete front (every rank the same)
                    const Front& fi = plan.fronts[L.first];
                    // sum the lower triangle over ranks: (m + 1) m / 2 doubles instead of m^2
                    const int64_t tri = (int64_t)fi.m * (fi.m + 1) / 2;
                    d_ifpack.ensure((size_t)tri);
                    launch_tri_pack(fi.m, d_arena.p + fi.F_off, d_ifpack.p, false, st);
                    iface_reduce(d_ifpack.p, tri);
                    launch_tri_pack(fi.m, d_arena.p + fi.F_off, d_ifpack.p, true, st);
                }
                if (inv) {
                    if (b0 == MF_B0_DIAG0) launch_big_diag0(a, L, L.count);
                    launch_inv_steps(a, L, L.count, b0 == MF_B0_STEP0);
                } else
                    launch_subst_steps(a, L, L.count);
            }
        }
    }
    MGB_HIP_CHECK(hipGetLastError());
    if (timers) timers->end();
}

void MfSolver::solve(const double* d_b, double* d_x, hipStream_t st, StageTimers* timers) {
    MGB_REQUIRE(analyzed, "MfSolver::solve before analyze");
    MGB_REQUIRE(!border_skipped, "MfSolver::solve on factors that carry a Newton right-hand side");      // no border pivot
    if (timers) timers->begin("trisolve");
    // the factored system is [H c; c' gamma] with c = 0 (set_border_identity): solve it for [b; 0]
    const size_t n = (size_t)plan.n;
    MGB_HIP_CHECK(hipMemcpyAsync(d_bx.p, d_b, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    MGB_HIP_CHECK(hipMemsetAsync(d_bx.p + n, 0, sizeof(double), st));
    forward_pass(d_bx.p, st, timers);
    backward_pass(d_xx.p, st, timers);
    MGB_HIP_CHECK(hipMemcpyAsync(d_x, d_xx.p, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    MGB_HIP_CHECK(hipGetLastError());
    if (timers) timers->end();
}

void MfSolver::solve_border(double* d_x_np1, hipStream_t st, StageTimers* timers) {
    MGB_REQUIRE(analyzed, "MfSolver::solve_border before analyze");
    if (timers) timers->begin("trisolve");
    // factors of [H -g; -g' -1]: the forward substitution of H x = g already ran as the border row of every
    // front.  L' x = e_n backwards from x_n = 1 gives x[0:n] = H^{-1} g.
    const size_t n = (size_t)plan.n;
    if (!y_zero) {                   // the backward sweeps only read y: it stays zero from one Newton iteration to the next
        MGB_HIP_CHECK(hipMemsetAsync(d_y.p, 0, n * sizeof(double), st));
        y_zero = true;
    }
    if (!y_border_one) {             // y[n] = 1 survives the backward sweeps: set once (a generic forward sweep overwrites it)
        MGB_HIP_CHECK(hipMemcpyAsync(d_y.p + n, d_one.p, sizeof(double), hipMemcpyDeviceToDevice, st));
        y_border_one = true;
    }
    // Without the border front's launch (factor() with carried_x) x[n] = 1 is the caller's: the kernel that wrote this
    // system's border column stored it, after every earlier writer of the output on the stream and with nothing between
    // it and this sweep.  Any other output gets its own copy.
    if (border_skipped && d_x_np1 != carried_x)
        MGB_HIP_CHECK(hipMemcpyAsync(d_x_np1 + n, d_one.p, sizeof(double), hipMemcpyDeviceToDevice, st));
    backward_pass(d_x_np1, st, timers, border_skipped);
    MGB_HIP_CHECK(hipGetLastError());
    if (timers) timers->end();
}

void MfSolver::forward_pass(const double* d_b, hipStream_t st, StageTimers* timers) {
    y_border_one = false;
    y_zero = false;
    const SolveArgs a = solve_args(d_b, nullptr, st);
    int lvno = -1;
    for (auto& lev : level_solves) {
        LevelScope lvscope(timers, "fwd", ++lvno);
        for (auto& L : lev) {
            if (L.count == 0) continue;
            if (L.tiny) launch_forward_tiny(a, L);
            else if (L.cls) launch_forward_small(a, L);
            else if (L.inv && factored_inv) launch_fwd_inv(a, L);
            else if (L.max_m <= BIG1_MAX_M) launch_fwd_big1(a, L);
            else launch_fwd_big_steps(a, L);
        }
    }
}

void MfSolver::backward_pass(double* d_x, hipStream_t st, StageTimers* timers, bool without_border) {
    const SolveArgs a = solve_args(nullptr, d_x, st);
    // without_border: the last level, the border front, only stores x[n] = y[n] = 1, which d_x already holds
    for (int32_t l = (int32_t)level_solves.size() - (without_border ? 2 : 1); l >= 0; --l) {
        LevelScope lvscope(timers, "bwd", l);
        for (auto it = level_solves[l].rbegin(); it != level_solves[l].rend(); ++it) {
            const MfLaunch& L = *it;
            if (L.count == 0) continue;
            if (L.tiny) launch_backward_tiny(a, L);
            else if (L.cls) launch_backward_small(a, L);
            else if (L.inv && factored_inv) launch_bwd_inv(a, L);
            else if (L.max_m <= BIG1_MAX_M) launch_bwd_big1(a, L);
            else launch_bwd_big_steps(a, L);
        }
    }
}

#ifdef MGB_STEP_PROBE
void mf_debug_probe(long long* out64) {
    (void)hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_probe), 64 * sizeof(long long));
    long long init[64];
    for (int i = 0; i < 64; ++i) init[i] = 0;
    init[56] = 0x7fffffffffffffffll;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_probe), init, sizeof(init));
}
#endif

void MfSolver::chain_stats(double* out) const {
    double blocks = 0, big_levels = 0, fac = 0, bwd = 0, extra = 0;
    for (auto& lev : level_launches) {
        int lev_blocks = 0;
        for (auto& L : lev) {
            if (L.count == 0) continue;
            if (L.tiny || L.wave || L.cls) { fac += 1; continue; }
            const int nb = (L.max_k + NB - 1) / NB;
            lev_blocks = std::max(lev_blocks, nb);
            fac += 1 + nb + (L.iface ? 3 : 0);
            for (int32_t q = L.first; q < L.first + L.count; ++q) {
                const Front& f = plan.fronts[q];
                const double mk = (double)(f.m - f.k), steps = (double)((f.k + NB - 1) / NB);
                // every 32-column step reads and writes the trailing lower triangle it updates; one pass is the floor
                extra += 2.0 * 0.5 * (mk * mk + mk * f.k) * std::max(0.0, steps - 1.0);
            }
        }
        if (lev_blocks) { big_levels += 1; blocks += lev_blocks; }
    }
    for (auto& lev : level_solves)
        for (auto& L : lev)
            if (L.count) bwd += 1;
    out[0] = blocks; out[1] = big_levels; out[2] = fac; out[3] = bwd;
    out[4] = (double)plan.arena_doubles; out[5] = (double)plan.factor_flops; out[6] = extra; out[7] = 0.0;
}

int64_t MfSolver::launches(int32_t* out, int64_t cap) const {
    return launch_rows(level_launches, level_solves, leaf_packed, robust, out, cap);
}

void MfSolver::status_async(int32_t* h_dst2, hipStream_t st) const {
    MGB_HIP_CHECK(hipMemcpyAsync(h_dst2, d_status.p, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
}

int MfSolver::status(hipStream_t st) {
    int32_t h[2] = {0, 0};
    d_status.download(h, 2, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    return status_from(h, factored_condensed);
}

// ---- condensed leaves ----------------------------------------------------------------------------------------
bool MfSolver::enable_condensed(int64_t N, int P, const int32_t* ucol, int64_t slack0, int64_t nnz, int64_t tail_base,
                                hipStream_t st) {
    condensed_ok = false;
    int why = 0;
    struct Report { int& w; ~Report() { if (w) if (debug_level() >= 2) fprintf(stderr, "[mgbhip] condensed leaves: plan shape check %d failed\n", w); } } report{why};
    const int32_t nlev = (int32_t)plan.level_ptr.size() - 1;
    if (!analyzed || !plan.border || nlev < 2 || P > 7) { why = 1; return false; }
    const int32_t n0 = plan.level_ptr[1];
    if ((int64_t)n0 != N) { why = 2; return false; }
    const int32_t nbor = (int32_t)plan.n;
    std::vector<LeafDesc> desc((size_t)N);
    std::vector<char> seen((size_t)N, 0);
    for (int32_t i = 0; i < n0; ++i) {
        const Front& f = plan.fronts[i];
        const int32_t* idx = plan.front_idx.data() + f.idx_off;
        if (f.k != P + 1 || f.m > 15 || f.nchild != 0 || idx[f.m - 1] != nbor) { why = 3; return false; }
        const int64_t e = ((int64_t)idx[0] - slack0) / P;
        if (e < 0 || e >= N || seen[(size_t)e]) { why = 4; return false; }
        for (int q = 0; q < P; ++q)
            if ((int64_t)idx[q] != slack0 + e * P + q) { why = 5; return false; }           // pivots: the element's slacks in node order ...
        if (idx[P] != ucol[e * P + (P - 1)] || idx[P] < 0) { why = 6; return false; }       // ... then its interior u node
        uint32_t packed = (uint32_t)f.m;
        int found = 0;
        for (int q = 0; q < P - 1; ++q) {
            uint32_t pos = 15;
            const int32_t c = ucol[e * P + q];
            if (c >= 0)
                for (int32_t t = P + 1; t < f.m - 1; ++t)
                    if (idx[t] == c) { pos = (uint32_t)t; ++found; break; }
            packed |= pos << (4 + 4 * q);
        }
        if (found != f.m - 1 - (P + 1)) { why = 7; return false; }                           // every boundary unknown is a node of the element
        for (int q = 0; q < P - 1; ++q)                                          // ... and every node that is an unknown is on the boundary
            if (ucol[e * P + q] >= 0 && ((packed >> (4 + 4 * q)) & 15u) == 15u) { why = 8; return false; }
        packed |= 15u << (4 + 4 * (P - 1));
        desc[(size_t)e] = LeafDesc{f.F_off, idx[P], packed};
        seen[(size_t)e] = 1;
    }
    // A lists of the other fronts without the matrix entries (which arrive through the leaves): the border column only
    const int32_t nf = (int32_t)plan.fronts.size();
    std::vector<FrontDev> fd(h_fronts);
    std::vector<int32_t> as, ad, ac;
    for (int32_t i = 0; i < nf; ++i) {
        const Front& f = plan.fronts[i];
        fd[i].a_off = (int64_t)as.size();
        fd[i].acol_off = (int64_t)ac.size();
        const int32_t* cp = plan.a_colptr.data() + f.acol_off;
        for (int32_t c = 0; c < f.k; ++c) {
            ac.push_back((int32_t)((int64_t)as.size() - fd[i].a_off));
            if (i < n0) continue;
            for (int32_t t = cp[c]; t < cp[c + 1]; ++t) {
                const int64_t src = plan.a_src[f.a_off + t];
                if (src < nnz) continue;
                const int64_t v = tail_base + (src - nnz);
                if (v >= (int64_t)INT32_MAX) return false;
                as.push_back((int32_t)v);
                ad.push_back(h_a_dst[f.a_off + t]);
            }
        }
        fd[i].a_cnt = (int32_t)((int64_t)as.size() - fd[i].a_off);
        ac.push_back(fd[i].a_cnt);
    }
    if (as.empty()) { as.push_back(0); ad.push_back(0); }
    d_fronts_c.upload(fd, st);
    d_a_src_c.upload(as, st);
    d_a_dst_c.upload(ad, st);
    d_a_colptr_c.upload(ac, st);
    d_leaf_desc.upload(desc, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    condensed_ok = true;
    return true;
}

}  // namespace mgbhip
