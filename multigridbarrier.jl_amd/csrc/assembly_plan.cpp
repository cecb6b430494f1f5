// assembly_plan.cpp -- host side of the assembly plan for H = R' H_blk R (assembly_plan.hpp).  No HIP.
#include "assembly_plan.hpp"

#include <algorithm>

#include "../../include/mgbhip.h"   // MGBHIP_MAX_NU
#include "host_util.hpp"            // MGB_REQUIRE
#include "panel_layout.hpp"         // hel_layout, panel staging sizes

namespace mgbhip {

static constexpr int64_t ACC_MAX_M = 384;

ElementColumns element_columns(const PlanShape& S) {
    const int64_t NE = S.NE, nn = S.n;
    const int pp = S.p, nu = S.nu;
    ElementColumns C;
    C.selection = true;
    for (int64_t q = 0; q < S.Rnnz && C.selection; ++q) C.selection = (S.Rval[q] == 1.0);
    for (int64_t i = 0; i < S.rows && C.selection; ++i) C.selection = (S.Rptr[i + 1] - S.Rptr[i] <= 1);
    C.ecol_ptr.assign((size_t)NE * nu + 1, 0);
    C.ecols.reserve((size_t)NE * nu * pp);
    std::vector<int32_t> tmp;
    for (int64_t e = 0; e < NE; ++e)
        for (int a = 0; a < nu; ++a) {
            tmp.clear();
            for (int r = 0; r < pp; ++r) {
                const int64_t row = (int64_t)a * nn + e * pp + r;
                for (int32_t q = S.Rptr[row]; q < S.Rptr[row + 1]; ++q) tmp.push_back(S.Rcol[q]);
            }
            std::sort(tmp.begin(), tmp.end());
            tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
            C.ecols.insert(C.ecols.end(), tmp.begin(), tmp.end());
            C.ecol_ptr[e * nu + a + 1] = (int32_t)C.ecols.size();
            MGB_REQUIRE(C.ecols.size() < (size_t)INT32_MAX, "assembly plan exceeds 32-bit indexing");
        }
    C.cmax = 1;
    for (size_t q = 0; q + 1 < C.ecol_ptr.size(); ++q) C.cmax = std::max(C.cmax, C.ecol_ptr[q + 1] - C.ecol_ptr[q]);
    C.ctmax = 1;
    C.eoff.assign((size_t)NE + 1, 0);
    for (int64_t e = 0; e < NE; ++e) {
        const int64_t ct = C.ecol_ptr[(e + 1) * nu] - C.ecol_ptr[e * nu];
        C.eoff[e + 1] = C.eoff[e] + ct * ct;
        C.ctmax = std::max(C.ctmax, ct);
    }
    C.slab_est = C.eoff[NE];
    return C;
}

AccumulateDecision decide_accumulate(int p, int nu, int64_t NE, int64_t m, bool selection, int64_t ctmax, int64_t slab_est) {
    // LDS accumulate (launch_panel_accumulate): chunks of the packed upper triangle sized so that
    // chunk + one element's staging fit the LDS budget; element streams fill the GPU once
    const int64_t mt = m * (m + 1) / 2;
    const int64_t stage = (int64_t)panel_stage_doubles(p, nu, (int)ctmax);
    const int64_t room = (int64_t)(PANEL_ACC_LDS_MAX / sizeof(double)) - stage;
    int64_t nsplit = room > 0 ? (mt + room - 1) / room : 1 << 20;
    if (nsplit < 1) nsplit = 1;
    const int64_t chunk = (mt + nsplit - 1) / nsplit;
    const int64_t waves = std::max<int64_t>(8, std::min<int64_t>(NE, (nsplit == 1 ? 512 : 256) / nsplit));
    // wide coarse supports only (3-D hierarchies): many contributions per entry, few enough
    // elements per stream; narrow supports are faster through slab + gather
    constexpr int64_t acc_ne_max = 65536;
    const bool acc = !selection && m > 0 && m <= ACC_MAX_M && room > 0 && nsplit <= 4 && NE <= acc_ne_max && slab_est >= 16 * mt &&
                     panel_accumulate_fits(p, nu, (int)ctmax);
    return {acc, (int32_t)waves, (int32_t)nsplit, (int32_t)chunk, mt};
}

void dense_pattern(int64_t m, std::vector<int32_t>& ptr, std::vector<int32_t>& col) {
    ptr.resize((size_t)m + 1);
    col.resize((size_t)(m * m));
    for (int64_t i = 0; i <= m; ++i) ptr[i] = (int32_t)(i * m);
    for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < m; ++j) col[i * m + j] = (int32_t)j;
}

// Every structural element contribution of a selection level, in the order that fixes the sums: emit(ci, cj, src) with
// the columns of nodes i (state a) and j (state b) of element e and the slab index of Hel_ab[i, j].
// Blocks (a, b) whose D rows are all identity operators are diagonal per element
// (Hel_ab[i, j] = sum_r delta_ri Y_r delta_rj): on selection levels their off-diagonal slots
// are structural zeros, exactly as in the reference's sparse products, and stay out of the
// pattern.  (With default_D this decouples the broken slack unknowns of an element.)
template <class Emit>
static void selection_pairs(const PlanShape& S, Emit&& emit) {
    const int64_t NE = S.NE, nn = S.n;
    const int pp = S.p, nu = S.nu;
    int64_t sel_off[MGBHIP_MAX_NU * (MGBHIP_MAX_NU + 1) / 2];
    hel_layout(nu, NE, pp, S.diag_mask_sel, sel_off);
    auto state_id = [&](int a) { return ((S.state_id_mask >> a) & 1u) != 0; };
    auto structural = [&](int a, int i, int b, int j) { return !(state_id(a) && state_id(b) && i != j); };
    auto colof = [&](int a, int64_t e, int r) -> int32_t {
        const int64_t row = (int64_t)a * nn + e * pp + r;
        return S.Rptr[row + 1] > S.Rptr[row] ? S.Rcol[S.Rptr[row]] : -1;
    };
    for (int64_t e = 0; e < NE; ++e)
        for (int a = 0; a < nu; ++a)
            for (int i = 0; i < pp; ++i) {
                const int32_t ci = colof(a, e, i);
                if (ci < 0) continue;
                for (int b = 0; b < nu; ++b)
                    for (int j = 0; j < pp; ++j) {
                        if (!structural(a, i, b, j)) continue;
                        const int32_t cj = colof(b, e, j);
                        if (cj < 0) continue;
                        int64_t src;   // slab index of Hel_ab[i, j] (upper block triangle stored)
                        const int blk = a <= b ? hel_block_index(a, b, nu) : hel_block_index(b, a, nu);
                        if ((S.diag_mask_sel >> blk) & 1) src = sel_off[blk] + e * pp + i;            // i == j here
                        else if (a <= b) src = sel_off[blk] + (e * pp + j) * (int64_t)pp + i;
                        else src = sel_off[blk] + (e * pp + i) * (int64_t)pp + j;
                        emit(ci, cj, src);
                    }
            }
}

void host_pattern(const PlanShape& S, const ElementColumns& C, std::vector<int32_t>& ptr, std::vector<int32_t>& col) {
    const int64_t NE = S.NE, m = S.m;
    const int nu = S.nu;
    ptr.assign((size_t)m + 1, 0);
    col.clear();
    if (C.selection) {
        // (row, col) pairs of every structural element contribution, bucketed by row
        std::vector<int32_t> rc(m + 1, 0);
        selection_pairs(S, [&](int32_t ci, int32_t, int64_t) { rc[ci + 1]++; });
        std::vector<int64_t> off(m + 1, 0);
        for (int64_t i = 0; i < m; ++i) off[i + 1] = off[i] + rc[i + 1];
        std::vector<int32_t> cols((size_t)off[m]);
        {
            std::vector<int64_t> fill(off.begin(), off.end() - 1);
            selection_pairs(S, [&](int32_t ci, int32_t cj, int64_t) { cols[(size_t)fill[ci]++] = cj; });
        }
        for (int64_t i = 0; i < m; ++i) {
            int32_t* lo = cols.data() + off[i];
            int32_t* hi = cols.data() + off[i + 1];
            std::sort(lo, hi);
            hi = std::unique(lo, hi);
            if (lo == hi) col.push_back((int32_t)i);     // unknown untouched by any element: keep a diagonal slot
            else col.insert(col.end(), lo, hi);
            MGB_REQUIRE(col.size() < (size_t)INT32_MAX, "Hessian pattern exceeds 32-bit indexing");
            ptr[i + 1] = (int32_t)col.size();
        }
    } else {
        // union over elements of (all columns of e) x (all columns of e)
        const std::vector<int32_t>& ecol_ptr = C.ecol_ptr;
        const std::vector<int32_t>& ecols = C.ecols;
        std::vector<int32_t> cnt(m + 1, 0);
        for (int64_t e = 0; e < NE; ++e)
            for (int32_t q = ecol_ptr[e * nu]; q < ecol_ptr[(e + 1) * nu]; ++q) cnt[ecols[q] + 1]++;
        for (int64_t j = 0; j < m; ++j) cnt[j + 1] += cnt[j];
        std::vector<int32_t> c2e(cnt[m]);
        {
            std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
            for (int64_t e = 0; e < NE; ++e)
                for (int32_t q = ecol_ptr[e * nu]; q < ecol_ptr[(e + 1) * nu]; ++q) c2e[fill[ecols[q]]++] = (int32_t)e;
        }
        std::vector<int32_t> rowbuf;
        for (int64_t i = 0; i < m; ++i) {
            rowbuf.clear();
            for (int32_t t = cnt[i]; t < cnt[i + 1]; ++t) {
                const int64_t e = c2e[t];
                rowbuf.insert(rowbuf.end(), ecols.begin() + ecol_ptr[e * nu], ecols.begin() + ecol_ptr[(e + 1) * nu]);
            }
            if (rowbuf.empty()) rowbuf.push_back((int32_t)i);   // unknown untouched by any element: keep a diagonal slot
            std::sort(rowbuf.begin(), rowbuf.end());
            rowbuf.erase(std::unique(rowbuf.begin(), rowbuf.end()), rowbuf.end());
            col.insert(col.end(), rowbuf.begin(), rowbuf.end());
            MGB_REQUIRE(col.size() < (size_t)INT32_MAX, "Hessian pattern exceeds 32-bit indexing");
            ptr[i + 1] = (int32_t)col.size();
        }
    }
}

HostLists host_lists(const PlanShape& S, const ElementColumns& C, const std::vector<int32_t>& ptr, const std::vector<int32_t>& col) {
    const int64_t nnz = (int64_t)col.size();
    auto find = [&](int32_t row, int32_t c) {
        const int32_t* lo = col.data() + ptr[row];
        const int32_t* hi = col.data() + ptr[row + 1];
        return (int32_t)(std::lower_bound(lo, hi, c) - col.data());
    };
    // one pass over the contributions: remember (position, source) pairs so that the binary
    // searches behind `find` run once, then bucket them by position
    HostLists out;
    std::vector<int32_t>& ccount = out.cptr;
    ccount.assign((size_t)nnz + 1, 0);
    std::vector<int32_t> ppos, psrc;
    auto emit = [&](int32_t ci, int32_t cj, int64_t src) {
        MGB_REQUIRE(src < (int64_t)INT32_MAX, "slab exceeds 32-bit indexing");
        const int32_t pos = find(ci, cj);
        ccount[pos + 1]++;
        ppos.push_back(pos);
        psrc.push_back((int32_t)src);
    };
    if (C.selection) {
        selection_pairs(S, emit);
    } else {
        for (int64_t e = 0; e < S.NE; ++e) {
            const int32_t base = C.ecol_ptr[e * S.nu];
            const int32_t ct = C.ecol_ptr[(e + 1) * S.nu] - base;
            for (int32_t gj = 0; gj < ct; ++gj)
                for (int32_t gi = 0; gi < ct; ++gi)
                    emit(C.ecols[base + gi], C.ecols[base + gj], C.eoff[e] + gi + (int64_t)ct * gj);
        }
    }
    int64_t total = 0;
    for (int64_t q = 0; q < nnz; ++q) {
        total += ccount[q + 1];
        MGB_REQUIRE(total < (int64_t)INT32_MAX, "contribution list exceeds 32-bit indexing");
        ccount[q + 1] += ccount[q];
    }
    out.total = total;
    out.long_lists = nnz > 0 && total / nnz > 48;
    std::vector<int32_t> fill(ccount.begin(), ccount.end() - 1);
    out.cidx.resize((size_t)total);
    for (size_t t = 0; t < ppos.size(); ++t) out.cidx[fill[ppos[t]]++] = psrc[t];   // element order within a list
    return out;
}

GatherChunks decide_gather_chunks(const int32_t* cptr, int64_t nnz) {
    if (nnz <= 0 || cptr[nnz] / nnz <= 2048) return {0, 0};
    int64_t maxlen = 0;
    for (int64_t q = 0; q < nnz; ++q) maxlen = std::max<int64_t>(maxlen, cptr[q + 1] - cptr[q]);
    const int32_t chunk = (int32_t)std::max<int64_t>(1024, (maxlen + 63) / 64);
    return {chunk, (int32_t)((maxlen + chunk - 1) / chunk)};
}

std::vector<int32_t> upper_positions(const std::vector<int32_t>& ptr, const std::vector<int32_t>& col, int64_t m, bool row_major) {
    // positions of the upper triangle: `symmetric(H)` (src/newton.jl:253) and the factorization read nothing else, so the
    // Newton loop projects and gathers only those (half the slab stores, half the gather traffic)
    // ... in COLUMN-major order (column j, rows i <= j ascending): the summands of (i, j) and (i + 1, j) sit next to each
    // other in every element block that holds both (block entry ci + ct cj, columns sorted), so neighbouring waves of the
    // gather share their cache lines; in row-major order every 8-byte summand was a line of its own.  The order of the
    // POSITIONS changes, not the order inside a sum: same values.
    std::vector<int32_t> up;
    std::vector<int32_t> cnt((size_t)m + 1, 0);
    for (int64_t i = 0; i < m; ++i)
        for (int32_t q = ptr[i]; q < ptr[i + 1]; ++q)
            if (col[q] >= i) cnt[(size_t)col[q] + 1]++;
    for (int64_t j = 0; j < m; ++j) cnt[(size_t)j + 1] += cnt[(size_t)j];
    up.resize((size_t)cnt[(size_t)m]);
    size_t w = 0;
    for (int64_t i = 0; i < m; ++i)
        for (int32_t q = ptr[i]; q < ptr[i + 1]; ++q)
            if (col[q] >= i) {
                if (row_major) up[w++] = q;
                else up[(size_t)cnt[(size_t)col[q]]++] = q;
            }
    return up;
}

std::vector<double> element_panels(const PlanShape& S, const ElementColumns& C) {
    const int pp = S.p, nu = S.nu;
    std::vector<double> panels((size_t)pp * C.ecols.size(), 0.0);
    for (int64_t e = 0; e < S.NE; ++e)
        for (int a = 0; a < nu; ++a) {
            const int32_t o = C.ecol_ptr[e * nu + a], c = C.ecol_ptr[e * nu + a + 1] - o;
            for (int r = 0; r < pp; ++r) {
                const int64_t row = (int64_t)a * S.n + e * pp + r;
                for (int32_t q = S.Rptr[row]; q < S.Rptr[row + 1]; ++q) {
                    const int32_t* lo = C.ecols.data() + o;
                    const int32_t ia = (int32_t)(std::lower_bound(lo, lo + c, S.Rcol[q]) - lo);
                    panels[(size_t)pp * o + r + (size_t)pp * ia] += S.Rval[q];
                }
            }
        }
    return panels;
}

}  // namespace mgbhip
