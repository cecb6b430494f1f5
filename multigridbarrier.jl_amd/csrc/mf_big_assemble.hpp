// mf_big_assemble.hpp -- assembly of the large fronts (m > lds_cap), both generations: the column-tiled kernel
// mf_big_assemble (zero, scatter A, extend-add child by child: any number of children, the path of MGBHIP_OLD_BIG=1 too)
// and the gathering kernel mf_big_gather for fronts with few children, whose extra workgroup per front also factors
// block 0 of the pivot chain (block0_to_slot, mf_big_inv.hpp).  launch_big_assemble chooses (big_assembly_kind).
#pragma once
#include "mf_device.hpp"
#include "mf_big_inv.hpp"       // the block-0 tail and its slot format

namespace mgbhip {
namespace {

// Assembly of destination columns [c0, c0 + CT): zero, scatter A, extend-add the children.
__global__ __launch_bounds__(256) void mf_big_assemble(const FrontDev* __restrict__ fr, int32_t first,
                                                       const int32_t* __restrict__ children,
                                                       const int32_t* __restrict__ rel,
                                                       const int32_t* __restrict__ a_src,
                                                       const int32_t* __restrict__ a_dst,
                                                       const int32_t* __restrict__ a_colptr,
                                                       const double* __restrict__ Hval, double* __restrict__ arena) {
    __shared__ int32_t rls[ASM_REL_LDS];
    const FrontDev F = fr[first + blockIdx.y];
    const int m = F.m;
    const int c0 = blockIdx.x * CT;
    if (c0 >= m) return;
    const int c1 = min(c0 + CT, m);
    double* W = arena + F.F_off;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;     // one wave per destination column, lanes on the rows
    for (int c = c0 + wave; c < c1; c += 4) {
        double* Wc = W + (int64_t)c * m;
        for (int r = c + lane; r < m; r += 64) Wc[r] = 0.0;
    }
    __syncthreads();
    {   // A entries are grouped by pivot column: the per-column offsets give the range of [c0, c1)
        const int32_t* cp = a_colptr + F.acol_off;
        const int beg = cp[min(c0, F.k)], end = cp[min(c1, F.k)];
        const int32_t* ad = a_dst + F.a_off;
        for (int t = beg + tid; t < end; t += 256) W[ad[t]] = Hval[a_src[F.a_off + t]];
    }
    __syncthreads();
    for (int c = 0; c < F.nchild; ++c) {
        const FrontDev C = fr[children[F.child_off + c]];
        const double* U = arena + C.F_off;
        const int mc = C.m, kc = C.k, b = mc - kc;
        const int32_t* rlg = rel + C.rel_off;
        // relative indices of this child in LDS: the two searches and the scatter below read them
        // from there instead of chasing ~2 log2(b) dependent global loads
        const bool in_lds = b <= ASM_REL_LDS;
        if (in_lds)
            for (int j = tid; j < b; j += 256) rls[j] = rlg[j];
        __syncthreads();
        const int32_t* rl = in_lds ? rls : rlg;
        // child columns whose destination lies in [c0, c1): rel is increasing
        int lo = 0, hi = b;
        while (lo < hi) { int mid = (lo + hi) >> 1; if (rl[mid] < c0) lo = mid + 1; else hi = mid; }
        const int jb = lo;
        hi = b;
        while (lo < hi) { int mid = (lo + hi) >> 1; if (rl[mid] < c1) lo = mid + 1; else hi = mid; }
        const int je = lo;
        for (int j = jb + wave; j < je; j += 4) {
            double* Wc = W + (int64_t)rl[j] * m;
            const double* Uc = U + (int64_t)(kc + j) * mc + kc;
            // the read-modify-write chain rl -> W is latency bound and W may alias U for the
            // compiler: stage four independent rows per lane so their loads are in flight together
            for (int r = j + lane; r < b; r += 256) {
                const int r1 = r + 64, r2 = r + 128, r3 = r + 192;
                const int i0 = rl[r];
                const int i1 = r1 < b ? rl[r1] : i0;
                const int i2 = r2 < b ? rl[r2] : i0;
                const int i3 = r3 < b ? rl[r3] : i0;
                const double u0 = Uc[r];
                const double u1 = r1 < b ? Uc[r1] : 0.0;
                const double u2 = r2 < b ? Uc[r2] : 0.0;
                const double u3 = r3 < b ? Uc[r3] : 0.0;
                const double w0 = Wc[i0], w1 = Wc[i1], w2 = Wc[i2], w3 = Wc[i3];
                Wc[i0] = w0 + u0;
                if (r1 < b) Wc[i1] = w1 + u1;
                if (r2 < b) Wc[i2] = w2 + u2;
                if (r3 < b) Wc[i3] = w3 + u3;
            }
        }
        __syncthreads();
    }
}

// Gather form of the assembly for fronts with few children (every front of a nested-dissection tree above the
// leaves has two to four).  It works from the inverse of every child's relative index list -- for each front row its
// position in the child's update block, or -1 -- and the children's update-block addresses.  Where they come from is
// the ONLY specialised part of the kernel:
//   LDS_MAPS = false   static gather maps, laid out once by analyze() (build_gather_maps, mf_launch_plan.hpp): the
//                      GatherRec in registers and rows c0 .. m - 1 of the maps copied into LDS, coalesced (reading the
//                      maps from global memory inside the row loop instead was slower: DESIGN.md section 4);
//   LDS_MAPS = true    (MGBHIP_GATHER_LDS_MAPS=1) rebuilt by every workgroup of every launch, as before the static maps:
//                      children -> descriptor -> rel, a fill pass and a scatter into the whole table in LDS, cU / cM
//                      there too.  The A/B lever of the maps (tests/test_gpu_gather_maps.py) and nothing else: the
//                      arguments grec / gmap resp. children / rel / mstride of the other form are unused.
// `ct` destination columns per workgroup: big_gather_ct on the maps, CT on the LDS tables.  Each destination entry is
// formed ONCE in a register -- the children's entries that land on it, added in child order, all their loads in flight
// together -- and stored once.  No zero pass, no read-modify-write of the arena, and the dependent-load chains of the
// children run side by side instead of one child after the other.
template <bool LDS_MAPS>
__global__ __launch_bounds__(256) void mf_big_gather(const FrontDev* __restrict__ fr, int32_t first,
                                                     const GatherRec* __restrict__ grec, const int32_t* __restrict__ gmap,
                                                     const int32_t* __restrict__ a_src,
                                                     const int32_t* __restrict__ a_dst,
                                                     const int32_t* __restrict__ a_colptr,
                                                     const double* __restrict__ Hval, double* __restrict__ arena,
                                                     double* __restrict__ dscr, int32_t* __restrict__ status, int with_diag,
                                                     int ct /* destination columns per workgroup */,
                                                     const int32_t* __restrict__ children,
                                                     const int32_t* __restrict__ rel, int mstride,
                                                     int roles /* BlockRoles: the grid's layout (with_diag) */) {
    extern __shared__ int32_t inv[];               // [nchild][stride]: rows row0 .. of the tables (column workgroups)
    __shared__ int64_t cU[GATHER_MAX_CHILD];       // LDS_MAPS only: the children's update blocks, relative lists,
    __shared__ int64_t cR[GATHER_MAX_CHILD];       // leading dimensions and sizes
    __shared__ int32_t cM[GATHER_MAX_CHILD], cB[GATHER_MAX_CHILD];
    // with_diag: the block-0 workgroup is the front's chain workgroup, the column groups its tiles (mf_block_roles.hpp);
    // a launch without one is the plain grid (column groups, fronts)
    const BlockRole BR = with_diag ? role_of_block(roles, blockIdx.x, blockIdx.y, gridDim.x)
                                   : tile_of_block(blockIdx.x, blockIdx.y);
    const FrontDev F = fr[first + BR.front];
    const int m = F.m, tid = threadIdx.x, nch = F.nchild;
    GatherRec G;                                   // grec: the record of the launch's first front
    const int64_t* base;                           // per child: start of its update block in the arena ...
    const int32_t* ld;                             // ... and its leading dimension
    if constexpr (LDS_MAPS) {
        if (tid < nch) {                           // published by the first barrier of the staging below
            const FrontDev C = fr[children[F.child_off + tid]];
            cU[tid] = C.F_off + (int64_t)C.k * C.m + C.k;
            cR[tid] = C.rel_off;
            cM[tid] = C.m;
            cB[tid] = C.m - C.k;
        }
        base = cU;
        ld = cM;
    } else {
        G = grec[BR.front];
        base = G.base;
        ld = G.ld;
    }
    const int32_t* mp = LDS_MAPS ? nullptr : gmap + G.map_off;         // static maps: [nchild][m]
    const int32_t* ad = a_dst + F.a_off;
    if (BR.chain()) {
        // One extra workgroup per front forms ONLY the first 32 x 32 diagonal block (same gather, same order as
        // the column workgroups, which write it to the arena), factors and inverts it and leaves W_0 / d_0 in slot 0:
        // step 0 of the factorization finds its diagonal block ready, as every later step does from the look-ahead
        // workgroup.  Its time hides under the column workgroups of the same launch (was: a launch of its own for
        // batches of many fronts, a redundant factorization inside every tile of step 0 for the others).
        __shared__ double Wv[NB][NB + 1];
        __shared__ double Dn[NB][NB + 1];
        __shared__ double Tm[16][17];
        __shared__ double dq[NB];
        __shared__ int32_t inv0[GATHER_MAX_CHILD][NB];      // the tables' first 32 rows
        const int nb = min(NB, F.k);
        // the first batch of A entries of the block (cp -> a_dst / a_src -> Hval: three dependent loads) is requested
        // beside the tables
        int a_d0 = -1;
        double a_v0 = 0.0;
        const int a_end = (a_colptr + F.acol_off)[nb];
        if (tid < a_end) {
            a_d0 = ad[tid];
            a_v0 = Hval[a_src[F.a_off + tid]];
        }
        if constexpr (LDS_MAPS) {
            for (int i = tid; i < GATHER_MAX_CHILD * NB; i += 256) inv0[i / NB][i % NB] = -1;
            __syncthreads();
            for (int ch = 0; ch < nch; ++ch) {               // rel is increasing: only its first entries can be < 32
                const int32_t* rl = rel + cR[ch];
                const int lim = min(cB[ch], NB);
                if (tid < lim) {
                    const int g = rl[tid];
                    if (g < NB) inv0[ch][g] = tid;
                }
            }
        } else {
            const int ch = tid / NB, g = tid % NB;          // GATHER_MAX_CHILD * NB = 256 threads
            inv0[ch][g] = (ch < nch && g < m) ? mp[(int64_t)ch * m + g] : -1;
        }
        __syncthreads();
        for (int i = tid; i < NB * NB; i += 256) {
            const int rr = i % NB, c = i / NB;
            double v = 0.0;
            if (rr >= c && rr < nb) {
#pragma unroll
                for (int ch = 0; ch < GATHER_MAX_CHILD; ++ch) {        // child order: the summation order of the extend-add
                    if (ch < nch) {
                        const int jc = inv0[ch][c], ir = inv0[ch][rr];
                        if (jc >= 0 && ir >= 0) v += arena[base[ch] + (int64_t)jc * ld[ch] + ir];
                    }
                }
            }
            Dn[rr][c] = v;
        }
        __syncthreads();
        if (a_d0 >= 0) {
            const int lu = a_d0 % m, lv = a_d0 / m;
            if (lu < nb) Dn[lu][lv] += a_v0;
        }
        for (int t = tid + 256; t < a_end; t += 256) {
            const int d = ad[t], lu = d % m, lv = d / m;
            if (lu < nb) Dn[lu][lv] += Hval[a_src[F.a_off + t]];
        }
        __syncthreads();
        block0_to_slot(Dn, Wv, Tm, dq, nb, tid, status, dscr + (int64_t)BR.front * 2 * (NB * NB));
        return;
    }
    const int c0 = BR.tile() * ct;
    if (c0 >= m) return;
    const int c1 = min(c0 + ct, m);
    double* W = arena + F.F_off;
    const int lane = tid & 63, wave = tid >> 6;     // one wave per destination column, lanes on the rows
    // A entries are grouped by pivot column: the per-column offsets give the range of [c0, c1).  Its first batch is
    // requested now (cp -> a_dst / a_src -> Hval) and runs under the children's loads; it is added after their sums.
    const int32_t* cp = a_colptr + F.acol_off;
    const int a_beg = cp[min(c0, F.k)], a_end = cp[min(c1, F.k)];
    int a_d0 = -1;
    double a_v0 = 0.0;
    if (a_beg + tid < a_end) {
        a_d0 = ad[a_beg + tid];
        a_v0 = Hval[a_src[F.a_off + a_beg + tid]];
    }
    // static maps: rows c0 .. m - 1 of every child's map (the lower triangle below column c0 needs no others);
    // LDS tables: all m rows, at the launch's stride
    const int row0 = LDS_MAPS ? 0 : c0, stride = LDS_MAPS ? mstride : m - c0;
    if constexpr (LDS_MAPS) {
        for (int i = tid; i < nch * mstride; i += 256) inv[i] = -1;
        __syncthreads();
        for (int ch = 0; ch < nch; ++ch) {
            const int32_t* rl = rel + cR[ch];
            const int b = cB[ch];
            for (int j = tid; j < b; j += 256) inv[ch * mstride + rl[j]] = j;
        }
    } else {
        for (int r = tid; r < stride; r += 256) {  // one coalesced copy, the children's loads in flight together
            int32_t t[GATHER_MAX_CHILD];
#pragma unroll
            for (int ch = 0; ch < GATHER_MAX_CHILD; ++ch) t[ch] = ch < nch ? mp[(int64_t)ch * m + c0 + r] : -1;
#pragma unroll
            for (int ch = 0; ch < GATHER_MAX_CHILD; ++ch)
                if (ch < nch) inv[ch * stride + r] = t[ch];
        }
    }
    __syncthreads();
    for (int c = c0 + wave; c < c1; c += 4) {
        double* Wc = W + (int64_t)c * m;
        int64_t colbase[GATHER_MAX_CHILD];         // child column offset, -1 when the child does not reach column c
#pragma unroll
        for (int ch = 0; ch < GATHER_MAX_CHILD; ++ch) {
            const int jc = ch < nch ? inv[ch * stride + c - row0] : -1;
            colbase[ch] = jc >= 0 ? base[ch] + (int64_t)jc * ld[ch] : -1;
        }
        for (int r = c + lane; r < m; r += 128) {  // two rows per lane in flight (four: 2 % slower end to end, measured in round 4)
            const int r1 = r + 64;
            double u0[GATHER_MAX_CHILD], u1[GATHER_MAX_CHILD];
#pragma unroll
            for (int ch = 0; ch < GATHER_MAX_CHILD; ++ch) {
                u0[ch] = 0.0;
                u1[ch] = 0.0;
                if (colbase[ch] >= 0) {
                    const int i0 = inv[ch * stride + r - row0];
                    const int i1 = r1 < m ? inv[ch * stride + r1 - row0] : -1;
                    if (i0 >= 0) u0[ch] = arena[colbase[ch] + i0];
                    if (i1 >= 0) u1[ch] = arena[colbase[ch] + i1];
                }
            }
            double v0 = 0.0, v1 = 0.0;
#pragma unroll
            for (int ch = 0; ch < GATHER_MAX_CHILD; ++ch) {      // child order: the summation order of the extend-add
                v0 += u0[ch];
                v1 += u1[ch];
            }
            Wc[r] = v0;
            if (r1 < m) Wc[r1] = v1;
        }
    }
    __syncthreads();
    if (a_d0 >= 0) W[a_d0] += a_v0;
    for (int t = a_beg + tid + 256; t < a_end; t += 256) W[ad[t]] += Hval[a_src[F.a_off + t]];
}

// ---- host launchers ------------------------------------------------------------------------------------------
inline dim3 big_assemble_grid(const MfLaunch& L) { return dim3((L.max_m + CT - 1) / CT, L.count); }
inline void launch_big_assemble_cols(const FactorArgs& a, const MfLaunch& L) {
    hipLaunchKernelGGL(mf_big_assemble, big_assemble_grid(L), dim3(256), 0, a.st, a.fr, L.first, a.children, a.rel, a.a_src,
                       a.a_dst, a.a_colptr, a.values, a.arena);
}

// Assembly of the fronts of a large-front launch: the gathering kernel when it applies (big_assembly_kind,
// mf_launch_plan.hpp), the column-tiled one otherwise.  with_diag asks the gather launch for an extra workgroup per
// front that factors block 0 (big_block0_kind says MF_B0_GATHER only when the gathering kernel applies).
inline void launch_big_assemble(const FactorArgs& a, const MfLaunch& L, bool with_diag) {
    if (big_assembly_kind(L) != MF_ASM_GATHER) {
        launch_big_assemble_cols(a, L);
        return;
    }
    const bool lds_maps = !a.grec;     // no static gather maps (analyze()): MGBHIP_GATHER_LDS_MAPS=1
    // (one column per wave on levels with few fronts, ct = 4: no gain, measured in round 4)
    const int ct = lds_maps ? CT : big_gather_ct(L, a.gather_ct);
    const int ncol = (L.max_m + ct - 1) / ct;
    // the column groups of every front + its diagonal-block workgroup, or the column groups alone
    const RolesGrid ga = with_diag ? roles_grid(a.gather_roles, L.count, ncol) : tiles_only_grid(L.count, ncol);
    const auto gather = lds_maps ? mf_big_gather<true> : mf_big_gather<false>;
    // LDS: rows c0 .. m - 1 of the maps of one front, or its whole tables
    hipLaunchKernelGGL(gather, dim3(ga.x, ga.y), dim3(256), big_gather_lds(L), a.st, a.fr, L.first, lds_maps ? nullptr : a.grec + L.grec_first,
                       a.gmap, a.a_src, a.a_dst, a.a_colptr, a.values, a.arena, a.dscr, a.status, with_diag ? 1 : 0, ct,
                       a.children, a.rel, L.max_m, a.gather_roles);
}

}  // namespace
}  // namespace mgbhip
