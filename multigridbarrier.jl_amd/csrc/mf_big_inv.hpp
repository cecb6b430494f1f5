// mf_big_inv.hpp -- large fronts, inverse-based generation (fronts with lds_cap < m <= BIG_INV_MAX_M): the MFMA step
// kernel mf_big_step, the block-0 kernel mf_big_diag0 with the block-0 tail and the slot format it shares with the gathering
// assembly (mf_big_assemble.hpp), the triangle pack of the interface front (mf_tri_pack) and the single-workgroup solves
// mf_fwd_inv / mf_bwd_inv (mf_bwd_inv_split: the boundary product of a backward launch of few fronts shared among several
// workgroups per front).
//
// One launch per 32-column step.  The diagonal block of step j is factored AND inverted ahead of
// time by the look-ahead workgroup of step j-1 (W_j = L_jj^{-1}, d_j); every trailing tile then
// forms the two panel slices it needs by a small matrix-core product with W_j,
//     S = A21 W_j'  (= L21 D),   L = S D^{-1},
// instead of waiting for a separate triangular-solve kernel, and applies  C -= S L'  on the matrix
// cores (v_mfma_f64_16x16x4_f64).  The panel itself is never written back: the arena keeps the
// fully updated, UNSOLVED rows A21, and the triangular sweeps need one matrix per block,
// M_j = W_j' D_j^{-1} W_j (the inverse of the updated diagonal block):  forward u_j = M_j t_j,
// t_r -= A_rj u_j;  backward x_j = u_j - M_j G_j with G = A21' x_r.  Home layout of a factored
// diagonal block: strictly UPPER triangle = off-diagonal of M_j, its diagonal lives in `dvec`;
// the lower triangle keeps the unfactored block (sibling workgroups of step 0 still read it).
#pragma once
#include "mf_block_roles.hpp"
#include "mf_device.hpp"

namespace mgbhip {
namespace {

constexpr int BIGI_THREADS = 1024;

#include "ldlt32.hpp"

// The 32 x 32 LDL' of the pivot chain and the inverse of its factor: one wave each, every product on the matrix cores
// (ldlt32.hpp; the 256-thread forms of round 2 -- 4 x 4-blocked LDL', seven-barrier recursive doubling -- were removed in
// round 4: no build selected them).
__device__ __forceinline__ void block_ldlt32(double (*Dn)[NB + 1], double* dq, int nb, int tid, int32_t* __restrict__ status) {
    block_ldlt32_mfma(Dn, dq, nb, tid, status);
}
__device__ __forceinline__ void block_inverse32_sel(const double (*Ls)[NB + 1], double (*Wv)[NB + 1], double (*Tm)[17], int tid) {
    block_inverse32_mfma(Ls, Wv, Tm, tid);
}

// A factored diagonal block travels between launches in a `dscr` slot of NB x NB doubles: column-major, stride NB, the
// pivots d on the diagonal and W = L^{-1} strictly below it; the upper triangle is never touched.
// Block 0 of a front's pivot chain, assembled in Dn (lower triangle, published by a barrier): factor it, invert the
// factor, leave d / W in `slot`.  256 threads (mf_big_diag0 and the block-0 workgroup of mf_big_gather, mf_big_assemble.hpp;
// mf_big_step keeps its own text of the same three phases and of the slot's decoding: profiles/gather_merge_isa.txt).
__device__ __forceinline__ void block0_to_slot(double (*Dn)[NB + 1], double (*Wv)[NB + 1], double (*Tm)[17], double* dq, int nb,
                                               int tid, int32_t* __restrict__ status, double* __restrict__ slot) {
    block_ldlt32(Dn, dq, nb, tid, status);
    block_inverse32_sel(Dn, Wv, Tm, tid);
    for (int i = tid; i < NB * NB; i += 256) {
        const int rr = i % NB, c = i / NB;
        if (rr >= c && rr < nb) slot[rr + NB * c] = (rr == c) ? dq[rr] : Wv[rr][c];
    }
}

// S = A W' for a 64-row slice held raw in P[c][rr] (LDS, overwritten in place); wave w owns rows
// 16w .. 16w+15, so no cross-wave hazard.  scale != nullptr: result columns are multiplied by
// scale[q] (the reciprocal pivots) and written to Pout (may alias P).
__device__ __forceinline__ void slice_transform(double (*P)[ST + 1], double (*Pout)[ST + 1], double (*P2)[ST + 1],
                                                const double (*Wv)[NB + 1], const double* rd, int lane, int wave) {
    const int fr = lane & 15, fk = lane >> 4;
    const int rr = 16 * wave + fr;
    double4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < NB / 4; ++kk) {
        const double a = P[4 * kk + fk][rr];                       // y[k][j]: A[rr = j][c = k]
        if (kk < 4) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(Wv[fr][4 * kk + fk], a, acc0, 0, 0, 0);   // q tile 0: c < 16 only
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Wv[16 + fr][4 * kk + fk], a, acc1, 0, 0, 0);
    }
    // D[i][j]: i = fk + 4 reg -> q within the tile, j = fr -> rr
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q0 = fk + 4 * r, q1 = 16 + fk + 4 * r;
        Pout[q0][rr] = acc0[r];
        Pout[q1][rr] = acc1[r];
        if (P2) {
            P2[q0][rr] = acc0[r] * rd[q0];
            P2[q1][rr] = acc1[r] * rd[q1];
        }
    }
}

#ifdef MGB_STEP_PROBE      // development probe build only (tools/gpu_probe.py): per-phase timestamps of one step
#define PROBE_NFRONTS (roles == ROLES_CHAIN_FIRST ? gridDim.x : gridDim.y)      // of the launch (roles_grid)
#define PROBE(i) do { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_waitcnt(0); if (is_la && BR.front == 0 && tid == 0 && j0 == 64 && PROBE_NFRONTS == 1 && F.k > 400) g_probe[i] = wall_clock64(); if (!is_la && BR.first_tile() && BR.front == 0 && tid == 0 && j0 == 64 && PROBE_NFRONTS == 1 && F.k > 400) g_probe[16 + i] = wall_clock64(); __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PROBE(i) do { } while (0)
#endif

__global__ __launch_bounds__(256, 3) void mf_big_step(const FrontDev* __restrict__ fr, int32_t first, int j0,
                                                   double* __restrict__ arena, double* __restrict__ dscr,
                                                   double* __restrict__ dvec, int32_t* __restrict__ status,
                                                   int do_diag, int roles /* BlockRoles: the grid's layout */) {
    __shared__ double Wv[NB][NB + 1];
    __shared__ double Dn[NB][NB + 1];
    __shared__ double Tm[16][17];
    __shared__ double dq[NB], rdq[NB];
    __shared__ double Pa[NB][ST + 1];
    __shared__ double Pb[NB][ST + 1];
    const BlockRole BR = role_of_block(roles, blockIdx.x, blockIdx.y, gridDim.x);      // mf_block_roles.hpp
    const FrontDev F = fr[first + BR.front];        // (as kernel arguments for launches of few fronts: the kernel sits at its
                                                      // 168-register cap and spilled, 6 % slower end to end: measured in round 4)
    const int m = F.m, k = F.k;
    if (j0 >= k) return;
    const int nb = min(NB, k - j0);
    const int j1 = j0 + nb;
    const int T = (m - j1 + ST - 1) / ST;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* W = arena + F.F_off;
    double* slot = dscr + ((int64_t)BR.front * 2 + ((j0 / NB) & 1)) * (NB * NB);
    const bool is_la = BR.chain();
    int ti = 0, tj = 0;
    if (!is_la) {
        const int lin = BR.tile();
        ti = (int)((sqrt(8.0 * lin + 1.0) - 1.0) * 0.5);
        while ((ti + 1) * (ti + 2) / 2 <= lin) ++ti;
        while (ti * (ti + 1) / 2 > lin) --ti;
        tj = lin - ti * (ti + 1) / 2;
        if (ti >= T) return;
    }
    const bool look = j1 < k;
    const int nbn = look ? min(NB, k - j1) : 0;
    const int rbase = is_la ? j1 : j1 + ti * ST, cbase = j1 + tj * ST;
    PROBE(0);
#ifdef MGB_STEP_PROBE
    if (is_la && BR.front == 0 && tid == 0 && j0 == 64 && PROBE_NFRONTS == 1 && F.k > 400) g_probe[34] = clock64();
#endif
    const int fr16 = lane & 15, fk = lane >> 4;

    // ---- global loads first: raw panel slices and this wave's part of the C tile -----------------
    double pa[NB * ST / 256], pb[NB * ST / 256];
#pragma unroll
    for (int u = 0; u < NB * ST / 256; ++u) {
        const int i = tid + 256 * u, rr = i % ST, q = i / ST;
        const int r = rbase + rr, c = cbase + rr;
        const bool rin = is_la ? (rr < nbn) : (r < m);
        pa[u] = (q < nb && rin) ? W[r + (int64_t)(j0 + q) * m] : 0.0;
        pb[u] = (!is_la && ti != tj && q < nb && c < m) ? W[c + (int64_t)(j0 + q) * m] : 0.0;
    }
    double cw[4][4];
    if (!is_la) {
#pragma unroll
        for (int tb = 0; tb < 4; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rbase + 16 * wave + fr16, col = cbase + 16 * tb + fk + 4 * r;
                cw[tb][r] = (row < m && col < m && row >= col) ? W[row + (int64_t)col * m] : 0.0;
            }
    } else {
        // corner of the next diagonal block, entry (rr, c) per thread x 4
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = tid + 256 * t, rr = i % NB, c = i / NB;
            cw[0][t] = (look && rr >= c && rr < nbn) ? W[(j1 + rr) + (int64_t)(j1 + c) * m] : 0.0;
        }
    }
    // ---- W_j, d_j ----------------------------------------------------------------------------------
    if (do_diag) {
        for (int i = tid; i < NB * NB; i += 256) {
            const int rr = i % NB, c = i / NB;
            Dn[rr][c] = (rr >= c && rr < nb) ? W[(j0 + rr) + (int64_t)(j0 + c) * m] : 0.0;
        }
        __syncthreads();
        block_ldlt32(Dn, dq, nb, tid, is_la ? status : nullptr);
        block_inverse32_sel(Dn, Wv, Tm, tid);
    } else {
        for (int i = tid; i < NB * NB; i += 256) {        // the slot format of block0_to_slot, read back
            const int rr = i % NB, c = i / NB;
            const double v = (rr >= c && rr < nb) ? slot[rr + NB * c] : 0.0;
            Wv[rr][c] = (rr > c) ? v : (rr == c ? 1.0 : 0.0);
            if (rr == c) dq[rr] = (rr < nb) ? v : 1.0;
        }
    }
#pragma unroll
    for (int u = 0; u < NB * ST / 256; ++u) {
        const int i = tid + 256 * u, rr = i % ST, q = i / ST;
        Pa[q][rr] = pa[u];
        Pb[q][rr] = pb[u];
    }
    __syncthreads();
    PROBE(1);
    if (tid < NB) rdq[tid] = 1.0 / dq[tid];
    // home of block j (nobody reads it during this step): M_j = W_j' D_j^{-1} W_j, the inverse of the updated
    // diagonal block -- the triangular sweeps need nothing else of the block (mf_fwd_inv / mf_bwd_inv).
    // Strictly upper triangle = off-diagonal of M_j, diagonal of M_j to dvec.  One 16 x 16 tile per wave on the
    // matrix cores, straight from the accumulators (the tile above the diagonal is the mirror image: skipped).
    // Written by tile workgroup 0 (done at 6 us, every workgroup has W_j staged) rather than by the look-ahead
    // workgroup, whose 1.7 us for it sat on the critical path of the pivot chain; steps without tiles keep it there.
    if (is_la ? T == 0 : BR.first_tile()) {          // T is this front's own tile count (a batch is launched for its largest front)
        {
            const int rt = wave & 1, ct = wave >> 1;
            if (ct <= rt) {
                double4_t accm = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = 0; kk < NB / 4; ++kk) {
                    const int kq = 4 * kk + fk;
                    accm = __builtin_amdgcn_mfma_f64_16x16x4f64(kq < nb ? Wv[kq][16 * ct + fr16] / dq[kq] : 0.0, Wv[kq][16 * rt + fr16], accm, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * rt + fr16, col = 16 * ct + fk + 4 * r;
                    if (row < nb && col < row) W[(j0 + col) + (int64_t)(j0 + row) * m] = accm[r];
                    else if (row < nb && col == row) dvec[F.idx_off + j0 + row] = accm[r];
                }
            }
        }
    }
    if (is_la && !look) return;
    __syncthreads();
    PROBE(2);
    // ---- S (into Pa) and L (into Pb) ---------------------------------------------------------------
    if (is_la) {
        if (wave < 2) slice_transform(Pa, Pa, Pb, Wv, rdq, lane, wave);     // 32 rows of the next block
        __syncthreads();
        PROBE(3);
        {   // D_{j+1} = corner - S L' on the matrix cores: wave w -> (row tile w & 1, column tile w >> 1)
            const int rt = wave & 1, ct = wave >> 1;
            double4_t accd = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < NB / 4; ++kk)
                accd = __builtin_amdgcn_mfma_f64_16x16x4f64(Pb[4 * kk + fk][16 * ct + fr16], Pa[4 * kk + fk][16 * rt + fr16],
                                                            accd, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = 16 * rt + fr16, c = 16 * ct + fk + 4 * r;
                Dn[rr][c] = -accd[r];        // the corner entries are added by their loader threads below
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = tid + 256 * t, rr = i % NB, c = i / NB;
            Dn[rr][c] = (rr >= c && rr < nbn) ? cw[0][t] + Dn[rr][c] : 0.0;
        }
        __syncthreads();
        double* nslot = dscr + ((int64_t)BR.front * 2 + ((j1 / NB) & 1)) * (NB * NB);
        PROBE(4);
#ifdef MGB_STEP_PROBE
        // cold / warm experiment: the same factorization twice (Dn saved and restored in between)
        double sv[4];
        for (int t = 0; t < 4; ++t) { const int i = tid + 256 * t; sv[t] = Dn[i % NB][i / NB]; }
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        if (is_la && BR.front == 0 && tid == 0 && j0 == 64 && PROBE_NFRONTS == 1 && F.k > 400) { g_probe[32] = clock64(); g_probe[36] = wall_clock64(); }
        __builtin_amdgcn_sched_barrier(0);
        block_ldlt32(Dn, dq, nbn, tid, nullptr);
        __builtin_amdgcn_sched_barrier(0);
        if (is_la && BR.front == 0 && tid == 0 && j0 == 64 && PROBE_NFRONTS == 1 && F.k > 400) { g_probe[33] = clock64(); g_probe[37] = wall_clock64(); }
        __builtin_amdgcn_sched_barrier(0);
        for (int t = 0; t < 4; ++t) { const int i = tid + 256 * t; Dn[i % NB][i / NB] = sv[t]; }
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        if (is_la && BR.front == 0 && tid == 0 && j0 == 64 && PROBE_NFRONTS == 1 && F.k > 400) { g_probe[38] = clock64(); g_probe[44] = wall_clock64(); }
        __builtin_amdgcn_sched_barrier(0);
#endif
        block_ldlt32(Dn, dq, nbn, tid, status);
#ifdef MGB_STEP_PROBE
        __builtin_amdgcn_sched_barrier(0);
        if (is_la && BR.front == 0 && tid == 0 && j0 == 64 && PROBE_NFRONTS == 1 && F.k > 400) { g_probe[39] = clock64(); g_probe[45] = wall_clock64(); }
        __builtin_amdgcn_sched_barrier(0);
#endif
        PROBE(5);
        block_inverse32_sel(Dn, Wv, Tm, tid);
        PROBE(6);
        for (int i = tid; i < NB * NB; i += 256) {        // block0_to_slot's store (its phases written out: the probe stamps each)
            const int rr = i % NB, c = i / NB;
            if (rr >= c && rr < nbn) nslot[rr + NB * c] = (rr == c) ? dq[rr] : Wv[rr][c];
        }
        PROBE(7);
#ifdef MGB_STEP_PROBE
        if (is_la && BR.front == 0 && tid == 0 && j0 == 64 && PROBE_NFRONTS == 1 && F.k > 400) g_probe[35] = clock64();
#endif
        return;
    }
    if (ti == tj) {
        slice_transform(Pa, Pa, Pb, Wv, rdq, lane, wave);
    } else {
        slice_transform(Pa, Pa, nullptr, Wv, rdq, lane, wave);
        // the column-side slice: L = (A W') D^{-1}
        {
            const int rr = 16 * wave + fr16;
            double4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < NB / 4; ++kk) {
                const double a = Pb[4 * kk + fk][rr];
                if (kk < 4) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(Wv[fr16][4 * kk + fk], a, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Wv[16 + fr16][4 * kk + fk], a, acc1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q0 = fk + 4 * r, q1 = 16 + fk + 4 * r;
                Pb[q0][rr] = acc0[r] * rdq[q0];
                Pb[q1][rr] = acc1[r] * rdq[q1];
            }
        }
    }
    __syncthreads();
    PROBE(3);
    // ---- C -= S L' : wave w owns rows 16w..16w+15, four 16-column tiles ---------------------------
    double4_t acc[4];
#pragma unroll
    for (int tb = 0; tb < 4; ++tb) acc[tb] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < NB / 4; ++kk) {
        const double s = Pa[4 * kk + fk][16 * wave + fr16];            // y[k][j]: S[rr = j][q = k]
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) {
            if (ti == tj && tb > wave) continue;                          // strictly above the diagonal
            acc[tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(Pb[4 * kk + fk][16 * tb + fr16], s, acc[tb], 0, 0, 0);
        }
    }
    const int nskip = (BR.first_tile() && look) ? nbn : 0;               // corner owned by the look-ahead workgroup
#pragma unroll
    for (int tb = 0; tb < 4; ++tb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = rbase + 16 * wave + fr16, col = cbase + 16 * tb + fk + 4 * r;
            if (row < m && col < m && row >= col && !(row - j1 < nskip && col - j1 < nskip))
                W[row + (int64_t)col * m] = cw[tb][r] - acc[tb][r];
        }
    PROBE(4);
}

// Interface front of a domain-decomposed system: only its lower triangle is meaningful, so only that crosses ranks --
// packed column by column (column c at c*m - c(c-1)/2, rows c .. m-1), summed, unpacked in place.
__global__ __launch_bounds__(256) void mf_tri_pack(int m, const double* __restrict__ F, double* __restrict__ packed, int unpack,
                                                   double* __restrict__ Fout) {
    const int c = blockIdx.x;
    if (c >= m) return;
    const int64_t base = (int64_t)c * m - ((int64_t)c * (c - 1)) / 2;
    for (int r = c + threadIdx.x; r < m; r += 256) {
        if (unpack) Fout[r + (int64_t)c * m] = packed[base + (r - c)];
        else packed[base + (r - c)] = F[r + (int64_t)c * m];
    }
}

// First diagonal block of every front of a batch, factored and inverted once (one workgroup per front)
// into slot 0.  Used for batches of many fronts, where the redundant factorization inside every trailing
// tile of step 0 (do_diag) would occupy all compute units with copies of the same 32 x 32 problem.
__global__ __launch_bounds__(256) void mf_big_diag0(const FrontDev* __restrict__ fr, int32_t first,
                                                    const double* __restrict__ arena, double* __restrict__ dscr,
                                                    int32_t* __restrict__ status) {
    __shared__ double Wv[NB][NB + 1];
    __shared__ double Dn[NB][NB + 1];
    __shared__ double Tm[16][17];
    __shared__ double dq[NB];
    const FrontDev F = fr[first + blockIdx.x];
    const int m = F.m, nb = min(NB, F.k), tid = threadIdx.x;
    const double* W = arena + F.F_off;
    for (int i = tid; i < NB * NB; i += 256) {
        const int rr = i % NB, c = i / NB;
        Dn[rr][c] = (rr >= c && rr < nb) ? W[rr + (int64_t)c * m] : 0.0;
    }
    __syncthreads();
    block0_to_slot(Dn, Wv, Tm, dq, nb, tid, status, dscr + (int64_t)blockIdx.x * 2 * (NB * NB));
}

// ---- triangular solves on the inverse-based layout: one workgroup per front --------------------
// forward, block j of a front:  u_j = M_j t_j,  t[r] -= A[r, j] u_j  (r below);  the stored intermediate is u
// (M_j = A_jj^{-1} of the updated diagonal block = W_j' D_j^{-1} W_j, written home by mf_big_step)
__global__ __launch_bounds__(BIGI_THREADS) void mf_fwd_inv(const FrontDev* __restrict__ fr, int32_t first,
                                                           const int32_t* __restrict__ front_idx,
                                                           const int64_t* __restrict__ ug_ptr,
                                                           const int64_t* __restrict__ ug_src,
                                                           const double* __restrict__ arena,
                                                           const double* __restrict__ dvec,
                                                           const double* __restrict__ b, double* __restrict__ y,
                                                           double* __restrict__ uvec) {
    extern __shared__ double sh[];
#ifdef MGB_STEP_PROBE
#define FP(i) do { if (threadIdx.x == 0 && gridDim.x > 150) { const long long _t = wall_clock64(); if (blockIdx.x == 0) g_probe[48 + i] = _t; if (i == 0) atomicMin((unsigned long long*)&g_probe[56], (unsigned long long)_t); if (i == 5) { atomicMax((unsigned long long*)&g_probe[57], (unsigned long long)_t); atomicAdd((unsigned long long*)&g_probe[58], (unsigned long long)(_t - g_probe[56])); } } } while (0)
#else
#define FP(i) do { } while (0)
#endif
    FP(0);
    const FrontDev F = fr[first + blockIdx.x];
    const int m = F.m, k = F.k;
    const int tid = threadIdx.x, nt = BIGI_THREADS;
    double* tl = sh;                               // [m]
    double* Ml = sh + ((m + 1) & ~1);              // [NB][NB + 1]: M_j, full symmetric
    double* uq = Ml + NB * (NB + 1);               // [NB]
    double* part = uq + 2 * NB;                    // [BIGI_THREADS] partial sums of the column-split row update
    const int32_t* idx = front_idx + F.idx_off;
    const double* Fm = arena + F.F_off;
    const double* dv = dvec + F.idx_off;
    {   // t = [b(piv); 0] + the children's update vectors: one gather per entry, contributions in child order
        const int64_t* up = ug_ptr + F.ug_off;
        for (int j = tid; j < m; j += nt) {
            double v = (j < k) ? b[idx[j]] : 0.0;
            const int64_t e1 = up[j + 1];
            for (int64_t e = up[j]; e < e1; e += 4) {           // four contributions in flight, added in list order
                double a[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] = (e + u < e1) ? uvec[ug_src[e + u]] : 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) v += a[u];
            }
            tl[j] = v;
        }
    }
    const int wa = tid % NB, wb = tid / NB;          // M_j[wb][wa] = M_j[wa][wb] sits at (j0 + wa, j0 + wb), wa < wb
    {
        const double w0 = (wa < wb && wb < k) ? Fm[wa + (int64_t)wb * m] : 0.0;
        if (wa < wb) { Ml[wb * (NB + 1) + wa] = w0; Ml[wa * (NB + 1) + wb] = w0; }
        if (tid < NB) Ml[tid * (NB + 1) + tid] = (tid < k) ? dv[tid] : 0.0;
    }
    __syncthreads();
    FP(1);
    for (int j0 = 0; j0 < k; j0 += NB) {
        const int nb = min(NB, k - j0), j1 = j0 + nb;
        // next block's M and the first 16 panel entries of this thread's row update: neither depends on this
        // block's product, so both are requested now and their latency runs under it
        const int jn = j0 + NB;
        const double wnext = (wa < wb && jn + wb < k) ? Fm[(jn + wa) + (int64_t)(jn + wb) * m] : 0.0;
        const double dnext = (tid < NB && jn + tid < k) ? dv[jn + tid] : 0.0;
        const int rows = m - j1;
        int G = 1;
        while (G < 8 && 2 * G * rows <= nt) G *= 2;
        const int cgp = (G > 1 && rows > 0) ? tid / rows : 0, rr = (G > 1 && rows > 0) ? tid - cgp * rows : tid;
        const bool mine = rows > 0 && (G == 1 ? tid < rows : cgp < G);
        const int cstep = G == 1 ? 1 : G;                 // G == 1: columns 0..15 now, 16..31 later; G > 1: all 32 / G columns
        double pa[16], pc[16];
        {
            const double* Ar = Fm + (j1 + rr) + (int64_t)j0 * m;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int col = cgp + u * cstep;
                pa[u] = (mine && col < NB) ? Ar[(int64_t)min(col, nb - 1) * m] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) pc[u] = (mine && G == 1) ? Ar[(int64_t)min(16 + u, nb - 1) * m] : 0.0;
        }
        {   // u = M_j t_j on all 1024 threads: thread (q, c) forms one term, a 32-lane butterfly sums the row
            const int q = tid >> 5, c = tid & 31;
            double pu = Ml[q * (NB + 1) + c] * (c < nb ? tl[j0 + c] : 0.0);
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) pu += __shfl_xor(pu, off, 32);
            if (c == 0) uq[q] = (q < nb) ? pu : 0.0;
        }
        __syncthreads();
        FP(3);
        // M_j is consumed: stage M_{j+1} (the barrier at the end of the step publishes it)
        if (wa < wb) { Ml[wb * (NB + 1) + wa] = wnext; Ml[wa * (NB + 1) + wb] = wnext; }
        if (tid < NB) {
            Ml[tid * (NB + 1) + tid] = dnext;
            if (tid < nb) tl[j0 + tid] = uq[tid];          // the intermediate the backward sweep starts from
        }
        {   // rows below the block: t[r] -= A[r, j0 .. j1) u.  The panel is column-major, so a thread's 32 terms are
            // 32 strided loads; they are issued in groups (a rolled loop waits one memory latency per term, a 32-way
            // unroll spills at 1024 threads), and fronts with few rows split the columns over G thread groups so that
            // all 1024 threads carry loads; the partial sums meet in LDS in a fixed order.
            if (rows > 0 && G == 1) {
                if (mine) {
                    double v = 0.0;
#pragma unroll
                    for (int u = 0; u < 16; ++u) v += pa[u] * uq[u];                  // uq is zero beyond nb
#pragma unroll
                    for (int u = 0; u < 16; ++u) v += pc[u] * uq[16 + u];
                    tl[j1 + tid] -= v;
                }
                for (int r = j1 + tid + nt; r < m; r += nt) {
                    const double* Ar = Fm + r + (int64_t)j0 * m;
                    double v = 0.0;
                    for (int c0 = 0; c0 < nb; c0 += 8) {
                        double a[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) a[u] = Ar[(int64_t)min(c0 + u, nb - 1) * m];
#pragma unroll
                        for (int u = 0; u < 8; ++u) v += a[u] * uq[c0 + u];
                    }
                    tl[r] -= v;
                }
            } else if (rows > 0) {
                if (cgp < G) {
                    double v = 0.0;
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const int col = cgp + u * G;
                        v += pa[u] * (col < nb ? uq[col] : 0.0);
                    }
                    part[cgp * rows + rr] = v;
                }
                __syncthreads();
                if (tid < rows) {
                    double v = 0.0;
                    for (int gg = 0; gg < G; ++gg) v += part[gg * rows + tid];
                    tl[j1 + tid] -= v;
                }
            }
        }
        __syncthreads();
        FP(4);
    }
    for (int j = tid; j < m; j += nt) {
        if (j < k) y[idx[j]] = tl[j];
        else uvec[F.u_off + j - k] = tl[j];
    }
    FP(5);
}

// backward:  x_j = u_j - M_j G_j,  G[q] = sum over solved rows r of A[r, q] x[r]
#ifdef MGB_PROBE_BWD       // root front of a sweep: phase timestamps (tools/gpu_probe_bwd.py; build with -DMGB_STEP_PROBE -DMGB_PROBE_BWD:
                           // the slots are shared with the mf_big_step probes).  -DMGB_PROBE_BWD=2: the first front of the
                           // two-front level below the root instead (k about 255 with a boundary of about 512 rows at L = 9)
#define BP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0 && gridDim.x == (MGB_PROBE_BWD) && fr[first].k > 400 / (MGB_PROBE_BWD)) g_probe[(i)] = wall_clock64(); } while (0)
#else
#define BP(i) do { } while (0)
#endif
// One front of a backward launch.  SPLIT = false: the whole front in this workgroup (mf_bwd_inv, `fi` = blockIdx.x).
// SPLIT = true (mf_bwd_inv_split, grid (S, count)): the boundary product of front `fi` is shared by columns among the S
// workgroups of blockIdx.x -- 4-column group g goes to wave g % 16 of workgroup (g / 16) % S, the loop and the reductions
// are those of the unsplit kernel -- and lands in gscr (gstride doubles per front of the launch).  Hand-off without
// waiting: a workgroup publishes its columns (write-through stores, drained by every wave; one agent-scope release), then
// takes a ticket on cnt[fi]; every ticket but the last returns, the last workgroup to arrive resets the counter, reads all
// k products back past its L1 and runs the block recurrence.  No loop waits on another workgroup's memory.
template <bool SPLIT>
__device__ __forceinline__ void bwd_inv_front(const FrontDev* __restrict__ fr, int32_t first, uint32_t fi,
                                              const int32_t* __restrict__ front_idx, const double* __restrict__ arena,
                                              const double* __restrict__ dvec, const double* __restrict__ y,
                                              double* __restrict__ x, double* gscr, int gstride, uint32_t* cnt) {
    extern __shared__ double sh[];
    BP(0);
    const FrontDev F = fr[first + fi];
    const int m = F.m, k = F.k;
    const int tid = threadIdx.x, nt = BIGI_THREADS;
    const int lane = tid & 63, wave = tid >> 6;
    double* tl = sh;                               // [m]: u on the pivots (then x), x(boundary) below
    double* gl = sh + ((m + 1) & ~1);              // [k]
    double* Ml = gl + ((k + 1) & ~1);              // [NB][NB + 1]
    double* zq = Ml + NB * (NB + 1);               // [NB]
    int32_t* il = reinterpret_cast<int32_t*>(zq + 2 * NB);    // [m]: the front's index list (x_j is scattered through it)
    const int32_t* idx = front_idx + F.idx_off;
    const double* Fm = arena + F.F_off;
    const double* dv = dvec + F.idx_off;
    for (int j = tid; j < m; j += nt) {
        const int32_t ij = idx[j];
        il[j] = ij;
        tl[j] = (j < k) ? y[ij] : x[ij];
    }
    __syncthreads();
    BP(1);
    // boundary rows: one wave per pivot column, coalesced along rows; four columns per pass so that their loads
    // and butterflies overlap (a wave owns up to k / 16 columns, each a dependent load -> reduce chain)
    // A front with a handful of boundary rows (the root: the border row alone) takes one thread per column instead: the
    // butterflies of 511 columns for one row each kept the LDS pipeline of the workgroup busy for 17 us.
    if (SPLIT) {
        const bool thin = m - k <= 8;
        const int S = (int)gridDim.x, part = (int)blockIdx.x;
        double* gs = gscr + (int64_t)fi * gstride;                     // k <= gstride: the launch's max_k, rounded up
        if (!thin)
            for (int q0 = 4 * (wave + (nt / 64) * part); q0 < k; q0 += 4 * (nt / 64) * S) {
                double s[4] = {0.0, 0.0, 0.0, 0.0};                    // the unsplit loop below, column for column
                for (int r = k + lane; r < m; r += 64) {
                    const double t = tl[r];
#pragma unroll
                    for (int u = 0; u < 4; ++u) s[u] += Fm[(int64_t)min(q0 + u, k - 1) * m + r] * t;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s[u] += quad_perm_f64<0xB1>(s[u]);
                    s[u] += quad_perm_f64<0x4E>(s[u]);
                    s[u] += quad_perm_f64<0x124>(s[u]);
                    s[u] += quad_perm_f64<0x128>(s[u]);
                    s[u] += __shfl_xor(s[u], 16, 64);
                    s[u] += __shfl_xor(s[u], 32, 64);
                }
                if (lane < 4 && q0 + lane < k)
                    __hip_atomic_store(gs + q0 + lane, s[lane == 0 ? 0 : (lane == 1 ? 1 : (lane == 2 ? 2 : 3))], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // every storing wave drains its stores ...
        __syncthreads();
        uint32_t* ticket = reinterpret_cast<uint32_t*>(zq);            // (zq is first written inside the block loop)
        if (tid == 0) {                                                // ... one lane releases and takes the ticket
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t t = __hip_atomic_fetch_add(cnt + fi, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t == (uint32_t)(S - 1)) {                              // last to arrive: every other workgroup's columns are out
                __hip_atomic_store(cnt + fi, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            ticket[0] = t;
        }
        __syncthreads();
        if (ticket[0] != (uint32_t)(S - 1)) return;
        if (!thin)
            for (int q = tid; q < k; q += nt) gl[q] = __hip_atomic_load(gs + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (m - k <= 8) {
        for (int q = tid; q < k; q += nt) {
            const double* Aq = Fm + (int64_t)q * m;
            double sq = 0.0;
            for (int r = k; r < m; ++r) sq += Aq[r] * tl[r];
            gl[q] = sq;
        }
    } else if (!SPLIT)
    for (int q0 = 4 * wave; q0 < k; q0 += 4 * (nt / 64)) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int r = k + lane; r < m; r += 64) {
            const double t = tl[r];
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] += Fm[(int64_t)min(q0 + u, k - 1) * m + r] * t;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {           // rows of 16 lanes on the data-parallel path, the four rows through the crossbar
            s[u] += quad_perm_f64<0xB1>(s[u]);
            s[u] += quad_perm_f64<0x4E>(s[u]);
            s[u] += quad_perm_f64<0x124>(s[u]);
            s[u] += quad_perm_f64<0x128>(s[u]);
            s[u] += __shfl_xor(s[u], 16, 64);
            s[u] += __shfl_xor(s[u], 32, 64);
        }
        if (lane < 4 && q0 + lane < k) gl[q0 + lane] = s[lane == 0 ? 0 : (lane == 1 ? 1 : (lane == 2 ? 2 : 3))];
    }
    BP(2);
    const int wa = tid % NB, wb = tid / NB;
    const int last = ((k - 1) / NB) * NB;
    {
        const double w0 = (wa < wb && last + wb < k) ? Fm[(last + wa) + (int64_t)(last + wb) * m] : 0.0;
        if (wa < wb) { Ml[wb * (NB + 1) + wa] = w0; Ml[wa * (NB + 1) + wb] = w0; }
        if (tid < NB) Ml[tid * (NB + 1) + tid] = (last + tid < k) ? dv[last + tid] : 0.0;
    }
    __syncthreads();
    // Panel rows of a block step: G[q] += sum_u A[j0 + u, q] x[j0 + u] for every unsolved pivot column q < j0.  Column q
    // holds its 32 entries contiguously (256 B), so FOUR lanes share a column: per load instruction they cover 64
    // contiguous bytes (16-byte loads, 8-byte aligned) and a wave touches 16 cache lines instead of 64 -- one lane per
    // column made the texture addresser the bottleneck (6 us per step on the 511-pivot root front).  The four partial
    // sums meet in two butterfly steps, in a fixed order.
    struct __attribute__((aligned(8))) D2 { double a, b; };
    const int cq = tid >> 2, cp = tid & 3;           // column within a pass of nt / 4 columns, quarter of the column
    constexpr int CPP = BIGI_THREADS / 4;
    // The first two passes of a step's panel rows are requested at the top of the step and run under the block
    // product.  A column's base address is formed once.
    const double* col0 = Fm + (int64_t)min(cq, k - 1) * m + 2 * cp;
    const double* col1 = Fm + (int64_t)min(cq + CPP, k - 1) * m + 2 * cp;
    BP(3);
    for (int j0 = last; j0 >= 0; j0 -= NB) {
        const int nb = min(NB, k - j0);
        const int jn = j0 - NB;              // the next block is a full one
        if (j0 == 256) BP(4);
        if (j0 == 224) BP(8);
        const double wnext = (wa < wb && jn >= 0) ? Fm[(jn + wa) + (int64_t)(jn + wb) * m] : 0.0;
        const double dnext = (tid < NB && jn >= 0) ? dv[jn + tid] : 0.0;
        D2 pa[2][4];
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const double* Aq = (ps ? col1 : col0) + j0;
            if (cq + ps * CPP < j0) {
                if (nb == NB) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) pa[ps][t] = *reinterpret_cast<const D2*>(Aq + 8 * t);
                } else {             // only the first step of a sweep can be a partial block
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int o = 2 * cp + 8 * t;
                        pa[ps][t].a = Aq[min(o, nb - 1) - 2 * cp];
                        pa[ps][t].b = Aq[min(o + 1, nb - 1) - 2 * cp];
                    }
                }
            }
        }
        {   // x_j = u_j - M_j G_j with all 1024 threads (see the forward sweep)
            const int q = tid >> 5, c = tid & 31;
            double ph = Ml[q * (NB + 1) + c] * (c < nb ? gl[j0 + c] : 0.0);
            ph += quad_perm_f64<0xB1>(ph);          // quads, then rotations by 4 and 8 inside the row of 16 lanes (DPP) ...
            ph += quad_perm_f64<0x4E>(ph);
            ph += quad_perm_f64<0x124>(ph);
            ph += quad_perm_f64<0x128>(ph);
            ph += __shfl_xor(ph, 16, 32);           // ... and one exchange between the two rows through the LDS crossbar
            if (c == 0) zq[q] = (q < nb) ? tl[j0 + q] - ph : 0.0;
        }
        if (j0 == 256) BP(5);
        __syncthreads();
        if (j0 == 256) BP(6);
        if (tid < nb) x[il[j0 + tid]] = zq[tid];
        if (wa < wb) { Ml[wb * (NB + 1) + wa] = wnext; Ml[wa * (NB + 1) + wb] = wnext; }
        if (tid < NB) Ml[tid * (NB + 1) + tid] = dnext;
        double zr[8];                        // this lane's eight entries of x_j (zero beyond nb)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            zr[2 * t] = zq[2 * cp + 8 * t];
            zr[2 * t + 1] = zq[2 * cp + 8 * t + 1];
        }
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int q = cq + ps * CPP;
            if (q < j0) {                    // the four lanes of a column decide alike
                double v = 0.0;
#pragma unroll
                for (int t = 0; t < 4; ++t) v += pa[ps][t].a * zr[2 * t] + pa[ps][t].b * zr[2 * t + 1];
                v += quad_perm_f64<0xB1>(v);
                v += quad_perm_f64<0x4E>(v);
                if (cp == 0) gl[q] += v;
            }
        }
        for (int q = cq + 2 * CPP; q - cq < j0; q += CPP) {          // fronts with more than 512 unsolved columns
            const double* Aq = Fm + (int64_t)min(q, j0 - 1) * m + j0 + 2 * cp;
            D2 a[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (nb == NB) a[t] = *reinterpret_cast<const D2*>(Aq + 8 * t);
                else {
                    const int o = 2 * cp + 8 * t;
                    a[t].a = Aq[min(o, nb - 1) - 2 * cp];
                    a[t].b = Aq[min(o + 1, nb - 1) - 2 * cp];
                }
            }
            double v = 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) v += a[t].a * zr[2 * t] + a[t].b * zr[2 * t + 1];
            v += quad_perm_f64<0xB1>(v);
            v += quad_perm_f64<0x4E>(v);
            if (cp == 0 && q < j0) gl[q] += v;
        }
        if (j0 == 256) BP(7);
        __syncthreads();
    }
    BP(9);
}

__global__ __launch_bounds__(BIGI_THREADS) void mf_bwd_inv(const FrontDev* __restrict__ fr, int32_t first,
                                                           const int32_t* __restrict__ front_idx,
                                                           const double* __restrict__ arena,
                                                           const double* __restrict__ dvec,
                                                           const double* __restrict__ y, double* __restrict__ x) {
    bwd_inv_front<false>(fr, first, blockIdx.x, front_idx, arena, dvec, y, x, nullptr, 0, nullptr);
}
// grid (S, count), S = bwd_inv_split of the launch (mf_launch_plan.hpp)
__global__ __launch_bounds__(BIGI_THREADS) void mf_bwd_inv_split(const FrontDev* __restrict__ fr, int32_t first,
                                                                 const int32_t* __restrict__ front_idx,
                                                                 const double* __restrict__ arena,
                                                                 const double* __restrict__ dvec,
                                                                 const double* __restrict__ y, double* __restrict__ x,
                                                                 double* gscr, int gstride, uint32_t* cnt) {
    bwd_inv_front<true>(fr, first, blockIdx.y, front_idx, arena, dvec, y, x, gscr, gstride, cnt);
}

// ---- host launchers ------------------------------------------------------------------------------------------
inline void launch_big_diag0(const FactorArgs& a, const MfLaunch& L, int nfronts) {
    hipLaunchKernelGGL(mf_big_diag0, dim3(nfronts), dim3(256), 0, a.st, a.fr, L.first, a.arena, a.dscr, a.status);
}
// The pivot chain of `nfronts` assembled fronts, one launch per 32-column step.  Block 0 is already factored (by the
// gather launch or mf_big_diag0) unless diag_in_step0: then every tile of step 0 factors it redundantly.
inline void launch_inv_steps(const FactorArgs& a, const MfLaunch& L, int nfronts, bool diag_in_step0) {
    for (int j0 = 0; j0 < L.max_k; j0 += NB) {
        const int rem = L.max_m - j0;
        const int T = std::max(0, (rem - 1 + ST - 1) / ST);
        const RolesGrid g = roles_grid(a.step_roles, nfronts, T * (T + 1) / 2);     // the look-ahead workgroup + the trailing tiles
        hipLaunchKernelGGL(mf_big_step, dim3(g.x, g.y), dim3(256), 0, a.st, a.fr, L.first, j0, a.arena, a.dscr, a.dvec, a.status,
                           (j0 == 0 && diag_in_step0) ? 1 : 0, a.step_roles);
    }
}

// lower triangle of an m x m front <-> (m + 1) m / 2 packed doubles (the interface front's sum over ranks)
inline void launch_tri_pack(int m, double* F, double* packed, bool unpack, hipStream_t st) {
    hipLaunchKernelGGL(mf_tri_pack, dim3(m), dim3(256), 0, st, m, unpack ? (const double*)nullptr : F, packed, unpack ? 1 : 0,
                       unpack ? F : (double*)nullptr);
}

// mf_fwd_inv: work vector, diagonal block, two block vectors, the partial sums of the column-split row update
inline size_t fwd_inv_lds(int max_m) {
    return (size_t)(((max_m + 1) & ~1) + NB * (NB + 1) + 2 * NB + BIGI_THREADS) * sizeof(double);
}
// mf_bwd_inv: work vector, pivot part, diagonal block, two block vectors, half a vector of partial sums
inline size_t bwd_inv_lds(int max_m, int max_k) {
    return (size_t)(((max_m + 1) & ~1) + ((max_k + 1) & ~1) + NB * (NB + 1) + 2 * NB + (max_m + 1) / 2) * sizeof(double);
}
inline void launch_fwd_inv(const SolveArgs& a, const MfLaunch& L) {
    hipLaunchKernelGGL(mf_fwd_inv, dim3(L.count), dim3(BIGI_THREADS), fwd_inv_lds(L.max_m), a.st, a.fr, L.first, a.front_idx,
                       a.ug_ptr, a.ug_src, a.arena, a.dvec, a.b, a.y, a.uvec);
}
inline void launch_bwd_inv(const SolveArgs& a, const MfLaunch& L) {
    // few fronts with a real boundary: S workgroups per front share the boundary product (bwd_inv_split, mf_launch_plan.hpp)
    const int S = a.bwd_cnt ? bwd_inv_split(L.count, L.max_k, L.max_m) : 1;
    if (S > 1) {
        hipLaunchKernelGGL(mf_bwd_inv_split, dim3(S, L.count), dim3(BIGI_THREADS), bwd_inv_lds(L.max_m, L.max_k), a.st, a.fr, L.first,
                           a.front_idx, a.arena, a.dvec, a.y, a.x, a.bwd_g, (int)bwd_split_stride(L.max_k), a.bwd_cnt);
        return;
    }
    hipLaunchKernelGGL(mf_bwd_inv, dim3(L.count), dim3(BIGI_THREADS), bwd_inv_lds(L.max_m, L.max_k), a.st, a.fr, L.first,
                       a.front_idx, a.arena, a.dvec, a.y, a.x);
}

}  // namespace
}  // namespace mgbhip
