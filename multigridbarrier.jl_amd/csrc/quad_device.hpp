// quad_device.hpp -- what the lane kernels of quadrature.hip and faces.hip share beyond the plan of quad_layout.hpp:
// the table repack, the write-out of the item values, the column reduction and the launcher.
// Internal linkage, like dsum.hpp and device_prims.hpp: each translation unit carries its own copy of what it uses, so
// only the two .hip files include it (the event record of their objects is CallEvents in common.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "common.hpp"
#include "dsum.hpp"
#include "quad_layout.hpp"

namespace mgbhip {

namespace {

// ---- host -----------------------------------------------------------------------------------------------------------

// 1: p = 1, 2: p = 2 (neither calls pow), 0: any other exponent
inline int quad_pmode(double pexp) { return pexp == 1.0 ? 1 : pexp == 2.0 ? 2 : 0; }

// phi (Q x p) and dphi (Q x p x d) to the kernels' tab [p][1 + d][Q], point fastest
inline void quad_repack_tables(int d, int p, int Q, const double* phi, const double* dphi, double* tab) {
    for (int q = 0; q < Q; ++q)
        for (int i = 0; i < p; ++i) {
            const size_t src = (size_t)q * p + i;
            tab[((size_t)i * (1 + d)) * Q + q] = phi[src];
            for (int b = 0; b < d; ++b) tab[((size_t)i * (1 + d) + 1 + b) * Q + q] = dphi[src * d + b];
        }
}

// One lane kernel over plan.grid workgroups; `who` ("quadrature", "faces") heads the error text.
template <auto Kernel, class Params>
void quad_launch(const char* who, const Params& P, const QuadPlan& plan, hipStream_t st) {
    static const bool big_lds = [] {          // opt-in to more than 64 KB of dynamic LDS, once per instantiation
        return hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)QUAD_LDS_MAX) == hipSuccess;
    }();
    if (plan.lds > 64 * 1024 && !big_lds) throw HipError(std::string(who) + ": the device refused the dynamic LDS opt-in");
    hipLaunchKernelGGL(Kernel, dim3((unsigned)plan.grid), dim3(QUAD_THREADS), plan.lds, st, P);
    MGB_HIP_CHECK(hipGetLastError());
}

// ---- device ---------------------------------------------------------------------------------------------------------

// a NaN on either side stays
__device__ __forceinline__ double quad_max(double a, double b) { return (b > a || b != b) ? b : a; }

// Three steps stay written out in both kernels, because as functions here they changed the kernels' device code
// (profiles/quad_faces_merge_isa.txt): the table staging and the tree width (the smallest power of two >= S) change the
// instruction streams of the element kernels that stage tables, and the halving tree over an item's S lanes (off = width
// / 2, ..., 1: lane s < off adds lane s + off while s + off < S, a barrier before every step and after the last; the
// element kernel's has a max branch, the face kernel's has not) took 2 more VGPRs in 26 of the 48 element kernels and 5
// of the 16 face kernels.  The tree leaves an item's sum in its first lane.

// the values of the group's nitems items, columns c0 .. c0 + nc, from the items' first lanes to out (items x ncol)
__device__ __forceinline__ void quad_write_items(double* out, const double* red, int tid, int64_t item0, int nitems, int S, int ncol,
                                                 int c0, int nc) {
    if (tid < nitems * nc) {
        const int gg = tid / nc, c = tid - gg * nc;
        out[(item0 + gg) * ncol + c0 + c] = red[c * QUAD_THREADS + gg * S];
    }
}

// totals[col] = the compensated sum (or the maximum) of column col of rows (n x ncol): one workgroup of 1024 lanes per
// column, lane t takes the rows t, t + 1024, ..., then the fixed shuffle tree and the 16 wave sums in order
__global__ __launch_bounds__(QUAD_REDUCE_THREADS) void quad_reduce_kernel(const double* __restrict__ rows, int64_t n, int ncol,
                                                                          int is_max, double* __restrict__ totals) {
    __shared__ double ws[QUAD_REDUCE_THREADS / 64], wc[QUAD_REDUCE_THREADS / 64];
    const int tid = threadIdx.x, col = blockIdx.x;
    constexpr int W = QUAD_REDUCE_THREADS / 64;
    if (is_max) {
        double m = 0.0;
        for (int64_t i = tid; i < n; i += QUAD_REDUCE_THREADS) m = quad_max(m, rows[i * ncol + col]);
        for (int off = 32; off > 0; off >>= 1) m = quad_max(m, __shfl_down(m, off, 64));
        if ((tid & 63) == 0) ws[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < W; ++w) m = quad_max(m, ws[w]);
            totals[col] = m;
        }
        return;
    }
    DSum a;
#pragma unroll 4                // the loads do not depend on the sum: four in flight per lane, added in order
    for (int64_t i = tid; i < n; i += QUAD_REDUCE_THREADS) a.add(rows[i * ncol + col]);
    dsum_wave_reduce(a);
    if ((tid & 63) == 0) { ws[tid >> 6] = a.s; wc[tid >> 6] = a.c; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < W; ++w) a.merge(ws[w], wc[w]);
        totals[col] = a.value();
    }
}

void quad_reduce_columns(const double* rows, int64_t n, int32_t ncol, bool is_max, double* totals, hipStream_t st) {
    hipLaunchKernelGGL(quad_reduce_kernel, dim3((unsigned)ncol), dim3(QUAD_REDUCE_THREADS), 0, st, rows, n, (int)ncol, is_max ? 1 : 0,
                       totals);
    MGB_HIP_CHECK(hipGetLastError());
}

}  // namespace

}  // namespace mgbhip
