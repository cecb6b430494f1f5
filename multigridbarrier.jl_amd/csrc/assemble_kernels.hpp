// assemble_kernels.hpp -- gather assembly of R'HR from the element-block slab (included by kernels.hip).
#pragma once
#include "reduce_kernels.hpp"

namespace mgbhip {

namespace {

// ---- assembly ------------------------------------------------------------------------------------

// Row-owner gather: every structural nonzero of R'HR sums its contributions from the
// element-block slab in a fixed order -- no atomics (the reference's CUDA path uses fp64
// atomics, ext/MultiGridBarrierCUDAExt/block_ops.jl:229-249).
// cidx == nullptr: the slab is already in list order (projected levels: the projection kernels scatter through
// PanelParams::spos, so a list is a contiguous run and the gather streams it).
// qmap (optional): the positions to assemble -- the Newton loop forms the UPPER triangle only (`symmetric(H)` and the
// factorization read nothing else, mf_analysis.cpp), nq of the nnz structural nonzeros.
__global__ __launch_bounds__(256) void gather_assemble_kernel(int64_t nq, const int32_t* __restrict__ qmap,
                                                              const int32_t* __restrict__ cptr,
                                                              const int32_t* __restrict__ cidx,
                                                              const double* __restrict__ slab,
                                                              double* __restrict__ Hval) {
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    const int64_t q = qmap ? qmap[qi] : qi;
    const int32_t beg = cptr[q], end = cptr[q + 1];
    if (end - beg <= 4) {              // a handful of element contributions: nothing to compensate
        double s = 0.0;
        for (int32_t t = beg; t < end; ++t) s += slab[cidx ? cidx[t] : t];
        Hval[q] = s;
        return;
    }
    DSum a;
    for (int32_t t = beg; t < end; ++t) a.add(slab[cidx ? cidx[t] : t]);
    Hval[q] = a.value();
}

// Direct-value levels: only the structural nonzeros shared between elements are summed (into a compact array
// behind the slab); the single-contribution ones are read from the slab by the factorization itself.
__global__ __launch_bounds__(256) void gather_shared_kernel(int64_t nshared, const int32_t* __restrict__ sh_q,
                                                            const int32_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
                                                            const double* __restrict__ slab, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nshared) return;
    const int32_t q = sh_q[i];
    const int32_t beg = cptr[q], end = cptr[q + 1];
    if (end - beg <= 4) {                                    // same rule and order as gather_assemble_kernel: bitwise the same sums
        double a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = (beg + u < end) ? slab[cidx[beg + u]] : 0.0;
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (beg + u < end) s += a[u];
        out[i] = s;
        return;
    }
    DSum acc;
    for (int32_t t = beg; t < end; t += 4) {                 // four contributions in flight, added in list order
        double a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = (t + u < end) ? slab[cidx[t + u]] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (t + u < end) acc.add(a[u]);
    }
    out[i] = acc.value();
}

// Long contribution lists (coarse levels: few unknowns, every element contributes): one wave per
// structural nonzero, lanes stride over the list, fixed-order shuffle reduction.
__global__ __launch_bounds__(256) void gather_assemble_wave_kernel(int64_t nq, const int32_t* __restrict__ qmap,
                                                                   const int32_t* __restrict__ cptr,
                                                                   const int32_t* __restrict__ cidx,
                                                                   const double* __restrict__ slab,
                                                                   double* __restrict__ Hval) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const int64_t q = qmap ? qmap[qi] : qi;
    DSum a;
    for (int32_t t = cptr[q] + lane; t < cptr[q + 1]; t += 64) a.add(slab[cidx ? cidx[t] : t]);
    dsum_wave_reduce(a);
    if (lane == 0) Hval[q] = a.value();
}

// Very long lists (the coarsest levels: a handful of nonzeros, each summing every element): one wave per
// (nonzero, chunk of the list), then one wave per nonzero over the chunk sums.  Fixed chunking and fixed
// shuffle trees: the result does not depend on scheduling.
__global__ __launch_bounds__(256) void gather_assemble_chunk_kernel(int64_t nq, const int32_t* __restrict__ qmap, int32_t ch,
                                                                    int32_t nchunk,
                                                                    const int32_t* __restrict__ cptr,
                                                                    const int32_t* __restrict__ cidx,
                                                                    const double* __restrict__ slab,
                                                                    double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nq * nchunk) return;
    const int64_t qi = w / nchunk;
    const int32_t c = (int32_t)(w - qi * nchunk);
    const int64_t q = qmap ? qmap[qi] : qi;
    const int32_t beg = cptr[q] + c * ch, end = min(cptr[q + 1], beg + ch);
    DSum a;
    for (int32_t t = beg + lane; t < end; t += 256) {      // four loads in flight per lane
        const int32_t t1 = t + 64, t2 = t + 128, t3 = t + 192;
        const double a0 = slab[cidx ? cidx[t] : t];
        const double a1 = t1 < end ? slab[cidx ? cidx[t1] : t1] : 0.0;
        const double a2 = t2 < end ? slab[cidx ? cidx[t2] : t2] : 0.0;
        const double a3 = t3 < end ? slab[cidx ? cidx[t3] : t3] : 0.0;
        a.add(a0); a.add(a1); a.add(a2); a.add(a3);
    }
    dsum_wave_reduce(a);
    if (lane == 0) { part[2 * w] = a.s; part[2 * w + 1] = a.c; }
}

__global__ __launch_bounds__(256) void gather_assemble_chunk_reduce(int64_t nq, const int32_t* __restrict__ qmap, int32_t nchunk,
                                                                    const double* __restrict__ part, double* __restrict__ Hval) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    DSum a;
    for (int32_t c = lane; c < nchunk; c += 64) a.merge(part[2 * (qi * nchunk + c)], part[2 * (qi * nchunk + c) + 1]);
    dsum_wave_reduce(a);
    if (lane == 0) Hval[qmap ? qmap[qi] : qi] = a.value();
}

}  // namespace

void launch_gather_assemble(int64_t nnz, const int32_t* cptr, const int32_t* cidx, const double* slab,
                            double* Hval, bool long_lists, hipStream_t st, int32_t chunk, int32_t nchunk, double* part,
                            const int32_t* qmap, int64_t nq) {
    if (nnz == 0) return;
    if (!qmap) nq = nnz;
    if (nq == 0) return;
    if (long_lists && nchunk > 1) {
        hipLaunchKernelGGL(gather_assemble_chunk_kernel, dim3((unsigned)((nq * nchunk + 3) / 4)), dim3(256), 0, st, nq, qmap, chunk,
                           nchunk, cptr, cidx, slab, part);
        hipLaunchKernelGGL(gather_assemble_chunk_reduce, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, nq, qmap, nchunk, part, Hval);
    } else if (long_lists)
        hipLaunchKernelGGL(gather_assemble_wave_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, nq, qmap, cptr,
                           cidx, slab, Hval);
    else
        hipLaunchKernelGGL(gather_assemble_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, nq, qmap, cptr,
                           cidx, slab, Hval);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_gather_shared(int64_t nshared, const int32_t* sh_q, const int32_t* cptr, const int32_t* cidx, const double* slab,
                          double* out, hipStream_t st) {
    if (nshared == 0) return;
    hipLaunchKernelGGL(gather_shared_kernel, dim3((unsigned)((nshared + 255) / 256)), dim3(256), 0, st, nshared, sh_q, cptr, cidx,
                       slab, out);
    MGB_HIP_CHECK(hipGetLastError());
}

}  // namespace mgbhip
