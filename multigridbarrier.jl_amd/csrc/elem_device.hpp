// elem_device.hpp -- device helpers shared by the element kernels (included by kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "node_core.hpp"

namespace mgbhip {

namespace {

// Sum of one double per thread over a 256-thread workgroup, result in thread 0: rows of 16 lanes on the data-parallel
// path (v_mov dpp: quad_perm 0xB1 / 0x4E, row_ror 4 / 8), the four rows of a wave through the crossbar, the four waves
// through LDS -- one barrier instead of the eight of an LDS tree (the tail of every element-kernel workgroup).
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)(b & 0xffffffffll), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// z0 + R s at row i.  Selection levels: the same arithmetic as prolong_kernel with a unit entry (v = z0; v += 1 * s[col]).
__device__ __forceinline__ double z_at(const ElemParams& P, int64_t i) {
    double v = P.z0[i];
    if (P.zsel) {
        const int32_t c = P.zsel[i];
        if (c >= 0) v += P.zx ? __builtin_fma(-P.zalpha, P.zx[c], P.zs[c]) : P.zs[c];      // the same fma as step_kernel
        if (P.zout) P.zout[i] = v;
    }
    return v;
}
__device__ __forceinline__ double wave_sum_dpp(double v) {
    v += dpp_mov_f64<0xB1>(v);
    v += dpp_mov_f64<0x4E>(v);
    v += dpp_mov_f64<0x124>(v);
    v += dpp_mov_f64<0x128>(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ double block_sum_256(double v, double* scratch4) {      // scratch4: 4 doubles of LDS, free to use
    v = wave_sum_dpp(v);
    if ((threadIdx.x & 63) == 0) scratch4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (scratch4[0] + scratch4[1]) + (scratch4[2] + scratch4[3]);
}

// fine broken-basis values of this lane's node, z0 + R*s (src/convex.jl:156), into zl [EPB][nu][G]
__device__ __forceinline__ void stage_z(const ElemParams& P, double* zl, int el, int nu, int G, int r, int64_t n, int64_t node) {
    for (int a = 0; a < nu; ++a) zl[(el * nu + a) * G + r] = z_at(P, (int64_t)a * n + node);
}
// One operator stage of a fast kernel -> LDS with 256 threads: all NIT loads are issued before the first LDS store (a
// rolled copy loop waits one memory latency per iteration).
template <int NIT>
__device__ __forceinline__ void copy_unrolled(const double* src, double* dst, int64_t lim, int tid) {
    double v[NIT];
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
        const int i = tid + 256 * u;
        v[u] = i < lim ? src[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
        const int i = tid + 256 * u;
        if (i < lim) dst[i] = v[u];
    }
}

}  // namespace


}  // namespace mgbhip
