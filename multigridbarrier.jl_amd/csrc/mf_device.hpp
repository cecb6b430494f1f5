// mf_device.hpp -- what the kernel families of the numeric multifrontal LDL' share (mf_numeric.hip): tile constants,
// wave helpers (wave_sync, readlane / DPP broadcasts, row and wave sums, the v_rcp_f64 reciprocal), the offsets of
// packed triangles, the in-register LDL' of a diagonal block.
//
// Frontal layout: column-major m x m, ld = m.  After factorization columns [0,k) hold the
// strictly lower part of the unit-lower L panel with D on the diagonal; the trailing (m-k)^2
// lower triangle is the update matrix the parent reads.  Every extend-add runs child by child in a
// fixed order on disjoint destination columns: no atomics, bitwise reproducible factors.
//
// mf_device.hpp, mf_small.hpp, mf_big_subst.hpp, mf_big_inv.hpp and mf_big_assemble.hpp are included by mf_numeric.hip alone and form ONE
// translation unit on purpose: the probe build (-DMGB_STEP_PROBE, tools/gpu_probe*.py) shares one __device__ g_probe
// between the families, and the library is built without relocatable device code.  Each family header keeps the host
// launchers of its kernels beside them; a kernel with dynamic LDS has ONE size function (*_lds) that its launch and
// the > 64 KB opt-in of MfSolver::analyze() both use.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mf_solver.hpp"

namespace mgbhip {
namespace {

#ifdef MGB_STEP_PROBE      // development probe build only (tools/gpu_probe.py)
__device__ long long g_probe[64];
#define SPL(i) do { if (threadIdx.x == 0 && gridDim.x == 1024 && blockIdx.x == 700 && j0 == 0) g_probe[48 + i] = wall_clock64(); } while (0)
#define SP(i) do { if (threadIdx.x == 0 && gridDim.x == 4096 && blockIdx.x == 3000) g_probe[40 + i] = wall_clock64(); if (threadIdx.x == 0 && gridDim.x == 1024 && blockIdx.x == 700) g_probe[24 + i] = wall_clock64(); } while (0)
#else
#define SPL(i) do { } while (0)
#define SP(i) do { } while (0)
#endif

typedef double double4_t __attribute__((ext_vector_type(4)));
constexpr int TX = 16;    // row lanes of the 2-D thread maps
constexpr int NB = 32;    // panel width of the large-front path
constexpr int CT = 8;     // destination columns per workgroup in the large-front assembly (2 per wave)
constexpr int TR = 256;   // rows per workgroup in the panel solve
constexpr int ST = 64;    // tile edge of the symmetric update
constexpr int ASM_REL_LDS = 2048; // relative indices of one child kept in LDS by the large-front assembly
constexpr int CHILD_CHUNK = 64;   // child descriptors staged in LDS at a time

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Broadcast of a double from a compile-time lane through SGPRs (v_readlane_b32 x 2): cheaper than
// the LDS-crossbar path of __shfl when the source lane is a constant after unrolling.
__device__ __forceinline__ double readlane_f64(double v, int srclane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), srclane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), srclane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// Exchange of a double inside a quad of lanes on the data-parallel path (two v_mov_b32 dpp): quad_perm control
// 0xB1 = lanes [1,0,3,2] (xor 1), 0x4E = [2,3,0,1] (xor 2).  __shfl_xor goes through ds_bpermute, i.e. the LDS pipeline.
template <int CTRL>
__device__ __forceinline__ double quad_perm_f64(double v) {      // also row_ror:n (0x120 + n): rotation inside 16 lanes
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)(b & 0xffffffffll), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// Sum over a row of 16 lanes (every lane ends with it): no LDS traffic.
__device__ __forceinline__ double row16_sum_f64(double v) {
    v += quad_perm_f64<0xB1>(v);
    v += quad_perm_f64<0x4E>(v);
    v += quad_perm_f64<0x124>(v);
    v += quad_perm_f64<0x128>(v);
    return v;
}
// Sum over the wave: rows on the data-parallel path, the four rows through the crossbar (2 exchanges instead of 6).
__device__ __forceinline__ double wave_sum_f64(double v) {
    v = row16_sum_f64(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// 1/d by v_rcp_f64 and two Newton steps (the pivot chain of the in-register LDL' is latency
// bound; the full IEEE division sequence is twice as long).  Error < 1 ulp of the quotient, and
// LDL' is backward stable under any such perturbation of the multipliers.
__device__ __forceinline__ double fast_recip(double d) {
    double x = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, x, 1.0);
    x = __builtin_fma(x, e, x);
    e = __builtin_fma(-d, x, 1.0);
    x = __builtin_fma(x, e, x);
    return x;
}

// Entry (r, j), r >= j, of a child's update block.  Square children: U = offset of (k, k), M = the child's m (> 0).
// Packed leaf children (FrontDev::packed): U = offset of (k, k) in the packed triangle, M = -(m - k).
__device__ __forceinline__ int64_t child_entry(int64_t U, int32_t M, int j, int r) {
    return M > 0 ? U + (int64_t)j * M + r : U + (int64_t)j * (-M) - (j * (j - 1)) / 2 + (r - j);
}
__device__ __forceinline__ void child_update_desc(const FrontDev& C, int64_t& U, int32_t& M) {
    if (C.packed) {
        U = C.F_off + (int64_t)C.k * C.m - (C.k * (C.k - 1)) / 2;
        M = -(C.m - C.k);
    } else {
        U = C.F_off + (int64_t)C.k * C.m + C.k;
        M = C.m;
    }
}
__device__ __forceinline__ int64_t tiny_entry(const FrontDev& F, int r, int c) {        // (r, c), r >= c, of a leaf front
    return F.packed ? (int64_t)c * F.m - (c * (c - 1)) / 2 + (r - c) : r + (int64_t)c * F.m;
}

// In-register LDL' of an nb x nb block: lane r holds row r of the lower triangle in a[0..r].
// 32 x 31 / 2 shuffle + FMA pairs, no memory traffic; nb is wave-uniform.
template <int NBT>
__device__ __forceinline__ bool wave_ldlt_regs(double (&a)[NBT], int nb, int lane) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
        if (j < nb) {
            const double d = readlane_f64(a[j], j);
            if (d == 0.0 || !isfinite(d)) bad = true;
            const double inv = fast_recip(d);
            const double aj = a[j];          // this lane's unscaled entry of column j
            const double lr = aj * inv;
#pragma unroll
            for (int c = j + 1; c < NBT; ++c) {
                // unscaled entry (c, j).  No lane predicate: lanes above the diagonal (lane < c)
                // only touch their never-read upper-triangle slots, and rows/columns >= nb hold
                // zeros, so the update is a plain FMA with an SGPR operand.
                const double v = readlane_f64(aj, c);
                a[c] -= lr * v;
            }
            if (lane > j) a[j] = lr;
        }
    }
    return bad;
}

}  // namespace
}  // namespace mgbhip
