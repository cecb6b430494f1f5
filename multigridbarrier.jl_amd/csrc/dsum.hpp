// dsum.hpp -- the compensated sum every translation unit that adds long columns shares (reduce_kernels.hpp and its
// users in kernels.hip; quad_device.hpp and its users quadrature.hip and faces.hip).  Internal linkage, like
// device_prims.hpp: the library is built without relocatable device code, so each translation unit carries its own copy
// of what it inlines.
#pragma once
#include <hip/hip_runtime.h>

namespace mgbhip {

namespace {

// ---- compensated sums --------------------------------------------------------------------------
// The coarse-level sums run over every element of the mesh, and near the end of a barrier solve one node's term can
// exceed the rest by sixteen orders of magnitude (an iterate 1e-13 from the cone's wall: Hessian entries ~ 1e16, soft
// eigenvalues ~ 1e1).  A plain running sum then loses the other 10^5 terms below the ulp of the large one -- an
// absolute error of hundreds in a matrix whose smallest eigenvalue is 34: H comes out indefinite by summation
// noise alone (tests/dev/logs/gpu_coarse_noise_probe_L8_p1.5.txt).  TwoSum accumulation (Knuth) carries the rounding
// error of every addition in a second word: the sum is the correctly rounded one to a few ulps, whatever the order.
// Used by the gather_assemble_* kernels and the long-row restrictions.  (At cond(H) ~ 1e15 the sign of lambda^2 also
// depends on the rounding of the per-node terms themselves, which no summation scheme removes: DESIGN.md section 5.)
struct DSum {
    double s = 0.0, c = 0.0;
    __device__ __forceinline__ void add(double x) {
#ifdef MGB_PLAIN_SUMS
        s += x;
        return;
#endif
        const double t = s + x;
        const double bp = t - s;
        c += (s - (t - bp)) + (x - bp);
        s = t;
    }
    __device__ __forceinline__ void merge(double s2, double c2) { add(s2); c += c2; }
    __device__ __forceinline__ double value() const { return s + c; }
};
__device__ __forceinline__ void dsum_wave_reduce(DSum& a) {      // fixed shuffle tree over the 64 lanes; result in lane 0
    for (int off = 32; off > 0; off >>= 1) {
        const double s2 = __shfl_down(a.s, off, 64), c2 = __shfl_down(a.c, off, 64);
        a.merge(s2, c2);
    }
}

}  // namespace

}  // namespace mgbhip
