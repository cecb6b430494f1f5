// node_core.hpp -- the arithmetic of one node, shared by the element kernels (elem_kernels.hpp) and the dense node
// kernels (dense.hip).  Every helper is an expression evaluated in place: the kernels' instruction streams do not change.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mgbhip {

namespace {

__device__ __forceinline__ int tri_index(int k, int k2, int NY) {   // k <= k2
    return k * NY - (k * (k - 1)) / 2 + (k2 - k);
}

// Barrier scale of a node: bwv is its barrier weight where the problem has them (a masked node, weight 0, contributes
// an exact 0 whatever the cone returned), 1/n otherwise.
__device__ __forceinline__ double scale_by(const ElemParams& P, double bwv, double x) {
    return P.bw ? ((bwv == 0.0) ? 0.0 : bwv * x) : P.invn * x;
}
// MODE_F0 only.  Unlike scale_by it also guards invn == 0: the linear-only call (c_dot_Dz) evaluates with invn = 0
// at points where the barrier may be infinite, and must give 0, not 0 * inf.  The two forms are not interchangeable.
__device__ __forceinline__ double barrier_f0(const ElemParams& P, int64_t node, double F) {
    double bar;
    if (P.bw != nullptr) {
        const double bwv = P.bw[node];
        bar = (bwv == 0.0) ? 0.0 : bwv * F;
    } else {
        bar = (P.invn == 0.0) ? 0.0 : P.invn * F;
    }
    return bar;
}

}  // namespace

}  // namespace mgbhip
