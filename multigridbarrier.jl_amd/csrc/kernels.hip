// kernels.hip -- evaluate / assemble kernels of the barrier functional on gfx950.
//
// One fused element kernel family replaces the reference's chain
//   R*s (SpMV) -> apply_D (nD block matvecs) -> map_rows_gpu(F) -> D' back-multiplies ->
//   16 fused triple products + _hess_add! temporaries
// (reference: src/convex.jl:155-202, src/BlockMatrices.jl:170-188, :604-640; CUDA twins
// ext/MultiGridBarrierCUDAExt/block_ops.jl:31-148, map_rows_gpu.jl:20-28): a group of
// G = 2^ceil(log2 p) lanes owns one element, lane r owns node r.  The element's operator
// blocks are staged through LDS with a flat coalesced copy (they are contiguous in the
// reference's p x p x N layout), Dz, the cone functor and the per-element 14x14 (nu*p)
// Hessian block never leave the CU.  HBM traffic is the compulsory one of SURVEY.md
// section 8(d): operators + z + grids in, element blocks out.
//
// One translation unit, cut along its kernel families; each header ends with the host launchers of its own kernels:
//   elem_device.hpp / elem_kernels.hpp   element evaluation (launch_elem, launch_elem_f2_condense)
//   reduce_kernels.hpp                   compensated sums, reductions, finishing launches
//   vector_kernels.hpp                   CSR matvecs, prolong, step, axpy, fill, index gather / scatter
//   assemble_kernels.hpp                 gather assembly
//   panel_kernels.hpp                    panel projection and accumulation
#include "elem_kernels.hpp"
#include "reduce_kernels.hpp"
#include "vector_kernels.hpp"
#include "assemble_kernels.hpp"
#include "panel_kernels.hpp"

namespace mgbhip {

// Workgroups of a vector reduction (reduce_kernels.hpp): ceil(n / 256), capped.  tests/gate_cases.py reads the cap from
// this file to place its reduction lengths around it.
static int reduce_blocks(int64_t n) {
    int64_t b = (n + 255) / 256;
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace mgbhip
