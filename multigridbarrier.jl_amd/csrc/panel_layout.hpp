// panel_layout.hpp -- layout of the element Hessian slab and staging sizes of the coarse-level projection kernels.  Plain C++
// (no HIP): the kernels' launchers (panel_kernels.hpp), the accumulate gate of the assembly plan (assembly_plan.cpp) and the
// host test read the one definition here.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mgbhip {

// element Hessian slab layout: block-major [block][element][p*p]; blocks (a,b), a <= b, in
// row-major order of the upper block triangle, each p x p column-major.
inline int hel_blocks(int nu) { return nu * (nu + 1) / 2; }
inline int hel_block_index(int a, int b, int nu) { return a * nu - a * (a - 1) / 2 + (b - a); }
// Offsets of the blocks in the slab: full blocks hold p*p doubles per element, blocks flagged in
// diag_mask (both states carry identity operators only) hold their p diagonal entries.
inline int64_t hel_layout(int nu, int64_t N, int p, int diag_mask, int64_t* off) {
    int64_t total = 0;
    for (int blk = 0; blk < hel_blocks(nu); ++blk) {
        off[blk] = total;
        total += ((diag_mask >> blk) & 1) ? N * p : N * (int64_t)p * p;
    }
    return total;
}

// LDS budget of launch_panel_accumulate and launch_panel_project_staged
constexpr size_t PANEL_ACC_LDS_MAX = 144 * 1024;
inline size_t panel_stage_doubles(int p, int nu, int ctmax) {        // staging of one element, one workgroup
    return (size_t)p * ctmax + (size_t)(nu * (nu + 1) / 2) * p * p + (size_t)nu * p * ctmax + ctmax;
}
inline size_t panel_accumulate_lds(int p, int nu, int ctmax) {      // slab variant: 4 waves x one element's staging
    return 4 * panel_stage_doubles(p, nu, ctmax) * sizeof(double);
}
inline bool panel_accumulate_fits(int p, int nu, int ctmax) {        // register staging limits of panel_accumulate_kernel
    return p * ctmax <= 4 * 256 && (nu * (nu + 1) / 2) * p * p <= 3 * 256 && ctmax <= 256;
}

}  // namespace mgbhip
