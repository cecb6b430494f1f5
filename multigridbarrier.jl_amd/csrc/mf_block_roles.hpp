// mf_block_roles.hpp -- which workgroup of a large-front launch does what.  A launch of `nfronts` fronts gives every front
// one CHAIN workgroup (role 0: the look-ahead workgroup of mf_big_step, the block-0 workgroup of mf_big_gather -- the
// longest workgroup of its launch, and the one the next launch waits for) and `ntiles` tile workgroups (role 1 + t, t the
// tile's linear index; column group t of the gather).  No workgroup of such a launch reads what another one of the same
// launch writes, so the place of a role in the grid is free to choose; the hardware dispatches x fastest:
//   ROLES_LEGACY        grid (ntiles + 1, nfronts): front = blockIdx.y, tiles at x = 0 .. ntiles - 1, the chain LAST in its
//                       row (MGBHIP_CHAIN_ORDER=legacy; the layout up to the chain-first launches);
//   ROLES_CHAIN_FIRST   grid (nfronts, ntiles + 1): front = blockIdx.x, row y = 0 holds every front's chain workgroup, so
//                       all of them are dispatched ahead of every tile of the launch; tile t of every front in row 1 + t.
// Plain host/device C++ without a HIP header: the kernels, their launchers and tests/csrc/block_roles_check.cpp read it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGB_ROLES_HD __host__ __device__
#else
#define MGB_ROLES_HD
#endif

namespace mgbhip {

enum BlockRoles : int { ROLES_LEGACY = 0, ROLES_CHAIN_FIRST = 1 };

struct RolesGrid { uint32_t x, y; };
struct BlockRole {
    int front;     // of the launch: fr[first + front], the front's dscr slot
    int role;      // 0: the chain workgroup; 1 + t: tile t
    MGB_ROLES_HD bool chain() const { return role == 0; }
    MGB_ROLES_HD int tile() const { return role - 1; }              // linear tile index (tile workgroups only)
    MGB_ROLES_HD bool first_tile() const { return role == 1; }      // the tile workgroup with the per-front extra duties
};

MGB_ROLES_HD inline RolesGrid roles_grid(int layout, int nfronts, int ntiles) {
    return layout == ROLES_CHAIN_FIRST ? RolesGrid{(uint32_t)nfronts, (uint32_t)ntiles + 1u}
                                       : RolesGrid{(uint32_t)ntiles + 1u, (uint32_t)nfronts};
}

// (blockIdx.x, blockIdx.y) of a grid of roles_grid(layout, ...) whose x extent is gx.  All operands are uniform over the
// workgroup (scalar registers); CHAIN_FIRST needs neither gx nor an addition.
MGB_ROLES_HD inline BlockRole role_of_block(int layout, uint32_t bx, uint32_t by, uint32_t gx) {
    if (layout == ROLES_CHAIN_FIRST) return BlockRole{(int)bx, (int)by};
    return BlockRole{(int)by, bx == gx - 1u ? 0 : (int)bx + 1};
}

// A launch whose fronts have no chain workgroup (mf_big_gather without the block-0 workgroup) is the plain grid
// (ntiles, nfronts) whatever the layout: front = blockIdx.y, tile = blockIdx.x.
MGB_ROLES_HD inline RolesGrid tiles_only_grid(int nfronts, int ntiles) { return RolesGrid{(uint32_t)ntiles, (uint32_t)nfronts}; }
MGB_ROLES_HD inline BlockRole tile_of_block(uint32_t bx, uint32_t by) { return BlockRole{(int)by, (int)bx + 1}; }

}  // namespace mgbhip
