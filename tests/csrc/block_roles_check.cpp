// block_roles_check.cpp -- the role map of the large-front launches (csrc/mf_block_roles.hpp) for
// tests/test_block_roles_host.py, which builds it with plain g++ (the header is plain C++) and feeds it one command per line.
//   names                              -> LEGACY n CHAIN_FIRST n
//   grid LAYOUT NFRONTS NTILES         -> x y
//   role LAYOUT BX BY GX               -> front role chain tile first_tile
//   tiles NFRONTS NTILES BX BY         -> x y front role chain tile   (a launch without chain workgroups)
//   order LAYOUT NFRONTS NTILES       -> the (front, role) pairs of the grid in x-fastest linear order: "f:r f:r ..."
//   sweep LAYOUT F0 F1 T0 T1           -> checks every grid with nfronts F0..F1, ntiles T0..T1; "ok GRIDS BLOCKS" or "FAIL ..."
// The sweep's checks: every (front, role) pair exactly once; dimensions within HIP's limits for 256-thread workgroups;
// LEGACY equal to the indices of the kernels before the map (written out here, not read from the header); CHAIN_FIRST with
// the chain workgroups in the first NFRONTS positions of the x-fastest order.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../multigridbarrier.jl_amd/csrc/mf_block_roles.hpp"

using namespace mgbhip;

namespace {

// HIP: gridDim.x <= 2^31 - 1, gridDim.y <= 65535, and gridDim.x * blockDim.x below 2^32 threads
bool within_hip_limits(RolesGrid g) {
    return g.x >= 1 && g.y >= 1 && g.x <= 2147483647u && g.y <= 65535u && (uint64_t)g.x * 256u < (1ull << 32);
}

std::string check_grid(int layout, int nfronts, int ntiles, int64_t& blocks) {
    const RolesGrid g = roles_grid(layout, nfronts, ntiles);
    char msg[160];
    if (!within_hip_limits(g)) { snprintf(msg, sizeof msg, "grid %u x %u outside HIP's limits", g.x, g.y); return msg; }
    if ((int64_t)g.x * g.y != (int64_t)nfronts * (ntiles + 1)) { snprintf(msg, sizeof msg, "grid %u x %u has the wrong size", g.x, g.y); return msg; }
    if (layout == ROLES_LEGACY && (g.x != (uint32_t)ntiles + 1 || g.y != (uint32_t)nfronts)) return "LEGACY grid is not (ntiles + 1, nfronts)";
    std::vector<uint8_t> seen((size_t)nfronts * (size_t)(ntiles + 1), 0);        // exactly this many: a role beyond it trips the sanitizer
    int64_t lin = 0;
    for (uint32_t by = 0; by < g.y; ++by)
        for (uint32_t bx = 0; bx < g.x; ++bx, ++lin) {
            const BlockRole r = role_of_block(layout, bx, by, g.x);
            if (r.front < 0 || r.front >= nfronts || r.role < 0 || r.role > ntiles) {
                snprintf(msg, sizeof msg, "block (%u, %u): front %d role %d out of range", bx, by, r.front, r.role);
                return msg;
            }
            uint8_t& s = seen[(size_t)r.front * (size_t)(ntiles + 1) + (size_t)r.role];
            if (s) { snprintf(msg, sizeof msg, "front %d role %d twice", r.front, r.role); return msg; }
            s = 1;
            if (r.chain() != (r.role == 0) || r.first_tile() != (r.role == 1) || r.tile() != r.role - 1) return "accessors disagree with role";
            if (layout == ROLES_LEGACY) {
                // the kernels before the map: front = blockIdx.y, chain = (blockIdx.x == gridDim.x - 1), tile index = blockIdx.x
                const bool chain = bx == g.x - 1;
                if (r.front != (int)by || r.chain() != chain || (!chain && r.tile() != (int)bx) || (!chain && r.first_tile() != (bx == 0))) {
                    snprintf(msg, sizeof msg, "LEGACY block (%u, %u) is not today's", bx, by);
                    return msg;
                }
            } else if (r.chain() != (lin < nfronts)) {
                snprintf(msg, sizeof msg, "CHAIN_FIRST: position %lld is %s chain workgroup", (long long)lin, r.chain() ? "a" : "no");
                return msg;
            }
        }
    blocks += lin;           // every pair at most once and as many blocks as pairs: every pair exactly once
    return "";
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "names") {
            printf("LEGACY %d CHAIN_FIRST %d\n", (int)ROLES_LEGACY, (int)ROLES_CHAIN_FIRST);
        } else if (cmd == "grid") {
            int layout, nfronts, ntiles;
            in >> layout >> nfronts >> ntiles;
            const RolesGrid g = roles_grid(layout, nfronts, ntiles);
            printf("%u %u\n", g.x, g.y);
        } else if (cmd == "role") {
            int layout; uint32_t bx, by, gx;
            in >> layout >> bx >> by >> gx;
            const BlockRole r = role_of_block(layout, bx, by, gx);
            printf("%d %d %d %d %d\n", r.front, r.role, r.chain() ? 1 : 0, r.tile(), r.first_tile() ? 1 : 0);
        } else if (cmd == "tiles") {          // tiles NFRONTS NTILES BX BY -> the grid without chain workgroups and one block of it
            int nfronts, ntiles; uint32_t bx, by;
            in >> nfronts >> ntiles >> bx >> by;
            const RolesGrid g = tiles_only_grid(nfronts, ntiles);
            const BlockRole r = tile_of_block(bx, by);
            printf("%u %u %d %d %d %d\n", g.x, g.y, r.front, r.role, r.chain() ? 1 : 0, r.tile());
        } else if (cmd == "order") {
            int layout, nfronts, ntiles;
            in >> layout >> nfronts >> ntiles;
            const RolesGrid g = roles_grid(layout, nfronts, ntiles);
            for (uint32_t by = 0; by < g.y; ++by)
                for (uint32_t bx = 0; bx < g.x; ++bx) {
                    const BlockRole r = role_of_block(layout, bx, by, g.x);
                    printf("%s%d:%d", (bx || by) ? " " : "", r.front, r.role);
                }
            printf("\n");
        } else if (cmd == "sweep") {
            int layout, f0, f1, t0, t1;
            in >> layout >> f0 >> f1 >> t0 >> t1;
            int64_t grids = 0, blocks = 0;
            std::string bad;
            for (int nf = f0; nf <= f1 && bad.empty(); ++nf)
                for (int nt = t0; nt <= t1 && bad.empty(); ++nt, ++grids) {
                    bad = check_grid(layout, nf, nt, blocks);
                    if (!bad.empty()) bad = "nfronts " + std::to_string(nf) + " ntiles " + std::to_string(nt) + ": " + bad;
                }
            if (bad.empty()) printf("ok %lld %lld\n", (long long)grids, (long long)blocks);
            else printf("FAIL %s\n", bad.c_str());
        } else {
            fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
