// surface.hpp -- rays against a triangle soup behind mgbhip_surface_* (surface.hip): a uniform grid of cells over the
// triangles' boxes, a per-ray traversal kernel that keeps the K nearest hits, and a per-hit shading kernel.
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"

namespace mgbhip {

constexpr int SURFACE_MAX_HITS = 8;

struct SurfaceGrid {
    double lo[3], hi[3], inv[3], size[3];   // the padded union box, cells per unit length, cell side
    double pad;                             // every triangle's box is widened by this much on every side
    int32_t n[3];
    int64_t ncell;
};

// Resident: the soup (72 bytes per triangle), the sorted (cell, triangle) pair list (4 bytes per pair) and the cell
// starts (4 bytes per cell).  The per-call buffers grow to the largest call seen and are kept.
struct Surface {
    int64_t T = 0, P = 0;
    SurfaceGrid g{};
    DevBuf<double> pts;                     // T x 3 x 3
    DevBuf<int32_t> start, cand;            // ncell + 1, P
    DevBuf<double> o, dn, t, u, v, values, table, layer;
    DevBuf<int32_t> tri;
};

// boxes, union, count pass, exclusive scan, emit pass, stable sort by cell; complete on return
void surface_build(Surface& S, int64_t T, const double* points, hipStream_t st);
// o, dn host R x 3 (dn of unit length); t, u, v host R x K doubles, tri host R x K: the K nearest hits by (t, triangle)
void surface_trace(Surface& S, int64_t R, const double* o, const double* dn, double t_min, double t_max, int32_t K,
                   double* t, int32_t* tri, double* u, double* v, hipStream_t st);
// tri, u, v as trace returned them; values host T x 3, table host Kt x 4 (r, g, b, alpha); layer host R x K x 4
void surface_shade(Surface& S, int64_t R, int32_t K, const double* dn, const int32_t* tri, const double* u,
                   const double* v, const double* values, int32_t Kt, const double* table, double lo, double hi,
                   double ambient, double* layer, hipStream_t st);

}  // namespace mgbhip
