// surface.hpp -- rays against a triangle soup behind mgbhip_surface_* (surface.hip): a uniform grid of cells over the
// triangles' boxes, a per-ray traversal kernel that keeps the K nearest hits, and a per-hit shading kernel.
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "cell_grid.hpp"
#include "common.hpp"

namespace mgbhip {

constexpr int SURFACE_MAX_HITS = 8;

// What a soup of n primitives in a grid keeps, whatever the primitive (soup_trace.hpp): the grid, the sorted (cell,
// primitive) pair list (4 bytes per pair) and the cell starts (4 bytes per cell) are resident; the per-call buffers (the
// rays, the hits as t, id and up to two parameters of the hit point, the vertex values, the colour table, the layers) grow
// to the largest call seen and are kept.
struct Soup {
    int64_t n = 0, P = 0;
    Grid g{};
    DevBuf<int32_t> start, cand;            // ncell + 1, P
    DevBuf<double> o, dn, t, par[2], values, table, layer;
    DevBuf<int32_t> id;
};

// the triangles (72 bytes each); the hit parameters are the barycentric u, v
struct Surface : Soup {
    DevBuf<double> pts;                     // n x 3 x 3
};

// boxes, union, count pass, exclusive scan, emit pass, stable sort by cell; complete on return
void surface_build(Surface& S, int64_t T, const double* points, hipStream_t st);
// the same for a soup already on the device (d_points, T x 3 x 3; S.pts.p itself is allowed and then nothing is copied).
// The buffers of S and w grow and are kept, so S may be built again; T = 0 leaves an empty surface.
void surface_build_device(Surface& S, int64_t T, const double* d_points, GridWork& w, hipStream_t st);
// o, dn host R x 3 (dn of unit length); t, u, v host R x K doubles, tri host R x K: the K nearest hits by (t, triangle)
void surface_trace(Surface& S, int64_t R, const double* o, const double* dn, double t_min, double t_max, int32_t K,
                   double* t, int32_t* tri, double* u, double* v, hipStream_t st);
// the same for rays on the device, T > 0: the hits are left in S.t, S.id, S.par[0], S.par[1] (R x K each); queued on st, not waited for
void surface_trace_device(Surface& S, int64_t R, const double* d_o, const double* d_dn, double t_min, double t_max,
                          int32_t K, hipStream_t st);
// tri, u, v as trace returned them; values host T x 3, table host Kt x 4 (r, g, b, alpha); layer host R x K x 4
void surface_shade(Surface& S, int64_t R, int32_t K, const double* dn, const int32_t* tri, const double* u,
                   const double* v, const double* values, int32_t Kt, const double* table, double lo, double hi,
                   double ambient, double* layer, hipStream_t st);

// the same for device pointers throughout, T > 0: d_layer is R x K x 4 on the device; queued on st, not waited for
void surface_shade_device(const Surface& S, int64_t R, int32_t K, const double* d_dn, const int32_t* d_tri, const double* d_u,
                          const double* d_v, const double* d_values, int32_t Kt, const double* d_table, double lo, double hi,
                          double ambient, double* d_layer, hipStream_t st);

}  // namespace mgbhip
