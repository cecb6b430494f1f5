// tubes.hpp -- rays against a soup of capsules (segments with a radius) behind mgbhip_tubes_* (tubes.hip): the uniform
// grid of cell_lists.hpp over the capsules' boxes, a per-ray traversal kernel that keeps the K nearest entry points, and a
// per-hit shading kernel.
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"
#include "surface.hpp"

namespace mgbhip {

constexpr int TUBES_MAX_HITS = SURFACE_MAX_HITS;

// the segments (48 bytes each) and their radii; the hit parameter is the axis parameter s
struct Tubes : Soup {
    DevBuf<double> pts, rad;                // n x 2 x 3, n
};

// boxes (end points widened by the radius), then the grid of cell_lists.hpp; complete on return
void tubes_build(Tubes& T, int64_t S, const double* points, const double* radii, hipStream_t st);
// o, dn host R x 3 (dn of unit length); t, s host R x K doubles, seg host R x K: the K nearest entries by (t, segment)
void tubes_trace(Tubes& T, int64_t R, const double* o, const double* dn, double t_min, double t_max, int32_t K, double* t,
                 int32_t* seg, double* s, hipStream_t st);
// t, seg, s as trace returned them; values host S x 2, table host Kt x 4 (r, g, b, alpha); layer host R x K x 4
void tubes_shade(Tubes& T, int64_t R, int32_t K, const double* o, const double* dn, const double* t, const int32_t* seg,
                 const double* s, const double* values, int32_t Kt, const double* table, double lo, double hi,
                 double ambient, double* layer, hipStream_t st);

}  // namespace mgbhip
