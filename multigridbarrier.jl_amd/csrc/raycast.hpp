// raycast.hpp -- rays sampled through a mesh behind mgbhip_raycast_* (raycast.hip): a point locator (interpolate.hpp) whose
// points are generated on the device, a per-ray integration kernel and a per-ray compositing kernel.
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"
#include "interpolate.hpp"

namespace mgbhip {

struct RayIn {
    InterpIn geo;                    // family, d, k, p, N, x, table (table_len set): QK (d = 2, 3), P1, P2
    int64_t R = 0;
    const double* origin = nullptr;  // host R x d, finite
    const double* dir = nullptr;     // host R x d, unit length
    const double* box = nullptr;     // host 2 d: the clip box, lo then hi
    double step = 0.0, t_min = 0.0, t_max = 0.0;
};

// Resident: per ray the origin, the direction, the first parameter, the step, the first sample and the length in the
// mesh; per sample what a Locator keeps (element, reference coordinates, place in the cell order) and, per call, the
// values.  The sample positions and the location grid are freed once the samples are located.
struct RayCaster {
    int32_t d = 0;
    int64_t R = 0, S = 0;
    DevBuf<double> origin, dir, tmin, h, length;   // R x d, R x d, R, R, R
    DevBuf<int64_t> off;                           // R + 1
    Locator loc;                                   // M = S
    DevBuf<double> transfer, result;               // per call: grown to the largest seen and kept
    DevBuf<double> t_hit, layer;                   // per call of render_layers: R x KH, R x KH x 4
};

// count pass, exclusive scan over the rays, emit pass, location; complete on return (RC.S is known)
void raycast_build(RayCaster& RC, const RayIn& in, hipStream_t st);
void raycast_offsets(const RayCaster& RC, int64_t* offsets, hipStream_t st);                 // R + 1
void raycast_lengths(const RayCaster& RC, double* step, double* length, hipStream_t st);     // R, R (either may be NULL)
void raycast_samples(const RayCaster& RC, double* pts, hipStream_t st);                      // S x d, regenerated
// z host (p*N) x ncomp, out host R x ncomp: h_r * sum of the finite sample values, in sample order
void raycast_integrate(RayCaster& RC, int32_t ncomp, const double* z, double* out, hipStream_t st);
// u host p*N, transfer host K x 4 (r, g, b, sigma), out host R x 4: front-to-back emission-absorption compositing
void raycast_render(RayCaster& RC, const double* u, int32_t K, const double* transfer, double lo, double hi, double* out,
                    hipStream_t st);
// the same with KH layers per ray (t_hit host R x KH ascending, +inf = none; layer host R x KH x 4 premultiplied colour and
// alpha) merged into the samples by depth: a hit is applied before sample i iff t_hit <= t_i
void raycast_render_layers(RayCaster& RC, const double* u, int32_t K, const double* transfer, double lo, double hi,
                           int32_t KH, const double* t_hit, const double* layer, double* out, hipStream_t st);

// render and render_layers for u, the table, the depths and the layers already on the device, R > 0: the image is left in
// RC.result (R x 4); queued on st, not waited for
void raycast_render_device(RayCaster& RC, const double* d_u, int32_t K, const double* d_transfer, double lo, double hi,
                           hipStream_t st);
void raycast_render_layers_device(RayCaster& RC, const double* d_u, int32_t K, const double* d_transfer, double lo, double hi,
                                  int32_t KH, const double* d_t_hit, const double* d_layer, hipStream_t st);

}  // namespace mgbhip
