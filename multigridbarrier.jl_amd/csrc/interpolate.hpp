// interpolate.hpp -- point evaluation behind mgbhip_interpolate / mgbhip_interpolate_grad and the point locator behind
// mgbhip_locator_* (interpolate.hip).
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "cell_grid.hpp"
#include "common.hpp"

namespace mgbhip {

constexpr int INTERP_MAX_DEGREE = 8;    // element degree k of the FEM families (the kernels are unrolled per k + 1)

// The families with elements (node coordinates and a basis table).  The ids are not ordered by kind: 5 and 6 are the
// spectral families, 7 (curved P2) is an element family again.
inline bool interp_is_fem(int32_t family) {
    return (family >= MGBHIP_INTERP_FEM1D && family <= MGBHIP_INTERP_P2) || family == MGBHIP_INTERP_P2C;
}
// the 2-D / 3-D element families, whose points are located through a grid of element boxes
inline bool interp_is_located(int32_t family) { return interp_is_fem(family) && family != MGBHIP_INTERP_FEM1D; }

struct InterpIn {
    int32_t family = 0, d = 0, k = 0, p = 0, ncomp = 0;
    int64_t N = 0, M = 0;
    int32_t sorted = 1;           // FEM1D: left endpoints non-decreasing (binary search) or not (the reference's scan)
    const double* x = nullptr;    // host (p*N) x d
    const double* table = nullptr;
    int64_t table_len = 0;
    const double* z = nullptr;    // host (p*N) x ncomp
    const double* pts = nullptr;  // host M x d
    double* out = nullptr;        // host M x ncomp (may be NULL when grad is given)
    double* grad = nullptr;       // host M x ncomp x d, or NULL: values only
    int32_t* elem = nullptr;      // host M, or NULL
};

// A location grid that stays resident: the cells (a Grid over the union of the padded element boxes, cell_grid.hpp), per
// cell its candidate elements in ascending element order (cell c
// owns cand[start[c] .. start[c+1]-1]) and the padded element boxes (lo then hi per element).  interpolate_run and
// locator_build free theirs once the points are located; a field-line tracer (stream.hpp) keeps one for its lifetime.
struct LocationGrid {
    Grid g{};
    DevBuf<int32_t> start, cand;
    DevBuf<double> box;
};

// in: family, d (2 or 3), k, p, N; d_x the node coordinates on the device ((p*N) x d); complete on return
void location_grid_build(LocationGrid& G, const InterpIn& in, const double* d_x, hipStream_t st);
// The same grid over N Q_k elements of p nodes each in e = 2 or 3 coordinates, whatever their own dimension (curves and
// surfaces: closest.hip).  The node boxes are padded as for Q_k (by QK_BOX_PAD x extent for k >= 2) and by `reach` more
// on every side, so a cell lists every element that comes within `reach` of one of its points.
void location_grid_build_embedded(LocationGrid& G, int32_t e, int32_t k, int32_t p, int64_t N, const double* d_x,
                                  double reach, hipStream_t st);
// order[i] = the point lane i of a query kernel processes: the M points (d_pts, M x e, on the device) sorted by their
// cell of G, as interpolate_run sorts its points; complete on return
void location_grid_sort_points(const LocationGrid& G, int32_t e, int64_t M, const double* d_pts, DevBuf<int32_t>& order,
                               hipStream_t st);

// one launch sequence on st; complete (results on the host) on return
void interpolate_run(const InterpIn& in, hipStream_t st);

// A point locator: the location half of interpolate_run done once, its result resident on the device, and the
// evaluation half run per z.  Resident: the node coordinates and the basis table (FEM families), per point the element,
// the reference coordinates and (2-D / 3-D) its place in the cell order; for the spectral families the points.
struct Locator {
    int32_t family = 0, d = 0, k = 0, p = 0;
    int64_t N = 0, M = 0;
    DevBuf<double> x, table, pts, ref;
    DevBuf<int32_t> elem, order, flag;
    DevBuf<double> z, out, grad;      // per evaluate call: grown to the largest ncomp seen and kept
};

// in.z / in.ncomp / in.out / in.grad / in.elem are not read
void locator_build(Locator& L, const InterpIn& in, hipStream_t st);
// the same for M points already on the device (d_pts, M x d; read, not kept; in.pts is not read): the 2-D / 3-D FEM
// families and fem1d.  raycast.hip locates the samples it generates through this entry.
void locator_build_device(Locator& L, const InterpIn& in, const double* d_pts, hipStream_t st);
void locator_elements(const Locator& L, int32_t* elem, hipStream_t st);
// z host (p*N) x ncomp; out host M x ncomp or NULL; grad host M x ncomp x d or NULL; complete on return
void locator_evaluate(Locator& L, int32_t ncomp, const double* z, double* out, double* grad, hipStream_t st);
// the launches of locator_evaluate alone: the values stay in L.out (M x ncomp, by point) and, with grad, the gradients
// in L.grad; queued on st, not waited for
void locator_evaluate_device(Locator& L, int32_t ncomp, const double* z, bool grad, hipStream_t st);
// the same for z already on the device (d_z, (p*N) x ncomp; read, not kept)
void locator_evaluate_resident(Locator& L, int32_t ncomp, const double* d_z, bool grad, hipStream_t st);

}  // namespace mgbhip
