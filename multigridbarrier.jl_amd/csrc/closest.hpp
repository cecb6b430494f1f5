// closest.hpp -- closest-point projection onto embedded curves and surfaces behind mgbhip_closest_* (closest.hip).
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"

namespace mgbhip {

constexpr int CLOSEST_MAXIT = 64;       // projected-Newton iterations per candidate element

// A closest-point locator: M points projected once onto N Q_k elements of dimension d (1: curves, 2: surfaces) in e > d
// coordinates.  Resident: the node coordinates and the reference nodes, and per point, in the cell order of the location
// grid it was found through (order[i] = the point of slot i), the element of its foot (-1: none within max_distance),
// the reference coordinates, the foot, the distance and whether the winning iteration converged.  The grid is freed once
// the points are projected; the evaluation reads (element, reference coordinates) only.
struct Closest {
    int32_t d = 0, e = 0, k = 0, p = 0;
    int64_t N = 0, M = 0;
    double max_distance = 0.0;
    DevBuf<double> x, table, ref, foot, dist;
    DevBuf<int32_t> elem, flag, order;
    DevBuf<double> z, out, grad;      // per evaluate call: grown to the largest ncomp seen and kept
};

// x host (p*N) x e, nodes host k + 1, pts host M x e; complete on return
void closest_build(Closest& Cl, int32_t d, int32_t e, int32_t k, int64_t N, const double* x, const double* nodes,
                   int64_t M, const double* pts, double max_distance, hipStream_t st);
// by point; any output may be NULL: elem M, xi M x d, foot M x e, dist M, flag M (NaN where elem is -1)
void closest_fetch(const Closest& Cl, int32_t* elem, double* xi, double* foot, double* dist, int32_t* flag,
                   hipStream_t st);
// z host (p*N) x ncomp; out host M x ncomp or NULL; grad host M x ncomp x e or NULL (values only); complete on return
void closest_evaluate(Closest& Cl, int32_t ncomp, const double* z, double* out, double* grad, hipStream_t st);

}  // namespace mgbhip
