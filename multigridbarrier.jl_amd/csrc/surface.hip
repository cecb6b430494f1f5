// Rays against a triangle soup: mgbhip_surface_* (include/mgbhip.h).
//
// reference: the isosurfaces and slices of `plot` for fem3d solutions, ext/MultiGridBarrierPyPlotExt/plot3d.jl:85-149
// (PyVista's add_mesh on the CPU).  Here the soup that mgbhip_contour_create cuts is put into a uniform grid of cells
// the way the point locator puts element boxes into one (interpolate.hip; restated here because that grid is tied to
// the element families and their containment tolerances): one thread per triangle forms its box, one block reduces
// the union, the host picks the cell counts, a count pass and an exclusive scan size the (cell, triangle) pair list, an
// emit pass writes it in triangle order and a stable radix sort by cell leaves every cell's list ascending in
// triangle index.  No atomics.  Everything after the boxes lives in cell_lists.hpp, and the walk of a ray through the
// cells, with its list of the K nearest hits, in soup_trace.hpp; tubes.hip includes both too.  This file brings the
// triangle: its box, its test and its shading.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "soup_trace.hpp"
#include "surface.hpp"

// No fused multiply-adds in this file: a plain IEEE transcription of the triangle test (tests/surface_twin.py) then
// gives the same t, u and v bit for bit.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

// ---------------------------------------------------------------------------------------------------------------
// the grid over the soup
// ---------------------------------------------------------------------------------------------------------------

// one thread per triangle: the box of its three vertices (lo then hi)
__global__ void __launch_bounds__(BLOCK) tri_boxes(int64_t T, const double* __restrict__ pts, double* __restrict__ box) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T) return;
    for (int a = 0; a < 3; ++a) {
        const double x0 = pts[e * 9 + a], x1 = pts[e * 9 + 3 + a], x2 = pts[e * 9 + 6 + a];
        box[e * 6 + a] = fmin(x0, fmin(x1, x2));
        box[e * 6 + 3 + a] = fmax(x0, fmax(x1, x2));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the triangle test
// ---------------------------------------------------------------------------------------------------------------

// ray o + t dn against the triangle at p (v0, v1, v2): two-sided, edges and vertices included
__device__ inline bool hit_test(const double* o, const double* dn, const double* __restrict__ p, double t_min,
                                double t_max, double& t, double& u, double& v) {
    double e1[3], e2[3], s[3], pv[3], q[3];
    for (int a = 0; a < 3; ++a) {
        e1[a] = p[3 + a] - p[a];
        e2[a] = p[6 + a] - p[a];
    }
    cross3(dn, e2, pv);
    const double det = dot3(e1, pv);
    if (!(det != 0.0) || !isfinite(det)) return false;
    for (int a = 0; a < 3; ++a) s[a] = o[a] - p[a];
    u = dot3(s, pv) / det;
    cross3(s, e1, q);
    v = dot3(dn, q) / det;
    t = dot3(e2, q) / det;
    return u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t_min <= t && t <= t_max;
}

// the primitive of soup_trace_k: the hit parameters are u and v
struct Triangles {
    static constexpr int NPAR = 2;
    const double* __restrict__ pts;
    __device__ inline bool test(const double* o, const double* dn, int32_t id, double t_min, double t_max, double& t,
                                double (&par)[2]) const {
        return hit_test(o, dn, pts + (int64_t)id * 9, t_min, t_max, t, par[0], par[1]);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// shade: one lane per (ray, hit)
// ---------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(BLOCK) surface_shade_k(int64_t n, int32_t K, const double* __restrict__ dir,
                                                         const int32_t* __restrict__ tri, const double* __restrict__ hu,
                                                         const double* __restrict__ hv, const double* __restrict__ pts,
                                                         const double* __restrict__ values, int32_t Kt,
                                                         const double* __restrict__ table, double lo, double hi,
                                                         double ambient, double* __restrict__ layer) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / K;
    const int32_t id = tri[i];
    double c = dnan();
    if (id >= 0) {
        const double u = hu[i], v = hv[i];
        const double w = (1.0 - u) - v;
        c = (w * values[(int64_t)id * 3] + u * values[(int64_t)id * 3 + 1]) + v * values[(int64_t)id * 3 + 2];
    }
    if (!isfinite(c)) return layer_zero(layer + i * 4);
    double col[4];
    table_row(c, lo, hi - lo, (double)(Kt - 1), Kt, table, col);
    const double* p = pts + (int64_t)id * 9;
    double e1[3], e2[3], nrm[3], dn[3];
    for (int a = 0; a < 3; ++a) {
        e1[a] = p[3 + a] - p[a];
        e2[a] = p[6 + a] - p[a];
        dn[a] = dir[r * 3 + a];
    }
    cross3(e1, e2, nrm);
    layer_shaded(col, nrm, dn, ambient, layer + i * 4);
}

}  // namespace

void surface_build_device(Surface& S, int64_t T, const double* d_points, GridWork& w, hipStream_t st) {
    S.n = T;
    S.P = 0;
    S.g = Grid{};
    if (T == 0) return;
    if (d_points != S.pts.p) {
        S.pts.ensure((size_t)T * 9);
        MGB_HIP_CHECK(hipMemcpyAsync(S.pts.p, d_points, (size_t)T * 9 * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    w.box.ensure((size_t)T * 6);
    hipLaunchKernelGGL(tri_boxes, dim3(grid_1d(T)), dim3(BLOCK), 0, st, T, S.pts.p, w.box.p);
    S.P = cell_lists_from_boxes<3>("surface", "triangle", T, w.box.p, SOUP_CELLS, S.g, S.start, S.cand, w, st);
}

void surface_build(Surface& S, int64_t T, const double* points, hipStream_t st) {
    if (T) S.pts.upload(points, (size_t)T * 9, st);
    GridWork w;                                // freed on return
    surface_build_device(S, T, S.pts.p, w, st);
}

void surface_trace_device(Surface& S, int64_t R, const double* d_o, const double* d_dn, double t_min, double t_max,
                          int32_t K, hipStream_t st) {
    soup_trace_device(S, "surface", Triangles{S.pts.p}, R, d_o, d_dn, t_min, t_max, K, st);
}

void surface_trace(Surface& S, int64_t R, const double* o, const double* dn, double t_min, double t_max, int32_t K,
                   double* t, int32_t* tri, double* u, double* v, hipStream_t st) {
    soup_trace(S, "surface", Triangles{S.pts.p}, R, o, dn, t_min, t_max, K, t, tri, {u, v}, st);
}

void surface_shade_device(const Surface& S, int64_t R, int32_t K, const double* d_dn, const int32_t* d_tri, const double* d_u,
                          const double* d_v, const double* d_values, int32_t Kt, const double* d_table, double lo, double hi,
                          double ambient, double* d_layer, hipStream_t st) {
    const int64_t n = R * K;
    hipLaunchKernelGGL(surface_shade_k, dim3(grid_1d(n)), dim3(BLOCK), 0, st, n, K, d_dn, d_tri, d_u, d_v, S.pts.p, d_values,
                       Kt, d_table, lo, hi, ambient, d_layer);
    MGB_HIP_CHECK(hipGetLastError());
}

void surface_shade(Surface& S, int64_t R, int32_t K, const double* dn, const int32_t* tri, const double* u,
                   const double* v, const double* values, int32_t Kt, const double* table, double lo, double hi,
                   double ambient, double* layer, hipStream_t st) {
    soup_shade<2>(S, R, K, nullptr, dn, nullptr, tri, {u, v}, values, 3, Kt, table, layer, st, [&] {
        surface_shade_device(S, R, K, S.dn.p, S.id.p, S.par[0].p, S.par[1].p, S.values.p, Kt, S.table.p, lo, hi, ambient,
                             S.layer.p, st);
    });
}

}  // namespace mgbhip
