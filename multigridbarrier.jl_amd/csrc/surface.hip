// Rays against a triangle soup: mgbhip_surface_* (include/mgbhip.h).
//
// reference: the isosurfaces and slices of `plot` for fem3d solutions, ext/MultiGridBarrierPyPlotExt/plot3d.jl:85-149
// (PyVista's add_mesh on the CPU).  Here the soup that mgbhip_contour_create cuts is put into a uniform grid of cells
// the way the point locator puts element boxes into one (interpolate.hip; restated here because that grid is tied to
// the element families and their containment tolerances): one thread per triangle forms its box, one block reduces
// the union, the host picks the cell counts, a count pass and an exclusive scan size the (cell, triangle) pair list, an
// emit pass writes it in triangle order and a stable radix sort by cell leaves every cell's list ascending in
// triangle index.  No atomics.  Everything after the boxes lives in box_grid.hpp, which tubes.hip includes too.  One lane per ray then walks the cells with a 3-D DDA and tests every triangle of a
// cell's list; what a ray hits is a function of the ray and the triangle alone, the grid only decides what is tested.
//
// Every index is bounded before it is used: a cell index is clamped to the grid, a candidate is < T by construction,
// the walk takes at most n[0] + n[1] + n[2] steps, and the hit list of a ray has the compile-time length K.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "box_grid.hpp"
#include "surface.hpp"

// No fused multiply-adds in this file: a plain IEEE transcription of the triangle test (tests/surface_twin.py) then
// gives the same t, u and v bit for bit.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

constexpr int32_t NO_TRIANGLE = 2147483647;            // in a lane's list; written out as -1

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

__device__ inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ inline void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

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

// ---------------------------------------------------------------------------------------------------------------
// trace: one lane per ray
// ---------------------------------------------------------------------------------------------------------------

// The lane keeps (t, triangle) of its K nearest hits in ascending order, indexed only by unrolled loops so that the
// list stays in registers; u and v are recomputed for the kept triangles at the end by the same operations.
template <int K>
__global__ void __launch_bounds__(BLOCK) surface_trace_k(int64_t R, const double* __restrict__ org,
                                                         const double* __restrict__ dir, double t_min, double t_max,
                                                         SurfaceGrid g, const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ cand, const double* __restrict__ pts,
                                                         double* __restrict__ out_t, int32_t* __restrict__ out_tri,
                                                         double* __restrict__ out_u, double* __restrict__ out_v) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double o[3], dn[3];
    for (int a = 0; a < 3; ++a) { o[a] = org[r * 3 + a]; dn[a] = dir[r * 3 + a]; }
    double kt[K];
    int32_t ki[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { kt[j] = INFINITY; ki[j] = NO_TRIANGLE; }

    // the slab test against the grid box
    double tin = t_min, tout = t_max;
    bool miss = false;
    for (int a = 0; a < 3; ++a) {
        if (dn[a] != 0.0) {
            const double t1 = (g.lo[a] - o[a]) / dn[a], t2 = (g.hi[a] - o[a]) / dn[a];
            tin = fmax(tin, fmin(t1, t2));
            tout = fmin(tout, fmax(t1, t2));
        } else if (!(g.lo[a] <= o[a] && o[a] <= g.hi[a])) {
            miss = true;
        }
    }
    if (!miss && tout >= tin) {
        int32_t c[3], step[3];
        double inv_d[3];
        for (int a = 0; a < 3; ++a) {
            c[a] = cell_axis(((o[a] + tin * dn[a]) - g.lo[a]) * g.inv[a], g.n[a]);
            step[a] = dn[a] > 0.0 ? 1 : (dn[a] < 0.0 ? -1 : 0);
            inv_d[a] = dn[a] != 0.0 ? 1.0 / dn[a] : 0.0;
        }
        const int32_t max_steps = g.n[0] + g.n[1] + g.n[2];
        for (int32_t it = 0; it <= max_steps; ++it) {
            // where the ray leaves this cell: the nearest of the planes ahead, or the end of the ray
            double texit = tout;
            int axis = -1;
            for (int a = 0; a < 3; ++a)
                if (step[a] != 0) {
                    const double plane = g.lo[a] + (double)(c[a] + (step[a] > 0 ? 1 : 0)) * g.size[a];
                    const double ta = (plane - o[a]) * inv_d[a];
                    if (ta < texit) { texit = ta; axis = a; }
                }
            const int64_t cell = ((int64_t)c[2] * g.n[1] + c[1]) * g.n[0] + c[0];
            const int32_t j1 = start[cell + 1];
            for (int32_t j = start[cell]; j < j1; ++j) {
                int32_t ic = cand[j];
                double tc, uc, vc;
                if (!hit_test(o, dn, pts + (int64_t)ic * 9, t_min, t_max, tc, uc, vc)) continue;
                bool seen = false;             // met in an earlier cell: the same triangle gives the same t
#pragma unroll
                for (int k = 0; k < K; ++k) seen = seen || ki[k] == ic;
                if (seen) continue;
#pragma unroll
                for (int k = 0; k < K; ++k) {  // insertion: the candidate sinks to its place, the last entry drops out
                    const bool less = tc < kt[k] || (tc == kt[k] && ic < ki[k]);
                    const double tt = less ? kt[k] : tc;
                    const int32_t ii = less ? ki[k] : ic;
                    kt[k] = less ? tc : kt[k];
                    ki[k] = less ? ic : ki[k];
                    tc = tt;
                    ic = ii;
                }
            }
            if (axis < 0) break;               // the ray ends in this cell
            if (kt[K - 1] <= texit) break;     // nothing ahead can come before the K-th kept hit
            c[axis] += step[axis];
            if (c[axis] < 0 || c[axis] >= g.n[axis]) break;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = INFINITY, u = dnan(), v = dnan();
        int32_t id = -1;
        if (ki[k] != NO_TRIANGLE) {
            id = ki[k];
            hit_test(o, dn, pts + (int64_t)id * 9, t_min, t_max, t, u, v);
        }
        out_t[r * K + k] = t;
        out_tri[r * K + k] = id;
        out_u[r * K + k] = u;
        out_v[r * K + k] = v;
    }
}

template <int K>
void launch_trace(const Surface& S, int64_t R, const double* d_o, const double* d_dn, double t_min, double t_max,
                  hipStream_t st) {
    hipLaunchKernelGGL((surface_trace_k<K>), dim3(grid_1d(R)), dim3(BLOCK), 0, st, R, d_o, d_dn, t_min, t_max, S.g,
                       S.start.p, S.cand.p, S.pts.p, S.t.p, S.tri.p, S.u.p, S.v.p);
}

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
    if (!isfinite(c)) {
        for (int k = 0; k < 4; ++k) layer[i * 4 + k] = 0.0;
        return;
    }
    const double width = hi - lo, km1 = (double)(Kt - 1);
    const double sc = fmin(1.0, fmax(0.0, (c - lo) / width));
    const double f = sc * km1;
    int32_t j = (int32_t)floor(f);
    j = j < Kt - 2 ? j : Kt - 2;
    const double w = f - (double)j;
    const double* t0 = table + (int64_t)j * 4;
    const double cr = t0[0] + w * (t0[4] - t0[0]);
    const double cg = t0[1] + w * (t0[5] - t0[1]);
    const double cb = t0[2] + w * (t0[6] - t0[2]);
    const double ca = t0[3] + w * (t0[7] - t0[3]);
    const double* p = pts + (int64_t)id * 9;
    double e1[3], e2[3], nrm[3], dn[3];
    for (int a = 0; a < 3; ++a) {
        e1[a] = p[3 + a] - p[a];
        e2[a] = p[6 + a] - p[a];
        dn[a] = dir[r * 3 + a];
    }
    cross3(e1, e2, nrm);
    const double len = sqrt(dot3(nrm, nrm));
    for (int a = 0; a < 3; ++a) nrm[a] = nrm[a] / len;
    const double shade = ambient + (1.0 - ambient) * fabs(dot3(nrm, dn));
    const double alpha = fmin(1.0, fmax(0.0, ca));
    const double as = alpha * shade;
    layer[i * 4] = as * cr;
    layer[i * 4 + 1] = as * cg;
    layer[i * 4 + 2] = as * cb;
    layer[i * 4 + 3] = alpha;
}

}  // namespace

void surface_build_device(Surface& S, int64_t T, const double* d_points, GridWork& w, hipStream_t st) {
    S.T = T;
    S.P = 0;
    S.g = SurfaceGrid{};
    if (T == 0) return;
    if (d_points != S.pts.p) {
        S.pts.ensure((size_t)T * 9);
        MGB_HIP_CHECK(hipMemcpyAsync(S.pts.p, d_points, (size_t)T * 9 * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    w.box.ensure((size_t)T * 6);
    hipLaunchKernelGGL(tri_boxes, dim3(grid_1d(T)), dim3(BLOCK), 0, st, T, S.pts.p, w.box.p);
    S.P = grid_from_boxes("surface", "triangle", T, w.box.p, S.g, S.start, S.cand, w, st);
}

void surface_build(Surface& S, int64_t T, const double* points, hipStream_t st) {
    if (T) S.pts.upload(points, (size_t)T * 9, st);
    GridWork w;                                // freed on return
    surface_build_device(S, T, S.pts.p, w, st);
}

void surface_trace_device(Surface& S, int64_t R, const double* d_o, const double* d_dn, double t_min, double t_max,
                          int32_t K, hipStream_t st) {
    const size_t n = (size_t)R * K;
    S.t.ensure(n); S.u.ensure(n); S.v.ensure(n); S.tri.ensure(n);
    switch (K) {
        case 1: launch_trace<1>(S, R, d_o, d_dn, t_min, t_max, st); break;
        case 2: launch_trace<2>(S, R, d_o, d_dn, t_min, t_max, st); break;
        case 3: launch_trace<3>(S, R, d_o, d_dn, t_min, t_max, st); break;
        case 4: launch_trace<4>(S, R, d_o, d_dn, t_min, t_max, st); break;
        case 5: launch_trace<5>(S, R, d_o, d_dn, t_min, t_max, st); break;
        case 6: launch_trace<6>(S, R, d_o, d_dn, t_min, t_max, st); break;
        case 7: launch_trace<7>(S, R, d_o, d_dn, t_min, t_max, st); break;
        case 8: launch_trace<8>(S, R, d_o, d_dn, t_min, t_max, st); break;
        default: throw InvalidArgument("surface: K must be 1..8");
    }
    MGB_HIP_CHECK(hipGetLastError());
}

void surface_trace(Surface& S, int64_t R, const double* o, const double* dn, double t_min, double t_max, int32_t K,
                   double* t, int32_t* tri, double* u, double* v, hipStream_t st) {
    if (R == 0) return;
    const size_t n = (size_t)R * K;
    if (S.T == 0) {                            // an empty soup: every ray misses
        for (size_t i = 0; i < n; ++i) {
            t[i] = std::numeric_limits<double>::infinity();
            tri[i] = -1;
            u[i] = v[i] = std::numeric_limits<double>::quiet_NaN();
        }
        return;
    }
    S.o.upload(o, (size_t)R * 3, st);
    S.dn.upload(dn, (size_t)R * 3, st);
    surface_trace_device(S, R, S.o.p, S.dn.p, t_min, t_max, K, st);
    S.t.download(t, n, st);
    S.tri.download(tri, n, st);
    S.u.download(u, n, st);
    S.v.download(v, n, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
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
    if (R == 0) return;
    const size_t n = (size_t)R * K;
    if (S.T == 0) {                            // the caller has checked that every tri is -1
        std::fill(layer, layer + n * 4, 0.0);
        return;
    }
    S.dn.upload(dn, (size_t)R * 3, st);
    S.tri.upload(tri, n, st);
    S.u.upload(u, n, st);
    S.v.upload(v, n, st);
    S.values.upload(values, (size_t)S.T * 3, st);
    S.table.upload(table, (size_t)Kt * 4, st);
    S.layer.ensure(n * 4);
    surface_shade_device(S, R, K, S.dn.p, S.tri.p, S.u.p, S.v.p, S.values.p, Kt, S.table.p, lo, hi, ambient, S.layer.p, st);
    S.layer.download(layer, n * 4, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
