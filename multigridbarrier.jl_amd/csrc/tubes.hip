// Rays against a soup of capsules: mgbhip_tubes_* (include/mgbhip.h).
//
// reference: curves drawn as tubes, ext/MultiGridBarrierPyPlotExt/plot3d.jl:209-224 and :279-308 (PyVista's poly.tube on
// the CPU).  Here a curve is a soup of segments, each with a radius: a capsule, the set of points within r of the
// segment [a, b] -- a cylinder body with a spherical cap at each end, so consecutive segments of a polyline join
// without a gap.  One thread per segment forms the box of its two end points widened by its radius; from there the grid
// is that of surface.hip (csrc/cell_lists.hpp) and so is the walk of a ray through its cells (csrc/soup_trace.hpp), the
// one copy of each that both files include.  This file brings the capsule: its box, its test and its shading.
//
// The capsule test reports where the ray enters the capsule, as the smallest of up to three candidates: the first root
// ts of the infinite cylinder around the axis, kept only if its point projects into the segment (0 <= y <= ba.ba), and
// the first roots ta, tb of the spheres of radius r around a and b.  That minimum is exact for the union: the capsule C
// is convex, so the ray meets it in one interval [t_in, t_out].  (i) Every kept candidate is a point of C (a cylinder
// point that projects into the segment is at distance r from it; the spheres lie in C), so each is >= t_in.  (ii) The
// point at t_in lies on the boundary of C, which is made of the cylinder's side over the segment and the two outer
// half spheres.  On the side, the ray is inside C and hence inside the infinite cylinder just after t_in, so t_in is
// the cylinder's first root and projects into the segment: ts = t_in is kept.  On a half sphere, C and that sphere
// coincide near the point, so t_in is that sphere's first root.  Hence the minimum is t_in.  A ray parallel to the axis
// (A = 0) never crosses the side and is decided by the caps; a segment with a == b is a sphere, reported by cap a.
// Exit points are never reported: a ray that starts inside a capsule has t_in < 0 <= t_min and misses it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "soup_trace.hpp"
#include "tubes.hpp"

// No fused multiply-adds in this file: a plain IEEE transcription of the capsule test (tests/tubes_twin.py) then runs
// the same additions and products; only the square roots and divisions could round differently.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

// one thread per segment: the box of its two end points widened by its radius (lo then hi)
__global__ void __launch_bounds__(BLOCK) seg_boxes(int64_t S, const double* __restrict__ pts,
                                                   const double* __restrict__ rad, double* __restrict__ box) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S) return;
    const double r = rad[e];
    for (int a = 0; a < 3; ++a) {
        const double x0 = pts[e * 6 + a], x1 = pts[e * 6 + 3 + a];
        box[e * 6 + a] = fmin(x0, x1) - r;
        box[e * 6 + 3 + a] = fmax(x0, x1) + r;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the capsule test
// ---------------------------------------------------------------------------------------------------------------

// ray o + t dn against the capsule of radius r around the segment at p (a, b): the entry parameter t and the axis
// parameter s of the entry point (0: cap a, 1: cap b, y / ba.ba on the side)
__device__ inline bool capsule_test(const double* o, const double* dn, const double* __restrict__ p, double r,
                                    double t_min, double t_max, double& t, double& s) {
    double ba[3], oa[3], ob[3];
    for (int a = 0; a < 3; ++a) {
        ba[a] = p[3 + a] - p[a];
        oa[a] = o[a] - p[a];
        ob[a] = o[a] - p[3 + a];
    }
    const double baba = dot3(ba, ba), bard = dot3(ba, dn), baoa = dot3(ba, oa), rdoa = dot3(dn, oa), oaoa = dot3(oa, oa);
    const double rr = r * r;
    const double A = baba - bard * bard;
    const double B = baba * rdoa - baoa * bard;
    const double Cq = (baba * oaoa - baoa * baoa) - rr * baba;
    const double h = B * B - A * Cq;
    t = INFINITY;
    s = dnan();
    if (A > 0.0 && h >= 0.0) {                 // the side
        const double ts = (-B - sqrt(h)) / A;
        const double y = baoa + ts * bard;
        if (y >= 0.0 && y <= baba) { t = ts; s = y / baba; }
    }
    {                                          // cap a
        const double c2 = oaoa - rr;
        const double h2 = rdoa * rdoa - c2;
        if (h2 >= 0.0) {
            const double ta = -rdoa - sqrt(h2);
            if (ta < t) { t = ta; s = 0.0; }
        }
    }
    {                                          // cap b
        const double b2 = dot3(dn, ob);
        const double c2 = dot3(ob, ob) - rr;
        const double h2 = b2 * b2 - c2;
        if (h2 >= 0.0) {
            const double tb = -b2 - sqrt(h2);
            if (tb < t) { t = tb; s = 1.0; }
        }
    }
    return t < INFINITY && t_min <= t && t <= t_max;   // t is +inf when no piece was valid
}

// the primitive of soup_trace_k: the hit parameter is s
struct Capsules {
    static constexpr int NPAR = 1;
    const double* __restrict__ pts;
    const double* __restrict__ rad;
    __device__ inline bool test(const double* o, const double* dn, int32_t id, double t_min, double t_max, double& t,
                                double (&par)[1]) const {
        return capsule_test(o, dn, pts + (int64_t)id * 6, rad[id], t_min, t_max, t, par[0]);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// shade: one lane per (ray, hit)
// ---------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(BLOCK) tube_shade_k(int64_t n, int32_t K, const double* __restrict__ org,
                                                      const double* __restrict__ dir, const double* __restrict__ ht,
                                                      const int32_t* __restrict__ seg, const double* __restrict__ hs,
                                                      const double* __restrict__ pts, const double* __restrict__ values,
                                                      int32_t Kt, const double* __restrict__ table, double lo, double hi,
                                                      double ambient, double* __restrict__ layer) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / K;
    const int32_t id = seg[i];
    double c = dnan(), s = dnan();
    if (id >= 0) {
        s = hs[i];
        c = (1.0 - s) * values[(int64_t)id * 2] + s * values[(int64_t)id * 2 + 1];
    }
    if (!isfinite(c)) return layer_zero(layer + i * 4);
    double col[4];
    table_row(c, lo, hi - lo, (double)(Kt - 1), Kt, table, col);
    // the normal: from the nearest point of the axis to the hit point
    const double* p = pts + (int64_t)id * 6;
    const double t = ht[i];
    double nrm[3], dn[3];
    for (int a = 0; a < 3; ++a) {
        dn[a] = dir[r * 3 + a];
        const double x = org[r * 3 + a] + t * dn[a];
        const double q = p[a] + s * (p[3 + a] - p[a]);
        nrm[a] = x - q;
    }
    layer_shaded(col, nrm, dn, ambient, layer + i * 4);
}

}  // namespace

void tubes_build(Tubes& T, int64_t S, const double* points, const double* radii, hipStream_t st) {
    T.n = S;
    T.P = 0;
    T.g = Grid{};
    if (S == 0) return;
    T.pts.upload(points, (size_t)S * 6, st);
    T.rad.upload(radii, (size_t)S, st);
    DevBuf<double> box;
    box.alloc((size_t)S * 6);
    hipLaunchKernelGGL(seg_boxes, dim3(grid_1d(S)), dim3(BLOCK), 0, st, S, T.pts.p, T.rad.p, box.p);
    T.P = cell_lists_from_boxes<3>("tubes", "segment", S, box.p, SOUP_CELLS, T.g, T.start, T.cand, st);
}

void tubes_trace(Tubes& T, int64_t R, const double* o, const double* dn, double t_min, double t_max, int32_t K, double* t,
                 int32_t* seg, double* s, hipStream_t st) {
    soup_trace(T, "tubes", Capsules{T.pts.p, T.rad.p}, R, o, dn, t_min, t_max, K, t, seg, {s}, st);
}

void tubes_shade(Tubes& T, int64_t R, int32_t K, const double* o, const double* dn, const double* t, const int32_t* seg,
                 const double* s, const double* values, int32_t Kt, const double* table, double lo, double hi,
                 double ambient, double* layer, hipStream_t st) {
    soup_shade<1>(T, R, K, o, dn, t, seg, {s}, values, 2, Kt, table, layer, st, [&] {
        const int64_t n = R * K;
        hipLaunchKernelGGL(tube_shade_k, dim3(grid_1d(n)), dim3(BLOCK), 0, st, n, K, T.o.p, T.dn.p, T.t.p, T.id.p, T.par[0].p,
                           T.pts.p, T.values.p, Kt, T.table.p, lo, hi, ambient, T.layer.p);
    });
}

}  // namespace mgbhip
