// Rays against a soup of capsules: mgbhip_tubes_* (include/mgbhip.h).
//
// reference: curves drawn as tubes, ext/MultiGridBarrierPyPlotExt/plot3d.jl:209-224 and :279-308 (PyVista's poly.tube on
// the CPU).  Here a curve is a soup of segments, each with a radius: a capsule, the set of points within r of the
// segment [a, b] -- a cylinder body with a spherical cap at each end, so consecutive segments of a polyline join
// without a gap.  One thread per segment forms the box of its two end points widened by its radius; from there the grid
// is that of surface.hip (csrc/box_grid.hpp, the one copy both files include).  One lane per ray then walks the cells
// with the 3-D DDA of surface_trace_k, restated here so that kernel's registers stay as they are, and tests every
// capsule of a cell's list; what a ray hits is a function of the ray and the capsule alone, the grid only decides what
// is tested.
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
//
// Every index is bounded before it is used: a cell index is clamped to the grid, a candidate is < S by construction,
// the walk takes at most n[0] + n[1] + n[2] steps, and the hit list of a ray has the compile-time length K.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "box_grid.hpp"
#include "tubes.hpp"

// No fused multiply-adds in this file: a plain IEEE transcription of the capsule test (tests/tubes_twin.py) then runs
// the same additions and products; only the square roots and divisions could round differently.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

constexpr int32_t NO_SEGMENT = 2147483647;             // in a lane's list; written out as -1

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

__device__ inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

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

// ---------------------------------------------------------------------------------------------------------------
// trace: one lane per ray
// ---------------------------------------------------------------------------------------------------------------

// The lane keeps (t, segment) of its K nearest hits in ascending order, indexed only by unrolled loops so that the list
// stays in registers; s is recomputed for the kept segments at the end by the same operations.  The walk is that of
// surface_trace_k.  A hit at t lies in the cell the ray is in at t, and the capsule's box covers its surface, so
// every hit before a cell's exit has been met by the time the cell is done.
template <int K>
__global__ void __launch_bounds__(BLOCK) tube_trace_k(int64_t R, const double* __restrict__ org,
                                                      const double* __restrict__ dir, double t_min, double t_max,
                                                      SurfaceGrid g, const int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ cand, const double* __restrict__ pts,
                                                      const double* __restrict__ rad, double* __restrict__ out_t,
                                                      int32_t* __restrict__ out_seg, double* __restrict__ out_s) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double o[3], dn[3];
    for (int a = 0; a < 3; ++a) { o[a] = org[r * 3 + a]; dn[a] = dir[r * 3 + a]; }
    double kt[K];
    int32_t ki[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { kt[j] = INFINITY; ki[j] = NO_SEGMENT; }

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
                bool seen = false;             // met in an earlier cell: the same capsule gives the same t
#pragma unroll
                for (int k = 0; k < K; ++k) seen = seen || ki[k] == ic;
                if (seen) continue;
                double tc, sc;
                if (!capsule_test(o, dn, pts + (int64_t)ic * 6, rad[ic], t_min, t_max, tc, sc)) continue;
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
        double t = INFINITY, s = dnan();
        int32_t id = -1;
        if (ki[k] != NO_SEGMENT) {
            id = ki[k];
            capsule_test(o, dn, pts + (int64_t)id * 6, rad[id], t_min, t_max, t, s);
        }
        out_t[r * K + k] = t;
        out_seg[r * K + k] = id;
        out_s[r * K + k] = s;
    }
}

template <int K>
void launch_trace(const Tubes& T, int64_t R, double t_min, double t_max, hipStream_t st) {
    hipLaunchKernelGGL((tube_trace_k<K>), dim3(grid_1d(R)), dim3(BLOCK), 0, st, R, T.o.p, T.dn.p, t_min, t_max, T.g,
                       T.start.p, T.cand.p, T.pts.p, T.rad.p, T.t.p, T.seg.p, T.s.p);
}

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
    if (!isfinite(c)) {
        for (int k = 0; k < 4; ++k) layer[i * 4 + k] = 0.0;
        return;
    }
    // the table row, as surface_shade_k finds it
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

void tubes_build(Tubes& T, int64_t S, const double* points, const double* radii, hipStream_t st) {
    T.S = S;
    T.P = 0;
    T.g = SurfaceGrid{};
    if (S == 0) return;
    T.pts.upload(points, (size_t)S * 6, st);
    T.rad.upload(radii, (size_t)S, st);
    DevBuf<double> box;
    box.alloc((size_t)S * 6);
    hipLaunchKernelGGL(seg_boxes, dim3(grid_1d(S)), dim3(BLOCK), 0, st, S, T.pts.p, T.rad.p, box.p);
    T.P = grid_from_boxes("tubes", "segment", S, box, T.g, T.start, T.cand, st);
}

void tubes_trace(Tubes& T, int64_t R, const double* o, const double* dn, double t_min, double t_max, int32_t K, double* t,
                 int32_t* seg, double* s, hipStream_t st) {
    if (R == 0) return;
    const size_t n = (size_t)R * K;
    if (T.S == 0) {                            // an empty soup: every ray misses
        for (size_t i = 0; i < n; ++i) {
            t[i] = std::numeric_limits<double>::infinity();
            seg[i] = -1;
            s[i] = std::numeric_limits<double>::quiet_NaN();
        }
        return;
    }
    T.o.upload(o, (size_t)R * 3, st);
    T.dn.upload(dn, (size_t)R * 3, st);
    T.t.ensure(n); T.s.ensure(n); T.seg.ensure(n);
    switch (K) {
        case 1: launch_trace<1>(T, R, t_min, t_max, st); break;
        case 2: launch_trace<2>(T, R, t_min, t_max, st); break;
        case 3: launch_trace<3>(T, R, t_min, t_max, st); break;
        case 4: launch_trace<4>(T, R, t_min, t_max, st); break;
        case 5: launch_trace<5>(T, R, t_min, t_max, st); break;
        case 6: launch_trace<6>(T, R, t_min, t_max, st); break;
        case 7: launch_trace<7>(T, R, t_min, t_max, st); break;
        case 8: launch_trace<8>(T, R, t_min, t_max, st); break;
        default: throw InvalidArgument("tubes: K must be 1..8");
    }
    MGB_HIP_CHECK(hipGetLastError());
    T.t.download(t, n, st);
    T.seg.download(seg, n, st);
    T.s.download(s, n, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void tubes_shade(Tubes& T, int64_t R, int32_t K, const double* o, const double* dn, const double* t, const int32_t* seg,
                 const double* s, const double* values, int32_t Kt, const double* table, double lo, double hi,
                 double ambient, double* layer, hipStream_t st) {
    if (R == 0) return;
    const size_t n = (size_t)R * K;
    if (T.S == 0) {                            // the caller has checked that every seg is -1
        std::fill(layer, layer + n * 4, 0.0);
        return;
    }
    T.o.upload(o, (size_t)R * 3, st);
    T.dn.upload(dn, (size_t)R * 3, st);
    T.t.upload(t, n, st);
    T.seg.upload(seg, n, st);
    T.s.upload(s, n, st);
    T.values.upload(values, (size_t)T.S * 2, st);
    T.table.upload(table, (size_t)Kt * 4, st);
    T.layer.ensure(n * 4);
    hipLaunchKernelGGL(tube_shade_k, dim3(grid_1d((int64_t)n)), dim3(BLOCK), 0, st, (int64_t)n, K, T.o.p, T.dn.p, T.t.p,
                       T.seg.p, T.s.p, T.pts.p, T.values.p, Kt, T.table.p, lo, hi, ambient, T.layer.p);
    MGB_HIP_CHECK(hipGetLastError());
    T.layer.download(layer, n * 4, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
