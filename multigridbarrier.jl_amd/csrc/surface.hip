// Rays against a triangle soup: mgbhip_surface_* (include/mgbhip.h).
//
// reference: the isosurfaces and slices of `plot` for fem3d solutions, ext/MultiGridBarrierPyPlotExt/plot3d.jl:85-149
// (PyVista's add_mesh on the CPU).  Here the soup that mgbhip_contour_create cuts is put into a uniform grid of cells
// the way the point locator puts element boxes into one (interpolate.hip; restated here because that grid is tied to
// the element families and their containment tolerances): one thread per triangle forms its box, one block reduces
// the union, the host picks the cell counts, a count pass and an exclusive scan size the (cell, triangle) pair list, an
// emit pass writes it in triangle order and a stable radix sort by cell leaves every cell's list ascending in
// triangle index.  No atomics.  One lane per ray then walks the cells with a 3-D DDA and tests every triangle of a
// cell's list; what a ray hits is a function of the ray and the triangle alone, the grid only decides what is tested.
//
// Every index is bounded before it is used: a cell index is clamped to the grid, a candidate is < T by construction,
// the walk takes at most n[0] + n[1] + n[2] steps, and the hit list of a ray has the compile-time length K.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "surface.hpp"

// No fused multiply-adds in this file: a plain IEEE transcription of the triangle test (tests/surface_twin.py) then
// gives the same t, u and v bit for bit.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

constexpr int BLOCK = 256;
// Every triangle's box is widened by PAD_REL * (largest extent of the union + largest |coordinate|) per side before it
// is cut into cells.  The walk places a ray in a cell with an error of a few eps * (|origin| + |coordinate|) per axis,
// and a computed hit point leaves its triangle's box by as little; 2^-26 covers both for origins up to 2^20 box sizes
// away, and is far below any cell side, so it adds no pairs to speak of.
constexpr double PAD_REL = 1.4901161193847656e-08;   // 2^-26
constexpr int32_t NO_TRIANGLE = 2147483647;            // in a lane's list; written out as -1

inline unsigned grid_1d(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

__device__ inline double dnan() { return __builtin_nan(""); }

// cell index of a scaled coordinate; NaN and anything below the box go to cell 0, anything above to the last cell
__device__ inline int32_t cell_axis(double s, int32_t n) {
    if (!(s >= 0.0)) return 0;
    if (s >= (double)n) return n - 1;
    const int32_t c = (int32_t)s;
    return c < n - 1 ? c : n - 1;
}

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

// one block: the union of all boxes (6 doubles: lo then hi)
__global__ void __launch_bounds__(1024) union_box(int64_t T, const double* __restrict__ box, double* __restrict__ out) {
    __shared__ double s[6][1024];
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int64_t e = threadIdx.x; e < T; e += blockDim.x)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], box[e * 6 + a]);
            hi[a] = fmax(hi[a], box[e * 6 + 3 + a]);
        }
    for (int a = 0; a < 3; ++a) { s[a][threadIdx.x] = lo[a]; s[3 + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int h = blockDim.x / 2; h > 0; h /= 2) {
        if ((int)threadIdx.x < h)
            for (int a = 0; a < 3; ++a) {
                s[a][threadIdx.x] = fmin(s[a][threadIdx.x], s[a][threadIdx.x + h]);
                s[3 + a][threadIdx.x] = fmax(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + h]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) out[threadIdx.x] = s[threadIdx.x][0];
}

// the cells the padded box of a triangle overlaps
__device__ inline void box_cells(const SurfaceGrid& g, const double* b, int32_t* c0, int32_t* c1) {
    for (int a = 0; a < 3; ++a) {
        c0[a] = cell_axis(((b[a] - g.pad) - g.lo[a]) * g.inv[a], g.n[a]);
        c1[a] = cell_axis(((b[3 + a] + g.pad) - g.lo[a]) * g.inv[a], g.n[a]);
    }
}

__global__ void __launch_bounds__(BLOCK) box_counts(int64_t T, SurfaceGrid g, const double* __restrict__ box,
                                                    int64_t* __restrict__ count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T) return;
    int32_t c0[3], c1[3];
    box_cells(g, box + e * 6, c0, c1);
    int64_t c = 1;
    for (int a = 0; a < 3; ++a) c *= (int64_t)(c1[a] - c0[a] + 1);
    count[e] = c;
}

__global__ void __launch_bounds__(BLOCK) emit_pairs(int64_t T, SurfaceGrid g, const double* __restrict__ box,
                                                    const int64_t* __restrict__ off, uint32_t* __restrict__ keys,
                                                    int32_t* __restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T) return;
    int32_t c0[3], c1[3];
    box_cells(g, box + e * 6, c0, c1);
    int64_t o = off[e];
    for (int32_t l = c0[2]; l <= c1[2]; ++l)
        for (int32_t j = c0[1]; j <= c1[1]; ++j)
            for (int32_t i = c0[0]; i <= c1[0]; ++i, ++o) {
                keys[o] = (uint32_t)(((int64_t)l * g.n[1] + j) * g.n[0] + i);
                vals[o] = (int32_t)e;
            }
}

// start[c] = first sorted pair of cell c (start[ncell] = P): every cell is written exactly once
__global__ void __launch_bounds__(BLOCK) cell_starts(int64_t P, int64_t ncell, const uint32_t* __restrict__ keys,
                                                     int32_t* __restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > P) return;
    const int64_t a = i == 0 ? -1 : (int64_t)keys[i - 1];
    const int64_t b = i == P ? ncell : (int64_t)keys[i];
    for (int64_t c = a + 1; c <= b; ++c) start[c] = (int32_t)i;
}

// cells of side h with h^(#axes of positive extent) = volume / (cells_per_triangle * T), at most 1024 per axis
SurfaceGrid pick_grid(const double* hb, int64_t T, double cells_per_triangle) {
    SurfaceGrid g{};
    double ext_max = 0.0, mag = 0.0;
    for (int a = 0; a < 3; ++a) {
        ext_max = std::max(ext_max, hb[3 + a] - hb[a]);
        mag = std::max(mag, std::max(std::fabs(hb[a]), std::fabs(hb[3 + a])));
    }
    g.pad = PAD_REL * (ext_max + mag);
    double vol = 1.0;
    int nz = 0;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = hb[a] - 2.0 * g.pad;
        g.hi[a] = hb[3 + a] + 2.0 * g.pad;
        if (g.hi[a] > g.lo[a]) { vol *= g.hi[a] - g.lo[a]; ++nz; }
    }
    const double h = nz ? std::pow(vol / (cells_per_triangle * (double)T), 1.0 / nz) : 1.0;
    g.ncell = 1;
    for (int a = 0; a < 3; ++a) {
        const double ext = g.hi[a] - g.lo[a];
        int64_t n = ext > 0 && h > 0 ? (int64_t)std::ceil(ext / h) : 1;
        n = std::max<int64_t>(1, std::min<int64_t>(n, 1024));
        g.n[a] = (int32_t)n;
        g.inv[a] = ext > 0 ? (double)n / ext : 0.0;
        g.size[a] = ext > 0 ? ext / (double)n : 0.0;
        g.ncell *= n;
    }
    return g;
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
void launch_trace(const Surface& S, int64_t R, double t_min, double t_max, hipStream_t st) {
    hipLaunchKernelGGL((surface_trace_k<K>), dim3(grid_1d(R)), dim3(BLOCK), 0, st, R, S.o.p, S.dn.p, t_min, t_max, S.g,
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

void surface_build(Surface& S, int64_t T, const double* points, hipStream_t st) {
    S.T = T;
    S.P = 0;
    S.g = SurfaceGrid{};
    if (T == 0) return;
    S.pts.upload(points, (size_t)T * 9, st);
    DevBuf<double> box, ubox;
    box.alloc((size_t)T * 6);
    ubox.alloc(6);
    hipLaunchKernelGGL(tri_boxes, dim3(grid_1d(T)), dim3(BLOCK), 0, st, T, S.pts.p, box.p);
    hipLaunchKernelGGL(union_box, dim3(1), dim3(1024), 0, st, T, box.p, ubox.p);
    MGB_HIP_CHECK(hipGetLastError());
    double hb[6];
    ubox.download(hb, 6, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    for (int a = 0; a < 6; ++a) MGB_REQUIRE(std::isfinite(hb[a]), "surface: non-finite triangle box");
    DevBuf<int64_t> count, off;
    count.alloc((size_t)T);
    off.alloc((size_t)T);
    DevBuf<char> tmp;
    // About four cells per triangle.  Triangles that span many cells (a slice next to a fine isosurface) can make the
    // pair list far longer than the soup: the grid is then coarsened until the list is at most 16 T + 4096 pairs.
    double cells_per_triangle = 4.0;
    int64_t P = 0;
    for (;;) {
        S.g = pick_grid(hb, T, cells_per_triangle);
        hipLaunchKernelGGL(box_counts, dim3(grid_1d(T)), dim3(BLOCK), 0, st, T, S.g, box.p, count.p);
        MGB_HIP_CHECK(hipGetLastError());
        size_t scan_bytes = 0;
        MGB_HIP_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, count.p, off.p, (int64_t)0, (size_t)T,
                                              rocprim::plus<int64_t>(), st));
        tmp.ensure(scan_bytes + 16);
        MGB_HIP_CHECK(rocprim::exclusive_scan((void*)tmp.p, scan_bytes, count.p, off.p, (int64_t)0, (size_t)T,
                                              rocprim::plus<int64_t>(), st));
        int64_t last_off = 0, last_count = 0;
        MGB_HIP_CHECK(hipMemcpyAsync(&last_off, off.p + (T - 1), sizeof(int64_t), hipMemcpyDeviceToHost, st));
        MGB_HIP_CHECK(hipMemcpyAsync(&last_count, count.p + (T - 1), sizeof(int64_t), hipMemcpyDeviceToHost, st));
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        P = last_off + last_count;
        if (P <= 16 * T + 4096 || S.g.ncell == 1) break;
        cells_per_triangle *= 0.125;
    }
    MGB_REQUIRE(P > 0 && P < (int64_t)INT32_MAX, "surface: (cell, triangle) pair count exceeds 32-bit indexing");
    S.P = P;
    DevBuf<uint32_t> k0, k1;
    DevBuf<int32_t> v0;
    k0.alloc((size_t)P); k1.alloc((size_t)P); v0.alloc((size_t)P);
    S.cand.alloc((size_t)P);
    hipLaunchKernelGGL(emit_pairs, dim3(grid_1d(T)), dim3(BLOCK), 0, st, T, S.g, box.p, off.p, k0.p, v0.p);
    MGB_HIP_CHECK(hipGetLastError());
    unsigned bits = 1;
    while (bits < 32 && ((uint64_t)S.g.ncell >> bits) != 0) ++bits;
    size_t sort_bytes = 0;
    MGB_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, k0.p, k1.p, v0.p, S.cand.p, (size_t)P, 0u, bits, st));
    tmp.ensure(sort_bytes + 16);
    MGB_HIP_CHECK(rocprim::radix_sort_pairs((void*)tmp.p, sort_bytes, k0.p, k1.p, v0.p, S.cand.p, (size_t)P, 0u, bits, st));
    S.start.alloc((size_t)S.g.ncell + 1);
    hipLaunchKernelGGL(cell_starts, dim3(grid_1d(P + 1)), dim3(BLOCK), 0, st, P, S.g.ncell, k1.p, S.start.p);
    MGB_HIP_CHECK(hipGetLastError());
    MGB_HIP_CHECK(hipStreamSynchronize(st));
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
    S.t.ensure(n); S.u.ensure(n); S.v.ensure(n); S.tri.ensure(n);
    switch (K) {
        case 1: launch_trace<1>(S, R, t_min, t_max, st); break;
        case 2: launch_trace<2>(S, R, t_min, t_max, st); break;
        case 3: launch_trace<3>(S, R, t_min, t_max, st); break;
        case 4: launch_trace<4>(S, R, t_min, t_max, st); break;
        case 5: launch_trace<5>(S, R, t_min, t_max, st); break;
        case 6: launch_trace<6>(S, R, t_min, t_max, st); break;
        case 7: launch_trace<7>(S, R, t_min, t_max, st); break;
        case 8: launch_trace<8>(S, R, t_min, t_max, st); break;
        default: throw InvalidArgument("surface: K must be 1..8");
    }
    MGB_HIP_CHECK(hipGetLastError());
    S.t.download(t, n, st);
    S.tri.download(tri, n, st);
    S.u.download(u, n, st);
    S.v.download(v, n, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
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
    hipLaunchKernelGGL(surface_shade_k, dim3(grid_1d((int64_t)n)), dim3(BLOCK), 0, st, (int64_t)n, K, S.dn.p, S.tri.p,
                       S.u.p, S.v.p, S.pts.p, S.values.p, Kt, S.table.p, lo, hi, ambient, S.layer.p);
    MGB_HIP_CHECK(hipGetLastError());
    S.layer.download(layer, n * 4, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
