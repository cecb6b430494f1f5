// cell_lists.hpp -- axis-aligned boxes put into a uniform grid of cells (cell_grid.hpp), for every translation unit that
// needs one: interpolate.hip (the boxes of elements; closest.hip, stream.hip and raycast.hip go through it), surface.hip
// (the boxes of triangles; figure.hip goes through it) and tubes.hip (the boxes of capsules).  Nothing here depends on
// what is inside a box: one block reduces the union of the boxes, a host policy picks the cell counts, a count pass and an
// exclusive scan size the (cell, box) pair list, an emit pass writes it in box order and a stable radix sort by cell
// leaves every cell's list ascending in box index, so the first box of a list that accepts a point or a ray is the
// lowest-index one, whatever the launch configuration.  No atomics.
//
// Everything here has internal linkage (the library is built without relocatable device code, so every translation unit
// carries its own copy of the kernels it launches).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "cell_grid.hpp"
#include "device_prims.hpp"

// No fused multiply-adds in the code below or in a file that includes it: the cells of a box, of a point and of a ray
// come from the same products, and the NumPy twins of the tests transcribe them.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

// Every box of a soup is widened by PAD_REL * (largest extent of the union + largest |coordinate|) per side before it is
// cut into cells.  The walk places a ray in a cell with an error of a few eps * (|origin| + |coordinate|) per axis, and a
// computed hit point leaves the box of what it hit by as little; 2^-26 covers both for origins up to 2^20 box sizes
// away, and is far below any cell side, so it adds no pairs to speak of.
constexpr double PAD_REL = 1.4901161193847656e-08;   // 2^-26

// cell index of a scaled coordinate s = (v - lo) * inv; NaN and anything below the box go to cell 0, anything above to
// the last cell
__device__ inline int32_t cell_axis(double s, int32_t n) {
    if (!(s >= 0.0)) return 0;
    if (s >= (double)n) return n - 1;
    const int32_t c = (int32_t)s;
    return c < n - 1 ? c : n - 1;
}

// one block: the union of all boxes (2*D doubles: lo then hi)
template <int D>
__global__ void __launch_bounds__(1024) union_box(int64_t N, const double* __restrict__ box, double* __restrict__ out) {
    __shared__ double s[2 * D][1024];
    double lo[D], hi[D];
    for (int a = 0; a < D; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int64_t e = threadIdx.x; e < N; e += blockDim.x)
        for (int a = 0; a < D; ++a) {
            lo[a] = fmin(lo[a], box[e * 2 * D + a]);
            hi[a] = fmax(hi[a], box[e * 2 * D + D + a]);
        }
    for (int a = 0; a < D; ++a) { s[a][threadIdx.x] = lo[a]; s[D + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int h = blockDim.x / 2; h > 0; h /= 2) {
        if ((int)threadIdx.x < h)
            for (int a = 0; a < D; ++a) {
                s[a][threadIdx.x] = fmin(s[a][threadIdx.x], s[a][threadIdx.x + h]);
                s[D + a][threadIdx.x] = fmax(s[D + a][threadIdx.x], s[D + a][threadIdx.x + h]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 2 * D) out[threadIdx.x] = s[threadIdx.x][0];
}

// the cells a padded box overlaps
template <int D>
__device__ inline void box_cells(const Grid& g, const double* b, int32_t* c0, int32_t* c1) {
    for (int a = 0; a < D; ++a) {
        c0[a] = cell_axis(((b[a] - g.pad) - g.lo[a]) * g.inv[a], g.n[a]);
        c1[a] = cell_axis(((b[D + a] + g.pad) - g.lo[a]) * g.inv[a], g.n[a]);
    }
}

template <int D>
__global__ void __launch_bounds__(BLOCK) box_counts(int64_t N, Grid g, const double* __restrict__ box,
                                                    int64_t* __restrict__ count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    int32_t c0[D], c1[D];
    box_cells<D>(g, box + e * 2 * D, c0, c1);
    int64_t c = 1;
    for (int a = 0; a < D; ++a) c *= (int64_t)(c1[a] - c0[a] + 1);
    count[e] = c;
}

template <int D>
__global__ void __launch_bounds__(BLOCK) emit_pairs(int64_t N, Grid g, const double* __restrict__ box,
                                                    const int64_t* __restrict__ off, uint32_t* __restrict__ keys,
                                                    int32_t* __restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    int32_t c0[D], c1[D];
    box_cells<D>(g, box + e * 2 * D, c0, c1);
    int64_t o = off[e];
    if constexpr (D == 2) {
        for (int32_t j = c0[1]; j <= c1[1]; ++j)
            for (int32_t i = c0[0]; i <= c1[0]; ++i, ++o) {
                keys[o] = (uint32_t)((int64_t)j * g.n[0] + i);
                vals[o] = (int32_t)e;
            }
    } else {
        for (int32_t l = c0[2]; l <= c1[2]; ++l)
            for (int32_t j = c0[1]; j <= c1[1]; ++j)
                for (int32_t i = c0[0]; i <= c1[0]; ++i, ++o) {
                    keys[o] = (uint32_t)(((int64_t)l * g.n[1] + j) * g.n[0] + i);
                    vals[o] = (int32_t)e;
                }
    }
}

// How the host picks the cells of n boxes whose union is hb (2*D doubles): `pick` returns the grid for a number of cells
// per box, starting from `cells_per_box`.  With `coarsen`, the builder divides that number by 8 until the pair list has
// at most 16 n + 4096 pairs or one cell remains.
struct CellPolicy {
    Grid (*pick)(const double* hb, int64_t n, double cells_per_box);
    double cells_per_box;
    bool coarsen;
};

// A soup of primitives under rays, in three coordinates: cells of side h with h^(#axes of positive extent) = volume /
// (cells_per_box * T), at most 1024 per axis, over the union widened by twice the pad.
inline Grid pick_grid(const double* hb, int64_t T, double cells_per_box) {
    Grid g{};
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
    const double h = nz ? std::pow(vol / (cells_per_box * (double)T), 1.0 / nz) : 1.0;
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

// About four cells per box.  Boxes that span many cells (a slice next to a fine isosurface) can make the pair list far
// longer than the soup: the grid is then coarsened.
constexpr CellPolicy SOUP_CELLS{pick_grid, 4.0, true};

// Elements that points are located in, in D coordinates: about one element per cell, cells of side h with h^(#axes of
// positive extent) = volume / N, at most 4 N + 1 per axis, over the union as it is (the element boxes come padded, so
// pad = 0; size is not used).  A point is looked up in one cell, so a long pair list costs memory and not time: no
// coarsening.
template <int D>
inline Grid pick_location_grid(const double* hb, int64_t N, double) {
    double vol = 1.0;
    int nz = 0;
    for (int a = 0; a < D; ++a)
        if (hb[D + a] > hb[a]) { vol *= hb[D + a] - hb[a]; ++nz; }
    const double h = nz ? std::pow(vol / (double)N, 1.0 / nz) : 1.0;
    Grid g{};
    g.ncell = 1;
    for (int a = 0; a < 3; ++a) { g.lo[a] = g.hi[a] = 0.0; g.inv[a] = 0.0; g.n[a] = 1; }
    for (int a = 0; a < D; ++a) {
        const double ext = hb[D + a] - hb[a];
        g.lo[a] = hb[a];
        g.hi[a] = hb[D + a];
        int64_t n = ext > 0 && h > 0 ? (int64_t)std::ceil(ext / h) : 1;
        n = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)4 * N + 1));
        g.n[a] = (int32_t)n;
        g.inv[a] = ext > 0 ? (double)n / ext : 0.0;
        g.ncell *= n;
    }
    MGB_REQUIRE(g.ncell < (int64_t)INT32_MAX, "interpolate: location grid exceeds 32-bit cell indexing");
    return g;
}

template <int D>
constexpr CellPolicy LOCATION_CELLS{pick_location_grid<D>, 1.0, false};

// The cell lists of n > 0 boxes on the device (box: n x 2D, lo then hi): union, cell counts, count pass, scan, emit pass,
// stable sort by cell, cell starts.  Returns the pair count P; g, start (ncell + 1) and cand (P) are complete on return:
// cell c owns cand[start[c] .. start[c+1]-1].  start, cand and the buffers of w grow and are kept: only the first
// ncell + 1 and P entries are meant.  `who` and `what` name the caller and its primitive in the error messages
// ("surface", "triangle").
template <int D>
int64_t cell_lists_from_boxes(const char* who, const char* what, int64_t n, const double* box, const CellPolicy& policy,
                              Grid& g, DevBuf<int32_t>& start, DevBuf<int32_t>& cand, GridWork& w, hipStream_t st) {
    w.ubox.ensure(2 * D);
    hipLaunchKernelGGL((union_box<D>), dim3(1), dim3(1024), 0, st, n, box, w.ubox.p);
    MGB_HIP_CHECK(hipGetLastError());
    double hb[2 * D];
    w.ubox.download(hb, 2 * D, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    for (int a = 0; a < 2 * D; ++a)
        MGB_REQUIRE(std::isfinite(hb[a]), std::string(who) + ": non-finite " + what + " box");
    w.count.ensure((size_t)n);
    w.off.ensure((size_t)n);
    double cells_per_box = policy.cells_per_box;
    int64_t P = 0;
    for (;;) {
        g = policy.pick(hb, n, cells_per_box);
        hipLaunchKernelGGL((box_counts<D>), dim3(grid_1d(n)), dim3(BLOCK), 0, st, n, g, box, w.count.p);
        MGB_HIP_CHECK(hipGetLastError());
        exclusive_scan(w.count.p, w.off.p, n, w.tmp, st);
        P = scan_total(w.count.p, w.off.p, n, st);
        if (!policy.coarsen || P <= 16 * n + 4096 || g.ncell == 1) break;
        cells_per_box *= 0.125;
    }
    MGB_REQUIRE(P > 0 && P < (int64_t)INT32_MAX,
                std::string(who) + ": (cell, " + what + ") pair count exceeds 32-bit indexing");
    w.k0.ensure((size_t)P); w.k1.ensure((size_t)P); w.v0.ensure((size_t)P);
    cand.ensure((size_t)P);
    hipLaunchKernelGGL((emit_pairs<D>), dim3(grid_1d(n)), dim3(BLOCK), 0, st, n, g, box, w.off.p, w.k0.p, w.v0.p);
    MGB_HIP_CHECK(hipGetLastError());
    sort_pairs(w.k0.p, w.k1.p, w.v0.p, cand.p, P, key_bits((uint64_t)g.ncell), w.tmp, st);
    start.ensure((size_t)g.ncell + 1);
    hipLaunchKernelGGL(segment_starts<uint32_t>, dim3(grid_1d(P + 1)), dim3(BLOCK), 0, st, P, g.ncell, w.k1.p, start.p);
    MGB_HIP_CHECK(hipGetLastError());
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    return P;
}

// the same with the work buffers of this call alone, freed on return
template <int D>
int64_t cell_lists_from_boxes(const char* who, const char* what, int64_t n, const double* box, const CellPolicy& policy,
                              Grid& g, DevBuf<int32_t>& start, DevBuf<int32_t>& cand, hipStream_t st) {
    GridWork w;
    return cell_lists_from_boxes<D>(who, what, n, box, policy, g, start, cand, w, st);
}

}  // namespace

}  // namespace mgbhip
