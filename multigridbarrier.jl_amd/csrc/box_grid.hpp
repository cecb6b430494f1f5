// box_grid.hpp -- a soup of axis-aligned boxes put into a uniform grid of cells, shared by the translation units that
// trace rays against a soup: surface.hip (the boxes of triangles) and tubes.hip (the boxes of capsules).  Nothing here
// depends on what is inside a box: one block reduces the union of the boxes, the host picks the cell counts, a count
// pass and an exclusive scan size the (cell, box) pair list, an emit pass writes it in box order and a stable radix sort
// by cell leaves every cell's list ascending in box index.  No atomics.  One copy of each kernel: both files include
// this header, and both build the same grid from the same boxes.
//
// Everything here has internal linkage (the library is built without relocatable device code, so every translation unit
// carries its own copy of the kernels it launches).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "render_device.hpp"
#include "surface.hpp"

// No fused multiply-adds in the code below or in a file that includes it: see surface.hip.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

// Every box is widened by PAD_REL * (largest extent of the union + largest |coordinate|) per side before it is cut
// into cells.  The walk places a ray in a cell with an error of a few eps * (|origin| + |coordinate|) per axis, and a
// computed hit point leaves the box of what it hit by as little; 2^-26 covers both for origins up to 2^20 box sizes
// away, and is far below any cell side, so it adds no pairs to speak of.
constexpr double PAD_REL = 1.4901161193847656e-08;   // 2^-26

// cell index of a scaled coordinate; NaN and anything below the box go to cell 0, anything above to the last cell
__device__ inline int32_t cell_axis(double s, int32_t n) {
    if (!(s >= 0.0)) return 0;
    if (s >= (double)n) return n - 1;
    const int32_t c = (int32_t)s;
    return c < n - 1 ? c : n - 1;
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

// the cells a padded box overlaps
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

// cells of side h with h^(#axes of positive extent) = volume / (cells_per_box * T), at most 1024 per axis
inline SurfaceGrid pick_grid(const double* hb, int64_t T, double cells_per_box) {
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

// The grid over T > 0 boxes on the device (box: T x 6, lo then hi): union, cell counts, count pass, scan, emit pass,
// stable sort by cell, cell starts.  Returns the pair count P; g, start (ncell + 1) and cand (P) are complete on return.
// start, cand and the buffers of w grow and are kept: only the first ncell + 1 and P entries are meant.
// `who` and `what` name the caller and its primitive in the error messages ("surface", "triangle").
inline int64_t grid_from_boxes(const char* who, const char* what, int64_t T, const double* box, SurfaceGrid& g,
                               DevBuf<int32_t>& start, DevBuf<int32_t>& cand, GridWork& w, hipStream_t st) {
    w.ubox.ensure(6);
    hipLaunchKernelGGL(union_box, dim3(1), dim3(1024), 0, st, T, box, w.ubox.p);
    MGB_HIP_CHECK(hipGetLastError());
    double hb[6];
    w.ubox.download(hb, 6, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    for (int a = 0; a < 6; ++a)
        MGB_REQUIRE(std::isfinite(hb[a]), std::string(who) + ": non-finite " + what + " box");
    w.count.ensure((size_t)T);
    w.off.ensure((size_t)T);
    // About four cells per box.  Boxes that span many cells (a slice next to a fine isosurface) can make the pair list
    // far longer than the soup: the grid is then coarsened until the list is at most 16 T + 4096 pairs.
    double cells_per_box = 4.0;
    int64_t P = 0;
    for (;;) {
        g = pick_grid(hb, T, cells_per_box);
        hipLaunchKernelGGL(box_counts, dim3(grid_1d(T)), dim3(BLOCK), 0, st, T, g, box, w.count.p);
        MGB_HIP_CHECK(hipGetLastError());
        size_t scan_bytes = 0;
        MGB_HIP_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, w.count.p, w.off.p, (int64_t)0, (size_t)T,
                                              rocprim::plus<int64_t>(), st));
        w.tmp.ensure(scan_bytes + 16);
        MGB_HIP_CHECK(rocprim::exclusive_scan((void*)w.tmp.p, scan_bytes, w.count.p, w.off.p, (int64_t)0, (size_t)T,
                                              rocprim::plus<int64_t>(), st));
        int64_t last_off = 0, last_count = 0;
        MGB_HIP_CHECK(hipMemcpyAsync(&last_off, w.off.p + (T - 1), sizeof(int64_t), hipMemcpyDeviceToHost, st));
        MGB_HIP_CHECK(hipMemcpyAsync(&last_count, w.count.p + (T - 1), sizeof(int64_t), hipMemcpyDeviceToHost, st));
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        P = last_off + last_count;
        if (P <= 16 * T + 4096 || g.ncell == 1) break;
        cells_per_box *= 0.125;
    }
    MGB_REQUIRE(P > 0 && P < (int64_t)INT32_MAX,
                std::string(who) + ": (cell, " + what + ") pair count exceeds 32-bit indexing");
    w.k0.ensure((size_t)P); w.k1.ensure((size_t)P); w.v0.ensure((size_t)P);
    cand.ensure((size_t)P);
    hipLaunchKernelGGL(emit_pairs, dim3(grid_1d(T)), dim3(BLOCK), 0, st, T, g, box, w.off.p, w.k0.p, w.v0.p);
    MGB_HIP_CHECK(hipGetLastError());
    unsigned bits = 1;
    while (bits < 32 && ((uint64_t)g.ncell >> bits) != 0) ++bits;
    size_t sort_bytes = 0;
    MGB_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, w.k0.p, w.k1.p, w.v0.p, cand.p, (size_t)P, 0u, bits, st));
    w.tmp.ensure(sort_bytes + 16);
    MGB_HIP_CHECK(rocprim::radix_sort_pairs((void*)w.tmp.p, sort_bytes, w.k0.p, w.k1.p, w.v0.p, cand.p, (size_t)P, 0u, bits,
                                            st));
    start.ensure((size_t)g.ncell + 1);
    hipLaunchKernelGGL(cell_starts, dim3(grid_1d(P + 1)), dim3(BLOCK), 0, st, P, g.ncell, w.k1.p, start.p);
    MGB_HIP_CHECK(hipGetLastError());
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    return P;
}

// the same with the work buffers of this call alone, freed on return
inline int64_t grid_from_boxes(const char* who, const char* what, int64_t T, const DevBuf<double>& box, SurfaceGrid& g,
                               DevBuf<int32_t>& start, DevBuf<int32_t>& cand, hipStream_t st) {
    GridWork w;
    return grid_from_boxes(who, what, T, box.p, g, start, cand, w, st);
}

}  // namespace

}  // namespace mgbhip
