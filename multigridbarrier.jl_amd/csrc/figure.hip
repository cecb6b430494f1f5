// The default figure of a fem3d solution, frame after frame: mgbhip_figure_* (include/mgbhip.h).
//
// reference: `plot(M, ts, U)` and `plot(sol::ParabolicSOL, k)` animate a fem3d solution by drawing the figure of
// plot3d.jl:85-149 once per frame with colour limits and isosurface levels fixed over the whole trajectory
// (ext/MultiGridBarrierPyPlotExt/plot3d.jl:310-381).  Every part of that figure has its own translation unit here
// (contour.hip, surface.hip, raycast.hip); a host that chains their host-pointer entries moves the soup, the rays, the
// hits and the layers through pageable memory for every frame and locates the volume's samples again.  A Figure chains
// the device-pointer entries of the same stages instead: the kernels, their launch shapes and their inputs are those of
// the host chain, so a frame is the host chain's frame bit for bit, and the only transfers of a frame are u going in
// and the image coming out (plus the scalar read-backs the stages make themselves: simplex totals, grid sizing).
//
// The kernels of this file are the glue the host chain does in NumPy: the carried column of a slice's field
// (carry_column), the vertex values of the soup (soup_values), the compositing of the layers when there is no volume
// (layers_composite), and the conversion of an image to bytes (image_rgba8).  One lane per output item, every index
// below its bound, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "figure.hpp"
#include "render_device.hpp"

// No fused multiply-adds in this file: layers_composite and image_rgba8 then do the operations of their NumPy
// restatements (surface.composite_layers, tests/figure_twin.py) bit for bit.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

// one lane per mesh node: u into column 1 of a slice's two-column field (column 0, the coordinate function, is resident)
__global__ void __launch_bounds__(BLOCK) carry_column(int64_t rows, const double* __restrict__ u,
                                                      double* __restrict__ fields) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    fields[i * 2 + 1] = u[i];
}

// one lane per triangle vertex i of one part of the soup (n = 3 x its triangles): an isosurface triangle takes its
// level's value at all three vertices (level != NULL), a slice triangle the first carried field of its vertex
__global__ void __launch_bounds__(BLOCK) soup_values(int64_t n, const int32_t* __restrict__ level,
                                                     const double* __restrict__ levels,
                                                     const double* __restrict__ carried, int32_t ncarry,
                                                     double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = level ? levels[level[i / 3]] : carried[i * ncarry];
}

// one lane per ray: the K layers of the ray front to back from T = 1, C = 0 (surface.composite_layers)
__global__ void __launch_bounds__(BLOCK) layers_composite(int64_t R, int32_t K, const double* __restrict__ layer,
                                                          double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const double* ly = layer + r * K * 4;
    Composite acc;
    for (int32_t k = 0; k < K; ++k) acc.layer(ly + k * 4);
    acc.store(out + r * 4);
}

// floor(255 min(1, max(0, c)) + 0.5) as a byte; 0 for a c that is not finite
__device__ inline uint8_t to_byte(double c) {
    if (!isfinite(c)) return 0;
    const double s = fmin(1.0, fmax(0.0, c));
    return (uint8_t)floor(255.0 * s + 0.5);
}

// one lane per ray: premultiplied colour and alpha over the background (b0, b1, b2), four bytes
__global__ void __launch_bounds__(BLOCK) image_rgba8(int64_t R, const double* __restrict__ img, double b0, double b1,
                                                     double b2, uint8_t* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const double a = img[r * 4 + 3];
    const double rest = 1.0 - a;
    uchar4 q;
    q.x = to_byte(img[r * 4] + rest * b0);
    q.y = to_byte(img[r * 4 + 1] + rest * b1);
    q.z = to_byte(img[r * 4 + 2] + rest * b2);
    q.w = to_byte(a);
    reinterpret_cast<uchar4*>(out)[r] = q;
}

// the sizes of a contour call of this figure: nfield columns, nlevels levels, the default lattice (refine = k)
ContourIn contour_sizes(const Figure& F, int32_t nfield, int32_t nlevels) {
    const InterpIn& g = F.in.rays.geo;
    ContourIn c;
    c.family = g.family; c.d = 3; c.e = 3; c.k = g.k; c.p = g.p; c.N = g.N;
    c.nfield = nfield; c.nlevels = nlevels; c.refine = g.k;
    return c;
}

// One frame up to the image on the device; returns where it is (R x 4).  Queued on st; the stages wait where they read
// a total back.
const double* frame(Figure& F, const double* u, hipStream_t st) {
    const int32_t K = F.in.K, ns = F.in.nslices;
    const int64_t R = F.R;
    F.u.upload(u, (size_t)F.rows, st);

    // ---- the cuts: the isosurfaces of u, then every slice as the level set of its coordinate with u carried
    contour_build_device(F.iso, contour_sizes(F, 1, F.in.nlevels), F.x.p, F.ctable.p, F.table_len, F.u.p, F.levels.p,
                         F.cwork, st);
    int64_t T = F.iso.S;
    for (int32_t i = 0; i < ns; ++i) {
        double* f = F.slice_fields[i].p;               // column 0 is resident; column 1 takes this frame's u
        hipLaunchKernelGGL(carry_column, dim3(grid_1d(F.rows)), dim3(BLOCK), 0, st, F.rows, F.u.p, f);
        MGB_HIP_CHECK(hipGetLastError());
        contour_build_device(F.cuts[i], contour_sizes(F, 2, 1), F.x.p, F.ctable.p, F.table_len, f, F.coords.p + i,
                             F.cwork, st);
        T += F.cuts[i].S;
    }
    MGB_REQUIRE(T < (int64_t)INT32_MAX / 9, "figure: the soup of a frame exceeds 32-bit indexing");

    // ---- the soup in render_figure's order: points by device-to-device copies, values by soup_values
    F.sf.pts.ensure((size_t)T * 9);
    F.values.ensure((size_t)T * 3);
    int64_t at = 0;
    auto place = [&](const Contour& c, bool iso) {
        if (c.S == 0) return;
        MGB_HIP_CHECK(hipMemcpyAsync(F.sf.pts.p + at * 9, c.points.p, (size_t)c.S * 9 * sizeof(double),
                                     hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(soup_values, dim3(grid_1d(c.S * 3)), dim3(BLOCK), 0, st, c.S * 3, iso ? c.level.p : nullptr,
                           F.levels.p, c.carried.p, c.ncarry, F.values.p + at * 3);
        MGB_HIP_CHECK(hipGetLastError());
        at += c.S;
    };
    place(F.iso, true);
    for (int32_t i = 0; i < ns; ++i) place(F.cuts[i], false);

    // ---- grid, trace, shade
    surface_build_device(F.sf, T, F.sf.pts.p, F.gwork, st);
    F.T = T;
    F.P = F.sf.P;
    const size_t n = (size_t)R * K;
    F.sf.layer.ensure(n * 4);
    const double* t_hit = F.miss_t.p;
    if (T) {
        surface_trace_device(F.sf, R, F.o.p, F.dn.p, 0.0, std::numeric_limits<double>::infinity(), K, st);
        surface_shade_device(F.sf, R, K, F.dn.p, F.sf.id.p, F.sf.par[0].p, F.sf.par[1].p, F.values.p, F.in.ntable, F.stable.p,
                             F.in.lo, F.in.hi, F.in.ambient, F.sf.layer.p, st);
        t_hit = F.sf.t.p;
    } else {
        F.sf.layer.zero(st, n * 4);                    // an empty soup: every ray misses, every layer is zero
    }

    // ---- the image
    if (F.in.volume) {
        raycast_render_layers_device(F.rc, F.u.p, F.in.ntable, F.vtable.p, F.in.lo, F.in.hi, K, t_hit, F.sf.layer.p, st);
        return F.rc.result.p;
    }
    F.image.ensure((size_t)R * 4);
    hipLaunchKernelGGL(layers_composite, dim3(grid_1d(R)), dim3(BLOCK), 0, st, R, K, F.sf.layer.p, F.image.p);
    MGB_HIP_CHECK(hipGetLastError());
    return F.image.p;
}

}  // namespace

void figure_build(Figure& F, const FigureIn& in, hipStream_t st) {
    F.in = in;
    const InterpIn& g = in.rays.geo;
    const int64_t rows = (int64_t)g.p * g.N, R = in.rays.R;
    F.rows = rows;
    F.R = R;
    F.x.upload(g.x, (size_t)rows * 3, st);
    ContourIn c = contour_sizes(F, 1, 1);
    c.table = g.table;
    const std::vector<double> ctable = contour_lattice_table(c);
    F.table_len = (int32_t)ctable.size();
    F.ctable.upload(ctable, st);
    if (in.nlevels) F.levels.upload(in.levels, (size_t)in.nlevels, st);
    if (in.nslices) F.coords.upload(in.coords, (size_t)in.nslices, st);
    F.slice_fields.resize((size_t)in.nslices);
    F.cuts.resize((size_t)in.nslices);
    std::vector<double> f((size_t)(in.nslices ? rows * 2 : 0), 0.0);
    for (int32_t i = 0; i < in.nslices; ++i) {
        for (int64_t j = 0; j < rows; ++j) f[(size_t)j * 2] = g.x[j * 3 + in.axes[i]];
        F.slice_fields[i].upload(f, st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));       // f is written again for the next slice
    }
    F.o.upload(in.rays.origin, (size_t)R * 3, st);
    F.dn.upload(in.rays.dir, (size_t)R * 3, st);
    F.vtable.upload(in.vtable, (size_t)in.ntable * 4, st);
    F.stable.upload(in.stable, (size_t)in.ntable * 4, st);
    const std::vector<double> miss((size_t)R * in.K, std::numeric_limits<double>::infinity());
    F.miss_t.upload(miss, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    if (in.volume) raycast_build(F.rc, in.rays, st);
    // the host pointers of the caller are not read again
    F.in.rays.geo.x = F.in.rays.geo.table = nullptr;
    F.in.rays.origin = F.in.rays.dir = F.in.rays.box = nullptr;
    F.in.levels = F.in.coords = F.in.vtable = F.in.stable = nullptr;
    F.in.axes = nullptr;
}

void figure_render(Figure& F, const double* u, double* out, hipStream_t st) {
    const double* img = frame(F, u, st);
    MGB_HIP_CHECK(hipMemcpyAsync(out, img, (size_t)F.R * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void figure_render_rgba8(Figure& F, const double* u, const double* bg, uint8_t* out, hipStream_t st) {
    const double* img = frame(F, u, st);
    F.bytes.ensure((size_t)F.R * 4);
    hipLaunchKernelGGL(image_rgba8, dim3(grid_1d(F.R)), dim3(BLOCK), 0, st, F.R, img, bg[0], bg[1], bg[2], F.bytes.p);
    MGB_HIP_CHECK(hipGetLastError());
    F.bytes.download(out, (size_t)F.R * 4, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
