// Rays sampled through a mesh: mgbhip_raycast_* (include/mgbhip.h).
//
// reference: the volume rendering of `plot` for fem3d solutions, ext/MultiGridBarrierPyPlotExt/plot3d.jl:69-84 (PyVista's
// add_volume on the CPU).  Here every ray is clipped against the mesh's box and cut into equal steps, the midpoints of
// the steps are located once by the point locator of interpolate.hip (locator_build_device), and a field is then
// evaluated at them by the locator's eval_* kernels with the values left on the device, where one lane per ray sums
// or composites them in sample order.  The samples are laid out by a count pass, an exclusive scan over the rays and an
// emit pass (the pattern of contour.hip): no atomics, the place of every sample is a function of the input alone.
//
// Every index is bounded by R or S before it is used; the loops over a ray's samples run over [off[r], off[r + 1]).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "raycast.hpp"
#include "render_device.hpp"

// No fused multiply-adds in this file: a plain IEEE transcription of the algorithm (tests/raycast_twin.py) then places
// every sample at the same bits.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

constexpr double MAX_COUNT = 2147483648.0;     // a ray's count saturates at 2^31: the total then fails the S check

struct Box {
    double lo[3], hi[3];
};

// one lane per ray: the slab test against the clip box, then the number of steps and their length
template <int D>
__global__ void __launch_bounds__(BLOCK) ray_count(int64_t R, const double* __restrict__ o, const double* __restrict__ dn,
                                                   Box b, double step, double t_min, double t_max,
                                                   double* __restrict__ tmin_out, double* __restrict__ h_out,
                                                   int64_t* __restrict__ count) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double tmin = t_min, tmax = t_max;
    bool miss = false;
    for (int a = 0; a < D; ++a) {
        const double oa = o[r * D + a], da = dn[r * D + a];
        if (da != 0.0) {
            const double t1 = (b.lo[a] - oa) / da, t2 = (b.hi[a] - oa) / da;
            tmin = fmax(tmin, fmin(t1, t2));
            tmax = fmin(tmax, fmax(t1, t2));
        } else if (!(b.lo[a] <= oa && oa <= b.hi[a])) {
            miss = true;
        }
    }
    if (miss || !(tmax > tmin)) {
        tmin_out[r] = 0.0;
        h_out[r] = 0.0;
        count[r] = 0;
        return;
    }
    const double len = tmax - tmin;
    const double c = floor(len / step + 0.5);
    const int64_t n = c >= MAX_COUNT ? (int64_t)MAX_COUNT : (c >= 1.0 ? (int64_t)c : 1);
    tmin_out[r] = tmin;
    h_out[r] = len / (double)n;
    count[r] = n;
}

// one lane per sample: its ray is the last one whose first sample is not after it (rays without samples are skipped by
// the search), its position the midpoint of its step
template <int D>
__global__ void __launch_bounds__(BLOCK) ray_emit(int64_t S, int64_t R, const int64_t* __restrict__ off,
                                                  const double* __restrict__ o, const double* __restrict__ dn,
                                                  const double* __restrict__ tmin, const double* __restrict__ h,
                                                  double* __restrict__ pts) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    int64_t lo = 0, hi = R;                    // the first r in [0, R] with off[r] > s; off[R] = S > s
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= s) lo = mid + 1; else hi = mid;
    }
    const int64_t r = lo - 1;                  // off[0] = 0 <= s, so r >= 0
    const int64_t i = s - off[r];
    const double t = tmin[r] + ((double)i + 0.5) * h[r];
    for (int a = 0; a < D; ++a) pts[s * D + a] = o[r * D + a] + t * dn[r * D + a];
}

// the locator keeps the elements in its cell order: hit[sample] = 1 where the sample lies in an element
__global__ void __launch_bounds__(BLOCK) sample_hits(int64_t S, const int32_t* __restrict__ order,
                                                     const int32_t* __restrict__ elem, uint8_t* __restrict__ hit) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    hit[order[i]] = elem[i] >= 0 ? 1 : 0;
}

__global__ void __launch_bounds__(BLOCK) ray_length(int64_t R, const int64_t* __restrict__ off, const double* __restrict__ h,
                                                    const uint8_t* __restrict__ hit, double* __restrict__ length) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int64_t n = 0;
    const int64_t s1 = off[r + 1];
    for (int64_t s = off[r]; s < s1; ++s) n += hit[s];
    length[r] = h[r] * (double)n;
}

// one lane per (ray, component): the midpoint rule over the samples with a finite value, in sample order
__global__ void __launch_bounds__(BLOCK) ray_integrate(int64_t R, int32_t ncomp, const int64_t* __restrict__ off,
                                                       const double* __restrict__ h, const double* __restrict__ val,
                                                       double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * ncomp) return;
    const int64_t r = idx / ncomp;
    const int32_t c = (int32_t)(idx - r * ncomp);
    double acc = 0.0;
    const int64_t s1 = off[r + 1];
    for (int64_t s = off[r]; s < s1; ++s) {
        const double v = val[s * ncomp + c];
        if (isfinite(v)) acc += v;
    }
    out[idx] = h[r] * acc;
}

// one lane per ray: front-to-back emission-absorption compositing through a K x 4 table of (r, g, b, sigma) rows.  The
// lane reads 8 bytes per sample; the two table rows of a sample come from the cache (K = 256: 8 KiB).
__global__ void __launch_bounds__(BLOCK) ray_composite(int64_t R, int32_t K, const int64_t* __restrict__ off,
                                                       const double* __restrict__ h, const double* __restrict__ val,
                                                       const double* __restrict__ table, double lo, double hi,
                                                       double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const double hr = h[r], width = hi - lo, km1 = (double)(K - 1);
    Composite acc;
    const int64_t s1 = off[r + 1];
    for (int64_t s = off[r]; s < s1; ++s) {
        const double v = val[s];
        if (!isfinite(v)) continue;
        double c[4];
        table_row(v, lo, width, km1, K, table, c);
        acc.sample(c, hr);
    }
    acc.store(out + r * 4);
}

// ray_composite with up to KH opaque or translucent layers per ray merged into the samples by depth: hit k (t_hit
// ascending along the ray, +inf for a missing entry) is applied before sample i iff t_hit <= t_i, with t_i formed as
// ray_emit forms it; the hits behind the last sample are applied after it.  ray_composite itself is left as it is: a
// call without layers runs it unchanged.
__global__ void __launch_bounds__(BLOCK) ray_composite_layers(int64_t R, int32_t K, const int64_t* __restrict__ off,
                                                              const double* __restrict__ tmin, const double* __restrict__ h,
                                                              const double* __restrict__ val,
                                                              const double* __restrict__ table, double lo, double hi,
                                                              int32_t KH, const double* __restrict__ t_hit,
                                                              const double* __restrict__ layer, double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const double hr = h[r], t0r = tmin[r], width = hi - lo, km1 = (double)(K - 1);
    const double* th = t_hit + r * KH;
    const double* ly = layer + r * KH * 4;
    Composite acc;
    int32_t k = 0;
    const int64_t s0 = off[r], s1 = off[r + 1];
    for (int64_t s = s0; s < s1; ++s) {
        const double ti = t0r + ((double)(s - s0) + 0.5) * hr;
        for (; k < KH && th[k] <= ti; ++k) acc.layer(ly + k * 4);
        const double v = val[s];
        if (!isfinite(v)) continue;
        double c[4];
        table_row(v, lo, width, km1, K, table, c);
        acc.sample(c, hr);
    }
    for (; k < KH && th[k] < INFINITY; ++k) acc.layer(ly + k * 4);
    acc.store(out + r * 4);
}

template <int D>
void emit(const RayCaster& RC, double* d_pts, hipStream_t st) {
    hipLaunchKernelGGL((ray_emit<D>), dim3(grid_1d(RC.S)), dim3(BLOCK), 0, st, RC.S, RC.R, RC.off.p, RC.origin.p, RC.dir.p,
                       RC.tmin.p, RC.h.p, d_pts);
    MGB_HIP_CHECK(hipGetLastError());
}

}  // namespace

void raycast_build(RayCaster& RC, const RayIn& in, hipStream_t st) {
    const int32_t d = in.geo.d;
    const int64_t R = in.R;
    RC.d = d;
    RC.R = R;
    RC.S = 0;
    if (R == 0) return;
    RC.origin.upload(in.origin, (size_t)R * d, st);
    RC.dir.upload(in.dir, (size_t)R * d, st);
    RC.tmin.alloc((size_t)R);
    RC.h.alloc((size_t)R);
    RC.length.alloc((size_t)R);
    RC.off.alloc((size_t)R + 1);
    DevBuf<int64_t> count;
    count.alloc((size_t)R + 1);
    count.zero(st);                            // count[R] = 0: the scan then leaves the total in off[R]
    Box b{};
    for (int a = 0; a < d; ++a) { b.lo[a] = in.box[a]; b.hi[a] = in.box[d + a]; }
    if (d == 2)
        hipLaunchKernelGGL((ray_count<2>), dim3(grid_1d(R)), dim3(BLOCK), 0, st, R, RC.origin.p, RC.dir.p, b, in.step,
                           in.t_min, in.t_max, RC.tmin.p, RC.h.p, count.p);
    else
        hipLaunchKernelGGL((ray_count<3>), dim3(grid_1d(R)), dim3(BLOCK), 0, st, R, RC.origin.p, RC.dir.p, b, in.step,
                           in.t_min, in.t_max, RC.tmin.p, RC.h.p, count.p);
    MGB_HIP_CHECK(hipGetLastError());
    DevBuf<char> tmp;
    exclusive_scan(count.p, RC.off.p, R + 1, tmp, st);
    int64_t S = 0;
    MGB_HIP_CHECK(hipMemcpyAsync(&S, RC.off.p + R, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    if (S > (int64_t)INT32_MAX)
        throw InvalidArgument("raycast: S = " + std::to_string(S) + " samples exceed 2^31 - 1: use a larger step or fewer rays");
    RC.S = S;
    if (S == 0) {
        RC.length.zero(st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        return;
    }
    {
        DevBuf<double> pts;                    // freed at the end of this block: the evaluation reads only (element, xi)
        pts.alloc((size_t)S * d);
        if (d == 2) emit<2>(RC, pts.p, st); else emit<3>(RC, pts.p, st);
        InterpIn geo = in.geo;
        geo.M = S;
        locator_build_device(RC.loc, geo, pts.p, st);
    }
    DevBuf<uint8_t> hit;
    hit.alloc((size_t)S);
    hipLaunchKernelGGL(sample_hits, dim3(grid_1d(S)), dim3(BLOCK), 0, st, S, RC.loc.order.p, RC.loc.elem.p, hit.p);
    hipLaunchKernelGGL(ray_length, dim3(grid_1d(R)), dim3(BLOCK), 0, st, R, RC.off.p, RC.h.p, hit.p, RC.length.p);
    MGB_HIP_CHECK(hipGetLastError());
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void raycast_offsets(const RayCaster& RC, int64_t* offsets, hipStream_t st) {
    if (RC.R == 0) { offsets[0] = 0; return; }
    RC.off.download(offsets, (size_t)RC.R + 1, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void raycast_lengths(const RayCaster& RC, double* step, double* length, hipStream_t st) {
    if (RC.R == 0) return;
    if (step) RC.h.download(step, (size_t)RC.R, st);
    if (length) RC.length.download(length, (size_t)RC.R, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void raycast_samples(const RayCaster& RC, double* pts, hipStream_t st) {
    if (RC.S == 0) return;
    DevBuf<double> d_pts;
    d_pts.alloc((size_t)RC.S * RC.d);
    if (RC.d == 2) emit<2>(RC, d_pts.p, st); else emit<3>(RC, d_pts.p, st);
    d_pts.download(pts, (size_t)RC.S * RC.d, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void raycast_integrate(RayCaster& RC, int32_t ncomp, const double* z, double* out, hipStream_t st) {
    if (RC.R == 0) return;
    const int64_t n = RC.R * ncomp;
    RC.result.ensure((size_t)n);
    if (RC.S) locator_evaluate_device(RC.loc, ncomp, z, false, st);
    // without samples off is all zeros and no value is read
    hipLaunchKernelGGL(ray_integrate, dim3(grid_1d(n)), dim3(BLOCK), 0, st, RC.R, ncomp, RC.off.p, RC.h.p, RC.loc.out.p,
                       RC.result.p);
    MGB_HIP_CHECK(hipGetLastError());
    RC.result.download(out, (size_t)n, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void raycast_render_device(RayCaster& RC, const double* d_u, int32_t K, const double* d_transfer, double lo, double hi,
                           hipStream_t st) {
    RC.result.ensure((size_t)RC.R * 4);
    if (RC.S) locator_evaluate_resident(RC.loc, 1, d_u, false, st);
    hipLaunchKernelGGL(ray_composite, dim3(grid_1d(RC.R)), dim3(BLOCK), 0, st, RC.R, K, RC.off.p, RC.h.p, RC.loc.out.p,
                       d_transfer, lo, hi, RC.result.p);
    MGB_HIP_CHECK(hipGetLastError());
}

void raycast_render(RayCaster& RC, const double* u, int32_t K, const double* transfer, double lo, double hi, double* out,
                    hipStream_t st) {
    if (RC.R == 0) return;
    RC.transfer.upload(transfer, (size_t)K * 4, st);
    if (RC.S) RC.loc.z.upload(u, (size_t)RC.loc.p * RC.loc.N, st);     // without samples no value is read
    raycast_render_device(RC, RC.loc.z.p, K, RC.transfer.p, lo, hi, st);
    RC.result.download(out, (size_t)RC.R * 4, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void raycast_render_layers_device(RayCaster& RC, const double* d_u, int32_t K, const double* d_transfer, double lo, double hi,
                                  int32_t KH, const double* d_t_hit, const double* d_layer, hipStream_t st) {
    RC.result.ensure((size_t)RC.R * 4);
    if (RC.S) locator_evaluate_resident(RC.loc, 1, d_u, false, st);
    hipLaunchKernelGGL(ray_composite_layers, dim3(grid_1d(RC.R)), dim3(BLOCK), 0, st, RC.R, K, RC.off.p, RC.tmin.p, RC.h.p,
                       RC.loc.out.p, d_transfer, lo, hi, KH, d_t_hit, d_layer, RC.result.p);
    MGB_HIP_CHECK(hipGetLastError());
}

void raycast_render_layers(RayCaster& RC, const double* u, int32_t K, const double* transfer, double lo, double hi,
                           int32_t KH, const double* t_hit, const double* layer, double* out, hipStream_t st) {
    if (RC.R == 0) return;
    RC.transfer.upload(transfer, (size_t)K * 4, st);
    RC.t_hit.upload(t_hit, (size_t)RC.R * KH, st);
    RC.layer.upload(layer, (size_t)RC.R * KH * 4, st);
    if (RC.S) RC.loc.z.upload(u, (size_t)RC.loc.p * RC.loc.N, st);     // without samples no value is read
    raycast_render_layers_device(RC, RC.loc.z.p, K, RC.transfer.p, lo, hi, KH, RC.t_hit.p, RC.layer.p, st);
    RC.result.download(out, (size_t)RC.R * 4, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
