// soup_trace.hpp -- rays against a soup of primitives in the grid of cell_lists.hpp, whatever the primitive: the one trace
// kernel, its one dispatch over the hit count, and the host paths around the trace and shade kernels.  surface.hip
// (triangles) and tubes.hip (capsules) include it and bring the primitive: a small struct passed to the kernel by value
// that holds its device pointers, declares NPAR, the number of parameters that place a hit on the primitive (u, v: 2;
// s: 1), and has
//     bool test(o, dn, id, t_min, t_max, double& t, double (&par)[NPAR]) const
// for the ray o + t dn against primitive id.  What a ray hits is a function of the ray and the primitive alone; the grid
// only decides what is tested.
//
// Every index is bounded before it is used: a cell index is clamped to the grid, a candidate is < n by construction, the
// walk takes at most n[0] + n[1] + n[2] steps, and the hit list of a ray has the compile-time length K.
#pragma once
#include <algorithm>
#include <limits>
#include <string>

#include "cell_lists.hpp"
#include "render_device.hpp"
#include "surface.hpp"

// No fused multiply-adds in the code below or in a file that includes it: see surface.hip.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

constexpr int32_t NO_PRIMITIVE = 2147483647;           // in a lane's list; written out as -1

// where a trace leaves its hits (R x K each)
template <int NPAR>
struct SoupHits {
    double* t;
    int32_t* id;
    double* par[NPAR];
};

// One lane per ray.  The lane keeps (t, primitive) of its K nearest hits in ascending order, indexed only by unrolled
// loops so that the list stays in registers; the parameters are recomputed for the kept primitives at the end by the
// same operations.  The lane walks the cells with a 3-D DDA and tests every primitive of a cell's list.  A hit at t lies
// in the cell the ray is in at t, and the primitive's box covers it, so every hit before a cell's exit has been met by
// the time the cell is done.
template <class Prim, int K>
__global__ void __launch_bounds__(BLOCK) soup_trace_k(int64_t R, const double* __restrict__ org,
                                                      const double* __restrict__ dir, double t_min, double t_max,
                                                      Grid g, const int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ cand, Prim prim,
                                                      SoupHits<Prim::NPAR> out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double o[3], dn[3];
    for (int a = 0; a < 3; ++a) { o[a] = org[r * 3 + a]; dn[a] = dir[r * 3 + a]; }
    double kt[K];
    int32_t ki[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { kt[j] = INFINITY; ki[j] = NO_PRIMITIVE; }

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
                // Met in an earlier cell and kept: skipped before it is tested.  Testing first inserts the same (t, id)
                // pairs, since the same primitive gives the same t and is then found in the list; the order only saves
                // the test.
                bool seen = false;
#pragma unroll
                for (int k = 0; k < K; ++k) seen = seen || ki[k] == ic;
                if (seen) continue;
                double tc, pc[Prim::NPAR];
                if (!prim.test(o, dn, ic, t_min, t_max, tc, pc)) continue;
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
        double t = INFINITY, par[Prim::NPAR];
        for (int a = 0; a < Prim::NPAR; ++a) par[a] = dnan();
        int32_t id = -1;
        if (ki[k] != NO_PRIMITIVE) {
            id = ki[k];
            prim.test(o, dn, id, t_min, t_max, t, par);
        }
        out.t[r * K + k] = t;
        out.id[r * K + k] = id;
        for (int a = 0; a < Prim::NPAR; ++a) out.par[a][r * K + k] = par[a];
    }
}

// Rays on the device against a soup with S.n > 0: the hits are left in S.t, S.id and S.par[0..NPAR) (R x K each).
// Queued on st, not waited for.  `who` names the caller in the error message ("surface", "tubes").
template <class Prim>
void soup_trace_device(Soup& S, const char* who, Prim prim, int64_t R, const double* d_o, const double* d_dn, double t_min,
                       double t_max, int32_t K, hipStream_t st) {
    const size_t n = (size_t)R * K;
    SoupHits<Prim::NPAR> out;
    S.t.ensure(n); S.id.ensure(n);
    out.t = S.t.p; out.id = S.id.p;
    for (int a = 0; a < Prim::NPAR; ++a) { S.par[a].ensure(n); out.par[a] = S.par[a].p; }
#define MGB_SOUP_TRACE(k)                                                                                           \
    case k:                                                                                                         \
        hipLaunchKernelGGL((soup_trace_k<Prim, k>), dim3(grid_1d(R)), dim3(BLOCK), 0, st, R, d_o, d_dn, t_min, t_max, S.g, \
                           S.start.p, S.cand.p, prim, out);                                                         \
        break;
    switch (K) {
        MGB_SOUP_TRACE(1) MGB_SOUP_TRACE(2) MGB_SOUP_TRACE(3) MGB_SOUP_TRACE(4)
        MGB_SOUP_TRACE(5) MGB_SOUP_TRACE(6) MGB_SOUP_TRACE(7) MGB_SOUP_TRACE(8)
        default: throw InvalidArgument(std::string(who) + ": K must be 1..8");
    }
#undef MGB_SOUP_TRACE
    MGB_HIP_CHECK(hipGetLastError());
}

// The same for host arrays: o, dn R x 3; t, id and par[0..NPAR) R x K.  Complete on return.
template <class Prim>
void soup_trace(Soup& S, const char* who, Prim prim, int64_t R, const double* o, const double* dn, double t_min,
                double t_max, int32_t K, double* t, int32_t* id, double* const (&par)[Prim::NPAR], hipStream_t st) {
    if (R == 0) return;
    const size_t n = (size_t)R * K;
    if (S.n == 0) {                            // an empty soup: every ray misses
        std::fill(t, t + n, std::numeric_limits<double>::infinity());
        std::fill(id, id + n, -1);
        for (double* p : par) std::fill(p, p + n, std::numeric_limits<double>::quiet_NaN());
        return;
    }
    S.o.upload(o, (size_t)R * 3, st);
    S.dn.upload(dn, (size_t)R * 3, st);
    soup_trace_device(S, who, prim, R, S.o.p, S.dn.p, t_min, t_max, K, st);
    S.t.download(t, n, st);
    S.id.download(id, n, st);
    for (int a = 0; a < Prim::NPAR; ++a) S.par[a].download(par[a], n, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

// The host path around a shade kernel: the hits as trace returned them (o and t may be null where the kernel does not
// read them), values host S.n x nval, table host Kt x 4, layer host R x K x 4.  `launch` queues the kernel on the
// uploaded buffers of S and leaves the layers in S.layer.  Complete on return.
template <int NPAR, class Launch>
void soup_shade(Soup& S, int64_t R, int32_t K, const double* o, const double* dn, const double* t, const int32_t* id,
                const double* const (&par)[NPAR], const double* values, int nval, int32_t Kt, const double* table,
                double* layer, hipStream_t st, Launch launch) {
    if (R == 0) return;
    const size_t n = (size_t)R * K;
    if (S.n == 0) {                            // the caller has checked that every id is -1
        std::fill(layer, layer + n * 4, 0.0);
        return;
    }
    if (o) S.o.upload(o, (size_t)R * 3, st);
    S.dn.upload(dn, (size_t)R * 3, st);
    if (t) S.t.upload(t, n, st);
    S.id.upload(id, n, st);
    for (int a = 0; a < NPAR; ++a) S.par[a].upload(par[a], n, st);
    S.values.upload(values, (size_t)S.n * nval, st);
    S.table.upload(table, (size_t)Kt * 4, st);
    S.layer.ensure(n * 4);
    launch();
    MGB_HIP_CHECK(hipGetLastError());
    S.layer.download(layer, n * 4, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace

}  // namespace mgbhip
