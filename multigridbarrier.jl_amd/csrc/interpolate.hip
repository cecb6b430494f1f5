// Point evaluation of broken-basis vectors and of their gradients: mgbhip_interpolate, mgbhip_interpolate_grad
// (include/mgbhip.h).
//
// reference: `interpolate`, src/utils.jl:16-58 (1-D Q_k: src/TensorFEM.jl:967-1014; spectral1d: src/spectral1d.jl:140-170;
// spectral2d: src/spectral2d.jl:85-125).  The reference has no 2-D / 3-D FEM method; here those locate every point
// through a uniform grid of element bounding boxes built on the device (cell_lists.hpp), the same sort-by-key pattern as
// the assembly plans (plan_device.hip): each cell's candidate list is in ascending element order, so the first element
// that accepts a point is the lowest-index one, whatever the launch configuration.  Each query lane then inverts the element map of its candidates in order.
//
// Every loop is bounded (Newton iterations, bisection halvings, the candidate list of one cell, the 1-D scans), and
// a coordinate becomes a cell index only after it is known to be finite and inside the grid box.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "interp_device.hpp"      // the locate and evaluate device functions and their constants (shared with stream.hip)
#include "interpolate.hpp"

// No fused multiply-adds in this file: the 1-D path reproduces the reference's bisection operation for operation, so
// that a point at a node gives the same bits as a plain IEEE transcription of the reference.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

// ---------------------------------------------------------------------------------------------------------------
// location grid (2-D and 3-D FEM)
// ---------------------------------------------------------------------------------------------------------------

// one thread per element: the bounding box of its p nodes in D coordinates (the element's own dimension plays no part),
// padded by pad * (largest extent) plus the containment tolerance plus `reach` (absolute)
template <int D>
__global__ void elem_boxes(int64_t N, int32_t p, const double* __restrict__ x, double pad, double reach,
                           double* __restrict__ box) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    double lo[D], hi[D];
    for (int a = 0; a < D; ++a) lo[a] = hi[a] = x[(e * p) * D + a];
    for (int32_t i = 1; i < p; ++i)
        for (int a = 0; a < D; ++a) {
            const double v = x[(e * p + i) * D + a];
            lo[a] = fmin(lo[a], v);
            hi[a] = fmax(hi[a], v);
        }
    double ext = 0.0, xs = 0.0;
    for (int a = 0; a < D; ++a) {
        ext = fmax(ext, hi[a] - lo[a]);
        xs = fmax(xs, fmax(fabs(lo[a]), fabs(hi[a])));
    }
    // a point accepted within the containment tolerance lies at most ~ROUND_FACTOR eps max|x| (or ACCEPT_TOL of the
    // extent) outside the element
    const double w = (pad + 4 * ACCEPT_TOL) * ext + 4 * ROUND_FACTOR * EPS * xs + reach;
    for (int a = 0; a < D; ++a) {
        box[e * 2 * D + a] = lo[a] - w;
        box[e * 2 * D + D + a] = hi[a] + w;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// query, locate and evaluate kernels: one lane per point
// ---------------------------------------------------------------------------------------------------------------

// What a locate kernel leaves behind for the evaluate kernels of a point locator, per lane i (the stored cell order of
// the located families, the point index otherwise): the element (-1: none) and the reference coordinates the fused
// query kernel would have evaluated at.
struct LocArgs {
    int32_t* elem;             // M
    double* ref;               // Q_k: M x D (xi); P1 / P2 / P2C: M x 2 (l1, l2); fem1d: M (xi); spectral: unused
    int32_t* flag;             // fem1d: one of FEM1D_GENERAL .. FEM1D_CROSSED; unused otherwise
};

// Every query kernel consists of two device functions, *locate* (point -> element + reference coordinates) and
// *evaluate* (element + reference coordinates + z -> values and, with GRAD, the gradient).  The fused query_* kernels
// call one after the other; the locate_* / eval_* kernels of a point locator call them in separate launches with the
// reference coordinates stored in between, so both paths run the same operations on the same numbers.
//
// Every query / eval kernel has a compile-time GRAD flag: the GRAD = false instantiation is the value-only kernel, the
// GRAD = true one computes the same values by the same operations and also the gradient with respect to x.
template <int D, bool GRAD>
__device__ inline void write_nan(const QueryArgs& a, int64_t q) {
    for (int c = 0; c < a.ncomp; ++c) a.out[q * a.ncomp + c] = dnan();
    if constexpr (GRAD)
        for (int c = 0; c < a.ncomp * D; ++c) a.grad[q * a.ncomp * D + c] = dnan();
    if (a.elem) a.elem[q] = -1;
}

template <int D, int S, bool GRAD>
__global__ void __launch_bounds__(BLOCK) query_qk(QueryArgs a, Grid g) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int64_t q = a.order[i];
    double pt[D];
    for (int d = 0; d < D; ++d) pt[d] = a.pts[q * D + d];
    double nodes[S], L[D][S], xi[D];
    const int64_t found = qk_find<D, S>(a, g, pt, nodes, L, xi);
    if (found < 0 || !qk_evaluate<D, S, GRAD>(a, q, found, nodes, L, xi)) { write_nan<D, GRAD>(a, q); return; }
    if (a.elem) a.elem[q] = (int32_t)found;
}

// the xi stored is the one qk_locate returns, the point its closing lagrange<S> call produced L at
template <int D, int S>
__global__ void __launch_bounds__(BLOCK) locate_qk(QueryArgs a, Grid g, LocArgs l) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int64_t q = a.order[i];
    double pt[D];
    for (int d = 0; d < D; ++d) pt[d] = a.pts[q * D + d];
    double nodes[S], L[D][S], xi[D];
    const int64_t found = qk_find<D, S>(a, g, pt, nodes, L, xi);
    l.elem[i] = (int32_t)found;
    for (int d = 0; d < D; ++d) l.ref[i * D + d] = found < 0 ? 0.0 : xi[d];
}

template <int D, int S, bool GRAD>
__global__ void __launch_bounds__(BLOCK) eval_qk(QueryArgs a, LocArgs l) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int64_t q = a.order[i];
    const int64_t found = l.elem[i];
    if (found < 0) { write_nan<D, GRAD>(a, q); return; }
    double nodes[S];
    for (int j = 0; j < S; ++j) nodes[j] = a.table[j];
    double L[D][S], xi[D];
    for (int d = 0; d < D; ++d) xi[d] = l.ref[i * D + d];
#pragma unroll
    for (int d = 0; d < D; ++d) lagrange<S>(nodes, xi[d], L[d]);
    if (!qk_evaluate<D, S, GRAD>(a, q, found, nodes, L, xi)) write_nan<D, GRAD>(a, q);
}

template <int FAM, bool GRAD>
__global__ void __launch_bounds__(BLOCK) query_simplex(QueryArgs a, Grid g) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int64_t q = a.order[i];
    const double pt[2] = {a.pts[q * 2], a.pts[q * 2 + 1]};
    double l1 = 0.0, l2 = 0.0;
    const int64_t found = simplex_find<FAM>(a, g, pt, l1, l2);
    if (found < 0 || !simplex_evaluate<FAM, GRAD>(a, q, found, l1, l2)) { write_nan<2, GRAD>(a, q); return; }
    if (a.elem) a.elem[q] = (int32_t)found;
}

template <int FAM>
__global__ void __launch_bounds__(BLOCK) locate_simplex(QueryArgs a, Grid g, LocArgs l) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int64_t q = a.order[i];
    const double pt[2] = {a.pts[q * 2], a.pts[q * 2 + 1]};
    double l1 = 0.0, l2 = 0.0;
    const int64_t found = simplex_find<FAM>(a, g, pt, l1, l2);
    l.elem[i] = (int32_t)found;
    l.ref[i * 2] = found < 0 ? 0.0 : l1;
    l.ref[i * 2 + 1] = found < 0 ? 0.0 : l2;
}

template <int FAM, bool GRAD>
__global__ void __launch_bounds__(BLOCK) eval_simplex(QueryArgs a, LocArgs l) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int64_t q = a.order[i];
    const int64_t found = l.elem[i];
    if (found < 0) { write_nan<2, GRAD>(a, q); return; }
    if (!simplex_evaluate<FAM, GRAD>(a, q, found, l.ref[i * 2], l.ref[i * 2 + 1])) write_nan<2, GRAD>(a, q);
}

// d/dx of the Lagrange interpolant of element e at the reference point xi: (sum_j L_j'(xi) z_j) / (sum_j L_j'(xi) x_j)
template <int S>
__device__ inline void fem1d_gradient(const QueryArgs& a, int64_t q, int64_t e, double xi) {
    double nodes[S], L[S], dL[S];
    for (int j = 0; j < S; ++j) nodes[j] = a.table[j];
    lagrange_d<S>(nodes, xi, L, dL);
    double dx = 0.0;
    for (int j = 0; j < S; ++j) dx += dL[j] * a.x[e * S + j];
    for (int c = 0; c < a.ncomp; ++c) {
        double v = 0.0;
        for (int j = 0; j < S; ++j) v += dL[j] * a.z[(e * S + j) * a.ncomp + c];
        a.grad[q * a.ncomp + c] = v / dx;
    }
}

// how a located 1-D point is evaluated (the element is -1 for a NaN point)
constexpr int32_t FEM1D_GENERAL = 0;   // inside element e: the interpolant at the bisection's xi
constexpr int32_t FEM1D_NODE = 1;      // on an end node of element e (xi = -1 or 1): that node's value, one-sided derivative
constexpr int32_t FEM1D_CLAMPED = 2;   // outside the mesh: the value of the end node (xi = -1 or 1 of e), derivative 0
// x[0] > x[end] (elements not in ascending order) and t == x[end]: the first branch of the reference's clamp takes the first
// node's value, and the derivative is the one-sided one of the last element, as for any t == x[end]
constexpr int32_t FEM1D_CROSSED = 3;

// 1-D Q_k locate: the reference's algorithm step for step (src/TensorFEM.jl:967-1014), 0-based.  Returns the element
// (-1 for NaN) and sets xi and the flag.
template <int S>
__device__ inline int64_t fem1d_locate(const double* __restrict__ x, const double (&nodes)[S], int64_t N,
                                       int32_t sorted, double t, double& xi, int32_t& flag) {
    xi = 0.0;
    flag = FEM1D_GENERAL;
    if (isnan(t)) return -1;
    const double x_lo = x[0], x_hi = x[(N - 1) * S + S - 1];
    if (t <= x_lo || t >= x_hi) {
        xi = t <= x_lo ? -1.0 : 1.0;
        flag = t == x_lo ? FEM1D_NODE : (t == x_hi ? (t <= x_lo ? FEM1D_CROSSED : FEM1D_NODE) : FEM1D_CLAMPED);
        return t <= x_lo ? 0 : N - 1;
    }
    int64_t e;
    if (sorted) {       // searchsortedlast over the left endpoints, clamped to [0, N-1]
        int64_t lo = 0, hi = N;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (x[mid * S] <= t) lo = mid + 1; else hi = mid;
        }
        e = lo - 1 < 0 ? 0 : (lo - 1 > N - 1 ? N - 1 : lo - 1);
    } else {
        e = 0;
        while (e < N - 1 && t > x[e * S + S - 1]) ++e;
    }
    double xe[S];
    for (int j = 0; j < S; ++j) xe[j] = x[e * S + j];
    double lo = -1.0, hi = 1.0;
    double flo = xe[0] - t;
    if (flo == 0.0) { xi = -1.0; flag = FEM1D_NODE; return e; }
    const double fhi = xe[S - 1] - t;
    if (fhi == 0.0) { xi = 1.0; flag = FEM1D_NODE; return e; }
    double L[S];
    for (int it = 0; it < BISECT_MAXIT; ++it) {
        xi = (lo + hi) / 2;
        if (xi == lo || xi == hi) break;
        lagrange<S>(nodes, xi, L);
        double fmid = 0.0;
        for (int j = 0; j < S; ++j) fmid += L[j] * xe[j];
        fmid -= t;
        if (fmid == 0.0) break;
        if (signbit(fmid) == signbit(flo)) {
            lo = xi;
            flo = fmid;
        } else {
            hi = xi;
        }
    }
    return e;
}

// 1-D Q_k evaluate.  GRAD: the values are clamped outside [x_lo, x_hi], so the derivative there is 0; at x_lo / x_hi
// (and at any other element end the point hits exactly) it is the one-sided derivative of the element.
template <int S, bool GRAD>
__device__ inline void fem1d_evaluate(const QueryArgs& a, const double (&nodes)[S], int64_t N, int64_t q, int64_t e,
                                      double xi, int32_t flag) {
    const int nc = a.ncomp;
    if (flag != FEM1D_GENERAL) {
        const int64_t row = xi < 0.0 ? e * S : e * S + S - 1;
        for (int c = 0; c < nc; ++c) a.out[q * nc + c] = a.z[row * nc + c];
        if constexpr (GRAD) {
            if (flag == FEM1D_NODE) fem1d_gradient<S>(a, q, e, xi);
            else if (flag == FEM1D_CROSSED) fem1d_gradient<S>(a, q, N - 1, 1.0);
            else
                for (int c = 0; c < nc; ++c) a.grad[q * nc + c] = 0.0;
        }
        return;
    }
    double L[S];
    lagrange<S>(nodes, xi, L);
    for (int c = 0; c < nc; ++c) {
        double v = 0.0;
        for (int j = 0; j < S; ++j) v += L[j] * a.z[(e * S + j) * nc + c];
        a.out[q * nc + c] = v;
    }
    if constexpr (GRAD) fem1d_gradient<S>(a, q, e, xi);
}

template <int S, bool GRAD>
__global__ void __launch_bounds__(BLOCK) query_fem1d(QueryArgs a, int64_t N, int32_t sorted) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.M) return;
    double nodes[S], xi;
    for (int j = 0; j < S; ++j) nodes[j] = a.table[j];
    int32_t flag;
    const int64_t e = fem1d_locate<S>(a.x, nodes, N, sorted, a.pts[q], xi, flag);
    if (e < 0) { write_nan<1, GRAD>(a, q); return; }
    if (a.elem) a.elem[q] = (int32_t)e;
    fem1d_evaluate<S, GRAD>(a, nodes, N, q, e, xi, flag);
}

template <int S>
__global__ void __launch_bounds__(BLOCK) locate_fem1d(QueryArgs a, int64_t N, int32_t sorted, LocArgs l) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.M) return;
    double nodes[S], xi;
    for (int j = 0; j < S; ++j) nodes[j] = a.table[j];
    int32_t flag;
    l.elem[q] = (int32_t)fem1d_locate<S>(a.x, nodes, N, sorted, a.pts[q], xi, flag);
    l.ref[q] = xi;
    l.flag[q] = flag;
}

template <int S, bool GRAD>
__global__ void __launch_bounds__(BLOCK) eval_fem1d(QueryArgs a, int64_t N, LocArgs l) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.M) return;
    const int64_t e = l.elem[q];
    if (e < 0) { write_nan<1, GRAD>(a, q); return; }
    double nodes[S];
    for (int j = 0; j < S; ++j) nodes[j] = a.table[j];
    fem1d_evaluate<S, GRAD>(a, nodes, N, q, e, l.ref[q], l.flag[q]);
}

// spectral: sum_j c_j T_j(t) (1-D) and bx' C by (2-D) with the three-term recurrence of `_chebyshev_values`; GRAD carries
// the differentiated recurrence T_j' = 2 T_{j-1} + 2 x T_{j-1}' - T_{j-2}' next to it (finite at x = +-1).  There is
// nothing to locate: a point locator keeps the points, and eval_spectral* is the query without the element output.
__device__ inline double cheb_next(double x, double tm1, double tm2) { return 2 * x * tm1 - tm2; }
__device__ inline double cheb_d_next(double x, double tm1, double dm1, double dm2) { return 2 * tm1 + 2 * x * dm1 - dm2; }

template <bool GRAD>
__device__ inline void spectral1d_point(const QueryArgs& a, int64_t q, int32_t n) {
    const double t = a.pts[q];
    if (!isfinite(t)) { write_nan<1, GRAD>(a, q); return; }
    for (int c = 0; c < a.ncomp; ++c) {
        double v = 0.0, tm2 = 0.0, tm1 = 0.0;
        double dv = 0.0, dm2 = 0.0, dm1 = 0.0;
        for (int j = 0; j < n; ++j) {
            const double tj = j == 0 ? 1.0 : (j == 1 ? t : cheb_next(t, tm1, tm2));
            const double cj = a.z[(int64_t)j * a.ncomp + c];
            v += cj * tj;
            if constexpr (GRAD) {
                const double dj = j == 0 ? 0.0 : (j == 1 ? 1.0 : cheb_d_next(t, tm1, dm1, dm2));
                dv += cj * dj;
                dm2 = dm1;
                dm1 = dj;
            }
            tm2 = tm1;
            tm1 = tj;
        }
        a.out[q * a.ncomp + c] = v;
        if constexpr (GRAD) a.grad[q * a.ncomp + c] = dv;
    }
    if (a.elem) a.elem[q] = 0;
}

template <bool GRAD>
__device__ inline void spectral2d_point(const QueryArgs& a, int64_t q, int32_t n) {
    const double px = a.pts[q * 2], py = a.pts[q * 2 + 1];
    if (!isfinite(px) || !isfinite(py)) { write_nan<2, GRAD>(a, q); return; }
    for (int c = 0; c < a.ncomp; ++c) {
        double v = 0.0, xm2 = 0.0, xm1 = 0.0;
        double gx = 0.0, gy = 0.0, dxm2 = 0.0, dxm1 = 0.0;
        for (int i = 0; i < n; ++i) {
            const double bx = i == 0 ? 1.0 : (i == 1 ? px : cheb_next(px, xm1, xm2));
            double r = 0.0, ym2 = 0.0, ym1 = 0.0;
            double rd = 0.0, dym2 = 0.0, dym1 = 0.0;
            for (int j = 0; j < n; ++j) {
                const double by = j == 0 ? 1.0 : (j == 1 ? py : cheb_next(py, ym1, ym2));
                const double cij = a.z[((int64_t)i * n + j) * a.ncomp + c];
                r += cij * by;
                if constexpr (GRAD) {
                    const double dby = j == 0 ? 0.0 : (j == 1 ? 1.0 : cheb_d_next(py, ym1, dym1, dym2));
                    rd += cij * dby;
                    dym2 = dym1;
                    dym1 = dby;
                }
                ym2 = ym1;
                ym1 = by;
            }
            v += bx * r;
            if constexpr (GRAD) {
                const double dbx = i == 0 ? 0.0 : (i == 1 ? 1.0 : cheb_d_next(px, xm1, dxm1, dxm2));
                gx += dbx * r;
                gy += bx * rd;
                dxm2 = dxm1;
                dxm1 = dbx;
            }
            xm2 = xm1;
            xm1 = bx;
        }
        a.out[q * a.ncomp + c] = v;
        if constexpr (GRAD) {
            a.grad[(q * a.ncomp + c) * 2] = gx;
            a.grad[(q * a.ncomp + c) * 2 + 1] = gy;
        }
    }
    if (a.elem) a.elem[q] = 0;
}

template <bool GRAD>
__global__ void __launch_bounds__(BLOCK) query_spectral1d(QueryArgs a, int32_t n) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < a.M) spectral1d_point<GRAD>(a, q, n);
}

template <bool GRAD>
__global__ void __launch_bounds__(BLOCK) query_spectral2d(QueryArgs a, int32_t n) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < a.M) spectral2d_point<GRAD>(a, q, n);
}

// the locator's kernels: a.elem is NULL (the elements of a spectral locator are all 0 and never stored)
template <bool GRAD>
__global__ void __launch_bounds__(BLOCK) eval_spectral1d(QueryArgs a, int32_t n) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < a.M) spectral1d_point<GRAD>(a, q, n);
}

template <bool GRAD>
__global__ void __launch_bounds__(BLOCK) eval_spectral2d(QueryArgs a, int32_t n) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < a.M) spectral2d_point<GRAD>(a, q, n);
}

template <int D>
__global__ void query_keys(int64_t M, Grid g, const double* __restrict__ pts, uint32_t* __restrict__ keys,
                           int32_t* __restrict__ idx) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= M) return;
    double pt[D];
    for (int d = 0; d < D; ++d) pt[d] = pts[q * D + d];
    const int64_t c = point_cell<D>(g, pt);
    keys[q] = c < 0 ? (uint32_t)g.ncell : (uint32_t)c;
    idx[q] = (int32_t)q;
}

// which kernels a launch sequence runs: the fused query (mgbhip_interpolate*), or one half of it for a point locator
enum class Pass { FUSED, LOCATE, EVAL };

template <int D, int S>
void launch_qk(Pass pass, const QueryArgs& a, const Grid& g, const LocArgs& l, hipStream_t st) {
    const dim3 gr(grid_1d(a.M)), bl(BLOCK);
    if (pass == Pass::LOCATE) hipLaunchKernelGGL((locate_qk<D, S>), gr, bl, 0, st, a, g, l);
    else if (pass == Pass::EVAL) {
        if (a.grad) hipLaunchKernelGGL((eval_qk<D, S, true>), gr, bl, 0, st, a, l);
        else hipLaunchKernelGGL((eval_qk<D, S, false>), gr, bl, 0, st, a, l);
    } else {
        if (a.grad) hipLaunchKernelGGL((query_qk<D, S, true>), gr, bl, 0, st, a, g);
        else hipLaunchKernelGGL((query_qk<D, S, false>), gr, bl, 0, st, a, g);
    }
}

template <int D>
void launch_qk_d(int S, Pass pass, const QueryArgs& a, const Grid& g, const LocArgs& l, hipStream_t st) {
    switch (S) {
        case 2: launch_qk<D, 2>(pass, a, g, l, st); break;
        case 3: launch_qk<D, 3>(pass, a, g, l, st); break;
        case 4: launch_qk<D, 4>(pass, a, g, l, st); break;
        case 5: launch_qk<D, 5>(pass, a, g, l, st); break;
        case 6: launch_qk<D, 6>(pass, a, g, l, st); break;
        case 7: launch_qk<D, 7>(pass, a, g, l, st); break;
        case 8: launch_qk<D, 8>(pass, a, g, l, st); break;
        case 9: launch_qk<D, 9>(pass, a, g, l, st); break;
        default: throw InvalidArgument("interpolate: Q_k degree out of range");
    }
}

template <int FAM>
void launch_simplex(Pass pass, const QueryArgs& a, const Grid& g, const LocArgs& l, hipStream_t st) {
    const dim3 gr(grid_1d(a.M)), bl(BLOCK);
    if (pass == Pass::LOCATE) hipLaunchKernelGGL((locate_simplex<FAM>), gr, bl, 0, st, a, g, l);
    else if (pass == Pass::EVAL) {
        if (a.grad) hipLaunchKernelGGL((eval_simplex<FAM, true>), gr, bl, 0, st, a, l);
        else hipLaunchKernelGGL((eval_simplex<FAM, false>), gr, bl, 0, st, a, l);
    } else {
        if (a.grad) hipLaunchKernelGGL((query_simplex<FAM, true>), gr, bl, 0, st, a, g);
        else hipLaunchKernelGGL((query_simplex<FAM, false>), gr, bl, 0, st, a, g);
    }
}

// Q_k / P1 / P2 / P2C in D dimensions; EVAL needs no grid
template <int D>
void launch_located(int32_t family, int32_t k, Pass pass, const QueryArgs& a, const Grid& g, const LocArgs& l,
                    hipStream_t st) {
    if (family == MGBHIP_INTERP_QK) {
        launch_qk_d<D>(k + 1, pass, a, g, l, st);
    } else if constexpr (D == 2) {
        if (family == MGBHIP_INTERP_P1)
            launch_simplex<MGBHIP_INTERP_P1>(pass, a, g, l, st);
        else if (family == MGBHIP_INTERP_P2)
            launch_simplex<MGBHIP_INTERP_P2>(pass, a, g, l, st);
        else
            launch_simplex<MGBHIP_INTERP_P2C>(pass, a, g, l, st);
    }
    MGB_HIP_CHECK(hipGetLastError());
}

template <int S>
void launch_1d(Pass pass, const QueryArgs& a, int64_t N, int32_t sorted, const LocArgs& l, hipStream_t st) {
    const dim3 gr(grid_1d(a.M)), bl(BLOCK);
    if (pass == Pass::LOCATE) hipLaunchKernelGGL((locate_fem1d<S>), gr, bl, 0, st, a, N, sorted, l);
    else if (pass == Pass::EVAL) {
        if (a.grad) hipLaunchKernelGGL((eval_fem1d<S, true>), gr, bl, 0, st, a, N, l);
        else hipLaunchKernelGGL((eval_fem1d<S, false>), gr, bl, 0, st, a, N, l);
    } else {
        if (a.grad) hipLaunchKernelGGL((query_fem1d<S, true>), gr, bl, 0, st, a, N, sorted);
        else hipLaunchKernelGGL((query_fem1d<S, false>), gr, bl, 0, st, a, N, sorted);
    }
}

void launch_1d_s(int S, Pass pass, const QueryArgs& a, int64_t N, int32_t sorted, const LocArgs& l, hipStream_t st) {
    switch (S) {
        case 2: launch_1d<2>(pass, a, N, sorted, l, st); break;
        case 3: launch_1d<3>(pass, a, N, sorted, l, st); break;
        case 4: launch_1d<4>(pass, a, N, sorted, l, st); break;
        case 5: launch_1d<5>(pass, a, N, sorted, l, st); break;
        case 6: launch_1d<6>(pass, a, N, sorted, l, st); break;
        case 7: launch_1d<7>(pass, a, N, sorted, l, st); break;
        case 8: launch_1d<8>(pass, a, N, sorted, l, st); break;
        case 9: launch_1d<9>(pass, a, N, sorted, l, st); break;
        default: throw InvalidArgument("interpolate: fem1d degree out of range");
    }
    MGB_HIP_CHECK(hipGetLastError());
}

// FUSED: the query with the element output; EVAL: a locator's evaluation (a.elem is NULL)
void launch_spectral(int32_t family, Pass pass, const QueryArgs& a, int32_t n, hipStream_t st) {
    const dim3 gr(grid_1d(a.M)), bl(BLOCK);
    if (family == MGBHIP_INTERP_SPECTRAL1D) {
        if (pass == Pass::EVAL) {
            if (a.grad) hipLaunchKernelGGL(eval_spectral1d<true>, gr, bl, 0, st, a, n);
            else hipLaunchKernelGGL(eval_spectral1d<false>, gr, bl, 0, st, a, n);
        } else {
            if (a.grad) hipLaunchKernelGGL(query_spectral1d<true>, gr, bl, 0, st, a, n);
            else hipLaunchKernelGGL(query_spectral1d<false>, gr, bl, 0, st, a, n);
        }
    } else {
        if (pass == Pass::EVAL) {
            if (a.grad) hipLaunchKernelGGL(eval_spectral2d<true>, gr, bl, 0, st, a, n);
            else hipLaunchKernelGGL(eval_spectral2d<false>, gr, bl, 0, st, a, n);
        } else {
            if (a.grad) hipLaunchKernelGGL(query_spectral2d<true>, gr, bl, 0, st, a, n);
            else hipLaunchKernelGGL(query_spectral2d<false>, gr, bl, 0, st, a, n);
        }
    }
    MGB_HIP_CHECK(hipGetLastError());
}

// the uniform grid over the union of the element boxes and its candidate lists (cell -> elements in ascending order);
// D counts coordinates and in.p nodes per element, so the elements may be of a lower dimension than D (closest.hip).
// Complete on return.
template <int D>
void build_grid(const InterpIn& in, const double* d_x, hipStream_t st, Grid& g, DevBuf<int32_t>& start,
                DevBuf<int32_t>& cand, DevBuf<double>& box, double reach = 0.0) {
    const int64_t N = in.N;
    box.alloc((size_t)N * 2 * D);
    // Curved P2 takes the Q_k pad: the image of a valid element (det J > 0 throughout) is bounded by its three edge
    // curves, the bubble vanishes on the edges, and each edge is the quadratic through its three nodes.  A quadratic
    // Lagrange interpolant on three equispaced parameters leaves the interval of its node values by at most 1/8 of
    // their spread (ends 0 and 1 with mid-node 1 peak at 9/8), so 1/8 of the largest extent always suffices.
    const bool curved = (in.family == MGBHIP_INTERP_QK && in.k >= 2) || in.family == MGBHIP_INTERP_P2C;
    const double pad = curved ? QK_BOX_PAD : 0.0;
    hipLaunchKernelGGL((elem_boxes<D>), dim3(grid_1d(N)), dim3(BLOCK), 0, st, N, in.p, d_x, pad, reach, box.p);
    cell_lists_from_boxes<D>("interpolate", "element", N, box.p, LOCATION_CELLS<D>, g, start, cand, st);
    // the work buffers were freed on return; hipFree waits for the work that uses them
}

// order[i] = the point lane i processes: the M points sorted by cell (a point without a cell sorts last).  A wave then
// reads the same few candidate lists and runs a similar number of Newton steps (all kernels of a call, P2 at L = 9 with
// 4 M random points: 0.69 ms against 0.87 ms unsorted; fem3d k = 3 at L = 5 with 1 M points: 3.0 ms against 5.8 ms).
template <int D>
void sort_points(const Grid& g, int64_t M, const double* d_pts, DevBuf<int32_t>& order, hipStream_t st) {
    DevBuf<uint32_t> k0, k1;
    DevBuf<int32_t> i0;
    k0.alloc((size_t)M); k1.alloc((size_t)M); i0.alloc((size_t)M); order.alloc((size_t)M);
    hipLaunchKernelGGL((query_keys<D>), dim3(grid_1d(M)), dim3(BLOCK), 0, st, M, g, d_pts, k0.p, i0.p);
    DevBuf<char> tmp;
    sort_pairs(k0.p, k1.p, i0.p, order.p, M, key_bits((uint64_t)g.ncell), tmp, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));        // the sort buffers are freed on return
}

// The located families: build the grid, sort the points by cell and run the fused query (pass FUSED) or the locate
// kernel alone (pass LOCATE: l receives the result in cell order and `order` is left to the caller, who keeps it).  The
// grid, the candidate lists, the boxes and the sort buffers are freed on return.
template <int D>
void run_located(const InterpIn& in, Pass pass, QueryArgs a, const LocArgs& l, const double* d_x, hipStream_t st,
                 DevBuf<int32_t>& order) {
    Grid g;
    DevBuf<int32_t> start, cand;
    DevBuf<double> box;
    build_grid<D>(in, d_x, st, g, start, cand, box);
    a.start = start.p;
    a.cand = cand.p;
    a.box = box.p;
    sort_points<D>(g, a.M, a.pts, order, st);
    a.order = order.p;
    launch_located<D>(in.family, in.k, pass, a, g, l, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace

void location_grid_build(LocationGrid& G, const InterpIn& in, const double* d_x, hipStream_t st) {
    MGB_REQUIRE(in.d == 2 || in.d == 3, "interpolate: a location grid needs d = 2 or 3");
    if (in.d == 2) build_grid<2>(in, d_x, st, G.g, G.start, G.cand, G.box);
    else build_grid<3>(in, d_x, st, G.g, G.start, G.cand, G.box);
}

void location_grid_build_embedded(LocationGrid& G, int32_t e, int32_t k, int32_t p, int64_t N, const double* d_x,
                                  double reach, hipStream_t st) {
    MGB_REQUIRE(e == 2 || e == 3, "closest_point: a location grid needs e = 2 or 3");
    InterpIn in;
    in.family = MGBHIP_INTERP_QK; in.d = e; in.k = k; in.p = p; in.N = N;
    if (e == 2) build_grid<2>(in, d_x, st, G.g, G.start, G.cand, G.box, reach);
    else build_grid<3>(in, d_x, st, G.g, G.start, G.cand, G.box, reach);
}

void location_grid_sort_points(const LocationGrid& G, int32_t e, int64_t M, const double* d_pts, DevBuf<int32_t>& order,
                               hipStream_t st) {
    if (e == 2) sort_points<2>(G.g, M, d_pts, order, st);
    else sort_points<3>(G.g, M, d_pts, order, st);
}

void interpolate_run(const InterpIn& in, hipStream_t st) {
    if (in.M == 0) return;
    const int64_t rows = (int64_t)in.p * in.N;
    DevBuf<double> d_x, d_table, d_z, d_pts, d_out, d_grad;
    DevBuf<int32_t> d_elem, d_order;
    const bool fem = interp_is_fem(in.family);
    if (fem) d_x.upload(in.x, (size_t)rows * in.d, st);
    if (in.table) d_table.upload(in.table, (size_t)in.table_len, st);
    d_z.upload(in.z, (size_t)rows * in.ncomp, st);
    d_pts.upload(in.pts, (size_t)in.M * in.d, st);
    d_out.alloc((size_t)in.M * in.ncomp);
    if (in.grad) d_grad.alloc((size_t)in.M * in.ncomp * in.d);
    if (in.elem) d_elem.alloc((size_t)in.M);
    QueryArgs a{};
    a.M = in.M;
    a.p = in.p;
    a.ncomp = in.ncomp;
    a.x = d_x.p;
    a.table = d_table.p;
    a.z = d_z.p;
    a.pts = d_pts.p;
    a.out = d_out.p;
    a.grad = in.grad ? d_grad.p : nullptr;
    a.elem = in.elem ? d_elem.p : nullptr;
    const LocArgs none{};
    switch (in.family) {
        case MGBHIP_INTERP_FEM1D:
            launch_1d_s(in.k + 1, Pass::FUSED, a, in.N, in.sorted, none, st);
            break;
        case MGBHIP_INTERP_QK:
        case MGBHIP_INTERP_P1:
        case MGBHIP_INTERP_P2:
        case MGBHIP_INTERP_P2C:
            if (in.d == 2) run_located<2>(in, Pass::FUSED, a, none, d_x.p, st, d_order);
            else run_located<3>(in, Pass::FUSED, a, none, d_x.p, st, d_order);
            break;
        case MGBHIP_INTERP_SPECTRAL1D:
        case MGBHIP_INTERP_SPECTRAL2D:
            launch_spectral(in.family, Pass::FUSED, a, (int32_t)(in.k + 1), st);
            break;
        default: throw InvalidArgument("interpolate: unknown family");
    }
    if (in.out) d_out.download(in.out, (size_t)in.M * in.ncomp, st);
    if (in.grad) d_grad.download(in.grad, (size_t)in.M * in.ncomp * in.d, st);
    if (in.elem) d_elem.download(in.elem, (size_t)in.M, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

// ---------------------------------------------------------------------------------------------------------------
// point locator: locate once, evaluate many z
// ---------------------------------------------------------------------------------------------------------------

void locator_build(Locator& L, const InterpIn& in, hipStream_t st) {
    const bool fem = interp_is_fem(in.family);
    if (in.M == 0 || !fem) {
        L.family = in.family; L.d = in.d; L.k = in.k; L.p = in.p; L.N = in.N; L.M = in.M;
        if (in.M == 0) return;
        L.pts.upload(in.pts, (size_t)in.M * in.d, st);      // nothing to locate: the points are the resident state
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        return;
    }
    DevBuf<double> d_pts;                        // freed on return: the evaluation reads only (element, reference point)
    d_pts.upload(in.pts, (size_t)in.M * in.d, st);
    locator_build_device(L, in, d_pts.p, st);
}

void locator_build_device(Locator& L, const InterpIn& in, const double* d_pts, hipStream_t st) {
    L.family = in.family; L.d = in.d; L.k = in.k; L.p = in.p; L.N = in.N; L.M = in.M;
    if (in.M == 0) return;
    MGB_REQUIRE(interp_is_fem(in.family), "interpolate: only the FEM families locate device-resident points");
    const int64_t rows = (int64_t)in.p * in.N;
    L.x.upload(in.x, (size_t)rows * in.d, st);
    L.table.upload(in.table, (size_t)in.table_len, st);
    L.elem.alloc((size_t)in.M);
    L.ref.alloc((size_t)in.M * (in.family == MGBHIP_INTERP_FEM1D ? 1 : in.d));
    if (in.family == MGBHIP_INTERP_FEM1D) L.flag.alloc((size_t)in.M);
    QueryArgs a{};
    a.M = in.M;
    a.p = in.p;
    a.x = L.x.p;
    a.table = L.table.p;
    a.pts = d_pts;
    const LocArgs l{L.elem.p, L.ref.p, L.flag.p};
    if (in.family == MGBHIP_INTERP_FEM1D) {
        launch_1d_s(in.k + 1, Pass::LOCATE, a, in.N, in.sorted, l, st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
    } else if (in.d == 2) {
        run_located<2>(in, Pass::LOCATE, a, l, L.x.p, st, L.order);
    } else {
        run_located<3>(in, Pass::LOCATE, a, l, L.x.p, st, L.order);
    }
}

void locator_elements(const Locator& L, int32_t* elem, hipStream_t st) {
    if (L.M == 0) return;
    if (!interp_is_fem(L.family)) {              // spectral: one element; a non-finite point has none (as write_nan reports)
        std::vector<double> pts((size_t)L.M * L.d);
        L.pts.download(pts.data(), pts.size(), st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        for (int64_t q = 0; q < L.M; ++q) {
            bool fin = true;
            for (int a = 0; a < L.d; ++a) fin = fin && std::isfinite(pts[(size_t)(q * L.d + a)]);
            elem[q] = fin ? 0 : -1;
        }
        return;
    }
    if (!L.order.p) {                            // fem1d: stored by point
        L.elem.download(elem, (size_t)L.M, st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        return;
    }
    std::vector<int32_t> e((size_t)L.M), o((size_t)L.M);
    L.elem.download(e.data(), (size_t)L.M, st);
    L.order.download(o.data(), (size_t)L.M, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < L.M; ++i) elem[o[(size_t)i]] = e[(size_t)i];
}

void locator_evaluate(Locator& L, int32_t ncomp, const double* z, double* out, double* grad, hipStream_t st) {
    if (L.M == 0) return;
    locator_evaluate_device(L, ncomp, z, grad != nullptr, st);
    if (out) L.out.download(out, (size_t)L.M * ncomp, st);
    if (grad) L.grad.download(grad, (size_t)L.M * ncomp * L.d, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void locator_evaluate_device(Locator& L, int32_t ncomp, const double* z, bool grad, hipStream_t st) {
    if (L.M == 0) return;
    const int64_t rows = (int64_t)L.p * L.N;
    // grown to the largest ncomp seen and kept: no allocation in a run of calls with the same ncomp
    L.z.upload(z, (size_t)rows * ncomp, st);
    locator_evaluate_resident(L, ncomp, L.z.p, grad, st);
}

void locator_evaluate_resident(Locator& L, int32_t ncomp, const double* d_z, bool grad, hipStream_t st) {
    if (L.M == 0) return;
    L.out.ensure((size_t)L.M * ncomp);
    if (grad) L.grad.ensure((size_t)L.M * ncomp * L.d);
    QueryArgs a{};
    a.M = L.M;
    a.p = L.p;
    a.ncomp = ncomp;
    a.x = L.x.p;
    a.table = L.table.p;
    a.z = d_z;
    a.pts = L.pts.p;
    a.order = L.order.p;
    a.out = L.out.p;
    a.grad = grad ? L.grad.p : nullptr;
    const LocArgs l{L.elem.p, L.ref.p, L.flag.p};
    const Grid g{};
    switch (L.family) {
        case MGBHIP_INTERP_FEM1D:
            launch_1d_s(L.k + 1, Pass::EVAL, a, L.N, 1, l, st);
            break;
        case MGBHIP_INTERP_QK:
        case MGBHIP_INTERP_P1:
        case MGBHIP_INTERP_P2:
        case MGBHIP_INTERP_P2C:
            if (L.d == 2) launch_located<2>(L.family, L.k, Pass::EVAL, a, g, l, st);
            else launch_located<3>(L.family, L.k, Pass::EVAL, a, g, l, st);
            break;
        case MGBHIP_INTERP_SPECTRAL1D:
        case MGBHIP_INTERP_SPECTRAL2D:
            launch_spectral(L.family, Pass::EVAL, a, (int32_t)(L.k + 1), st);
            break;
        default: throw InvalidArgument("interpolate: unknown family");
    }
}

}  // namespace mgbhip
