// Closest-point projection onto embedded curves and surfaces and evaluation at the feet: mgbhip_closest_*
// (include/mgbhip.h).
//
// The reference has no counterpart (its `interpolate`, src/utils.jl:16-58, covers flat 1-D meshes and the spectral
// families).  A query point of R^e is never exactly on a discrete curve or surface, so it is first projected: among the
// elements that come within max_distance of it, the foot is the point of least distance, and the element function is
// evaluated there.
//
// Candidates come from the location grid of interpolate.hip, built over the node boxes in R^e padded by max_distance:
// (cell, element) pairs emitted in element order and radix-sorted stably by cell, so a cell lists its candidates in
// ascending element order.  A lane visits them in that order and a later one wins only on a strictly smaller squared
// distance, so the result does not depend on the launch configuration.
//
// Every loop is bounded (the iterations, the candidate list of one cell, the nodes of one element), and a coordinate
// becomes a cell index only after it is known to be finite and inside the grid box.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "closest.hpp"
#include "interp_device.hpp"      // lagrange, lagrange_d, pick, point_cell and the tolerances of the flat locate kernels

// No fused multiply-adds in this file, as in interpolate.hip: the values are those of a plain IEEE transcription.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

// 1-D Lagrange basis with its first two derivatives: the product rule applied twice, one factor at a time
template <int S>
__device__ inline void lagrange_dd(const double* nodes, double xv, double* L, double* dL, double* ddL) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
        double num = 1.0, den = 1.0, dnum = 0.0, ddnum = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j)
            if (i != j) {
                const double t = xv - nodes[j];
                ddnum = ddnum * t + 2.0 * dnum;
                dnum = dnum * t + num;
                num *= t;
                den *= nodes[i] - nodes[j];
            }
        L[i] = num / den;
        dL[i] = dnum / den;
        ddL[i] = ddnum / den;
    }
}

// number of distinct second derivatives of a map of DR reference coordinates: (00) or (00, 01, 11)
template <int DR>
constexpr int nsecond() { return DR == 1 ? 1 : 3; }

// r = x(xi) - q, J = dx/dxi and X2 = the second derivatives of x at xi, in one pass over the element's nodes.  Node
// lin = i0 + S i1, axis 0 fastest; axis 0 is unrolled, axis 1 is a loop that picks its factors without run-time register
// indexing.  Every sum runs over the nodes relative to the element's first node x_0 (sum phi_i = 1, sum dphi_i = 0), and
// r = sum_i phi_i (x_i - x_0) - (q - x_0): the differences are exact for a small element far from the origin, where sums of
// the coordinates themselves would carry the rounding of max|x| into a residual many orders smaller.
template <int DR, int E, int S>
__device__ inline void element_pass(const double* __restrict__ xe, const double (&nodes)[S], const double (&xi)[DR],
                                    const double (&q)[E], double (&r)[E], double (&J)[E][DR],
                                    double (&X2)[nsecond<DR>()][E]) {
    double L[DR][S], dL[DR][S], ddL[DR][S];
#pragma unroll
    for (int b = 0; b < DR; ++b) lagrange_dd<S>(nodes, xi[b], L[b], dL[b], ddL[b]);
    for (int a = 0; a < E; ++a) {
        r[a] = 0.0;
        for (int b = 0; b < DR; ++b) J[a][b] = 0.0;
        for (int b = 0; b < nsecond<DR>(); ++b) X2[b][a] = 0.0;
    }
    const int n1 = DR == 2 ? S : 1;
#pragma unroll 1
    for (int i1 = 0; i1 < n1; ++i1) {
        double l1 = 1.0, d1 = 0.0, dd1 = 0.0;
        if constexpr (DR == 2) {
            l1 = pick<S>(L[DR - 1], i1);
            d1 = pick<S>(dL[DR - 1], i1);
            dd1 = pick<S>(ddL[DR - 1], i1);
        }
#pragma unroll
        for (int i0 = 0; i0 < S; ++i0) {
            const int lin = i0 + S * i1;
            const double phi = L[0][i0] * l1, p0 = dL[0][i0] * l1, p00 = ddL[0][i0] * l1;
            const double p1 = L[0][i0] * d1, p01 = dL[0][i0] * d1, p11 = L[0][i0] * dd1;
            for (int a = 0; a < E; ++a) {
                const double xa = xe[lin * E + a] - xe[a];
                r[a] += phi * xa;
                J[a][0] += p0 * xa;
                X2[0][a] += p00 * xa;
                if constexpr (DR == 2) {
                    J[a][DR - 1] += p1 * xa;
                    X2[1][a] += p01 * xa;
                    X2[nsecond<DR>() - 1][a] += p11 * xa;
                }
            }
        }
    }
    for (int a = 0; a < E; ++a) r[a] -= q[a] - xe[a];
}

// foot = x(xi) of the element and |foot - q|^2, both from the sum relative to the first node (see element_pass)
template <int DR, int E, int S>
__device__ inline double element_point(const double* __restrict__ xe, const double (&nodes)[S], const double (&xi)[DR],
                                       const double (&q)[E], double (&pt)[E]) {
    double L[DR][S];
#pragma unroll
    for (int b = 0; b < DR; ++b) lagrange<S>(nodes, xi[b], L[b]);
    for (int a = 0; a < E; ++a) pt[a] = 0.0;
    const int n1 = DR == 2 ? S : 1;
#pragma unroll 1
    for (int i1 = 0; i1 < n1; ++i1) {
        double l1 = 1.0;
        if constexpr (DR == 2) l1 = pick<S>(L[DR - 1], i1);
#pragma unroll
        for (int i0 = 0; i0 < S; ++i0) {
            const double phi = L[0][i0] * l1;
            for (int a = 0; a < E; ++a) pt[a] += phi * (xe[(i0 + S * i1) * E + a] - xe[a]);
        }
    }
    double d2 = 0.0;
    for (int a = 0; a < E; ++a) {
        const double t = pt[a] - (q[a] - xe[a]);
        d2 += t * t;
        pt[a] = xe[a] + pt[a];
    }
    return d2;
}

// |(J^T J)^-1 J^T|_inf and A = J^T J (A[0], A[1], A[2] = 00, 01, 11); false when J^T J is singular or not finite
template <int DR, int E>
__device__ inline bool pinv_norm(const double (&J)[E][DR], double (&A)[3], double& ninv) {
    A[0] = A[1] = A[2] = 0.0;
    for (int a = 0; a < E; ++a) {
        A[0] += J[a][0] * J[a][0];
        if constexpr (DR == 2) {
            A[1] += J[a][0] * J[a][DR - 1];
            A[2] += J[a][DR - 1] * J[a][DR - 1];
        }
    }
    double det;
    if constexpr (DR == 1) {
        det = A[0];
        double s = 0.0;
        for (int a = 0; a < E; ++a) s += fabs(J[a][0]);
        ninv = s / det;
    } else {
        det = A[0] * A[2] - A[1] * A[1];
        double s0 = 0.0, s1 = 0.0;
        for (int a = 0; a < E; ++a) {
            s0 += fabs((A[2] * J[a][0] - A[1] * J[a][DR - 1]) / det);
            s1 += fabs((A[0] * J[a][DR - 1] - A[1] * J[a][0]) / det);
        }
        ninv = fmax(s0, s1);
    }
    return det > 0.0 && isfinite(det) && isfinite(ninv);
}

// The point of element xe closest to q: f(xi) = |x(xi) - q|^2 / 2 minimised over [-1, 1]^DR from the element's node
// nearest to q.  With r = x(xi) - q, g = J^T r, A = J^T J and C = r . (second derivatives of x): a coordinate on a bound
// whose descent direction -g points out of the cube is frozen; the free coordinates take the Newton step of the full
// Hessian A + C where that is positive definite (Gauss-Newton alone converges at the rate |r| x curvature, which is 1 at a
// centre of curvature) and the Gauss-Newton step of A otherwise, clamped to the cube.  An iterate whose |r|^2 exceeds
// that of the last accepted one by more than its rounding level is rejected and the step from the accepted iterate
// halved instead.  The stopping test is qk_locate's with the pseudo-inverse in place of the inverse.  Returns whether
// it was met; xi is the last iterate either way, a point of the element.
template <int DR, int E, int S>
__device__ bool closest_solve(const double* __restrict__ xe, const double (&nodes)[S], const double (&q)[E],
                              double (&xi)[DR]) {
    constexpr int P = DR == 1 ? S : S * S;
    double xs = 0.0, near_d2 = INFINITY;
    int near = 0;
    for (int a = 0; a < E; ++a) xs = fmax(xs, fabs(q[a]));
#pragma unroll 1
    for (int i = 0; i < P; ++i) {
        double d2 = 0.0;
        for (int a = 0; a < E; ++a) {
            const double xa = xe[i * E + a], t = xa - q[a];
            xs = fmax(xs, fabs(xa));
            d2 += t * t;
        }
        if (d2 < near_d2) { near_d2 = d2; near = i; }
    }
    xi[0] = pick<S>(nodes, near % S);
    if constexpr (DR == 2) xi[DR - 1] = pick<S>(nodes, near / S);
    const double rn = ROUND_FACTOR * EPS * xs;       // rounding level of a component of r
    double xa[DR], sa[DR], fa = INFINITY, ta = 0.0;  // the last accepted iterate, its step, |r|^2 and tolerance
    for (int b = 0; b < DR; ++b) { xa[b] = xi[b]; sa[b] = 0.0; }
#pragma unroll 1
    for (int it = 0; it < CLOSEST_MAXIT; ++it) {
        double r[E], J[E][DR], X2[nsecond<DR>()][E];
        element_pass<DR, E, S>(xe, nodes, xi, q, r, J, X2);
        double f = 0.0;
        for (int a = 0; a < E; ++a) f += r[a] * r[a];
        if (f > fa + 4.0 * rn * (sqrt(fa) + rn)) {   // uphill (never while fa is infinite): halve the step
            double big = 0.0;
            for (int b = 0; b < DR; ++b) {
                sa[b] *= 0.5;
                big = fmax(big, fabs(sa[b]));
            }
            const bool small = big <= ta;
            for (int b = 0; b < DR; ++b) xi[b] = small ? xa[b] : xa[b] + sa[b];
            if (small) return true;
            continue;
        }
        double g[DR], C[3] = {0.0, 0.0, 0.0}, A[3], ninv;
        for (int b = 0; b < DR; ++b) {
            g[b] = 0.0;
            for (int a = 0; a < E; ++a) g[b] += J[a][b] * r[a];
        }
        for (int b = 0; b < nsecond<DR>(); ++b)
            for (int a = 0; a < E; ++a) C[b] += X2[b][a] * r[a];
        if (!pinv_norm<DR, E>(J, A, ninv)) return false;
        bool fr[DR];
        for (int b = 0; b < DR; ++b) fr[b] = (xi[b] <= -1.0 && g[b] > 0.0) || (xi[b] >= 1.0 && g[b] < 0.0);
        double s[DR];
        if constexpr (DR == 1) {
            double h = A[0] + C[0];
            if (!(h > 0.0)) h = A[0];
            s[0] = fr[0] ? 0.0 : -g[0] / h;
        } else {
            double H0 = A[0] + C[0], H1 = A[1] + C[1], H2 = A[2] + C[2];
            double det = H0 * H2 - H1 * H1;
            if (!(H0 > 0.0 && det > 0.0)) {
                H0 = A[0]; H1 = A[1]; H2 = A[2];
                det = H0 * H2 - H1 * H1;
            }
            double h0 = A[0] + C[0], h1 = A[2] + C[2];
            if (!(h0 > 0.0)) h0 = A[0];
            if (!(h1 > 0.0)) h1 = A[2];
            const bool f0 = fr[0], f1 = fr[DR - 1];
            s[0] = f0 ? 0.0 : (f1 ? -g[0] / h0 : -(H2 * g[0] - H1 * g[DR - 1]) / det);
            s[DR - 1] = f1 ? 0.0 : (f0 ? -g[DR - 1] / h1 : -(H0 * g[DR - 1] - H1 * g[0]) / det);
        }
        for (int b = 0; b < DR; ++b)
            if (!isfinite(s[b])) return false;
        const double tol = fmax(NEWTON_STEP_TOL, ROUND_FACTOR * EPS * xs * ninv);
        double step = 0.0;
        for (int b = 0; b < DR; ++b) {
            const double xn = fmin(fmax(xi[b] + s[b], -1.0), 1.0);
            xa[b] = xi[b];
            sa[b] = xn - xi[b];
            xi[b] = xn;
            step = fmax(step, fabs(sa[b]));
        }
        fa = f;
        ta = tol;
        if (step <= tol) return true;
    }
    return false;
}

struct ClosestArgs {
    int64_t M;
    const double* x;
    const double* table;
    const double* pts;
    const int32_t* start;
    const int32_t* cand;
    const double* box;
    const int32_t* order;
    double max_distance;
    int32_t* elem;             // the outputs, by slot i of the cell order
    double* ref;               // M x DR
    double* foot;              // M x E
    double* dist;
    int32_t* flag;
};

// One lane per point, in cell order.  Every candidate of the point's cell whose padded box holds the point is projected;
// one that does not converge still competes with the distance at its last iterate, which is a point of the element, so
// the distance is never an underestimate.
template <int DR, int E, int S>
__global__ void __launch_bounds__(BLOCK) closest_qk(ClosestArgs a, Grid g) {
    constexpr int P = DR == 1 ? S : S * S;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int64_t q = a.order[i];
    double pt[E];
    for (int c = 0; c < E; ++c) pt[c] = a.pts[q * E + c];
    double nodes[S];
    for (int j = 0; j < S; ++j) nodes[j] = a.table[j];
    int64_t best = -1;
    double best_d2 = INFINITY, best_xi[DR], best_foot[E];
    bool best_conv = false;
    for (int b = 0; b < DR; ++b) best_xi[b] = 0.0;
    for (int c = 0; c < E; ++c) best_foot[c] = 0.0;
    const int64_t cell = point_cell<E>(g, pt);
    if (cell >= 0) {
        const int32_t j1 = a.start[cell + 1];
        for (int32_t j = a.start[cell]; j < j1; ++j) {
            const int64_t e = a.cand[j];
            bool inbox = true;         // outside the padded box the element is farther than max_distance
            for (int c = 0; c < E; ++c)
                inbox = inbox && pt[c] >= a.box[e * 2 * E + c] && pt[c] <= a.box[e * 2 * E + E + c];
            if (!inbox) continue;
            const double* xe = a.x + e * P * E;
            double xi[DR], foot[E];
            const bool conv = closest_solve<DR, E, S>(xe, nodes, pt, xi);
            const double d2 = element_point<DR, E, S>(xe, nodes, xi, pt, foot);
            if (d2 < best_d2) {        // strictly: the lowest element index wins a tie
                best_d2 = d2;
                best = e;
                best_conv = conv;
                for (int b = 0; b < DR; ++b) best_xi[b] = xi[b];
                for (int c = 0; c < E; ++c) best_foot[c] = foot[c];
            }
        }
    }
    const double dist = sqrt(best_d2);
    const bool ok = best >= 0 && dist <= a.max_distance;
    a.elem[i] = ok ? (int32_t)best : -1;
    a.dist[i] = ok ? dist : dnan();
    a.flag[i] = ok && best_conv ? 1 : 0;
    for (int b = 0; b < DR; ++b) a.ref[i * DR + b] = ok ? best_xi[b] : dnan();
    for (int c = 0; c < E; ++c) a.foot[i * E + c] = ok ? best_foot[c] : dnan();
}

struct EvalArgs {
    int64_t M;
    int32_t ncomp;
    const double* x;
    const double* table;
    const double* z;
    const int32_t* order;
    const int32_t* elem;
    const double* ref;
    double* out;               // M x ncomp, by point
    double* grad;              // M x ncomp x E (GRAD only)
};

// One lane per point in the stored cell order: the value sums at the stored xi and, with GRAD, the tangential gradient
// J (J^T J)^-1 grad_xi u in ambient coordinates (a curve: (du/dxi) x' / |x'|^2).  The values are the same sums in the
// same order with and without GRAD.
template <int DR, int E, int S, bool GRAD>
__global__ void __launch_bounds__(BLOCK) closest_eval(EvalArgs a) {
    constexpr int P = DR == 1 ? S : S * S;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int64_t q = a.order[i];
    const int64_t e = a.elem[i];
    const int nc = a.ncomp;
    if (e < 0) {
        for (int c = 0; c < nc; ++c) a.out[q * nc + c] = dnan();
        if constexpr (GRAD)
            for (int c = 0; c < nc * E; ++c) a.grad[q * nc * E + c] = dnan();
        return;
    }
    double nodes[S], xi[DR], L[DR][S], dL[GRAD ? DR : 1][S];
    for (int j = 0; j < S; ++j) nodes[j] = a.table[j];
    for (int b = 0; b < DR; ++b) xi[b] = a.ref[i * DR + b];
#pragma unroll
    for (int b = 0; b < DR; ++b) {
        if constexpr (GRAD) lagrange_d<S>(nodes, xi[b], L[b], dL[b]);
        else lagrange<S>(nodes, xi[b], L[b]);
    }
    const int n1 = DR == 2 ? S : 1;
    double J[E][DR], A[3] = {0.0, 0.0, 0.0}, det = 0.0;
    if constexpr (GRAD) {
        for (int r = 0; r < E; ++r)
            for (int b = 0; b < DR; ++b) J[r][b] = 0.0;
        const double* xe = a.x + e * P * E;
#pragma unroll 1
        for (int i1 = 0; i1 < n1; ++i1) {
            double l1 = 1.0, d1 = 0.0;
            if constexpr (DR == 2) {
                l1 = pick<S>(L[DR - 1], i1);
                d1 = pick<S>(dL[DR - 1], i1);
            }
#pragma unroll
            for (int i0 = 0; i0 < S; ++i0) {
                const double p0 = dL[0][i0] * l1, p1 = L[0][i0] * d1;
                for (int r = 0; r < E; ++r) {
                    const double xr = xe[(i0 + S * i1) * E + r] - xe[r];      // relative to the first node, as element_pass
                    J[r][0] += p0 * xr;
                    if constexpr (DR == 2) J[r][DR - 1] += p1 * xr;
                }
            }
        }
        for (int r = 0; r < E; ++r) {
            A[0] += J[r][0] * J[r][0];
            if constexpr (DR == 2) {
                A[1] += J[r][0] * J[r][DR - 1];
                A[2] += J[r][DR - 1] * J[r][DR - 1];
            }
        }
        det = DR == 1 ? A[0] : A[0] * A[2] - A[1] * A[1];
    }
    const double* ze = a.z + e * P * nc;
    for (int c = 0; c < nc; ++c) {
        double v = 0.0, g0 = 0.0, g1 = 0.0;
#pragma unroll 1
        for (int i1 = 0; i1 < n1; ++i1) {
            double l1 = 1.0, d1 = 0.0;
            if constexpr (DR == 2) {
                l1 = pick<S>(L[DR - 1], i1);
                if constexpr (GRAD) d1 = pick<S>(dL[DR - 1], i1);
            }
#pragma unroll
            for (int i0 = 0; i0 < S; ++i0) {
                const double zv = ze[(i0 + S * i1) * nc + c];
                v += L[0][i0] * l1 * zv;
                if constexpr (GRAD) {
                    g0 += dL[0][i0] * l1 * zv;
                    if constexpr (DR == 2) g1 += L[0][i0] * d1 * zv;
                }
            }
        }
        a.out[q * nc + c] = v;
        if constexpr (GRAD) {
            // w = (J^T J)^-1 grad_xi u; a singular J^T J leaves the value and gives a NaN gradient
            const bool ok = det > 0.0 && isfinite(det);
            double w0, w1 = 0.0;
            if constexpr (DR == 1) {
                w0 = g0 / det;
            } else {
                w0 = (A[2] * g0 - A[1] * g1) / det;
                w1 = (A[0] * g1 - A[1] * g0) / det;
            }
            for (int r = 0; r < E; ++r) {
                double s = J[r][0] * w0;
                if constexpr (DR == 2) s += J[r][DR - 1] * w1;
                a.grad[(q * nc + c) * E + r] = ok ? s : dnan();
            }
        }
    }
}

template <int DR, int E, int S>
void launch_closest(const ClosestArgs& a, const Grid& g, hipStream_t st) {
    hipLaunchKernelGGL((closest_qk<DR, E, S>), dim3(grid_1d(a.M)), dim3(BLOCK), 0, st, a, g);
}

template <int DR, int E, int S>
void launch_eval(const EvalArgs& a, hipStream_t st) {
    if (a.grad) hipLaunchKernelGGL((closest_eval<DR, E, S, true>), dim3(grid_1d(a.M)), dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((closest_eval<DR, E, S, false>), dim3(grid_1d(a.M)), dim3(BLOCK), 0, st, a);
}

// f.template operator()<DR, E, S>() for the (d, e, k + 1) of a locator
template <int DR, int E, class F>
void dispatch_s(int S, F&& f) {
    switch (S) {
        case 2: f.template operator()<DR, E, 2>(); break;
        case 3: f.template operator()<DR, E, 3>(); break;
        case 4: f.template operator()<DR, E, 4>(); break;
        case 5: f.template operator()<DR, E, 5>(); break;
        case 6: f.template operator()<DR, E, 6>(); break;
        case 7: f.template operator()<DR, E, 7>(); break;
        case 8: f.template operator()<DR, E, 8>(); break;
        case 9: f.template operator()<DR, E, 9>(); break;
        default: throw InvalidArgument("closest_point: element degree out of range");
    }
}

template <class F>
void dispatch(int d, int e, int S, F&& f) {
    if (d == 1 && e == 2) dispatch_s<1, 2>(S, f);
    else if (d == 1 && e == 3) dispatch_s<1, 3>(S, f);
    else if (d == 2 && e == 3) dispatch_s<2, 3>(S, f);
    else throw InvalidArgument("closest_point: (d, e) must be (1, 2), (1, 3) or (2, 3)");
}

struct LaunchClosest {
    const ClosestArgs& a;
    const Grid& g;
    hipStream_t st;
    template <int DR, int E, int S>
    void operator()() const { launch_closest<DR, E, S>(a, g, st); }
};

struct LaunchEval {
    const EvalArgs& a;
    hipStream_t st;
    template <int DR, int E, int S>
    void operator()() const { launch_eval<DR, E, S>(a, st); }
};

}  // namespace

void closest_build(Closest& Cl, int32_t d, int32_t e, int32_t k, int64_t N, const double* x, const double* nodes,
                   int64_t M, const double* pts, double max_distance, hipStream_t st) {
    int32_t p = k + 1;
    if (d == 2) p *= k + 1;
    Cl.d = d; Cl.e = e; Cl.k = k; Cl.p = p; Cl.N = N; Cl.M = M; Cl.max_distance = max_distance;
    if (M == 0) return;
    Cl.x.upload(x, (size_t)p * N * e, st);
    Cl.table.upload(nodes, (size_t)(k + 1), st);
    DevBuf<double> d_pts;                        // freed on return: the evaluation reads only (element, xi)
    d_pts.upload(pts, (size_t)M * e, st);
    LocationGrid G;                              // freed on return as well
    location_grid_build_embedded(G, e, k, p, N, Cl.x.p, max_distance, st);
    location_grid_sort_points(G, e, M, d_pts.p, Cl.order, st);
    Cl.elem.alloc((size_t)M);
    Cl.flag.alloc((size_t)M);
    Cl.dist.alloc((size_t)M);
    Cl.ref.alloc((size_t)M * d);
    Cl.foot.alloc((size_t)M * e);
    ClosestArgs a{};
    a.M = M;
    a.x = Cl.x.p;
    a.table = Cl.table.p;
    a.pts = d_pts.p;
    a.start = G.start.p;
    a.cand = G.cand.p;
    a.box = G.box.p;
    a.order = Cl.order.p;
    a.max_distance = max_distance;
    a.elem = Cl.elem.p;
    a.ref = Cl.ref.p;
    a.foot = Cl.foot.p;
    a.dist = Cl.dist.p;
    a.flag = Cl.flag.p;
    dispatch(d, e, k + 1, LaunchClosest{a, G.g, st});
    MGB_HIP_CHECK(hipGetLastError());
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void closest_fetch(const Closest& Cl, int32_t* elem, double* xi, double* foot, double* dist, int32_t* flag,
                   hipStream_t st) {
    const size_t M = (size_t)Cl.M;
    if (M == 0) return;
    std::vector<int32_t> o(M), ie(elem ? M : 0), ifl(flag ? M : 0);
    std::vector<double> rx(xi ? M * Cl.d : 0), rf(foot ? M * Cl.e : 0), rd(dist ? M : 0);
    Cl.order.download(o.data(), M, st);
    if (elem) Cl.elem.download(ie.data(), M, st);
    if (flag) Cl.flag.download(ifl.data(), M, st);
    if (xi) Cl.ref.download(rx.data(), M * Cl.d, st);
    if (foot) Cl.foot.download(rf.data(), M * Cl.e, st);
    if (dist) Cl.dist.download(rd.data(), M, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < M; ++i) {             // slot i of the cell order holds point o[i]
        const size_t q = (size_t)o[i];
        if (elem) elem[q] = ie[i];
        if (flag) flag[q] = ifl[i];
        if (dist) dist[q] = rd[i];
        if (xi)
            for (int b = 0; b < Cl.d; ++b) xi[q * Cl.d + b] = rx[i * Cl.d + b];
        if (foot)
            for (int c = 0; c < Cl.e; ++c) foot[q * Cl.e + c] = rf[i * Cl.e + c];
    }
}

void closest_evaluate(Closest& Cl, int32_t ncomp, const double* z, double* out, double* grad, hipStream_t st) {
    if (Cl.M == 0) return;
    // grown to the largest ncomp seen and kept: no allocation in a run of calls with the same ncomp
    Cl.z.upload(z, (size_t)Cl.p * Cl.N * ncomp, st);
    Cl.out.ensure((size_t)Cl.M * ncomp);
    if (grad) Cl.grad.ensure((size_t)Cl.M * ncomp * Cl.e);
    EvalArgs a{};
    a.M = Cl.M;
    a.ncomp = ncomp;
    a.x = Cl.x.p;
    a.table = Cl.table.p;
    a.z = Cl.z.p;
    a.order = Cl.order.p;
    a.elem = Cl.elem.p;
    a.ref = Cl.ref.p;
    a.out = Cl.out.p;
    a.grad = grad ? Cl.grad.p : nullptr;
    dispatch(Cl.d, Cl.e, Cl.k + 1, LaunchEval{a, st});
    MGB_HIP_CHECK(hipGetLastError());
    if (out) Cl.out.download(out, (size_t)Cl.M * ncomp, st);
    if (grad) Cl.grad.download(grad, (size_t)Cl.M * ncomp * Cl.e, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
