// quadrature.hip -- element quadrature of element-space functions (mgbhip_quadrature_*): integrals of u, |u - g|^p,
// |grad u - G|^p and the p-Laplace energy over a mesh, per element and in total, and the maxima behind the p = inf norms.
//
// The host hands over a rule and the basis at its points (phi, dphi: Q x p, Q x p x d), so nothing here knows an element
// family.  One lane takes one (element, point) pair:
//   x_q = sum_i phi_i(xi_q) x_i,  J = sum_i x_i (grad_xi phi_i)^T  (e x d),  g = J^T J,  measure = w_q sqrt(det g),
//   u_q = sum_i phi_i(xi_q) z_i,  grad u = J g^-1 sum_i z_i grad_xi phi_i  (the tangential gradient when e > d).
// Every sum over the nodes is a chain of fused multiply-adds in node order.
//
// Summation order.  No atomics.  Lane s of an element adds the terms of its points s, s + S, ... in that order
// (S = min(Q, 256)); the S lane sums are added by a halving tree over s.  Both depend on Q alone, so an element's value
// does not depend on N, on the number of columns or on its place in the workgroup.  The element values go to an N x ncol
// array, and the column reduction of quad_device.hpp adds each column over the elements with the compensated sums of
// dsum.hpp in a fixed shape, so totals are reproducible bit for bit and a column's total does not depend on the others.
// faces.hip takes the plan, the write-out and the reduction from the same headers and has the same lines for the tree.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <vector>

#include "quad_device.hpp"
#include "quadrature.hpp"

namespace mgbhip {

namespace {

struct QuadParams {
    const double* x;         // (p N) x e
    const double* wref;      // Q
    const double* tab;       // [p][1 + d][Q]
    const double* z;         // (p N) x ncol
    const double* minus;     // N x Q x ncol (LP), N x Q x ncol x e (W1P) or null
    const double* source;    // p N (ENERGY)
    double* elem;            // N x ncol
    int64_t N;
    int32_t p, Q, ncol, S, G;
    int32_t is_max;          // the largest |u - g| or |grad u - G| instead of the integral
    int32_t pmode;           // 1: p = 1, 2: p = 2 (neither calls pow), 0: any other exponent
    double pexp;
};

template <int D, int E>
struct QuadGeo {
    double J[E][D];          // dx / dxi
    double gi[D][D];         // (J^T J)^-1
    double sdet;             // sqrt(det J^T J)
};

// The geometry of point q of the element whose nodes are xs [p][E]; with X also the point itself.
template <int D, int E, bool X>
__device__ __forceinline__ void quad_geo(const double* xs, const double* tab, int p, int Q, int q, QuadGeo<D, E>& geo,
                                         double* xq) {
#pragma unroll
    for (int a = 0; a < E; ++a) {
        if (X) xq[a] = 0.0;
#pragma unroll
        for (int b = 0; b < D; ++b) geo.J[a][b] = 0.0;
    }
    for (int i = 0; i < p; ++i) {
        const double* t = tab + (size_t)i * (1 + D) * Q + q;
#pragma unroll
        for (int a = 0; a < E; ++a) {
            const double xa = xs[i * E + a];
            if (X) xq[a] = __builtin_fma(t[0], xa, xq[a]);
#pragma unroll
            for (int b = 0; b < D; ++b) geo.J[a][b] = __builtin_fma(t[(size_t)(1 + b) * Q], xa, geo.J[a][b]);
        }
    }
    double g[D][D];
#pragma unroll
    for (int b = 0; b < D; ++b)
#pragma unroll
        for (int c = 0; c < D; ++c) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < E; ++a) s = __builtin_fma(geo.J[a][b], geo.J[a][c], s);
            g[b][c] = s;
        }
    double det;
    if constexpr (D == 1) {
        det = g[0][0];
        geo.gi[0][0] = 1.0 / det;
    } else if constexpr (D == 2) {
        det = g[0][0] * g[1][1] - g[0][1] * g[0][1];
        const double r = 1.0 / det;
        geo.gi[0][0] = g[1][1] * r;
        geo.gi[1][1] = g[0][0] * r;
        geo.gi[0][1] = geo.gi[1][0] = -g[0][1] * r;
    } else {
        const double c00 = g[1][1] * g[2][2] - g[1][2] * g[1][2];
        const double c01 = g[0][2] * g[1][2] - g[0][1] * g[2][2];
        const double c02 = g[0][1] * g[1][2] - g[0][2] * g[1][1];
        det = g[0][0] * c00 + g[0][1] * c01 + g[0][2] * c02;
        const double r = 1.0 / det;
        geo.gi[0][0] = c00 * r;
        geo.gi[0][1] = geo.gi[1][0] = c01 * r;
        geo.gi[0][2] = geo.gi[2][0] = c02 * r;
        geo.gi[1][1] = (g[0][0] * g[2][2] - g[0][2] * g[0][2]) * r;
        geo.gi[1][2] = geo.gi[2][1] = (g[0][1] * g[0][2] - g[0][0] * g[1][2]) * r;
        geo.gi[2][2] = (g[0][0] * g[1][1] - g[0][1] * g[0][1]) * r;
    }
    geo.sdet = sqrt(det);
}

__device__ __forceinline__ double quad_power(double s2, int pmode, double pexp) {      // |v|^p from s2 = |v|^2
    return pmode == 2 ? s2 : pmode == 1 ? sqrt(s2) : pow(s2, 0.5 * pexp);
}

template <int D, int E, int KIND, bool TAB_LDS>
__global__ __launch_bounds__(QUAD_THREADS) void quad_kernel(const QuadParams P) {
    extern __shared__ __attribute__((aligned(16))) double quad_lds[];
    const int tid = threadIdx.x, p = P.p, Q = P.Q, S = P.S, G = P.G, ncol = P.ncol;
    double* xs = quad_lds;
    double* zs = xs + quad_lds_xs(G, p, E);
    double* fs = zs + quad_lds_zs(G, p);
    double* red = fs + quad_lds_fs(G, p);
    const double* tab = P.tab;
    if constexpr (TAB_LDS) {
        double* tl = red + quad_lds_red();
        const int n = (1 + D) * Q * p;
        for (int i = tid; i < n; i += QUAD_THREADS) tl[i] = P.tab[i];
        tab = tl;                                   // first read after the barrier behind the z chunk
    }
    const int g = tid / S, s = tid - g * S;
    int tree = 1;
    while (tree < S) tree <<= 1;
    const bool single = Q <= QUAD_THREADS;          // one point per lane: its geometry is formed once per element
    const int64_t groups = (P.N + G - 1) / G;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t el0 = grp * G;
        const int nel = (int)((P.N - el0) < (int64_t)G ? (P.N - el0) : (int64_t)G);
        const int rows = nel * p;
        __syncthreads();
        for (int i = tid; i < rows * E; i += QUAD_THREADS) xs[i] = P.x[el0 * p * E + i];
        if constexpr (KIND == QUAD_ENERGY)
            for (int i = tid; i < rows; i += QUAD_THREADS) fs[i] = P.source[el0 * p + i];
        const bool active = g < nel;
        const int64_t el = el0 + g;
        const double* xe = xs + g * p * E;
        QuadGeo<D, E> geo;
        bool have_geo = false;
        for (int c0 = 0; c0 < ncol; c0 += QUAD_CHUNK) {
            const int nc = (ncol - c0) < QUAD_CHUNK ? (ncol - c0) : QUAD_CHUNK;
            for (int i = tid; i < rows * nc; i += QUAD_THREADS) {
                const int row = i / nc, c = i - row * nc;
                zs[row * QUAD_CHUNK + c] = P.z[(el0 * p + row) * ncol + c0 + c];
            }
            __syncthreads();
            if (active) {
                bool first = true;
                for (int q = s; q < Q; q += S) {
                    if (!(single && have_geo)) quad_geo<D, E, false>(xe, tab, p, Q, q, geo, nullptr);
                    have_geo = true;
                    const double w = P.wref[q] * geo.sdet;
                    const int64_t pt = el * Q + q;
                    for (int c = 0; c < nc; ++c) {
                        const double* zc = zs + g * p * QUAD_CHUNK + c;
                        double u = 0.0, f = 0.0, gx[D];
#pragma unroll
                        for (int b = 0; b < D; ++b) gx[b] = 0.0;
                        for (int i = 0; i < p; ++i) {
                            const double* t = tab + (size_t)i * (1 + D) * Q + q;
                            const double zi = zc[i * QUAD_CHUNK];
                            u = __builtin_fma(t[0], zi, u);
                            if constexpr (KIND == QUAD_ENERGY) f = __builtin_fma(t[0], fs[g * p + i], f);
                            if constexpr (KIND == QUAD_W1P || KIND == QUAD_ENERGY) {
#pragma unroll
                                for (int b = 0; b < D; ++b) gx[b] = __builtin_fma(t[(size_t)(1 + b) * Q], zi, gx[b]);
                            }
                        }
                        double F;
                        if constexpr (KIND == QUAD_VALUE) {
                            F = u;
                        } else if constexpr (KIND == QUAD_LP) {
                            const double v = fabs(P.minus ? u - P.minus[pt * ncol + c0 + c] : u);
                            F = P.is_max ? v : P.pmode == 1 ? v : P.pmode == 2 ? v * v : pow(v, P.pexp);
                        } else {
                            double tb[D];
#pragma unroll
                            for (int b = 0; b < D; ++b) {
                                double a = 0.0;
#pragma unroll
                                for (int cc = 0; cc < D; ++cc) a = __builtin_fma(geo.gi[b][cc], gx[cc], a);
                                tb[b] = a;
                            }
                            double s2 = 0.0;
#pragma unroll
                            for (int a = 0; a < E; ++a) {
                                double ga = 0.0;
#pragma unroll
                                for (int b = 0; b < D; ++b) ga = __builtin_fma(geo.J[a][b], tb[b], ga);
                                if (KIND == QUAD_W1P && P.minus) ga -= P.minus[(pt * ncol + c0 + c) * E + a];
                                s2 = __builtin_fma(ga, ga, s2);
                            }
                            if constexpr (KIND == QUAD_W1P) F = P.is_max ? sqrt(s2) : quad_power(s2, P.pmode, P.pexp);
                            else F = quad_power(s2, P.pmode, P.pexp) / P.pexp - f * u;
                        }
                        double* r = red + c * QUAD_THREADS + tid;
                        if (P.is_max) *r = first ? F : quad_max(*r, F);
                        else *r = first ? w * F : *r + w * F;
                    }
                    first = false;
                }
            }
            for (int off = tree >> 1; off > 0; off >>= 1) {         // the halving tree: face_kernel has these lines without the max
                __syncthreads();
                if (active && s < off && s + off < S) {
                    for (int c = 0; c < nc; ++c) {
                        double* r = red + c * QUAD_THREADS + tid;
                        *r = P.is_max ? quad_max(r[0], r[off]) : r[0] + r[off];
                    }
                }
            }
            __syncthreads();
            quad_write_items(P.elem, red, tid, el0, nel, S, ncol, c0, nc);
        }
    }
}

// points (N x Q x e) and weights (N x Q) of the rule on the mesh; either may be null
template <int D, int E>
__global__ __launch_bounds__(QUAD_THREADS) void quad_geometry_kernel(const double* __restrict__ x, const double* __restrict__ wref,
                                                                     const double* __restrict__ tab, int64_t N, int p, int Q,
                                                                     double* __restrict__ points, double* __restrict__ weights) {
    const int64_t idx = (int64_t)blockIdx.x * QUAD_THREADS + threadIdx.x;
    if (idx >= N * Q) return;
    const int64_t el = idx / Q;
    const int q = (int)(idx - el * Q);
    QuadGeo<D, E> geo;
    double xq[E];
    quad_geo<D, E, true>(x + el * p * E, tab, p, Q, q, geo, xq);
    if (points) {
#pragma unroll
        for (int a = 0; a < E; ++a) points[idx * E + a] = xq[a];
    }
    if (weights) weights[idx] = wref[q] * geo.sdet;
}

template <int D, int E, int KIND>
void launch_quad_tab(const QuadParams& P, const QuadPlan& plan, hipStream_t st) {
    if (plan.tables_lds) quad_launch<quad_kernel<D, E, KIND, true>>("quadrature", P, plan, st);
    else quad_launch<quad_kernel<D, E, KIND, false>>("quadrature", P, plan, st);
}

template <int D, int E>
void launch_quad_kind(int kind, const QuadParams& P, const QuadPlan& plan, hipStream_t st) {
    switch (kind) {
        case QUAD_VALUE: launch_quad_tab<D, E, QUAD_VALUE>(P, plan, st); break;
        case QUAD_LP: launch_quad_tab<D, E, QUAD_LP>(P, plan, st); break;
        case QUAD_W1P: launch_quad_tab<D, E, QUAD_W1P>(P, plan, st); break;
        default: launch_quad_tab<D, E, QUAD_ENERGY>(P, plan, st); break;
    }
}

// the (d, e) pairs: flat meshes of dimension 1..3, curves in R^2 / R^3, surfaces in R^3
template <class F>
void dispatch_dims(int d, int e, F&& f) {
    if (d == 1 && e == 1) f(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
    else if (d == 1 && e == 2) f(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
    else if (d == 1 && e == 3) f(std::integral_constant<int, 1>{}, std::integral_constant<int, 3>{});
    else if (d == 2 && e == 2) f(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{});
    else if (d == 2 && e == 3) f(std::integral_constant<int, 2>{}, std::integral_constant<int, 3>{});
    else if (d == 3 && e == 3) f(std::integral_constant<int, 3>{}, std::integral_constant<int, 3>{});
    else throw InvalidArgument("quadrature: (d, e) must be (1, 1..3), (2, 2..3) or (3, 3)");
}

}  // namespace

void quadrature_build(Quadrature& Qd, int32_t d, int32_t e, int32_t p, int64_t N, const double* x, int32_t Q,
                      const double* wref, const double* phi, const double* dphi, hipStream_t st) {
    Qd.d = d; Qd.e = e; Qd.p = p; Qd.Q = Q; Qd.N = N;
    std::vector<double> tab((size_t)(1 + d) * Q * p);
    quad_repack_tables(d, p, Q, phi, dphi, tab.data());
    Qd.x.upload(x, (size_t)p * N * e, st);
    Qd.wref.upload(wref, (size_t)Q, st);
    Qd.tab.upload(tab, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));       // tab is a local
}

void quadrature_geometry(Quadrature& Qd, double* points, double* weights, hipStream_t st) {
    const int64_t n = Qd.N * Qd.Q;
    Qd.geo.ensure((size_t)n * (Qd.e + 1));
    double* dpts = points ? Qd.geo.p : nullptr;
    double* dw = weights ? Qd.geo.p + n * Qd.e : nullptr;
    dispatch_dims(Qd.d, Qd.e, [&](auto D, auto E) {
        hipLaunchKernelGGL((quad_geometry_kernel<decltype(D)::value, decltype(E)::value>), dim3((unsigned)((n + QUAD_THREADS - 1) / QUAD_THREADS)),
                           dim3(QUAD_THREADS), 0, st, Qd.x.p, Qd.wref.p, Qd.tab.p, Qd.N, Qd.p, Qd.Q, dpts, dw);
    });
    MGB_HIP_CHECK(hipGetLastError());
    if (points) MGB_HIP_CHECK(hipMemcpyAsync(points, dpts, (size_t)n * Qd.e * sizeof(double), hipMemcpyDeviceToHost, st));
    if (weights) MGB_HIP_CHECK(hipMemcpyAsync(weights, dw, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void quadrature_integrate(Quadrature& Qd, int32_t kind, double pexp, bool is_max, int32_t ncol, const double* z,
                          const double* minus, const double* source, double* per_element, double* totals, hipStream_t st) {
    const QuadPlan plan = quad_decide(Qd.d, Qd.e, Qd.p, Qd.Q, Qd.N);
    const size_t rows = (size_t)Qd.p * Qd.N, pts = (size_t)Qd.N * Qd.Q;
    Qd.z.upload(z, rows * ncol, st);
    if (minus) Qd.minus.upload(minus, pts * ncol * (kind == QUAD_W1P ? Qd.e : 1), st);
    if (kind == QUAD_ENERGY) Qd.source.upload(source, rows, st);
    Qd.elem.ensure((size_t)Qd.N * ncol);
    Qd.totals.ensure((size_t)ncol);
    QuadParams P{};
    P.x = Qd.x.p; P.wref = Qd.wref.p; P.tab = Qd.tab.p; P.z = Qd.z.p;
    P.minus = minus ? Qd.minus.p : nullptr;
    P.source = kind == QUAD_ENERGY ? Qd.source.p : nullptr;
    P.elem = Qd.elem.p;
    P.N = Qd.N; P.p = Qd.p; P.Q = Qd.Q; P.ncol = ncol; P.S = plan.S; P.G = plan.G;
    P.is_max = is_max ? 1 : 0;
    P.pmode = quad_pmode(pexp);
    P.pexp = pexp;
    Qd.ev.begin(st);
    dispatch_dims(Qd.d, Qd.e, [&](auto D, auto E) { launch_quad_kind<decltype(D)::value, decltype(E)::value>(kind, P, plan, st); });
    Qd.ev.mark(1, st);
    quad_reduce_columns(Qd.elem.p, Qd.N, ncol, is_max, Qd.totals.p, st);
    Qd.ev.mark(2, st);
    Qd.totals.download(totals, (size_t)ncol, st);
    if (per_element) Qd.elem.download(per_element, (size_t)Qd.N * ncol, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    Qd.ev.timed = true;
}

void quadrature_times(const Quadrature& Qd, double* ms) {
    if (!Qd.ev.timed) throw InvalidArgument("quadrature: no integrate call has completed yet");
    for (int i = 0; i < 2; ++i) ms[i] = Qd.ev.ms(i);
}

}  // namespace mgbhip
