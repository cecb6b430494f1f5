// residual.hip -- the element-interior residual of the p-Laplace equation (mgbhip_residual_*): the strong residual
// r = f + div a(grad u), a(g) = |g|^(p-2) g, at the points of a rule, and h_K^2 int_K r^2 per element and in total: the
// half of the residual a-posteriori estimator that the face jumps of faces.hip leave out.
//
// The host hands over a rule and the basis with its first and second reference derivatives at the rule's points (phi,
// dphi, d2phi), so nothing here knows an element family.  Flat meshes, d = e = 2 or 3.  One lane takes one (element,
// point) pair, exactly as in quadrature.hip; at point q of an element with nodes x_i and values z_i, with m running over
// the index pairs (b, c), b <= c, in the tables' order,
//   J = sum_i x_i (grad_xi phi_i)^T,   C = cof J (J^-T = C / det J),   measure = w_q det J,
//   Hx_a[m] = sum_i (x_i)_a d2phi_i[m],   Hz[m] = sum_i z_i d2phi_i[m],   xi = sum_i z_i grad_xi phi_i,
//   g = grad u = C xi / det J,   M = Hz - sum_a g_a Hx_a   (the physical Hessian is H = J^-T M J^-1, curved maps included),
//   tr H = sum_bc M_bc (J^T J)^-1_bc,   g^T H g = v^T M v with v = J^-1 g = C^T g / det J,
//   div a = |g|^(p-2) (tr H + (p - 2) g^T H g / |g|^2);   p = 2: tr H (no pow, no division);   g = 0, p != 2: 0.
// H itself is never formed: its trace and the one quadratic form are all div a needs, so a lane holds C (d^2), the Hx_a
// (d d (d + 1) / 2) and (J^T J)^-1 (d (d + 1) / 2) per point, and xi, Hz, g, M and v per column.  Every sum over the
// nodes is a chain of fused multiply-adds in node order.  The geometry of a point (C, det J, Hx, (J^T J)^-1, f_q) is
// formed once and reused across the columns where Q <= 256.
//
// Summation order.  No atomics.  The lane plan, the lanes' own sums, the halving tree, the write-out and the column
// reduction are quadrature.hip's (quad_layout.hpp, quad_device.hpp): an element's value depends on Q alone, not on N, on
// the number of columns or on its place in the workgroup, and the totals are reproducible bit for bit.  The first lane
// of an element multiplies its sum by h_K^2 before the write-out, h_K = |K|^(1/d), |K| the sum of the element's
// measures in point order.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "device_prims.hpp"
#include "quad_device.hpp"
#include "residual.hpp"

namespace mgbhip {

namespace {

struct ResParams {
    const double* x;         // (p N) x d
    const double* wref;      // Q
    const double* tab;       // [p][1 + d + d (d + 1) / 2][Q]
    const double* sizes;     // N: h_K
    const double* z;         // (p N) x ncol
    const double* source;    // p N: f in the element space, or null
    const double* fpts;      // N x Q: f at the points, or null (one of the two is given)
    double* out;             // N x ncol (the element values) or N x Q x ncol (POINTWISE)
    int64_t N;
    int32_t p, Q, ncol, S, G;
    int32_t pmode;           // 1: p = 1, 2: p = 2 (neither calls pow), 0: any other exponent
    double pexp;
};

template <int D>
struct ResGeo {
    static constexpr int M = D * (D + 1) / 2;
    double C[D][D];          // the cofactors of J = dx / dxi: J^-T = C / det J
    double Hx[D][M];         // the second reference derivatives of the map, one row per coordinate
    double Gi[M];            // (J^T J)^-1 in the tables' order, the off-diagonal entries doubled
    double det, rdet;        // det J and its reciprocal
};

// the cofactors and the determinant of J; no contraction, so that every kernel here forms the same det J bit for bit
template <int D>
__device__ __forceinline__ double res_cofactors(const double (&J)[D][D], double (&C)[D][D]) {
#pragma clang fp contract(off)
    if constexpr (D == 2) {
        C[0][0] = J[1][1];
        C[0][1] = -J[1][0];
        C[1][0] = -J[0][1];
        C[1][1] = J[0][0];
        return J[0][0] * J[1][1] - J[0][1] * J[1][0];
    } else {
        C[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        C[0][1] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        C[0][2] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        C[1][0] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
        C[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
        C[1][2] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
        C[2][0] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
        C[2][1] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
        C[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        return (J[0][0] * C[0][0] + J[0][1] * C[0][1]) + J[0][2] * C[0][2];
    }
}

// The geometry of point q of the element whose nodes are xe [p][D].
template <int D>
__device__ __forceinline__ void res_geo(const double* xe, const double* tab, int p, int Q, int q, ResGeo<D>& geo) {
    constexpr int M = ResGeo<D>::M, R = 1 + D + M;
    double J[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
#pragma unroll
        for (int b = 0; b < D; ++b) J[a][b] = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) geo.Hx[a][m] = 0.0;
    }
    for (int i = 0; i < p; ++i) {
        const double* t = tab + (size_t)i * R * Q + q;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const double xa = xe[i * D + a];
#pragma unroll
            for (int b = 0; b < D; ++b) J[a][b] = __builtin_fma(t[(size_t)(1 + b) * Q], xa, J[a][b]);
#pragma unroll
            for (int m = 0; m < M; ++m) geo.Hx[a][m] = __builtin_fma(t[(size_t)(1 + D + m) * Q], xa, geo.Hx[a][m]);
        }
    }
    geo.det = res_cofactors<D>(J, geo.C);
    geo.rdet = 1.0 / geo.det;
    int m = 0;
#pragma unroll
    for (int b = 0; b < D; ++b)
#pragma unroll
        for (int c = b; c < D; ++c) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) s = __builtin_fma(geo.C[a][b], geo.C[a][c], s);
            s = (s * geo.rdet) * geo.rdet;
            geo.Gi[m++] = b == c ? s : 2.0 * s;
        }
}

// div a(grad u) at the point, for the column whose nodal values are zc[i * QUAD_CHUNK]
template <int D>
__device__ __forceinline__ double res_diva(const ResGeo<D>& geo, const double* zc, const double* tab, int p, int Q, int q, int pmode,
                                           double pexp) {
    constexpr int M = ResGeo<D>::M, R = 1 + D + M;
    double xi[D], Hz[M];
#pragma unroll
    for (int b = 0; b < D; ++b) xi[b] = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) Hz[m] = 0.0;
    for (int i = 0; i < p; ++i) {
        const double* t = tab + (size_t)i * R * Q + q;
        const double zi = zc[i * QUAD_CHUNK];
#pragma unroll
        for (int b = 0; b < D; ++b) xi[b] = __builtin_fma(t[(size_t)(1 + b) * Q], zi, xi[b]);
#pragma unroll
        for (int m = 0; m < M; ++m) Hz[m] = __builtin_fma(t[(size_t)(1 + D + m) * Q], zi, Hz[m]);
    }
    double g[D], s2 = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < D; ++b) s = __builtin_fma(geo.C[a][b], xi[b], s);
        g[a] = s * geo.rdet;
        s2 = __builtin_fma(g[a], g[a], s2);
    }
    double tr = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double t = Hz[m];
#pragma unroll
        for (int a = 0; a < D; ++a) t = __builtin_fma(-g[a], geo.Hx[a][m], t);
        Hz[m] = t;                                  // M = Hz - sum_a g_a Hx_a
        tr = __builtin_fma(geo.Gi[m], t, tr);
    }
    if (pmode == 2) return tr;
    if (s2 == 0.0) return 0.0;                      // a(0) = 0 for every p >= 1, the convention of the flux in faces.hip
    double v[D];
#pragma unroll
    for (int b = 0; b < D; ++b) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) s = __builtin_fma(geo.C[a][b], g[a], s);
        v[b] = s * geo.rdet;
    }
    double gHg = 0.0;
    int m = 0;
#pragma unroll
    for (int b = 0; b < D; ++b)
#pragma unroll
        for (int c = b; c < D; ++c) {
            const double vv = v[b] * v[c];
            gHg = __builtin_fma(b == c ? vv : 2.0 * vv, Hz[m++], gHg);
        }
    const double t = tr + (pexp - 2.0) * (gHg / s2);
    return pmode == 1 ? t / sqrt(s2) : pow(s2, 0.5 * (pexp - 2.0)) * t;
}

template <int D, bool POINTWISE, bool TAB_LDS>
__global__ __launch_bounds__(QUAD_THREADS) void residual_kernel(const ResParams P) {
    extern __shared__ __attribute__((aligned(16))) double res_lds[];
    constexpr int R = residual_rows(D);
    const int tid = threadIdx.x, p = P.p, Q = P.Q, S = P.S, G = P.G, ncol = P.ncol;
    double* xs = res_lds;
    double* zs = xs + quad_lds_xs(G, p, D);
    double* fs = zs + quad_lds_zs(G, p);
    double* red = fs + quad_lds_fs(G, p);
    const double* tab = P.tab;
    if constexpr (TAB_LDS) {
        double* tl = red + quad_lds_red();
        const int n = R * Q * p;
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
        for (int i = tid; i < rows * D; i += QUAD_THREADS) xs[i] = P.x[el0 * p * D + i];
        if (P.source)
            for (int i = tid; i < rows; i += QUAD_THREADS) fs[i] = P.source[el0 * p + i];
        const bool active = g < nel;
        const int64_t el = el0 + g;
        const double* xe = xs + g * p * D;
        ResGeo<D> geo;
        double w = 0.0, f = 0.0, h2 = 0.0;
        bool have_geo = false;
        if constexpr (!POINTWISE)
            if (active) {
                const double hK = P.sizes[el];
                h2 = hK * hK;
            }
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
                    const int64_t pt = el * Q + q;
                    if (!(single && have_geo)) {
                        res_geo<D>(xe, tab, p, Q, q, geo);
                        w = P.wref[q] * geo.det;
                        if (P.fpts) {
                            f = P.fpts[pt];
                        } else {
                            f = 0.0;
                            for (int i = 0; i < p; ++i) f = __builtin_fma(tab[(size_t)i * R * Q + q], fs[g * p + i], f);
                        }
                    }
                    have_geo = true;
                    for (int c = 0; c < nc; ++c) {
                        const double r = f + res_diva<D>(geo, zs + g * p * QUAD_CHUNK + c, tab, p, Q, q, P.pmode, P.pexp);
                        if constexpr (POINTWISE) {
                            P.out[pt * ncol + c0 + c] = r;
                        } else {
                            const double term = w * (r * r);
                            double* rr = red + c * QUAD_THREADS + tid;
                            *rr = first ? term : *rr + term;
                        }
                    }
                    first = false;
                }
            }
            if constexpr (POINTWISE) {
                __syncthreads();                    // the next chunk overwrites zs
            } else {
                for (int off = tree >> 1; off > 0; off >>= 1) {         // the halving tree of quad_kernel, without the max
                    __syncthreads();
                    if (active && s < off && s + off < S) {
                        for (int c = 0; c < nc; ++c) {
                            double* rr = red + c * QUAD_THREADS + tid;
                            *rr = rr[0] + rr[off];
                        }
                    }
                }
                if (active && s == 0)               // the lane that holds the element's sum (it made the tree's last step)
                    for (int c = 0; c < nc; ++c) red[c * QUAD_THREADS + tid] *= h2;
                __syncthreads();
                quad_write_items(P.out, red, tid, el0, nel, S, ncol, c0, nc);
            }
        }
    }
}

// points (N x Q x d) and measures (N x Q) of the rule on the mesh; points may be null
template <int D>
__global__ __launch_bounds__(QUAD_THREADS) void residual_geometry_kernel(const double* __restrict__ x, const double* __restrict__ wref,
                                                                         const double* __restrict__ tab, int64_t N, int p, int Q,
                                                                         double* __restrict__ points, double* __restrict__ weights) {
    constexpr int R = residual_rows(D);
    const int64_t idx = (int64_t)blockIdx.x * QUAD_THREADS + threadIdx.x;
    if (idx >= N * Q) return;
    const int64_t el = idx / Q;
    const int q = (int)(idx - el * Q);
    const double* xe = x + el * p * D;
    double J[D][D], C[D][D], xq[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        xq[a] = 0.0;
#pragma unroll
        for (int b = 0; b < D; ++b) J[a][b] = 0.0;
    }
    for (int i = 0; i < p; ++i) {
        const double* t = tab + (size_t)i * R * Q + q;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const double xa = xe[i * D + a];
            xq[a] = __builtin_fma(t[0], xa, xq[a]);
#pragma unroll
            for (int b = 0; b < D; ++b) J[a][b] = __builtin_fma(t[(size_t)(1 + b) * Q], xa, J[a][b]);
        }
    }
    const double det = res_cofactors<D>(J, C);
    if (points) {
#pragma unroll
        for (int a = 0; a < D; ++a) points[idx * D + a] = xq[a];
    }
    weights[idx] = wref[q] * det;
}

// sizes[e] = |K|^(1/d), |K| the sum of the element's Q measures in point order; bad[e] = 1 where a measure is not positive
// and finite (the reference weights are positive, so that is det J)
__global__ __launch_bounds__(BLOCK) void residual_size_kernel(const double* __restrict__ weights, int64_t N, int Q, int d,
                                                              double* __restrict__ sizes, int32_t* __restrict__ bad) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    double s = 0.0;
    int32_t b = 0;
    for (int q = 0; q < Q; ++q) {
        const double w = weights[e * Q + q];
        if (!(w > 0.0) || w > 1.79e308) b = 1;
        s += w;
    }
    sizes[e] = d == 2 ? sqrt(s) : cbrt(s);
    bad[e] = b;
}

template <int D, bool POINTWISE>
void launch_residual(const ResParams& P, const QuadPlan& plan, hipStream_t st) {
    if (plan.tables_lds) quad_launch<residual_kernel<D, POINTWISE, true>>("residual", P, plan, st);
    else quad_launch<residual_kernel<D, POINTWISE, false>>("residual", P, plan, st);
}

void launch_geometry(Residual& Rd, double* points, double* weights, hipStream_t st) {
    const int64_t n = Rd.N * Rd.Q;
    const dim3 grid((unsigned)((n + QUAD_THREADS - 1) / QUAD_THREADS));
    if (Rd.d == 2)
        hipLaunchKernelGGL((residual_geometry_kernel<2>), grid, dim3(QUAD_THREADS), 0, st, Rd.x.p, Rd.wref.p, Rd.tab.p, Rd.N, Rd.p, Rd.Q,
                           points, weights);
    else
        hipLaunchKernelGGL((residual_geometry_kernel<3>), grid, dim3(QUAD_THREADS), 0, st, Rd.x.p, Rd.wref.p, Rd.tab.p, Rd.N, Rd.p, Rd.Q,
                           points, weights);
    MGB_HIP_CHECK(hipGetLastError());
}

// the element kernel of a call into Rd.out; z and the source are uploaded here
void run_residual(Residual& Rd, bool pointwise, double pexp, int32_t ncol, const double* z, const double* source, bool at_points,
                  hipStream_t st) {
    const QuadPlan plan = residual_decide(Rd.d, Rd.p, Rd.Q, Rd.N);
    const size_t rows = (size_t)Rd.p * Rd.N, pts = (size_t)Rd.N * Rd.Q;
    Rd.z.upload(z, rows * ncol, st);
    Rd.source.upload(source, at_points ? pts : rows, st);
    Rd.out.ensure(pointwise ? pts * ncol : (size_t)Rd.N * ncol);
    ResParams P{};
    P.x = Rd.x.p; P.wref = Rd.wref.p; P.tab = Rd.tab.p; P.sizes = Rd.sizes.p; P.z = Rd.z.p;
    P.source = at_points ? nullptr : Rd.source.p;
    P.fpts = at_points ? Rd.source.p : nullptr;
    P.out = Rd.out.p;
    P.N = Rd.N; P.p = Rd.p; P.Q = Rd.Q; P.ncol = ncol; P.S = plan.S; P.G = plan.G;
    P.pmode = quad_pmode(pexp);
    P.pexp = pexp;
    Rd.ev.begin(st);
    if (Rd.d == 2) {
        if (pointwise) launch_residual<2, true>(P, plan, st);
        else launch_residual<2, false>(P, plan, st);
    } else {
        if (pointwise) launch_residual<3, true>(P, plan, st);
        else launch_residual<3, false>(P, plan, st);
    }
    Rd.ev.mark(1, st);
}

}  // namespace

void residual_build(Residual& Rd, int32_t d, int32_t p, int64_t N, const double* x, int32_t Q, const double* wref,
                    const double* phi, const double* dphi, const double* d2phi, hipStream_t st) {
    Rd.d = d; Rd.p = p; Rd.Q = Q; Rd.N = N;
    const int M = d * (d + 1) / 2, R = residual_rows(d);
    std::vector<double> tab((size_t)R * Q * p);
    for (int q = 0; q < Q; ++q)
        for (int i = 0; i < p; ++i) {
            const size_t src = (size_t)q * p + i;
            tab[((size_t)i * R) * Q + q] = phi[src];
            for (int b = 0; b < d; ++b) tab[((size_t)i * R + 1 + b) * Q + q] = dphi[src * d + b];
            for (int m = 0; m < M; ++m) tab[((size_t)i * R + 1 + d + m) * Q + q] = d2phi[src * M + m];
        }
    Rd.x.upload(x, (size_t)p * N * d, st);
    Rd.wref.upload(wref, (size_t)Q, st);
    Rd.tab.upload(tab, st);
    // the measures, and from them the element sizes and the sign of det J at every point
    Rd.geo.ensure((size_t)N * Q * (d + 1));
    Rd.sizes.alloc((size_t)N);
    DevBuf<int32_t> bad;
    bad.alloc((size_t)N);
    launch_geometry(Rd, nullptr, Rd.geo.p, st);
    hipLaunchKernelGGL(residual_size_kernel, dim3(grid_1d(N)), dim3(BLOCK), 0, st, Rd.geo.p, N, (int)Q, (int)d, Rd.sizes.p, bad.p);
    MGB_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> hb((size_t)N);
    bad.download(hb.data(), (size_t)N, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));       // tab, bad are locals
    for (int64_t e = 0; e < N; ++e)
        if (hb[(size_t)e])
            throw InvalidArgument("residual: det J is not positive and finite at a point of element " + std::to_string(e));
}

void residual_geometry(Residual& Rd, double* points, double* weights, double* sizes, hipStream_t st) {
    const int64_t n = Rd.N * Rd.Q;
    if (points || weights) {
        Rd.geo.ensure((size_t)n * (Rd.d + 1));
        double* dw = Rd.geo.p;
        double* dpts = points ? Rd.geo.p + n : nullptr;
        launch_geometry(Rd, dpts, dw, st);
        if (points) MGB_HIP_CHECK(hipMemcpyAsync(points, dpts, (size_t)n * Rd.d * sizeof(double), hipMemcpyDeviceToHost, st));
        if (weights) MGB_HIP_CHECK(hipMemcpyAsync(weights, dw, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (sizes) Rd.sizes.download(sizes, (size_t)Rd.N, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void residual_pointwise(Residual& Rd, double pexp, int32_t ncol, const double* z, const double* source, bool at_points,
                        double* r, hipStream_t st) {
    run_residual(Rd, true, pexp, ncol, z, source, at_points, st);
    Rd.ev.mark(2, st);
    Rd.out.download(r, (size_t)Rd.N * Rd.Q * ncol, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    Rd.ev.timed = true;
}

void residual_integrate(Residual& Rd, double pexp, int32_t ncol, const double* z, const double* source, bool at_points,
                        double* per_element, double* totals, hipStream_t st) {
    Rd.totals.ensure((size_t)ncol);
    run_residual(Rd, false, pexp, ncol, z, source, at_points, st);
    quad_reduce_columns(Rd.out.p, Rd.N, ncol, false, Rd.totals.p, st);
    Rd.ev.mark(2, st);
    Rd.totals.download(totals, (size_t)ncol, st);
    if (per_element) Rd.out.download(per_element, (size_t)Rd.N * ncol, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    Rd.ev.timed = true;
}

void residual_times(const Residual& Rd, double* ms) {
    if (!Rd.ev.timed) throw InvalidArgument("residual: no pointwise or integrate call has completed yet");
    for (int i = 0; i < 2; ++i) ms[i] = Rd.ev.ms(i);
}

}  // namespace mgbhip
