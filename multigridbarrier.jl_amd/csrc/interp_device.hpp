// interp_device.hpp -- the device code that locates a point in a mesh and evaluates an element-space function there,
// shared by the translation units that do so: interpolate.hip (the fused query_* kernels and the locate_* / eval_* kernels
// of a point locator) and stream.hip (the field-line tracer, which calls locate and evaluate again at every stage).  One
// copy of each formula: both include this header, and both run the same operations on the same numbers.
//
// Everything here has internal linkage (the library is built without relocatable device code, so every translation unit
// carries its own copy of the device functions it calls).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cell_lists.hpp"         // Grid, cell_axis, BLOCK
#include "interpolate.hpp"

// No fused multiply-adds in the code below or in a file that includes it: see interpolate.hip.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

constexpr int NEWTON_MAXIT = 32;
constexpr int BISECT_MAXIT = 128;
constexpr double ACCEPT_TOL = 1e-11;       // containment tolerance in reference coordinates (at least)
constexpr double NEWTON_STEP_TOL = 1e-13;  // converged once max |dxi| falls below this (at least)
// Rounding level of a reference coordinate: x(xi) - q carries an error of about eps * max|x|, which moves xi by that
// much times |J^{-1}|.  On a small or far-translated element this exceeds the fixed tolerances above, so both the
// Newton stopping test and the containment test use max(fixed tolerance, ROUND_FACTOR * eps * max|x| * |J^{-1}|_inf).
constexpr double ROUND_FACTOR = 64.0;
constexpr double EPS = 2.220446049250313e-16;
constexpr double QK_BOX_PAD = 0.125;       // a curved Q_k image can leave its nodes' box: pad by 1/8 of the extent

__device__ inline double dnan() { return __builtin_nan(""); }

// cell of a point, or -1 if it is not finite or outside the grid box
template <int D>
__device__ inline int64_t point_cell(const Grid& g, const double* q) {
    for (int a = 0; a < D; ++a)
        if (!(q[a] >= g.lo[a] && q[a] <= g.hi[a])) return -1;     // also false for NaN; +-Inf is outside the box
    int64_t c = 0;
    for (int a = D - 1; a >= 0; --a) c = c * g.n[a] + cell_axis((q[a] - g.lo[a]) * g.inv[a], g.n[a]);
    return c;
}

// ---------------------------------------------------------------------------------------------------------------
// element maps
// ---------------------------------------------------------------------------------------------------------------

// 1-D Lagrange basis on S nodes, in the reference's operation order (src/TensorFEM.jl:162-176)
template <int S>
__device__ inline void lagrange(const double* nodes, double xv, double* L) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
        double num = 1.0, den = 1.0;
#pragma unroll
        for (int j = 0; j < S; ++j)
            if (i != j) {
                num *= xv - nodes[j];
                den *= nodes[i] - nodes[j];
            }
        L[i] = num / den;
    }
}

template <int S>
__device__ inline void lagrange_d(const double* nodes, double xv, double* L, double* dL) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
        double num = 1.0, den = 1.0, dnum = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j)
            if (i != j) {
                dnum = dnum * (xv - nodes[j]) + num;      // product rule, one factor at a time
                num *= xv - nodes[j];
                den *= nodes[i] - nodes[j];
            }
        L[i] = num / den;
        dL[i] = dnum / den;
    }
}

// L[j] of a runtime index j < S without indexing a register array at run time (which would put it in scratch)
template <int S>
__device__ inline double pick(const double (&L)[S], int j) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < S; ++i)
        if (i == j) v = L[i];
    return v;
}

// inverse Jacobian (adjugate / det); false if the determinant is zero or not finite
template <int D>
__device__ inline bool jac_inverse(const double (&J)[D][D], double (&Ji)[D][D]) {
    if constexpr (D == 2) {
        const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        if (!(det != 0.0) || !isfinite(det)) return false;
        Ji[0][0] = J[1][1] / det;
        Ji[0][1] = -J[0][1] / det;
        Ji[1][0] = -J[1][0] / det;
        Ji[1][1] = J[0][0] / det;
    } else {
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
        if (!(det != 0.0) || !isfinite(det)) return false;
        Ji[0][0] = c00 / det;
        Ji[1][0] = c01 / det;
        Ji[2][0] = c02 / det;
        Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det;
        Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det;
        Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) / det;
        Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) / det;
        Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
        Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) / det;
    }
    return true;
}

// Q_k element e: Newton on sum_i phi_i(xi) x_i = q from xi = 0; returns true (and the basis factors at xi) when it
// converges to a point of [-1, 1]^D within the containment tolerance; xi is that point.  Node lin = i0 + S i1 (+ S^2 i2),
// axis 0 fastest; axis 0 is unrolled, the outer axes are loops that pick their basis factor without run-time register
// indexing.
template <int D, int S>
__device__ bool qk_locate(const double* __restrict__ x, int64_t e, const double* nodes, const double* q,
                          double (&L)[D][S], double (&xi)[D]) {
    constexpr int P = D == 2 ? S * S : S * S * S;
    double dL[D][S];
    for (int a = 0; a < D; ++a) xi[a] = 0.0;
    const double* xe = x + e * P * D;
    bool conv = false;
    double xs = 0.0, tol = NEWTON_STEP_TOL;
    for (int a = 0; a < D; ++a) xs = fmax(xs, fabs(q[a]));
    for (int it = 0; it < NEWTON_MAXIT && !conv; ++it) {
#pragma unroll
        for (int a = 0; a < D; ++a) lagrange_d<S>(nodes, xi[a], L[a], dL[a]);
        double F[D], J[D][D];
        for (int a = 0; a < D; ++a) {
            F[a] = -q[a];
            for (int b = 0; b < D; ++b) J[a][b] = 0.0;
        }
        const int n2 = D == 3 ? S : 1;
#pragma unroll 1
        for (int i2 = 0; i2 < n2; ++i2) {
            double l2 = 1.0, d2 = 0.0;
            if constexpr (D == 3) {
                l2 = pick<S>(L[D - 1], i2);
                d2 = pick<S>(dL[D - 1], i2);
            }
#pragma unroll 1
            for (int i1 = 0; i1 < S; ++i1) {
                const double l1 = pick<S>(L[1], i1), d1 = pick<S>(dL[1], i1);
#pragma unroll
                for (int i0 = 0; i0 < S; ++i0) {
                    const int lin = i0 + S * i1 + S * S * i2;
                    double phi, dphi[D];
                    if constexpr (D == 2) {
                        phi = L[0][i0] * l1;
                        dphi[0] = dL[0][i0] * l1;
                        dphi[1] = L[0][i0] * d1;
                    } else {
                        phi = L[0][i0] * l1 * l2;
                        dphi[0] = dL[0][i0] * l1 * l2;
                        dphi[1] = L[0][i0] * d1 * l2;
                        dphi[D - 1] = L[0][i0] * l1 * d2;
                    }
                    for (int a = 0; a < D; ++a) {
                        const double xa = xe[lin * D + a];
                        if (it == 0) xs = fmax(xs, fabs(xa));
                        F[a] += phi * xa;
                        for (int b = 0; b < D; ++b) J[a][b] += dphi[b] * xa;
                    }
                }
            }
        }
        double Ji[D][D];
        if (!jac_inverse<D>(J, Ji)) return false;
        double step = 0.0, big = 0.0, ninv = 0.0;
        for (int a = 0; a < D; ++a) {
            double dx = 0.0, row = 0.0;
            for (int b = 0; b < D; ++b) {
                dx += Ji[a][b] * F[b];
                row += fabs(Ji[a][b]);
            }
            xi[a] -= dx;
            step = fmax(step, fabs(dx));
            big = fmax(big, fabs(xi[a]));
            ninv = fmax(ninv, row);
        }
        if (!(big <= 8.0)) return false;         // diverging (or NaN): not this element
        tol = fmax(NEWTON_STEP_TOL, ROUND_FACTOR * EPS * xs * ninv);
        conv = step <= tol;
    }
    if (!conv) return false;
    const double acc = fmax(ACCEPT_TOL, tol);
    for (int a = 0; a < D; ++a)
        if (!(fabs(xi[a]) <= 1.0 + acc)) return false;
#pragma unroll
    for (int a = 0; a < D; ++a) lagrange<S>(nodes, xi[a], L[a]);
    return true;
}

// P1 / P2: (l1, l2) with q = l1 c0 + l2 c1 + (1 - l1 - l2) c2 from the three corner slots
template <int FAM>
__device__ inline bool simplex_locate(const double* __restrict__ x, int64_t e, int32_t p, const double* q, double& l1,
                                      double& l2) {
    constexpr int s0 = 0, s1 = FAM == MGBHIP_INTERP_P1 ? 1 : 2, s2 = FAM == MGBHIP_INTERP_P1 ? 2 : 4;
    const double* xe = x + e * p * 2;
    const double ox = xe[2 * s2], oy = xe[2 * s2 + 1];
    const double ax = xe[2 * s0] - ox, ay = xe[2 * s0 + 1] - oy;
    const double bx = xe[2 * s1] - ox, by = xe[2 * s1 + 1] - oy;
    const double rx = q[0] - ox, ry = q[1] - oy;
    const double det = ax * by - ay * bx;
    if (!(det != 0.0)) return false;
    l1 = (rx * by - ry * bx) / det;
    l2 = (ax * ry - ay * rx) / det;
    // the differences above carry an error of about eps * max|x|, which the inverse map scales by |J^{-1}|_inf
    const double xs = fmax(fmax(fmax(fabs(ox), fabs(oy)), fmax(fabs(q[0]), fabs(q[1]))),
                           fmax(fmax(fabs(xe[2 * s0]), fabs(xe[2 * s0 + 1])), fmax(fabs(xe[2 * s1]), fabs(xe[2 * s1 + 1]))));
    const double ninv = fmax(fabs(by) + fabs(bx), fabs(ay) + fabs(ax)) / fabs(det);
    const double tol = fmax(ACCEPT_TOL, ROUND_FACTOR * EPS * xs * ninv);
    return l1 >= -tol && l2 >= -tol && 1.0 - l1 - l2 >= -tol;
}

// phi_j and its derivatives in l1 and l2 at (l1, l2) from the 10-monomial table, formed as simplex_evaluate forms them
__device__ inline void simplex_basis_d(const double* __restrict__ table, int j, const double (&mono)[10],
                                       const double (&m1)[10], const double (&m2)[10], double& v, double& v1, double& v2) {
    v = v1 = v2 = 0.0;
    for (int m = 0; m < 10; ++m) v += table[j * 10 + m] * mono[m];
    for (int m = 1; m < 10; ++m) {
        v1 += table[j * 10 + m] * m1[m];
        v2 += table[j * 10 + m] * m2[m];
    }
}

// Curved (isoparametric) P2 element e: Newton on sum_j phi_j(l1, l2) x_j = q over all p nodes, started from the affine
// barycentric pair of the three corner slots (what simplex_locate computes; (1/3, 1/3) if those corners are collinear).
// Stopping and acceptance are those of qk_locate: the step tolerance follows the rounding level of the element, the
// iteration gives up on |l| > 8, on a non-finite value or after NEWTON_MAXIT steps, and the pair is accepted when l1, l2
// and 1 - l1 - l2 are >= -max(ACCEPT_TOL, tol).  l1, l2 are the pair the basis is then evaluated at.
__device__ inline bool p2c_locate(const double* __restrict__ x, int64_t e, int32_t p, const double* __restrict__ table,
                                  const double* q, double& l1, double& l2) {
    constexpr int PMAX = 7;
    const double* xe = x + e * p * 2;
    {
        const double ox = xe[8], oy = xe[9];
        const double ax = xe[0] - ox, ay = xe[1] - oy;
        const double bx = xe[4] - ox, by = xe[5] - oy;
        const double rx = q[0] - ox, ry = q[1] - oy;
        const double det = ax * by - ay * bx;
        if (det != 0.0) {
            l1 = (rx * by - ry * bx) / det;
            l2 = (ax * ry - ay * rx) / det;
        } else {
            l1 = l2 = 1.0 / 3.0;
        }
    }
    bool conv = false;
    double xs = fmax(fabs(q[0]), fabs(q[1])), tol = NEWTON_STEP_TOL;
    for (int it = 0; it < NEWTON_MAXIT && !conv; ++it) {
        const double mono[10] = {1.0, l1, l2, l1 * l1, l1 * l2, l2 * l2, l1 * l1 * l1, l1 * l1 * l2, l1 * l2 * l2, l2 * l2 * l2};
        const double m1[10] = {0.0, 1.0, 0.0, 2 * l1, l2, 0.0, 3 * (l1 * l1), 2 * (l1 * l2), l2 * l2, 0.0};
        const double m2[10] = {0.0, 0.0, 1.0, 0.0, l1, 2 * l2, 0.0, l1 * l1, 2 * (l1 * l2), 3 * (l2 * l2)};
        double F[2] = {-q[0], -q[1]}, J[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        for (int j = 0; j < PMAX; ++j)
            if (j < p) {
                double v, v1, v2;
                simplex_basis_d(table, j, mono, m1, m2, v, v1, v2);
                for (int a = 0; a < 2; ++a) {
                    const double xa = xe[2 * j + a];
                    if (it == 0) xs = fmax(xs, fabs(xa));
                    F[a] += v * xa;
                    J[a][0] += v1 * xa;
                    J[a][1] += v2 * xa;
                }
            }
        double Ji[2][2];
        if (!jac_inverse<2>(J, Ji)) return false;
        const double d1 = Ji[0][0] * F[0] + Ji[0][1] * F[1], d2 = Ji[1][0] * F[0] + Ji[1][1] * F[1];
        l1 -= d1;
        l2 -= d2;
        const double step = fmax(fabs(d1), fabs(d2)), big = fmax(fabs(l1), fabs(l2));
        const double ninv = fmax(fabs(Ji[0][0]) + fabs(Ji[0][1]), fabs(Ji[1][0]) + fabs(Ji[1][1]));
        if (!(big <= 8.0)) return false;         // diverging (or NaN): not this element
        tol = fmax(NEWTON_STEP_TOL, ROUND_FACTOR * EPS * xs * ninv);
        conv = step <= tol;
    }
    if (!conv) return false;
    const double acc = fmax(ACCEPT_TOL, tol);
    return l1 >= -acc && l2 >= -acc && 1.0 - l1 - l2 >= -acc;
}

// ---------------------------------------------------------------------------------------------------------------
// locate and evaluate: one lane per point
// ---------------------------------------------------------------------------------------------------------------

struct QueryArgs {
    int64_t M;
    int32_t p, ncomp;
    const double* x;
    const double* table;
    const double* z;
    const double* pts;
    const int32_t* start;
    const int32_t* cand;
    const double* box;         // 2-D / 3-D FEM: the padded element boxes (lo then hi per element)
    const int32_t* order;      // located families: the point processed by lane i (points sorted by cell)
    double* out;
    double* grad;              // M x ncomp x D (GRAD kernels only)
    int32_t* elem;
};

// Q_k locate: the lowest-index candidate of the point's cell whose element map inverts to a point of the reference
// cube; on success L holds the basis factors at xi (as qk_locate leaves them) and nodes the reference nodes of the
// table.  -1: no element.
template <int D, int S>
__device__ inline int64_t qk_find(const QueryArgs& a, const Grid& g, const double (&pt)[D], double (&nodes)[S],
                                  double (&L)[D][S], double (&xi)[D]) {
    const int64_t cell = point_cell<D>(g, pt);
    if (cell < 0) return -1;
    for (int j = 0; j < S; ++j) nodes[j] = a.table[j];
    const int32_t j1 = a.start[cell + 1];
    for (int32_t j = a.start[cell]; j < j1; ++j) {
        const int64_t e = a.cand[j];
        bool inbox = true;             // a point outside the element's padded box is not in the element: skip Newton
        for (int d = 0; d < D; ++d)
            inbox = inbox && pt[d] >= a.box[e * 2 * D + d] && pt[d] <= a.box[e * 2 * D + D + d];
        if (inbox && qk_locate<D, S>(a.x, e, nodes, pt, L, xi)) return e;
    }
    return -1;
}

// Q_k evaluate at xi of element `found`; L holds lagrange<S>(nodes, xi[d]) on entry.  False (nothing written) when the
// Jacobian at xi cannot be inverted (GRAD only).
// GRAD: the Jacobian J[a][b] = sum_i dphi_i/dxi_b x_i[a] at the located xi in one pass over the element's nodes,
// then per component gxi[b] = sum_i dphi_i/dxi_b z_i next to the value sum and grad = J^{-T} gxi.  The live state
// is that of a Newton step (L, dL, a D x D matrix, D sums), so no variant needs more registers than qk_locate.
template <int D, int S, bool GRAD>
__device__ inline bool qk_evaluate(const QueryArgs& a, int64_t q, int64_t found, const double (&nodes)[S],
                                   double (&L)[D][S], const double (&xi)[D]) {
    constexpr int P = D == 2 ? S * S : S * S * S;
    const int n2 = D == 3 ? S : 1;
    double dL[GRAD ? D : 1][S], Ji[D][D];
    if constexpr (GRAD) {
#pragma unroll
        for (int d = 0; d < D; ++d) lagrange_d<S>(nodes, xi[d], L[d], dL[d]);
        double J[D][D];
        for (int r = 0; r < D; ++r)
            for (int b = 0; b < D; ++b) J[r][b] = 0.0;
        const double* xe = a.x + found * P * D;
#pragma unroll 1
        for (int i2 = 0; i2 < n2; ++i2) {
            double l2 = 1.0, d2 = 0.0;
            if constexpr (D == 3) {
                l2 = pick<S>(L[D - 1], i2);
                d2 = pick<S>(dL[D - 1], i2);
            }
#pragma unroll 1
            for (int i1 = 0; i1 < S; ++i1) {
                const double l1 = pick<S>(L[1], i1), d1 = pick<S>(dL[1], i1);
#pragma unroll
                for (int i0 = 0; i0 < S; ++i0) {
                    const int lin = i0 + S * i1 + S * S * i2;
                    double dphi[D];
                    if constexpr (D == 2) {
                        dphi[0] = dL[0][i0] * l1;
                        dphi[1] = L[0][i0] * d1;
                    } else {
                        dphi[0] = dL[0][i0] * l1 * l2;
                        dphi[1] = L[0][i0] * d1 * l2;
                        dphi[D - 1] = L[0][i0] * l1 * d2;
                    }
                    for (int r = 0; r < D; ++r)
                        for (int b = 0; b < D; ++b) J[r][b] += dphi[b] * xe[lin * D + r];
                }
            }
        }
        if (!jac_inverse<D>(J, Ji)) return false;
    }
    const double* ze = a.z + found * P * a.ncomp;
    for (int c = 0; c < a.ncomp; ++c) {
        double v = 0.0, gxi[D];
        for (int b = 0; b < D; ++b) gxi[b] = 0.0;
#pragma unroll 1
        for (int i2 = 0; i2 < n2; ++i2) {
            const double l2 = D == 3 ? pick<S>(L[D - 1], i2) : 1.0;
            double d2 = 0.0;
            if constexpr (GRAD && D == 3) d2 = pick<S>(dL[D - 1], i2);
#pragma unroll 1
            for (int i1 = 0; i1 < S; ++i1) {
                const double l1 = pick<S>(L[1], i1);
                double d1 = 0.0;
                if constexpr (GRAD) d1 = pick<S>(dL[1], i1);
#pragma unroll
                for (int i0 = 0; i0 < S; ++i0) {
                    const int lin = i0 + S * i1 + S * S * i2;
                    const double phi = D == 2 ? L[0][i0] * l1 : L[0][i0] * l1 * l2;
                    const double zv = ze[lin * a.ncomp + c];
                    v += phi * zv;
                    if constexpr (GRAD) {
                        if constexpr (D == 2) {
                            gxi[0] += dL[0][i0] * l1 * zv;
                            gxi[1] += L[0][i0] * d1 * zv;
                        } else {
                            gxi[0] += dL[0][i0] * l1 * l2 * zv;
                            gxi[1] += L[0][i0] * d1 * l2 * zv;
                            gxi[D - 1] += L[0][i0] * l1 * d2 * zv;
                        }
                    }
                }
            }
        }
        a.out[q * a.ncomp + c] = v;
        if constexpr (GRAD)
            for (int r = 0; r < D; ++r) {
                double s = 0.0;
                for (int b = 0; b < D; ++b) s += Ji[b][r] * gxi[b];
                a.grad[(q * a.ncomp + c) * D + r] = s;
            }
    }
    return true;
}

// P1 / P2 locate: the lowest-index candidate of the point's cell that contains it, with its barycentric pair.  Curved
// P2 (P2C) is located like Q_k: the padded-box test, then Newton on the element map.
template <int FAM>
__device__ inline int64_t simplex_find(const QueryArgs& a, const Grid& g, const double (&pt)[2], double& l1, double& l2) {
    const int64_t cell = point_cell<2>(g, pt);
    if (cell < 0) return -1;
    const int32_t j1 = a.start[cell + 1];
    for (int32_t j = a.start[cell]; j < j1; ++j) {
        const int64_t e = a.cand[j];
        if constexpr (FAM == MGBHIP_INTERP_P2C) {
            bool inbox = true;         // a point outside the element's padded box is not in the element: skip Newton
            for (int d = 0; d < 2; ++d) inbox = inbox && pt[d] >= a.box[e * 4 + d] && pt[d] <= a.box[e * 4 + 2 + d];
            if (inbox && p2c_locate(a.x, e, a.p, a.table, pt, l1, l2)) return e;
        } else {
            if (simplex_locate<FAM>(a.x, e, a.p, pt, l1, l2)) return e;
        }
    }
    return -1;
}

// P2C with the gradient: the basis and its two derivatives once, the Jacobian from all p nodes, then per component the
// value (the sum of simplex_evaluate, term for term) next to du/dl1, du/dl2 and grad = J^{-T} (du/dl1, du/dl2).
__device__ inline bool p2c_evaluate_grad(const QueryArgs& a, int64_t q, int64_t found, double l1, double l2) {
    const double mono[10] = {1.0, l1, l2, l1 * l1, l1 * l2, l2 * l2, l1 * l1 * l1, l1 * l1 * l2, l1 * l2 * l2, l2 * l2 * l2};
    const double m1[10] = {0.0, 1.0, 0.0, 2 * l1, l2, 0.0, 3 * (l1 * l1), 2 * (l1 * l2), l2 * l2, 0.0};
    const double m2[10] = {0.0, 0.0, 1.0, 0.0, l1, 2 * l2, 0.0, l1 * l1, 2 * (l1 * l2), 3 * (l2 * l2)};
    constexpr int PMAX = 7;
    double phi[PMAX], p1[PMAX], p2[PMAX], J[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, Ji[2][2];
    const double* xe = a.x + found * a.p * 2;
    for (int j = 0; j < PMAX; ++j) {
        phi[j] = p1[j] = p2[j] = 0.0;
        if (j < a.p) {
            simplex_basis_d(a.table, j, mono, m1, m2, phi[j], p1[j], p2[j]);
            for (int r = 0; r < 2; ++r) {
                J[r][0] += p1[j] * xe[2 * j + r];
                J[r][1] += p2[j] * xe[2 * j + r];
            }
        }
    }
    if (!jac_inverse<2>(J, Ji)) return false;
    const double* ze = a.z + found * a.p * a.ncomp;
    for (int c = 0; c < a.ncomp; ++c) {
        double v = 0.0, g1 = 0.0, g2 = 0.0;
        for (int j = 0; j < PMAX; ++j)
            if (j < a.p) {
                const double zv = ze[j * a.ncomp + c];
                v += phi[j] * zv;
                g1 += p1[j] * zv;
                g2 += p2[j] * zv;
            }
        a.out[q * a.ncomp + c] = v;
        a.grad[(q * a.ncomp + c) * 2] = Ji[0][0] * g1 + Ji[1][0] * g2;
        a.grad[(q * a.ncomp + c) * 2 + 1] = Ji[0][1] * g1 + Ji[1][1] * g2;
    }
    return true;
}

// P1 / P2 / P2C evaluate at (l1, l2) of element `found`.  False (nothing written) when the Jacobian there cannot be
// inverted: only P2C with GRAD, whose map is not affine: J[a][b] = sum_j dphi_j/dl_b x_j[a] from all p nodes at the
// located pair, and grad = J^{-T} (du/dl1, du/dl2).  The values are the same sums in the same order for every family.
template <int FAM, bool GRAD>
__device__ inline bool simplex_evaluate(const QueryArgs& a, int64_t q, int64_t found, double l1, double l2) {
    if constexpr (FAM == MGBHIP_INTERP_P2C && GRAD) return p2c_evaluate_grad(a, q, found, l1, l2);
    const double mono[10] = {1.0, l1, l2, l1 * l1, l1 * l2, l2 * l2, l1 * l1 * l1, l1 * l1 * l2, l1 * l2 * l2, l2 * l2 * l2};
    constexpr int PMAX = 7;
    double phi[PMAX];
    for (int j = 0; j < PMAX; ++j) {
        double v = 0.0;
        if (j < a.p)
            for (int m = 0; m < 10; ++m) v += a.table[j * 10 + m] * mono[m];
        phi[j] = v;
    }
    const double* ze = a.z + found * a.p * a.ncomp;
    for (int c = 0; c < a.ncomp; ++c) {
        double v = 0.0;
        for (int j = 0; j < PMAX; ++j)
            if (j < a.p) v += phi[j] * ze[j * a.ncomp + c];
        a.out[q * a.ncomp + c] = v;
    }
    if constexpr (GRAD) {
        // the ten monomials differentiated in l1 and l2; x = c2 + l1 (c0 - c2) + l2 (c1 - c2), so with the edge vectors
        // ea, eb of simplex_locate the gradient is [ea eb]^{-T} (du/dl1, du/dl2)
        const double m1[10] = {0.0, 1.0, 0.0, 2 * l1, l2, 0.0, 3 * (l1 * l1), 2 * (l1 * l2), l2 * l2, 0.0};
        const double m2[10] = {0.0, 0.0, 1.0, 0.0, l1, 2 * l2, 0.0, l1 * l1, 2 * (l1 * l2), 3 * (l2 * l2)};
        double p1[PMAX], p2[PMAX];
        for (int j = 0; j < PMAX; ++j) {
            double v1 = 0.0, v2 = 0.0;
            if (j < a.p)
                for (int m = 1; m < 10; ++m) {
                    v1 += a.table[j * 10 + m] * m1[m];
                    v2 += a.table[j * 10 + m] * m2[m];
                }
            p1[j] = v1;
            p2[j] = v2;
        }
        constexpr int s0 = 0, s1 = FAM == MGBHIP_INTERP_P1 ? 1 : 2, s2 = FAM == MGBHIP_INTERP_P1 ? 2 : 4;
        const double* xe = a.x + found * a.p * 2;
        const double ox = xe[2 * s2], oy = xe[2 * s2 + 1];
        const double ax = xe[2 * s0] - ox, ay = xe[2 * s0 + 1] - oy;
        const double bx = xe[2 * s1] - ox, by = xe[2 * s1 + 1] - oy;
        const double det = ax * by - ay * bx;
        for (int c = 0; c < a.ncomp; ++c) {
            double g1 = 0.0, g2 = 0.0;
            for (int j = 0; j < PMAX; ++j)
                if (j < a.p) {
                    const double zv = ze[j * a.ncomp + c];
                    g1 += p1[j] * zv;
                    g2 += p2[j] * zv;
                }
            a.grad[(q * a.ncomp + c) * 2] = (by * g1 - ay * g2) / det;
            a.grad[(q * a.ncomp + c) * 2 + 1] = (ax * g2 - bx * g1) / det;
        }
    }
    return true;
}

}  // namespace

}  // namespace mgbhip
