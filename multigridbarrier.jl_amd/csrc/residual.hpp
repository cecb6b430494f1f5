// residual.hpp -- the element-interior residual of the p-Laplace equation behind mgbhip_residual_* (residual.hip).
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"
#include "quad_layout.hpp"

namespace mgbhip {

// the table rows of a node: phi, d dphi, and the d (d + 1) / 2 second reference derivatives (0,0), (0,1), .., (d-1,d-1)
constexpr int residual_rows(int d) { return 1 + d + d * (d + 1) / 2; }

// N elements of p nodes in d = e coordinates, Q points each: the lane plan of the element quadrature (quad_decide) with
// the longer tables.  The base is quad_decide's, so S, G and the base bytes are those of a Quadrature of the same shape.
constexpr QuadPlan residual_decide(int d, int p, int Q, long long N) {
    return quad_decide_lanes(Q < QUAD_THREADS ? Q : QUAD_THREADS, (size_t)p * d, (size_t)p * QUAD_CHUNK, (size_t)p,
                             quad_lds_tables(residual_rows(d), p, Q), N);
}

// A quadrature rule on a flat mesh with the second derivatives of the basis: N elements of p nodes in d = e = 2 or 3
// coordinates, Q points per element.  Resident: the node coordinates, the reference weights, the tables point fastest
// (tab[i][0][q] = phi_i, tab[i][1 + b][q] = d phi_i / d xi_b, tab[i][1 + d + m][q] = the m-th second derivative) and the
// element sizes h_K.  Nothing else depends on the family.
struct Residual {
    int32_t d = 0, p = 0, Q = 0;
    int64_t N = 0;
    DevBuf<double> x, wref, tab, sizes;
    DevBuf<double> z, source, out, totals, geo;           // per call: grown to the largest size seen and kept
    CallEvents<3> ev;                                     // around the element kernel and the reduction of the last call
};

// x host (p*N) x d, wref host Q, phi host Q x p, dphi host Q x p x d, d2phi host Q x p x d(d+1)/2; complete on return.
// InvalidArgument if det J is not positive and finite at a point.
void residual_build(Residual& Rd, int32_t d, int32_t p, int64_t N, const double* x, int32_t Q, const double* wref,
                    const double* phi, const double* dphi, const double* d2phi, hipStream_t st);
// points host N x Q x d, weights host N x Q, sizes host N; any may be NULL; complete on return
void residual_geometry(Residual& Rd, double* points, double* weights, double* sizes, hipStream_t st);
// z host (p*N) x ncol; source host p*N (at_points = false) or N x Q (at_points = true).  pointwise: r host N x Q x ncol.
// integrate: per_element host N x ncol or NULL, totals host ncol.  Complete on return.
void residual_pointwise(Residual& Rd, double pexp, int32_t ncol, const double* z, const double* source, bool at_points,
                        double* r, hipStream_t st);
void residual_integrate(Residual& Rd, double pexp, int32_t ncol, const double* z, const double* source, bool at_points,
                        double* per_element, double* totals, hipStream_t st);

// device milliseconds of the last pointwise or integrate call: ms[0] the element kernel, ms[1] the reduction (0: pointwise)
void residual_times(const Residual& Rd, double* ms);

}  // namespace mgbhip
