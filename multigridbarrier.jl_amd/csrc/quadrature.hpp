// quadrature.hpp -- element quadrature of element-space functions behind mgbhip_quadrature_* (quadrature.hip).
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"
#include "quad_layout.hpp"

namespace mgbhip {

// A quadrature rule on a mesh: N elements of p nodes and dimension d in e >= d coordinates, Q points per element.
// Resident: the node coordinates, the reference weights and the basis tables at the rule's points, point fastest
// (tab[i][0][q] = phi_i(xi_q), tab[i][1 + b][q] = d phi_i / d xi_b (xi_q)).  Nothing else depends on the family.
struct Quadrature {
    int32_t d = 0, e = 0, p = 0, Q = 0;
    int64_t N = 0;
    DevBuf<double> x, wref, tab;
    DevBuf<double> z, minus, source, elem, totals, geo;   // per call: grown to the largest size seen and kept
    CallEvents<3> ev;                                     // around the element kernel and the reduction of the last call
};

// x host (p*N) x e, wref host Q, phi host Q x p, dphi host Q x p x d; complete on return
void quadrature_build(Quadrature& Qd, int32_t d, int32_t e, int32_t p, int64_t N, const double* x, int32_t Q,
                      const double* wref, const double* phi, const double* dphi, hipStream_t st);
// points host N x Q x e or NULL, weights host N x Q or NULL; complete on return
void quadrature_geometry(Quadrature& Qd, double* points, double* weights, hipStream_t st);
// z host (p*N) x ncol; minus host N x Q x ncol (QUAD_LP) or N x Q x ncol x e (QUAD_W1P) or NULL; source host p*N
// (QUAD_ENERGY); per_element host N x ncol or NULL; totals host ncol.  is_max: the largest |u - g| (QUAD_LP) or
// |grad u - G| (QUAD_W1P) over the quadrature points instead of the integral.  Complete on return.
void quadrature_integrate(Quadrature& Qd, int32_t kind, double pexp, bool is_max, int32_t ncol, const double* z,
                          const double* minus, const double* source, double* per_element, double* totals, hipStream_t st);

// device milliseconds of the last integrate call: ms[0] the element kernel, ms[1] the reduction over the elements
void quadrature_times(const Quadrature& Qd, double* ms);

}  // namespace mgbhip
