// contour.hpp -- level sets of an element-space function behind mgbhip_contour_* (contour.hip).
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"

namespace mgbhip {

constexpr int CONTOUR_MAX_FIELDS = 5;      // the contoured function and up to four carried fields
constexpr int CONTOUR_MAX_REFINE_2D = 16;  // lattice of at most 17 x 17 points per element
constexpr int CONTOUR_MAX_REFINE_3D = 8;   // lattice of at most 9 x 9 x 9 points per element

struct ContourIn {
    int32_t family = 0, d = 0, k = 0, p = 0, nfield = 0, nlevels = 0, refine = 0;
    int64_t N = 0;
    const double* x = nullptr;       // host (p*N) x d
    const double* table = nullptr;   // host: Q_k: the k + 1 reference nodes; P1 / P2: p x 10 monomial coefficients
    const double* fields = nullptr;  // host (p*N) x nfield; column 0 is contoured, the others are carried
    const double* levels = nullptr;  // host nlevels, finite
};

// The simplex soup of one call, resident on the device until it is fetched or destroyed.
struct Contour {
    int32_t d = 0, ncarry = 0;
    int64_t S = 0;
    DevBuf<double> points, carried;  // S x d x d, S x d x ncarry
    DevBuf<int32_t> level, element;  // S, S
};

// count pass, exclusive scan over the elements, emit pass; complete on return (C.S is known)
void contour_build(Contour& C, const ContourIn& in, hipStream_t st);
// carried may be NULL; complete on return
void contour_fetch(const Contour& C, double* points, int32_t* level, int32_t* element, double* carried, hipStream_t st);

}  // namespace mgbhip
