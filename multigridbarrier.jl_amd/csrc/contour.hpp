// contour.hpp -- level sets of an element-space function behind mgbhip_contour_*, and the lattice triangles themselves
// behind mgbhip_tessellate_* (contour.hip).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mgbhip.h"
#include "common.hpp"

namespace mgbhip {

constexpr int CONTOUR_MAX_FIELDS = 5;      // the contoured function and up to four carried fields
constexpr int CONTOUR_MAX_REFINE_2D = 16;  // lattice of at most 17 x 17 points per element
constexpr int CONTOUR_MAX_REFINE_3D = 8;   // lattice of at most 9 x 9 x 9 points per element

struct ContourIn {
    int32_t family = 0, d = 0, k = 0, p = 0, nfield = 0, nlevels = 0, refine = 0;
    int32_t e = 0;                   // ambient dimension: d, or 3 for a Q_k 2-D surface in R^3
    int64_t N = 0;
    const double* x = nullptr;       // host (p*N) x e
    const double* table = nullptr;   // host: Q_k: the k + 1 reference nodes; P1 / P2: p x 10 monomial coefficients
    const double* fields = nullptr;  // host (p*N) x nfield; column 0 is contoured, the others are carried
                                     // (a tessellation: 0..CONTOUR_MAX_FIELDS columns, all alike; levels are unused)
    const double* levels = nullptr;  // host nlevels, finite
};

// The simplex soup of one call, resident on the device until it is fetched or destroyed.
struct Contour {
    int32_t d = 0, e = 0, ncarry = 0;
    int64_t S = 0;
    DevBuf<double> points, carried;  // S x d x e, S x d x ncarry
    DevBuf<int32_t> level, element;  // S, S
};

// count pass, exclusive scan over the elements, emit pass; complete on return (C.S is known)
void contour_build(Contour& C, const ContourIn& in, hipStream_t st);

// the per-element counts, their scan and the scan's scratch: grown to the largest call seen and kept by a caller that
// builds again and again (figure.hip)
struct ContourWork {
    DevBuf<int64_t> count, off;
    DevBuf<char> tmp;
};
// the table the kernels read, formed on the host from in.family, in.k, in.p, in.refine and in.table
std::vector<double> contour_lattice_table(const ContourIn& in);
// contour_build for a mesh, a table (contour_lattice_table), fields and levels already on the device: in.x, in.table,
// in.fields and in.levels are not read.  The buffers of C grow and are kept, so C may be built again; the valid part is
// the first C.S simplices.  Complete on return.
void contour_build_device(Contour& C, const ContourIn& in, const double* d_x, const double* d_table, int32_t table_len,
                          const double* d_fields, const double* d_levels, ContourWork& w, hipStream_t st);
// carried may be NULL; complete on return
void contour_fetch(const Contour& C, double* points, int32_t* level, int32_t* element, double* carried, hipStream_t st);

// Every lattice triangle of a 2-D mesh (Q_k with e = 2 or 3, P1 / P2), resident on the device until fetched or destroyed.
struct Tessellation {
    int32_t e = 0, nfield = 0;
    int64_t T = 0;
    DevBuf<double> points, values;   // T x 3 x e, T x 3 x nfield
    DevBuf<int32_t> element;         // T
};

// N x 2 refine^2 (Q_k) or N x refine^2 (P1 / P2): known before any device work
int64_t tessellate_count(const ContourIn& in);
// one launch, triangle i of element e at e * ntri + i; complete on return
void tessellate_build(Tessellation& T, const ContourIn& in, hipStream_t st);
// values may be NULL; complete on return
void tessellate_fetch(const Tessellation& T, double* points, int32_t* element, double* values, hipStream_t st);

}  // namespace mgbhip
