// faces.hpp -- the facets of a mesh behind mgbhip_faces_* (faces.hip): topology built on the device, integrals over the
// boundary faces and jumps across the interior faces.
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"
#include "faces_layout.hpp"

namespace mgbhip {

// What the host hands over: N elements of p nodes and dimension d = e, F local faces of NC = 2^(d-1) corners each and a
// rule of Qf points per face.  Nothing else depends on the family.
struct FacesIn {
    int32_t d = 0, p = 0, F = 0, Qf = 0, ncode = 0;
    int64_t N = 0;
    const double* x = nullptr;         // (p N) x d
    const int32_t* t = nullptr;        // N x p global node ids in [0, 2^31)
    const double* wf = nullptr;        // Qf
    const double* phi = nullptr;       // F x Qf x p
    const double* dphi = nullptr;      // F x Qf x p x d
    const double* tangents = nullptr;  // F x (d-1) x d
    const double* normals = nullptr;   // F x d
    const int32_t* corners = nullptr;  // F x NC local nodes
    const int32_t* perm = nullptr;     // ncode x Qf
};

struct Faces {
    int32_t d = 0, p = 0, F = 0, Qf = 0, ncode = 0;
    int64_t N = 0, B = 0, I = 0;
    DevBuf<double> x, wf, tab, fgeo;              // fgeo [F][(d-1) d tangents, then d normal]
    DevBuf<int32_t> t, corners, perm;
    DevBuf<int32_t> boundary, interior, orientation, element_faces;     // B x 2, I x 4, I, N x F
    DevBuf<double> hF;                            // I: |F|^(1/(d-1)) from the L side
    DevBuf<double> z, weight, face, elem, totals, geo;    // per call: grown to the largest size seen and kept
    CallEvents<5> ev;                             // 0..2 around the last call's face kernel and reduction, 3..4 around the topology build
};

// Builds the topology and checks det J at every face point; complete on return.  InvalidArgument for a face shared by
// more than two elements (naming the count) and for a non-positive or non-finite det J (naming the element).
void faces_build(Faces& Fc, const FacesIn& in, hipStream_t st);
// host arrays, any may be NULL: boundary B x 2, interior I x 4, orientation I, element_faces N x F
void faces_topology(const Faces& Fc, int32_t* boundary, int32_t* interior, int32_t* orientation, int32_t* element_faces, hipStream_t st);
// which = 0: the boundary faces, 1: the interior faces from their L side.  points nf x Qf x d, normals nf x Qf x d,
// measures nf x Qf; any may be NULL
void faces_geometry(Faces& Fc, int32_t which, double* points, double* normals, double* measures, hipStream_t st);
void faces_sizes(const Faces& Fc, double* hF, hipStream_t st);
// z host (p N) x ncol; weight host B x Qf or NULL; per_face host B x ncol or NULL; totals host ncol
void faces_integrate(Faces& Fc, int32_t kind, double pexp, int32_t ncol, const double* z, const double* weight,
                     double* per_face, double* totals, hipStream_t st);
// out host I x ncol
void faces_jumps(Faces& Fc, int32_t kind, double pexp, int32_t ncol, const double* z, double* out, hipStream_t st);
// eta2 host N x ncol, totals host ncol
void faces_indicator(Faces& Fc, double pexp, int32_t ncol, const double* z, double* eta2, double* totals, hipStream_t st);
// ms[0] the face kernel and ms[1] the reduction of the last integrate / jumps / indicator call (0 before the first),
// ms[2] the topology build
void faces_times(const Faces& Fc, double* ms);

}  // namespace mgbhip
