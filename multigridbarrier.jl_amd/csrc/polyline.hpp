// polyline.hpp -- the segments of an indexed curve mesh ordered into lines behind mgbhip_polyline_* (polyline.hip): edges,
// valence, successors, list ranking by pointer doubling, line numbering, arc length; and the stateless sampler.
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"

namespace mgbhip {

struct PolylineIn {
    int64_t V = 0, S = 0;
    int32_t e = 0;
    const double* vertices = nullptr;  // host V x e
    const int32_t* cells = nullptr;    // host S x 2, entries in [0, V)
};

// The lines of one segment mesh, resident on the device until they are fetched or destroyed.
struct Polyline {
    int32_t e = 0;
    int64_t S = 0, V = 0, L = 0, P = 0, ndropped = 0;
    int32_t rounds[2] = {0, 0};        // doubling rounds: the cycle pass (lowest vertex), the ranking pass
    DevBuf<int64_t> offsets;           // L + 1
    DevBuf<int32_t> vertex, segment;   // P
    DevBuf<uint8_t> closed;            // L
    DevBuf<double> arclength;          // P
};

// edges, vertex lists, successors, both doubling passes, numbering, scatter; complete on return (L, P and ndropped are
// known) and every work buffer is freed
void polyline_build(Polyline& Pl, const PolylineIn& in, hipStream_t st);
// length (L) is gathered from arclength; complete on return
void polyline_fetch(const Polyline& Pl, int64_t* offsets, int32_t* vertex, int32_t* segment, uint8_t* closed,
                    double* arclength, double* length, hipStream_t st);

struct PolylineSampleIn {
    int32_t e = 0, C = 0;
    int64_t P = 0, L = 0, Q = 0;
    const double* points = nullptr;     // host P x e
    const double* data = nullptr;       // host P x C, or NULL
    const int64_t* offsets = nullptr;   // host L + 1
    const double* arclength = nullptr;  // host P
    const int32_t* line = nullptr;      // host Q
    const double* s = nullptr;          // host Q
};

// one lane per query; out_points Q x e, out_data Q x C or NULL; complete on return
void polyline_sample(const PolylineSampleIn& in, double* out_points, double* out_data, hipStream_t st);

}  // namespace mgbhip
