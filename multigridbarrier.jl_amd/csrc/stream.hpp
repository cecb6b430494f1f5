// stream.hpp -- field lines traced through a mesh behind mgbhip_stream_* (stream.hip): a resident location grid
// (interpolate.hpp) and a kernel that keeps one lane on one line, locating and evaluating again at every Runge-Kutta stage.
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"
#include "interpolate.hpp"

namespace mgbhip {

// Resident for the life of a tracer: the node coordinates, the basis table, the location grid (cells, candidate lists,
// element boxes) and the field z.  stream_set_field replaces z alone.  Per trace call: the seeds, the lines and a stage
// buffer of one velocity per lane, grown to the largest call seen and kept.
struct StreamTracer {
    int32_t family = 0, d = 0, k = 0, p = 0, field = 0;     // field: MGBHIP_STREAM_VECTOR or MGBHIP_STREAM_GRADIENT
    int64_t N = 0;
    DevBuf<double> x, table, z;
    LocationGrid grid;
    DevBuf<double> seeds, points, stage_out, stage_grad;
    DevBuf<int32_t> n, status;
};

// geo: family, d, k, p, N, x, table (table_len set): QK (d = 2, 3), P1, P2, P2C.  z host (p*N) x d (VECTOR) or p*N (GRADIENT).
void stream_build(StreamTracer& T, const InterpIn& geo, int32_t field, const double* z, hipStream_t st);
void stream_set_field(StreamTracer& T, const double* z, hipStream_t st);
// seeds host S x d; points host S x (max_steps + 1) x d, n and status host S; h is the signed step; complete on return
void stream_trace(StreamTracer& T, int64_t S, const double* seeds, double h, int32_t max_steps, bool normalize,
                  double min_speed, double* points, int32_t* n, int32_t* status, hipStream_t st);

}  // namespace mgbhip
