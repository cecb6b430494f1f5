// interpolate.hpp -- point evaluation behind mgbhip_interpolate / mgbhip_interpolate_grad (interpolate.hip).
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"

namespace mgbhip {

constexpr int INTERP_MAX_DEGREE = 8;    // element degree k of the FEM families (the kernels are unrolled per k + 1)

struct InterpIn {
    int32_t family = 0, d = 0, k = 0, p = 0, ncomp = 0;
    int64_t N = 0, M = 0;
    int32_t sorted = 1;           // FEM1D: left endpoints non-decreasing (binary search) or not (the reference's scan)
    const double* x = nullptr;    // host (p*N) x d
    const double* table = nullptr;
    int64_t table_len = 0;
    const double* z = nullptr;    // host (p*N) x ncomp
    const double* pts = nullptr;  // host M x d
    double* out = nullptr;        // host M x ncomp (may be NULL when grad is given)
    double* grad = nullptr;       // host M x ncomp x d, or NULL: values only
    int32_t* elem = nullptr;      // host M, or NULL
};

// one launch sequence on st; complete (results on the host) on return
void interpolate_run(const InterpIn& in, hipStream_t st);

}  // namespace mgbhip
