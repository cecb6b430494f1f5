// render_device.hpp -- what the rendering translation units (surface.hip, tubes.hip, raycast.hip, figure.hip) share on
// the device, one definition each: the 3-vector products, the colour-table lookup, the tail of a shade
// kernel and the two front-to-back compositing steps.  The NumPy twins of the tests transcribe these operations in this
// order, and a frame of the figure pipeline is bitwise the host chain's frame only while every user runs the same text.
//
// Everything here has internal linkage (the library is built without relocatable device code).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "device_prims.hpp"        // BLOCK, grid_1d

// No fused multiply-adds in the code below or in a file that includes it.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

__device__ inline double dnan() { return __builtin_nan(""); }

__device__ inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ inline void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// The row of a K x 4 table at the finite value v, with width = hi - lo and km1 = K - 1: v is scaled to [0, 1] and clamped,
// the row index is clamped to K - 2 so that v = hi interpolates inside the last interval, and the four channels are
// interpolated linearly.
__device__ inline void table_row(double v, double lo, double width, double km1, int32_t K,
                                 const double* __restrict__ table, double* c) {
    const double sc = fmin(1.0, fmax(0.0, (v - lo) / width));
    const double f = sc * km1;
    int32_t j = (int32_t)floor(f);             // 0 <= f <= K - 1
    j = j < K - 2 ? j : K - 2;
    const double w = f - (double)j;
    const double* t0 = table + (int64_t)j * 4;
    for (int a = 0; a < 4; ++a) c[a] = t0[a] + w * (t0[4 + a] - t0[a]);
}

// a layer that adds nothing: a miss, or a hit whose value is not finite
__device__ inline void layer_zero(double* __restrict__ ly) {
    for (int k = 0; k < 4; ++k) ly[k] = 0.0;
}

// The tail of a shade kernel: the table colour c (r, g, b, alpha) of a hit with the unnormalised normal nrm, seen along
// dn, as a premultiplied layer: shade = ambient + (1 - ambient) |n . dn| (two-sided), alpha clamped to [0, 1].
__device__ inline void layer_shaded(const double* c, double* nrm, const double* dn, double ambient,
                                    double* __restrict__ ly) {
    const double len = sqrt(dot3(nrm, nrm));
    for (int a = 0; a < 3; ++a) nrm[a] = nrm[a] / len;
    const double shade = ambient + (1.0 - ambient) * fabs(dot3(nrm, dn));
    const double alpha = fmin(1.0, fmax(0.0, c[3]));
    const double as = alpha * shade;
    ly[0] = as * c[0];
    ly[1] = as * c[1];
    ly[2] = as * c[2];
    ly[3] = alpha;
}

// What a lane carries front to back along its ray: the transmittance so far and the premultiplied colour.
struct Composite {
    double T = 1.0, C0 = 0.0, C1 = 0.0, C2 = 0.0;

    // a layer (premultiplied r, g, b, then alpha) in front of everything behind it
    __device__ inline void layer(const double* __restrict__ ly) {
        C0 += T * ly[0];
        C1 += T * ly[1];
        C2 += T * ly[2];
        T = T * (1.0 - ly[3]);
    }
    // an emission-absorption sample of length h with the table row c (r, g, b, sigma)
    __device__ inline void sample(const double* c, double h) {
        const double e = exp(-(c[3] * h));
        const double alpha = 1.0 - e;
        const double ta = T * alpha;
        C0 += ta * c[0];
        C1 += ta * c[1];
        C2 += ta * c[2];
        T = T * e;
    }
    __device__ inline void store(double* __restrict__ px) const {
        px[0] = C0;
        px[1] = C1;
        px[2] = C2;
        px[3] = 1.0 - T;
    }
};

}  // namespace

}  // namespace mgbhip
