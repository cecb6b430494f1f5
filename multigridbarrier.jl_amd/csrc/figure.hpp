// figure.hpp -- the default figure of a fem3d solution rendered frame after frame behind mgbhip_figure_* (figure.hip): the
// stages of contour.hpp, surface.hpp and raycast.hpp chained through their device-pointer entries, with everything that
// does not depend on the field kept on the device between frames.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mgbhip.h"
#include "common.hpp"
#include "contour.hpp"
#include "raycast.hpp"
#include "surface.hpp"

namespace mgbhip {

constexpr int FIGURE_MAX_LEVELS = 64;      // isosurface levels of one figure
constexpr int FIGURE_MAX_SLICES = 16;      // slices of one figure

struct FigureIn {
    RayIn rays;                      // the mesh (Q_k, d = 3), the rays, the clip box and the step; t_min = 0, t_max = +inf
    int32_t volume = 1;              // 0: the surfaces alone
    int32_t nlevels = 0, nslices = 0;
    const double* levels = nullptr;  // host nlevels, finite
    const int32_t* axes = nullptr;   // host nslices, 0..2
    const double* coords = nullptr;  // host nslices, finite
    int32_t ntable = 0;
    const double* vtable = nullptr;  // host ntable x 4 (r, g, b, sigma): the volume's
    const double* stable = nullptr;  // host ntable x 4 (r, g, b, alpha): the surfaces'
    double lo = 0.0, hi = 0.0, ambient = 0.0;
    int32_t K = 1;                   // hits kept per ray, 1..8
};

// Resident for the life of the figure: the mesh, the contour table, the levels, per slice its coordinate and a two-column
// field (the coordinate function, then room for u), the rays, both colour tables, an all-miss depth list, and with the
// volume a RayCaster whose samples are located once.  Per frame, grown to the largest frame seen and kept: u, the cut
// soups, their work buffers, the Surface (soup, grid, hits, layers), the vertex values, the image.
struct Figure {
    FigureIn in;                     // sizes and scalars; the host pointers are dead after figure_build
    int64_t rows = 0, R = 0;
    int32_t table_len = 0;
    DevBuf<double> x, ctable, levels, coords, o, dn, vtable, stable, miss_t;
    std::vector<DevBuf<double>> slice_fields;      // nslices of rows x 2
    RayCaster rc;
    DevBuf<double> u, values, image;
    DevBuf<uint8_t> bytes;
    Contour iso;
    std::vector<Contour> cuts;                     // nslices
    ContourWork cwork;
    Surface sf;
    GridWork gwork;
    int64_t T = 0, P = 0;                          // triangles and (cell, triangle) pairs of the last frame
};

// uploads what is resident and, with the volume, samples and locates the rays; complete on return
void figure_build(Figure& F, const FigureIn& in, hipStream_t st);
// u host p*N; out host R x 4: one frame, bitwise what render_figure's chain of host entries gives; complete on return
void figure_render(Figure& F, const double* u, double* out, hipStream_t st);
// the same frame as four bytes per ray over the background bg (3 doubles); complete on return
void figure_render_rgba8(Figure& F, const double* u, const double* bg, uint8_t* out, hipStream_t st);

}  // namespace mgbhip
