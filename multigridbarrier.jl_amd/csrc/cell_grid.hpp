// cell_grid.hpp -- the uniform grid of cells that every spatial index here is (cell_lists.hpp builds it): the point
// locator's grid over element boxes (interpolate.hpp) and the ray tracers' grid over primitive boxes (surface.hpp).
#pragma once
#include <cstdint>

#include "common.hpp"

namespace mgbhip {

// Cells over a box in up to three coordinates (an unused axis has n = 1, inv = 0): kernels take it by value.  Every box
// is widened by `pad` on every side before it is cut into cells.  The location grid has pad = 0 (its boxes come padded)
// and leaves size at 0: only the walk of a ray reads the cell side.
struct Grid {
    double lo[3], hi[3], inv[3], size[3];   // the box, cells per unit length, cell side
    double pad;
    int32_t n[3];
    int64_t ncell;
};

// What building a grid needs besides its result: the boxes, their union, the per-box counts and their scan, the unsorted
// pairs and the scratch of the scan and the sort.  A caller that builds again and again (figure.hip) keeps one, and its
// buffers grow to the largest soup seen.
struct GridWork {
    DevBuf<double> box, ubox;
    DevBuf<int64_t> count, off;
    DevBuf<char> tmp;
    DevBuf<uint32_t> k0, k1;
    DevBuf<int32_t> v0;
};

}  // namespace mgbhip
