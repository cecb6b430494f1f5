// weld.hpp -- a simplex soup welded into an indexed mesh behind mgbhip_weld_* (weld.hip): vertex classes of the
// tolerance link relation, the connected components of the welded mesh and per-vertex normals.
#pragma once
#include <cstdint>

#include "../../include/mgbhip.h"
#include "common.hpp"

namespace mgbhip {

constexpr int WELD_MAX_CELL = 1024;        // corners in one grid cell above which a call is refused
constexpr int WELD_AXIS_BITS = 21;         // bits of the cell key per axis (cell indices reach 2^20 + 1)
constexpr int WELD_GRID_LOG2 = 20;         // the cell side is max(tol, largest extent / 2^20)

struct WeldIn {
    int64_t S = 0;
    int32_t nv = 0, e = 0;
    const double* points = nullptr;  // host S x nv x e
    const int32_t* group = nullptr;  // host S, or NULL (one group)
    double tol = 0.0;
    bool want_normals = false;
};

// The index of one soup, resident on the device until it is fetched or destroyed.
struct Weld {
    int32_t nv = 0, e = 0;
    int64_t S = 0, V = 0, ncomp = 0;
    int32_t vertex_rounds = 0, component_rounds = 0;
    bool has_normals = false;
    DevBuf<int32_t> cells;           // S x nv: the vertex of every corner
    DevBuf<int32_t> first_corner;    // V: the lowest corner of every vertex
    DevBuf<int32_t> component;       // V: the component of every vertex, numbered by lowest vertex
    DevBuf<double> normals;          // V x 3 (nv = e = 3, on request)
};

// grid, sort, occupancy guard, vertex classes, compaction, vertex -> corner lists, components, normals; complete on
// return (W.V and W.ncomp are known) and every work buffer is freed
void weld_build(Weld& W, const WeldIn& in, hipStream_t st);
// normals may be NULL; complete on return
void weld_fetch(const Weld& W, int32_t* cells, int32_t* first_corner, int32_t* component, double* normals, hipStream_t st);

}  // namespace mgbhip
