// faces_layout.hpp -- kinds, lane grouping and LDS layout of the face kernels (faces.hip).  Plain C++ (no HIP): the
// kernels, their launcher and mgbhip_faces_plan all read the one decision from here.
#pragma once
#include <cstddef>

namespace mgbhip {

enum FaceKind { FACE_VALUE = 0, FACE_FLUX = 1 };

constexpr int FACE_THREADS = 256;             // one lane per (face, face point)
constexpr int FACE_CHUNK = 4;                 // columns of z staged per pass
constexpr int FACE_MAX_G = 32;                // faces per workgroup, at most
constexpr int FACE_MAX_QF = 100;              // points per face, at most: 10 per face axis
constexpr int FACE_MAX_GRID = 2048;           // workgroups, at most: each strides over the face groups
constexpr int FACE_MAX_GRID_BIG = 256;        // ... of more than 64 KB of LDS: one per CU is resident, and each stages the tables once
constexpr int FACE_REDUCE_THREADS = 1024;     // the reduction over faces or elements: one workgroup of this size per column
constexpr size_t FACE_BASE_BUDGET = 48 * 1024;    // nodes + z chunk + partial sums of a workgroup while G > 1
constexpr size_t FACE_LDS_MAX = 160 * 1024;       // launch cap (the element kernels' ELEM_LDS_MAX)

// Dynamic LDS of a workgroup, four regions of doubles in this order (every offset a multiple of 2 doubles = 16 bytes);
// sides = 1 for a boundary face (its element), 2 for an interior face (the L element, then the R element):
//   xs  [G][sides][p][d]       node coordinates of the elements of the workgroup's faces
//   zs  [G][sides][p][CHUNK]   a chunk of z columns of the same elements
//   red [CHUNK][256]           one term per lane and column
//   tab [F][p][1 + d][Qf]      phi and dphi at the points of every local face, point fastest -- only while everything
//                              stays under the cap
constexpr size_t face_even(size_t n) { return (n + 1) & ~(size_t)1; }
constexpr size_t face_lds_xs(int G, int sides, int p, int d) { return face_even((size_t)G * sides * p * d); }
constexpr size_t face_lds_zs(int G, int sides, int p) { return face_even((size_t)G * sides * p * FACE_CHUNK); }
constexpr size_t face_lds_red() { return (size_t)FACE_CHUNK * FACE_THREADS; }
constexpr size_t face_lds_base(int G, int sides, int p, int d) {
    return (face_lds_xs(G, sides, p, d) + face_lds_zs(G, sides, p) + face_lds_red()) * sizeof(double);
}
constexpr size_t face_lds_tables(int d, int p, int Qf, int F) { return (size_t)F * (1 + d) * Qf * p * sizeof(double); }

struct FacePlan {
    int threads;         // FACE_THREADS
    int S;               // lanes per face: Qf, one point each
    int G;               // faces per workgroup; 0: a single face does not fit
    int chunk;           // FACE_CHUNK
    int tables_lds;      // 1: phi / dphi staged in LDS, 0: read through L2
    int reduce_threads;  // FACE_REDUCE_THREADS
    long long groups;    // ceil(nfaces / G)
    long long grid;      // workgroups: min(groups, FACE_MAX_GRID), or FACE_MAX_GRID_BIG above 64 KB of LDS
    size_t lds;          // dynamic LDS bytes
};

// The one decision: depends on the shape (d, p, Qf, F, sides) alone but for the grid, so that a face's value does not
// depend on how many faces or columns ride along.  G = 0: Qf exceeds the rule's largest, or the nodes of one face's
// elements exceed the cap.
constexpr FacePlan face_decide(int d, int p, int Qf, int F, int sides, long long nfaces) {
    if (Qf > FACE_MAX_QF) return FacePlan{FACE_THREADS, Qf, 0, FACE_CHUNK, 0, FACE_REDUCE_THREADS, 0, 0, 0};
    int G = FACE_THREADS / Qf;
    if (G > FACE_MAX_G) G = FACE_MAX_G;
    while (G > 1 && face_lds_base(G, sides, p, d) > FACE_BASE_BUDGET) --G;
    const size_t base = face_lds_base(G, sides, p, d);
    if (base > FACE_LDS_MAX) return FacePlan{FACE_THREADS, Qf, 0, FACE_CHUNK, 0, FACE_REDUCE_THREADS, 0, 0, base};
    const size_t tab = face_lds_tables(d, p, Qf, F);
    const bool staged = base + tab <= FACE_LDS_MAX;
    const long long groups = (nfaces + G - 1) / G;
    const size_t lds = base + (staged ? tab : 0);
    const long long cap = lds > 64 * 1024 ? FACE_MAX_GRID_BIG : FACE_MAX_GRID;
    return FacePlan{FACE_THREADS, Qf, G, FACE_CHUNK, staged ? 1 : 0, FACE_REDUCE_THREADS, groups, groups < cap ? groups : cap, lds};
}

}  // namespace mgbhip
