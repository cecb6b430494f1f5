// quad_layout.hpp -- lane grouping and LDS layout of the lane kernels: the element quadrature (quadrature.hip) and the
// face kernels (faces.hip).  Plain C++ (no HIP): the kernels, their launcher and the mgbhip_*_plan entry points all read
// the one decision from here.
#pragma once
#include <cstddef>

namespace mgbhip {

enum QuadKind { QUAD_VALUE = 0, QUAD_LP = 1, QUAD_W1P = 2, QUAD_ENERGY = 3 };

constexpr int QUAD_THREADS = 256;             // one lane per (item, point); an item is an element or a face
constexpr int QUAD_CHUNK = 4;                 // columns of z staged per pass
constexpr int QUAD_MAX_G = 32;                // items per workgroup, at most
constexpr int QUAD_MAX_GRID = 2048;           // workgroups, at most: each strides over the item groups
constexpr int QUAD_MAX_GRID_BIG = 256;        // ... of more than 64 KB of LDS: one per CU is resident, and each stages the tables once
constexpr int QUAD_REDUCE_THREADS = 1024;     // the reduction over items: one workgroup of this size per column
constexpr size_t QUAD_BASE_BUDGET = 48 * 1024;    // nodes + z chunk + source + partial sums of a workgroup while G > 1
constexpr size_t QUAD_LDS_MAX = 160 * 1024;       // launch cap (the element kernels' ELEM_LDS_MAX)

// Dynamic LDS of a workgroup, five regions of doubles in this order (every offset a multiple of 2 doubles = 16 bytes).
// The first three hold G items of a fixed number of doubles each; what an item is decides the numbers:
//   xs  nodes     element: [p][e]                    face: [sides][p][d], the L element, then the R element
//   zs  z chunk   element: [p][CHUNK]                face: [sides][p][CHUNK]
//   fs  source    element: [p] (energy only; reserved for every kind so that the layout depends on the shape alone)
//                                                    face: none
//   red [CHUNK][256]   one partial sum per lane and column
//   tab           phi and dphi at the rule's points, point fastest -- only while everything stays under the cap
//                 element: [p][1 + d][Q]             face: [F][p][1 + d][Qf], one table per local face
//                 element residual (residual.hip): [p][1 + d + d (d + 1) / 2][Q], the second derivatives behind dphi
constexpr size_t quad_even(size_t n) { return (n + 1) & ~(size_t)1; }
constexpr size_t quad_lds_region(int G, size_t per_item) { return quad_even((size_t)G * per_item); }
// the offsets the element kernel carves LDS with: xs at 0, zs = xs + quad_lds_xs, fs = zs + quad_lds_zs, red = fs + quad_lds_fs,
// tab = red + quad_lds_red (the face kernel's, without fs, are in faces_layout.hpp).  Their form is the kernels' device code:
// profiles/quad_faces_merge_isa.txt
constexpr size_t quad_lds_xs(int G, int p, int e) { return quad_even((size_t)G * p * e); }
constexpr size_t quad_lds_zs(int G, int p) { return quad_even((size_t)G * p * QUAD_CHUNK); }
constexpr size_t quad_lds_fs(int G, int p) { return quad_even((size_t)G * p); }
constexpr size_t quad_lds_red() { return (size_t)QUAD_CHUNK * QUAD_THREADS; }
constexpr size_t quad_lds_base(int G, size_t xs_item, size_t zs_item, size_t fs_item) {
    return (quad_lds_region(G, xs_item) + quad_lds_region(G, zs_item) + quad_lds_region(G, fs_item) + quad_lds_red()) * sizeof(double);
}
// rows: the table rows of a node, 1 + d for phi and dphi
constexpr size_t quad_lds_tables(int rows, int p, int Q) { return (size_t)rows * Q * p * sizeof(double); }

struct QuadPlan {
    int threads;         // QUAD_THREADS
    int S;               // lanes per item; lane s of an item takes the points s, s + S, ...
    int G;               // items per workgroup; 0: a single item does not fit
    int chunk;           // QUAD_CHUNK
    int tables_lds;      // 1: phi / dphi staged in LDS, 0: read through L2
    int reduce_threads;  // QUAD_REDUCE_THREADS
    long long groups;    // ceil(count / G)
    long long grid;      // workgroups: min(groups, QUAD_MAX_GRID), or QUAD_MAX_GRID_BIG above 64 KB of LDS
    size_t lds;          // dynamic LDS bytes
};

constexpr QuadPlan quad_no_fit(int S, size_t lds) { return QuadPlan{QUAD_THREADS, S, 0, QUAD_CHUNK, 0, QUAD_REDUCE_THREADS, 0, 0, lds}; }

// The one decision, from the lanes of an item (S <= 256), the doubles an item puts into xs / zs / fs, the bytes of the
// tables and the number of items.  It depends on the shape alone but for the grid, so that an item's value does not
// depend on how many items or columns ride along.  G = 0: one item's nodes exceed the cap.
constexpr QuadPlan quad_decide_lanes(int S, size_t xs_item, size_t zs_item, size_t fs_item, size_t tab, long long count) {
    int G = QUAD_THREADS / S;
    if (G > QUAD_MAX_G) G = QUAD_MAX_G;
    while (G > 1 && quad_lds_base(G, xs_item, zs_item, fs_item) > QUAD_BASE_BUDGET) --G;
    const size_t base = quad_lds_base(G, xs_item, zs_item, fs_item);
    if (base > QUAD_LDS_MAX) return quad_no_fit(S, base);
    const bool staged = base + tab <= QUAD_LDS_MAX;
    const long long groups = (count + G - 1) / G;
    const size_t lds = base + (staged ? tab : 0);
    const long long cap = lds > 64 * 1024 ? QUAD_MAX_GRID_BIG : QUAD_MAX_GRID;
    return QuadPlan{QUAD_THREADS, S, G, QUAD_CHUNK, staged ? 1 : 0, QUAD_REDUCE_THREADS, groups, groups < cap ? groups : cap, lds};
}

// N elements of p nodes in e coordinates, Q points each: S = min(Q, 256) lanes per element
constexpr QuadPlan quad_decide(int d, int e, int p, int Q, long long N) {
    return quad_decide_lanes(Q < QUAD_THREADS ? Q : QUAD_THREADS, (size_t)p * e, (size_t)p * QUAD_CHUNK, (size_t)p,
                             quad_lds_tables(1 + d, p, Q), N);
}

}  // namespace mgbhip
