// quad_layout.hpp -- kinds, lane grouping and LDS layout of the element quadrature (quadrature.hip).  Plain C++ (no HIP):
// the kernel, its launcher and mgbhip_quadrature_plan all read the one decision from here.
#pragma once
#include <cstddef>

namespace mgbhip {

enum QuadKind { QUAD_VALUE = 0, QUAD_LP = 1, QUAD_W1P = 2, QUAD_ENERGY = 3 };

constexpr int QUAD_THREADS = 256;             // one lane per (element, quadrature point)
constexpr int QUAD_CHUNK = 4;                 // columns of z staged per pass
constexpr int QUAD_MAX_G = 32;                // elements per workgroup, at most
constexpr int QUAD_MAX_GRID = 2048;           // workgroups, at most: each strides over the element groups
constexpr int QUAD_MAX_GRID_BIG = 256;        // ... of more than 64 KB of LDS: one per CU is resident, and each stages the tables once
constexpr int QUAD_REDUCE_THREADS = 1024;     // the reduction over elements: one workgroup of this size per column
constexpr size_t QUAD_BASE_BUDGET = 48 * 1024;    // nodes + z chunk + source + partial sums of a workgroup while G > 1
constexpr size_t QUAD_LDS_MAX = 160 * 1024;       // launch cap (the element kernels' ELEM_LDS_MAX)

// Dynamic LDS of a workgroup, five regions of doubles in this order (every offset a multiple of 2 doubles = 16 bytes):
//   xs  [G][p][e]          node coordinates of the workgroup's elements
//   zs  [G][p][CHUNK]      a chunk of z columns
//   fs  [G][p]             the source field (energy only; reserved for every kind so that the layout depends on the shape alone)
//   red [CHUNK][256]       one partial sum per lane and column
//   tab [p][1 + d][Q]      phi and dphi at the rule's points, point fastest -- only while everything stays under the cap
constexpr size_t quad_even(size_t n) { return (n + 1) & ~(size_t)1; }
constexpr size_t quad_lds_xs(int G, int p, int e) { return quad_even((size_t)G * p * e); }
constexpr size_t quad_lds_zs(int G, int p) { return quad_even((size_t)G * p * QUAD_CHUNK); }
constexpr size_t quad_lds_fs(int G, int p) { return quad_even((size_t)G * p); }
constexpr size_t quad_lds_red() { return (size_t)QUAD_CHUNK * QUAD_THREADS; }
constexpr size_t quad_lds_base(int G, int p, int e) {
    return (quad_lds_xs(G, p, e) + quad_lds_zs(G, p) + quad_lds_fs(G, p) + quad_lds_red()) * sizeof(double);
}
constexpr size_t quad_lds_tables(int d, int p, int Q) { return (size_t)(1 + d) * Q * p * sizeof(double); }

struct QuadPlan {
    int threads;         // QUAD_THREADS
    int S;               // lanes per element: min(Q, threads); lane s of an element takes the points s, s + S, ...
    int G;               // elements per workgroup
    int chunk;           // QUAD_CHUNK
    int tables_lds;      // 1: phi / dphi staged in LDS, 0: read through L2
    int reduce_threads;  // QUAD_REDUCE_THREADS
    long long groups;    // ceil(N / G)
    long long grid;      // workgroups: min(groups, QUAD_MAX_GRID), or QUAD_MAX_GRID_BIG above 64 KB of LDS
    size_t lds;          // dynamic LDS bytes
};

// The one decision: depends on the shape (d, e, p, Q) alone but for the grid, so that an element's value does not depend on
// how many elements or columns ride along.  fits == false (returned as G = 0): one element's nodes exceed the cap.
constexpr QuadPlan quad_decide(int d, int e, int p, int Q, long long N) {
    const int S = Q < QUAD_THREADS ? Q : QUAD_THREADS;
    int G = QUAD_THREADS / S;
    if (G > QUAD_MAX_G) G = QUAD_MAX_G;
    while (G > 1 && quad_lds_base(G, p, e) > QUAD_BASE_BUDGET) --G;
    const size_t base = quad_lds_base(G, p, e);
    if (base > QUAD_LDS_MAX) return QuadPlan{QUAD_THREADS, S, 0, QUAD_CHUNK, 0, QUAD_REDUCE_THREADS, 0, 0, base};
    const size_t tab = quad_lds_tables(d, p, Q);
    const bool staged = base + tab <= QUAD_LDS_MAX;
    const long long groups = (N + G - 1) / G;
    const size_t lds = base + (staged ? tab : 0);
    const long long cap = lds > 64 * 1024 ? QUAD_MAX_GRID_BIG : QUAD_MAX_GRID;
    return QuadPlan{QUAD_THREADS, S, G, QUAD_CHUNK, staged ? 1 : 0, QUAD_REDUCE_THREADS, groups, groups < cap ? groups : cap, lds};
}

}  // namespace mgbhip
