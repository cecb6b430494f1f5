// A simplex soup welded into an indexed mesh: mgbhip_weld_* (include/mgbhip.h).
//
// The reference hands its grids to PyVista, whose contour filter returns indexed PolyData; the soups of contour.hip,
// stream.hip and the tessellation are unindexed, and the copies of a vertex that two neighbouring elements compute can
// differ by rounding.  Here the M = S * nv corners of a soup are welded by tolerance:
//
//   linked(a, b)  iff  group(a) == group(b)  and  fabs(x_a[c] - x_b[c]) <= tol on every axis c
//
// (one IEEE subtraction and one compare per axis), a vertex is a connected component of the link graph (chains weld), and
// vertices are numbered by their lowest corner.  Nothing is averaged: every result is an integer or a gathered input.
//
//  1. One block reduces the union box of the corners and refuses a non-finite coordinate.
//  2. A uniform grid of cell side h = max(tol, largest extent / 2^20): one 64-bit key per corner (21 bits per axis, x
//     lowest) and one stable radix sort of (key, corner).  With h >= tol a linked pair lies in the same cell or in a
//     neighbouring one; the cells next to a corner along x are one contiguous key range, so a corner searches the sorted
//     keys 3^(e-1) times.  (A corner within 2^-20 of a cell face looks one cell further on that side, which covers the
//     rounding of the cell coordinate itself.)
//  3. The largest cell occupancy is reduced before any pair is tested; above WELD_MAX_CELL the call is refused, so the
//     pair work of a bad tolerance is bounded.
//  4. connected_components(): every node gets the lowest node index of its component, over an edge relation given by a
//     functor.  Hooking and shortcutting in the manner of FastSV (Zhang, Azad, Hu 2020): per round every node u takes
//     m = min(gf[u], gf[v] over its neighbours v) and lowers next[u] and next[f[u]] to m with integer atomicMin; then
//     f = next, gf[u] = f[f[u]].  A round reads f and gf and writes only next, so next (a minimum over a set) does not
//     depend on the order of the atomics, and neither does the number of rounds.  The host reads one changed flag per
//     round; when a round changes nothing, f is constant on every component, idempotent and so its lowest node.
//     Two users: the link relation scanned through the grid (nodes = corners), and the simplex edges through the
//     vertex -> corner lists (nodes = vertices).
//  5. A flag scan numbers the classes by lowest node: first_corner, cells; later component.
//  6. A second stable sort of (vertex, corner) gives the corners of every vertex in ascending order; the component pass
//     walks them, and the normal kernel sums cross3(p1 - p0, p2 - p0) over them, one lane per vertex.
//
// No floating-point atomics; two calls return bitwise equal arrays.
#include <hip/hip_runtime.h>

#include <cmath>

#include "render_device.hpp"
#include "weld.hpp"

// No fused multiply-adds in this file: the NumPy twin (tests/weld_twin.py) evaluates the same predicate and the same sums.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

constexpr int64_t CELL_MAX = ((int64_t)1 << WELD_AXIS_BITS) - 1;
constexpr double FACE_MARGIN = 9.5367431640625e-07;   // 2^-20 of a cell; the cell coordinate is good to about 2^-31
constexpr int MAX_ROUNDS = 1 << 20;                   // labels only decrease, so this is never reached

struct WeldGrid {
    double lo[3];
    double h;        // cell side; 0 when every corner is the same point and tol = 0 (one cell)
    double tol;
};

// one block: lo (3), hi (3) of all corners and, in out[6], 1.0 if any coordinate is not finite
template <int E>
__global__ void __launch_bounds__(1024) corner_box(int64_t M, const double* __restrict__ x, double* __restrict__ out) {
    __shared__ double s[7][1024];
    double lo[3], hi[3], bad = 0.0;
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int64_t i = threadIdx.x; i < M; i += blockDim.x)
        for (int a = 0; a < E; ++a) {
            const double v = x[i * E + a];
            if (!isfinite(v)) bad = 1.0;
            lo[a] = fmin(lo[a], v);
            hi[a] = fmax(hi[a], v);
        }
    for (int a = 0; a < 3; ++a) { s[a][threadIdx.x] = lo[a]; s[3 + a][threadIdx.x] = hi[a]; }
    s[6][threadIdx.x] = bad;
    __syncthreads();
    for (int h = blockDim.x / 2; h > 0; h /= 2) {
        if ((int)threadIdx.x < h) {
            for (int a = 0; a < 3; ++a) {
                s[a][threadIdx.x] = fmin(s[a][threadIdx.x], s[a][threadIdx.x + h]);
                s[3 + a][threadIdx.x] = fmax(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + h]);
            }
            s[6][threadIdx.x] = fmax(s[6][threadIdx.x], s[6][threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 7) out[threadIdx.x] = s[threadIdx.x][0];
}

// the cell of a coordinate and how far into it the coordinate lies (x >= lo: lo is the minimum itself)
__device__ inline int64_t cell_axis(double x, double lo, double h, double* frac) {
    if (!(h > 0.0)) { *frac = 0.5; return 0; }
    const double f = (x - lo) / h;
    int64_t c = (int64_t)f;
    c = c < CELL_MAX ? c : CELL_MAX;
    *frac = f - (double)c;
    return c;
}

__device__ inline uint64_t cell_key(int64_t cx, int64_t cy, int64_t cz) {
    return ((uint64_t)cz << (2 * WELD_AXIS_BITS)) | ((uint64_t)cy << WELD_AXIS_BITS) | (uint64_t)cx;
}

template <int E>
__global__ void __launch_bounds__(BLOCK) corner_keys(int64_t M, WeldGrid g, const double* __restrict__ x,
                                                     uint64_t* __restrict__ keys, int32_t* __restrict__ corner) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    int64_t c[3] = {0, 0, 0};
    double frac;
    for (int a = 0; a < E; ++a) c[a] = cell_axis(x[i * E + a], g.lo[a], g.h, &frac);
    keys[i] = cell_key(c[0], c[1], c[2]);
    corner[i] = (int32_t)i;
}

// first i in [0, n) with keys[i] >= k, or n
__device__ inline int64_t lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t k) {
    int64_t a = 0, b = n;
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (keys[m] < k) a = m + 1;
        else b = m;
    }
    return a;
}

// the last corner of every cell raises *most to the number of corners in its cell (integer atomicMax)
__global__ void __launch_bounds__(BLOCK) cell_occupancy(int64_t M, const uint64_t* __restrict__ keys, int32_t* most) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    if (i + 1 < M && keys[i + 1] == keys[i]) return;
    const int64_t first = lower_bound(keys, i + 1, keys[i]);
    atomicMax(most, (int32_t)(i + 1 - first));
}

// ---- the edge relations: for_each(u, visit) calls visit(v) for every neighbour v of node u (u itself may be visited)

// corners linked by tolerance, found through the sorted cell keys
template <int E>
struct LinkRelation {
    WeldGrid g;
    int64_t M;
    int32_t nv;
    const double* x;           // M x E
    const int32_t* group;      // S, or NULL
    const uint64_t* keys;      // sorted
    const int32_t* corner;     // the corner at every sorted position

    template <class Visit>
    __device__ inline void for_each(int32_t u, Visit visit) const {
        double p[E];
        int64_t c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
        for (int a = 0; a < E; ++a) {
            p[a] = x[(int64_t)u * E + a];
            double frac;
            const int64_t c = cell_axis(p[a], g.lo[a], g.h, &frac);
            c0[a] = c - 1 - (frac < FACE_MARGIN ? 1 : 0);
            c1[a] = c + 1 + (frac > 1.0 - FACE_MARGIN ? 1 : 0);
            c0[a] = c0[a] > 0 ? c0[a] : 0;
            c1[a] = c1[a] < CELL_MAX ? c1[a] : CELL_MAX;
        }
        const int32_t gu = group ? group[u / nv] : 0;
        for (int64_t cz = c0[2]; cz <= c1[2]; ++cz)
            for (int64_t cy = c0[1]; cy <= c1[1]; ++cy) {
                const uint64_t k1 = cell_key(c1[0], cy, cz);
                for (int64_t i = lower_bound(keys, M, cell_key(c0[0], cy, cz)); i < M && keys[i] <= k1; ++i) {
                    const int32_t v = corner[i];
                    if (group && group[v / nv] != gu) continue;
                    bool linked = true;
                    for (int a = 0; a < E; ++a) linked = linked && fabs(p[a] - x[(int64_t)v * E + a]) <= g.tol;
                    if (linked) visit(v);
                }
            }
    }
};

// vertices joined by a simplex edge: every vertex of every simplex that has a corner in u
struct SimplexRelation {
    int32_t nv;
    const int32_t* cells;      // M: the vertex of every corner
    const int32_t* start;      // V + 1: the corners of vertex v are list[start[v] .. start[v + 1])
    const int32_t* list;

    template <class Visit>
    __device__ inline void for_each(int32_t u, Visit visit) const {
        for (int32_t i = start[u]; i < start[u + 1]; ++i) {
            const int32_t s = list[i] / nv;
            for (int32_t q = 0; q < nv; ++q) visit(cells[(int64_t)s * nv + q]);
        }
    }
};

// ---- connected components: f[u] ends as the lowest node of u's component

__global__ void __launch_bounds__(BLOCK) cc_init(int64_t n, int32_t* __restrict__ f, int32_t* __restrict__ gf,
                                                 int32_t* __restrict__ next) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    f[u] = gf[u] = next[u] = (int32_t)u;
}

// reads f and gf, lowers next (= f on entry): next[u] and next[f[u]] to the least grandparent around u
template <class Rel>
__global__ void __launch_bounds__(BLOCK) cc_hook(int64_t n, Rel rel, const int32_t* __restrict__ f,
                                                 const int32_t* __restrict__ gf, int32_t* next) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    int32_t m = gf[u];
    rel.for_each((int32_t)u, [&](int32_t v) { m = min(m, gf[v]); });
    const int32_t fu = f[u];
    if (m < fu) {              // m <= gf[u] <= f[u] = next[u] on entry: with m == f[u] there is nothing to lower
        atomicMin(&next[u], m);
        atomicMin(&next[fu], m);
    }
}

// f = next, gf[u] = next[next[u]] (next is only read); *changed is set when any f moved
__global__ void __launch_bounds__(BLOCK) cc_shortcut(int64_t n, int32_t* __restrict__ f, int32_t* __restrict__ gf,
                                                     const int32_t* __restrict__ next, int32_t* changed) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    const int32_t nf = next[u];
    if (nf != f[u]) {
        f[u] = nf;
        *changed = 1;
    }
    gf[u] = next[nf];
}

struct CcWork {
    DevBuf<int32_t> f, gf, next, changed;
};

// Labels the n nodes of rel's graph; the labels are in w.f on return.  Returns the number of rounds, the last of which
// changed nothing.
template <class Rel>
int32_t connected_components(int64_t n, const Rel& rel, CcWork& w, hipStream_t st) {
    w.f.ensure((size_t)n); w.gf.ensure((size_t)n); w.next.ensure((size_t)n); w.changed.ensure(1);
    const dim3 gr(grid_1d(n)), bl(BLOCK);
    hipLaunchKernelGGL(cc_init, gr, bl, 0, st, n, w.f.p, w.gf.p, w.next.p);
    MGB_HIP_CHECK(hipGetLastError());
    for (int32_t round = 1; round <= MAX_ROUNDS; ++round) {
        w.changed.zero(st, 1);
        hipLaunchKernelGGL((cc_hook<Rel>), gr, bl, 0, st, n, rel, (const int32_t*)w.f.p, (const int32_t*)w.gf.p, w.next.p);
        MGB_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(cc_shortcut, gr, bl, 0, st, n, w.f.p, w.gf.p, (const int32_t*)w.next.p, w.changed.p);
        MGB_HIP_CHECK(hipGetLastError());
        int32_t changed = 0;
        w.changed.download(&changed, 1, st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        if (!changed) return round;
    }
    throw HipError("weld: the component labels did not settle");
}

// ---- compaction: classes numbered by their lowest node

__global__ void __launch_bounds__(BLOCK) root_flags(int64_t n, const int32_t* __restrict__ label, int32_t* __restrict__ flag) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    flag[u] = label[u] == (int32_t)u ? 1 : 0;
}

// id[u] = number of the class of node u; first[class] = its lowest node (first may be NULL)
__global__ void __launch_bounds__(BLOCK) class_ids(int64_t n, const int32_t* __restrict__ label,
                                                   const int32_t* __restrict__ rank, int32_t* __restrict__ id,
                                                   int32_t* __restrict__ first) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    const int32_t r = label[u];
    id[u] = rank[r];
    if (first && r == (int32_t)u) first[rank[r]] = (int32_t)u;
}

struct ScanWork {
    DevBuf<int32_t> flag, rank;
    DevBuf<char> tmp;
};

// the number of classes of label (n nodes); rank[root] is the class of a root on return
int64_t rank_roots(int64_t n, const int32_t* label, ScanWork& w, hipStream_t st) {
    w.flag.ensure((size_t)n); w.rank.ensure((size_t)n);
    hipLaunchKernelGGL(root_flags, dim3(grid_1d(n)), dim3(BLOCK), 0, st, n, label, w.flag.p);
    MGB_HIP_CHECK(hipGetLastError());
    exclusive_scan(w.flag.p, w.rank.p, n, w.tmp, st);
    return scan_total(w.flag.p, w.rank.p, n, st);
}

__global__ void __launch_bounds__(BLOCK) iota(int64_t n, int32_t* __restrict__ v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (int32_t)i;
}

// One lane per vertex: the sum of the face normals cross3(p1 - p0, p2 - p0) of the triangles of its corners, in ascending
// corner order, divided by its length; zeros when the length is 0 or not finite.
__global__ void __launch_bounds__(BLOCK) vertex_normals(int64_t V, const double* __restrict__ x,
                                                        const int32_t* __restrict__ start,
                                                        const int32_t* __restrict__ list, double* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    double n[3] = {0.0, 0.0, 0.0};
    for (int32_t i = start[v]; i < start[v + 1]; ++i) {
        const double* p = x + (int64_t)(list[i] / 3) * 9;
        double a[3], b[3], c[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = p[3 + k] - p[k];
            b[k] = p[6 + k] - p[k];
        }
        cross3(a, b, c);
        for (int k = 0; k < 3; ++k) n[k] += c[k];
    }
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool ok = len > 0.0 && isfinite(len);
    for (int k = 0; k < 3; ++k) normals[v * 3 + k] = ok ? n[k] / len : 0.0;
}

template <int E>
void build(Weld& W, const WeldIn& in, hipStream_t st) {
    const int64_t M = in.S * in.nv;
    const dim3 grM(grid_1d(M)), bl(BLOCK);
    DevBuf<double> x, ubox;
    DevBuf<int32_t> group;
    x.upload(in.points, (size_t)M * E, st);
    if (in.group) group.upload(in.group, (size_t)in.S, st);

    // ---- union box and grid
    ubox.alloc(7);
    hipLaunchKernelGGL(corner_box<E>, dim3(1), dim3(1024), 0, st, M, (const double*)x.p, ubox.p);
    MGB_HIP_CHECK(hipGetLastError());
    double hb[7];
    ubox.download(hb, 7, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    MGB_REQUIRE(hb[6] == 0.0, "weld: a corner has a non-finite coordinate");
    WeldGrid g{};
    double ext_max = 0.0;
    for (int a = 0; a < E; ++a) {
        g.lo[a] = hb[a];
        ext_max = std::fmax(ext_max, hb[3 + a] - hb[a]);
    }
    MGB_REQUIRE(std::isfinite(ext_max), "weld: the extent of the soup is not finite");
    g.tol = in.tol;
    g.h = std::fmax(in.tol, std::ldexp(ext_max, -WELD_GRID_LOG2));

    // ---- one key per corner, one stable sort
    DevBuf<uint64_t> k0, keys;
    DevBuf<int32_t> c0, corner;
    DevBuf<char> tmp;
    k0.alloc((size_t)M); keys.alloc((size_t)M); c0.alloc((size_t)M); corner.alloc((size_t)M);
    hipLaunchKernelGGL(corner_keys<E>, grM, bl, 0, st, M, g, (const double*)x.p, k0.p, c0.p);
    MGB_HIP_CHECK(hipGetLastError());
    sort_pairs(k0.p, keys.p, c0.p, corner.p, M, (unsigned)(E * WELD_AXIS_BITS), tmp, st);

    // ---- occupancy guard, before any pair is tested
    DevBuf<int32_t> most;
    most.alloc(1);
    most.zero(st);
    hipLaunchKernelGGL(cell_occupancy, grM, bl, 0, st, M, (const uint64_t*)keys.p, most.p);
    MGB_HIP_CHECK(hipGetLastError());
    int32_t occupancy = 0;
    most.download(&occupancy, 1, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    if (occupancy > WELD_MAX_CELL) {
        char buf[256];
        snprintf(buf, sizeof(buf), "weld: %d corners fall into one grid cell with tol = %.17g; at most WELD_MAX_CELL = %d "
                 "are welded (the tolerance is far too large for this soup, or the soup is one point)",
                 (int)occupancy, in.tol, WELD_MAX_CELL);
        throw InvalidArgument(buf);
    }

    // ---- vertex classes: components of the link relation over the corners
    CcWork cw;
    ScanWork sw;
    LinkRelation<E> link{g, M, in.nv, x.p, group.p, keys.p, corner.p};
    W.vertex_rounds = connected_components(M, link, cw, st);
    W.V = rank_roots(M, cw.f.p, sw, st);
    W.cells.alloc((size_t)M);
    W.first_corner.alloc((size_t)W.V);
    hipLaunchKernelGGL(class_ids, grM, bl, 0, st, M, (const int32_t*)cw.f.p, (const int32_t*)sw.rank.p, W.cells.p,
                       W.first_corner.p);
    MGB_HIP_CHECK(hipGetLastError());

    // ---- the corners of every vertex, ascending: a stable sort of (vertex, corner)
    DevBuf<int32_t> vkey, vlist, vstart;
    vkey.alloc((size_t)M); vlist.alloc((size_t)M); vstart.alloc((size_t)W.V + 1);
    hipLaunchKernelGGL(iota, grM, bl, 0, st, M, c0.p);
    MGB_HIP_CHECK(hipGetLastError());
    sort_pairs(W.cells.p, vkey.p, c0.p, vlist.p, M, key_bits((uint64_t)W.V), tmp, st);
    // every vertex has a corner, so no segment is empty
    hipLaunchKernelGGL(segment_starts<int32_t>, dim3(grid_1d(M + 1)), bl, 0, st, M, W.V, (const int32_t*)vkey.p, vstart.p);
    MGB_HIP_CHECK(hipGetLastError());

    // ---- components of the welded mesh: the same primitive over the simplex edges
    SimplexRelation edges{in.nv, W.cells.p, vstart.p, vlist.p};
    W.component_rounds = connected_components(W.V, edges, cw, st);
    W.ncomp = rank_roots(W.V, cw.f.p, sw, st);
    W.component.alloc((size_t)W.V);
    hipLaunchKernelGGL(class_ids, dim3(grid_1d(W.V)), bl, 0, st, W.V, (const int32_t*)cw.f.p, (const int32_t*)sw.rank.p,
                       W.component.p, (int32_t*)nullptr);
    MGB_HIP_CHECK(hipGetLastError());

    if constexpr (E == 3) {
        if (in.want_normals) {
            W.normals.alloc((size_t)W.V * 3);
            hipLaunchKernelGGL(vertex_normals, dim3(grid_1d(W.V)), bl, 0, st, W.V, (const double*)x.p,
                               (const int32_t*)vstart.p, (const int32_t*)vlist.p, W.normals.p);
            MGB_HIP_CHECK(hipGetLastError());
            W.has_normals = true;
        }
    }
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    // the soup, the sorted keys, the labels and the lists are freed at scope exit
}

}  // namespace

void weld_build(Weld& W, const WeldIn& in, hipStream_t st) {
    W.S = in.S;
    W.nv = in.nv;
    W.e = in.e;
    if (in.e == 3) build<3>(W, in, st);
    else build<2>(W, in, st);
}

void weld_fetch(const Weld& W, int32_t* cells, int32_t* first_corner, int32_t* component, double* normals, hipStream_t st) {
    W.cells.download(cells, (size_t)W.S * W.nv, st);
    W.first_corner.download(first_corner, (size_t)W.V, st);
    W.component.download(component, (size_t)W.V, st);
    if (normals && W.has_normals) W.normals.download(normals, (size_t)W.V * 3, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
