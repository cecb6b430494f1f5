// The segments of an indexed curve mesh ordered into lines: mgbhip_polyline_* (include/mgbhip.h).
//
// The reference gets ordered, indexed PolyData from PyVista; the level curves of contour.hip, the boundary edges of a welded
// surface and a welded Streamlines are unordered segments in launch order and random orientation.  Ordering a chain is
// list ranking, done here by pointer doubling: one lane per directed half-edge h = 2 * segment + dir (dir 0 runs from
// cells[s][0] to cells[s][1]), ceil(log2(2 S)) + 1 rounds, whatever the length of the longest line.
//
//  1. Edges.  One 64-bit key lo * V + hi per segment and one stable radix sort of (key, segment): a segment is dropped if
//     its two vertices are equal or if the sorted position before it holds the same key (the lower-numbered copy is kept).
//     Edges keep their segment numbers, so "the lowest segment of a line" needs no translation.
//  2. Vertex lists.  A second stable sort of (tail vertex, half-edge) over the half-edges of the edges (those of dropped
//     segments sort behind vertex V - 1) and segment_starts(): the half-edges that leave v are list[start[v] .. start[v+1]),
//     ascending, and val[v] is their number.
//  3. Successors.  h heads to v.  With val[v] == 2 succ(h) is the half-edge leaving v that is not the twin h ^ 1; else h
//     is terminal, succ(h) = NIL.  An open line is two NIL-terminated lists (one per direction), a closed line two cycles.
//  4. Pointer doubling; every round reads one set of arrays and writes the other, so neither the results nor the number of
//     rounds depend on scheduling.
//     a. The cycle pass carries (next, lowest tail vertex).  After the rounds a half-edge whose next is not NIL lies on a
//        cycle and knows the cycle's lowest vertex v0; the half-edge of each of the two directed cycles that heads to v0
//        becomes terminal.  Every line is now two lists, one the reverse of the other.
//     b. The ranking pass carries (next, last, count, lowest segment, length) over the half-edges from h to the end of its
//        list.  With the twin's values h knows the whole line: n = count[h] + count[h^1] - 1 edges, lowest segment
//        min(low[h], low[h^1]), its own rank count[h^1] - 1, the two ends last[h] and last[h^1], and the arc length at its
//        head, length[h^1]: the lengths of the edges before and including h, added in the order of the doubling tree.
//  5. Direction and numbering.  The list of h starts where the twin's list ends.  Open lines: the list that starts at the
//     smaller end vertex is kept, or with equal ends (a loop through a junction) the one whose first edge has the lower
//     segment number.  Closed lines: both lists start at v0 and the one with the smaller second vertex is kept.  A flag
//     scan over the segments that are the lowest of their line numbers the lines; an exclusive scan of n + 1 per line gives
//     offsets.  (line, rank) then names the position of every kept half-edge outright, so vertex, segment and arclength
//     are scattered there: the sort by (line, rank) that would do the same is not needed.
//
// No atomics at all and no floating-point sums outside the doubling tree; two calls return bitwise equal arrays.
//
// polyline_sample() is stateless: one lane per query (line, s) clamps s, searches the line's slice of arclength and
// interpolates the points and every data column between the two neighbours.
#include <hip/hip_runtime.h>

#include <cmath>
#include <utility>

#include "device_prims.hpp"
#include "polyline.hpp"

// No fused multiply-adds in this file: the twin (tests/polyline_twin.py) evaluates the same lengths and the same interpolant.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

constexpr int32_t NIL = -1;

__device__ inline int32_t tail_of(const int32_t* __restrict__ cells, int32_t h) { return cells[h]; }
__device__ inline int32_t head_of(const int32_t* __restrict__ cells, int32_t h) { return cells[h ^ 1]; }

// ---- 1. edges

__global__ void __launch_bounds__(BLOCK) edge_keys(int64_t S, int64_t V, const int32_t* __restrict__ cells,
                                                   uint64_t* __restrict__ keys, int32_t* __restrict__ seg) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int64_t a = cells[2 * s], b = cells[2 * s + 1];
    keys[s] = (uint64_t)((a < b ? a : b) * V + (a < b ? b : a));
    seg[s] = (int32_t)s;
}

// one lane per sorted position: kept[segment] = 1 for the first segment of every key whose two vertices differ
__global__ void __launch_bounds__(BLOCK) edge_flags(int64_t S, const uint64_t* __restrict__ keys,
                                                    const int32_t* __restrict__ seg, const int32_t* __restrict__ cells,
                                                    int32_t* __restrict__ kept) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const int32_t s = seg[i];
    const bool degenerate = cells[2 * (int64_t)s] == cells[2 * (int64_t)s + 1];
    const bool duplicate = i > 0 && keys[i - 1] == keys[i];
    kept[s] = (degenerate || duplicate) ? 0 : 1;
}

// ---- 2. the half-edges that leave every vertex

__global__ void __launch_bounds__(BLOCK) tail_keys(int64_t H, int64_t V, const int32_t* __restrict__ cells,
                                                   const int32_t* __restrict__ kept, int32_t* __restrict__ keys,
                                                   int32_t* __restrict__ half) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    keys[h] = kept[h >> 1] ? cells[h] : (int32_t)V;
    half[h] = (int32_t)h;
}

// ---- 3. successors, and the length of every half-edge

template <int E>
__global__ void __launch_bounds__(BLOCK) successors(int64_t H, const int32_t* __restrict__ cells,
                                                    const int32_t* __restrict__ kept, const int32_t* __restrict__ start,
                                                    const int32_t* __restrict__ list, const double* __restrict__ x,
                                                    int32_t* __restrict__ succ, double* __restrict__ len) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    int32_t nx = NIL;
    double l = 0.0;
    if (kept[h >> 1]) {
        const int32_t t = tail_of(cells, (int32_t)h), v = head_of(cells, (int32_t)h);
        const int32_t s0 = start[v];
        if (start[v + 1] - s0 == 2) {
            const int32_t a = list[s0], b = list[s0 + 1];
            nx = a == (int32_t)(h ^ 1) ? b : a;
        }
        double q = 0.0;
        for (int c = 0; c < E; ++c) {
            const double d = x[(int64_t)v * E + c] - x[(int64_t)t * E + c];
            q = c == 0 ? d * d : q + d * d;
        }
        l = sqrt(q);
    }
    succ[h] = nx;
    len[h] = l;
}

// ---- 4a. the cycle pass: next and the lowest tail vertex over the half-edges from h up to (not including) next

__global__ void __launch_bounds__(BLOCK) cycle_init(int64_t H, const int32_t* __restrict__ cells,
                                                    const int32_t* __restrict__ succ, int32_t* __restrict__ next,
                                                    int32_t* __restrict__ low) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    next[h] = succ[h];
    low[h] = cells[h];
}

__global__ void __launch_bounds__(BLOCK) cycle_round(int64_t H, const int32_t* __restrict__ next,
                                                     const int32_t* __restrict__ low, int32_t* __restrict__ next_out,
                                                     int32_t* __restrict__ low_out) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    const int32_t n = next[h];
    int32_t m = low[h], nn = NIL;
    if (n != NIL) {
        m = min(m, low[n]);
        nn = next[n];
    }
    next_out[h] = nn;
    low_out[h] = m;
}

// A half-edge whose next is still set lies on a cycle (on[h] = 1); the one that heads to the cycle's lowest vertex ends it.
__global__ void __launch_bounds__(BLOCK) cycle_cut(int64_t H, const int32_t* __restrict__ cells,
                                                   const int32_t* __restrict__ next, const int32_t* __restrict__ low,
                                                   int32_t* __restrict__ succ, uint8_t* __restrict__ on) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    const bool cyc = next[h] != NIL;
    on[h] = cyc ? 1 : 0;
    if (cyc && head_of(cells, (int32_t)h) == low[h]) succ[h] = NIL;
}

// ---- 4b. the ranking pass: over the half-edges from h up to (not including) next, the last of them, their number, their
// lowest segment and the sum of their lengths

struct Rank {
    int32_t* next;
    int32_t* last;
    int32_t* count;
    int32_t* low;
    double* length;
};

__global__ void __launch_bounds__(BLOCK) rank_init(int64_t H, const int32_t* __restrict__ succ,
                                                   const double* __restrict__ len, Rank r) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    r.next[h] = succ[h];
    r.last[h] = (int32_t)h;
    r.count[h] = 1;
    r.low[h] = (int32_t)(h >> 1);
    r.length[h] = len[h];
}

__global__ void __launch_bounds__(BLOCK) rank_round(int64_t H, Rank a, Rank b) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    const int32_t n = a.next[h];
    int32_t nn = NIL, last = a.last[h], count = a.count[h], low = a.low[h];
    double length = a.length[h];
    if (n != NIL) {
        nn = a.next[n];
        last = a.last[n];
        count += a.count[n];
        low = min(low, a.low[n]);
        length = length + a.length[n];
    }
    b.next[h] = nn;
    b.last[h] = last;
    b.count[h] = count;
    b.low[h] = low;
    b.length[h] = length;
}

// ---- 5. direction, numbering, scatter

// flag[s] = 1 for the lowest segment of every line
__global__ void __launch_bounds__(BLOCK) line_flags(int64_t S, const int32_t* __restrict__ kept,
                                                    const int32_t* __restrict__ low, int32_t* __restrict__ flag) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    flag[s] = (kept[s] && min(low[2 * s], low[2 * s + 1]) == (int32_t)s) ? 1 : 0;
}

// the lowest segment of a line writes its number of points and whether it is closed
__global__ void __launch_bounds__(BLOCK) line_sizes(int64_t S, const int32_t* __restrict__ flag,
                                                    const int32_t* __restrict__ id, const int32_t* __restrict__ count,
                                                    const uint8_t* __restrict__ on, int64_t* __restrict__ npoints,
                                                    uint8_t* __restrict__ closed) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S || !flag[s]) return;
    const int32_t l = id[s];
    npoints[l] = (int64_t)count[2 * s] + count[2 * s + 1];      // n edges = the sum - 1, n + 1 points
    closed[l] = on[2 * s];
}

// One lane per half-edge.  The list of h starts where the list of its twin ends (at e2 = last[h ^ 1]) and ends at
// e1 = last[h]; h is kept if its list starts at the smaller vertex, then along the lower segment (open), or has the smaller
// second vertex (closed).  A kept half-edge of rank j writes point j, the arc length of point j + 1, and the last one the
// closing point too.
__global__ void __launch_bounds__(BLOCK) scatter_points(int64_t H, const int32_t* __restrict__ cells,
                                                        const int32_t* __restrict__ kept, const uint8_t* __restrict__ on,
                                                        Rank r, const int32_t* __restrict__ id,
                                                        const int64_t* __restrict__ offsets, int32_t* __restrict__ vertex,
                                                        int32_t* __restrict__ segment, double* __restrict__ arclength) {
    const int64_t hh = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (hh >= H || !kept[hh >> 1]) return;
    const int32_t h = (int32_t)hh, w = h ^ 1;
    const int32_t e1 = r.last[h], e2 = r.last[w];
    bool forward;
    if (on[h]) {
        forward = tail_of(cells, e2) < tail_of(cells, e1);
    } else {
        const int32_t v1 = head_of(cells, e1), v2 = head_of(cells, e2);
        forward = v2 < v1 || (v2 == v1 && (e2 >> 1) < (e1 >> 1));
    }
    if (!forward) return;
    const int32_t l = id[min(r.low[h], r.low[w])];
    const int64_t p = offsets[l] + (r.count[w] - 1);
    vertex[p] = tail_of(cells, h);
    segment[p] = h >> 1;
    arclength[p + 1] = r.length[w];
    if (r.count[w] == 1) arclength[p] = 0.0;
    if (r.count[h] == 1) {
        vertex[p + 1] = head_of(cells, h);
        segment[p + 1] = -1;
    }
}

struct RankBuf {
    DevBuf<int32_t> next, last, count, low;
    DevBuf<double> length;
    void alloc(size_t n) { next.alloc(n); last.alloc(n); count.alloc(n); low.alloc(n); length.alloc(n); }
    Rank view() { return Rank{next.p, last.p, count.p, low.p, length.p}; }
};

template <int E>
void build(Polyline& Pl, const PolylineIn& in, hipStream_t st) {
    const int64_t S = in.S, V = in.V, H = 2 * S;
    const dim3 grS(grid_1d(S)), grH(grid_1d(H)), bl(BLOCK);
    DevBuf<double> x;
    DevBuf<int32_t> cells;
    x.upload(in.vertices, (size_t)V * E, st);
    cells.upload(in.cells, (size_t)H, st);

    // ---- 1. edges: one key per segment, one stable sort, the first of every key is kept
    DevBuf<uint64_t> k0, keys;
    DevBuf<int32_t> s0, seg, kept;
    DevBuf<char> tmp;
    k0.alloc((size_t)S); keys.alloc((size_t)S); s0.alloc((size_t)S); seg.alloc((size_t)S); kept.alloc((size_t)S);
    hipLaunchKernelGGL(edge_keys, grS, bl, 0, st, S, V, (const int32_t*)cells.p, k0.p, s0.p);
    MGB_HIP_CHECK(hipGetLastError());
    sort_pairs(k0.p, keys.p, s0.p, seg.p, S, key_bits((uint64_t)V * (uint64_t)V), tmp, st);
    hipLaunchKernelGGL(edge_flags, grS, bl, 0, st, S, (const uint64_t*)keys.p, (const int32_t*)seg.p,
                       (const int32_t*)cells.p, kept.p);
    MGB_HIP_CHECK(hipGetLastError());

    // ---- 2. the half-edges that leave every vertex, ascending: a stable sort of (tail, half-edge)
    DevBuf<int32_t> t0, tkey, h0, list, start;
    t0.alloc((size_t)H); tkey.alloc((size_t)H); h0.alloc((size_t)H); list.alloc((size_t)H); start.alloc((size_t)V + 2);
    hipLaunchKernelGGL(tail_keys, grH, bl, 0, st, H, V, (const int32_t*)cells.p, (const int32_t*)kept.p, t0.p, h0.p);
    MGB_HIP_CHECK(hipGetLastError());
    sort_pairs(t0.p, tkey.p, h0.p, list.p, H, key_bits((uint64_t)V), tmp, st);
    hipLaunchKernelGGL(segment_starts<int32_t>, dim3(grid_1d(H + 1)), bl, 0, st, H, V + 1, (const int32_t*)tkey.p, start.p);
    MGB_HIP_CHECK(hipGetLastError());

    // ---- 3. successors
    DevBuf<int32_t> succ;
    DevBuf<double> len;
    succ.alloc((size_t)H); len.alloc((size_t)H);
    hipLaunchKernelGGL(successors<E>, grH, bl, 0, st, H, (const int32_t*)cells.p, (const int32_t*)kept.p,
                       (const int32_t*)start.p, (const int32_t*)list.p, (const double*)x.p, succ.p, len.p);
    MGB_HIP_CHECK(hipGetLastError());

    // ---- 4. pointer doubling: 2^rounds >= 2 H exceeds the length of every list and of every cycle
    const int32_t rounds = (int32_t)key_bits((uint64_t)(H - 1)) + 1;      // ceil(log2 H) + 1 for H >= 2
    RankBuf ra, rb;
    ra.alloc((size_t)H); rb.alloc((size_t)H);
    DevBuf<uint8_t> on;
    on.alloc((size_t)H);
    {
        // a. next and lowest vertex, in the buffers of the ranking pass
        int32_t *na = ra.next.p, *la = ra.low.p, *nb = rb.next.p, *lb = rb.low.p;
        hipLaunchKernelGGL(cycle_init, grH, bl, 0, st, H, (const int32_t*)cells.p, (const int32_t*)succ.p, na, la);
        MGB_HIP_CHECK(hipGetLastError());
        for (int32_t r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(cycle_round, grH, bl, 0, st, H, (const int32_t*)na, (const int32_t*)la, nb, lb);
            MGB_HIP_CHECK(hipGetLastError());
            std::swap(na, nb);
            std::swap(la, lb);
        }
        hipLaunchKernelGGL(cycle_cut, grH, bl, 0, st, H, (const int32_t*)cells.p, (const int32_t*)na, (const int32_t*)la,
                           succ.p, on.p);
        MGB_HIP_CHECK(hipGetLastError());
    }
    Rank a = ra.view(), b = rb.view();
    hipLaunchKernelGGL(rank_init, grH, bl, 0, st, H, (const int32_t*)succ.p, (const double*)len.p, a);
    MGB_HIP_CHECK(hipGetLastError());
    for (int32_t r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(rank_round, grH, bl, 0, st, H, a, b);
        MGB_HIP_CHECK(hipGetLastError());
        std::swap(a, b);
    }
    Pl.rounds[0] = Pl.rounds[1] = rounds;

    // ---- 5. lines numbered by their lowest segment
    DevBuf<int32_t> flag, id;
    flag.alloc((size_t)S); id.alloc((size_t)S);
    hipLaunchKernelGGL(line_flags, grS, bl, 0, st, S, (const int32_t*)kept.p, (const int32_t*)a.low, flag.p);
    MGB_HIP_CHECK(hipGetLastError());
    exclusive_scan(flag.p, id.p, S, tmp, st);
    const int64_t L = scan_total(flag.p, id.p, S, st);
    Pl.L = L;
    Pl.offsets.alloc((size_t)L + 1);
    Pl.closed.alloc((size_t)L);
    if (L == 0) {                          // every segment was dropped
        Pl.offsets.zero(st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        Pl.P = 0;
        Pl.ndropped = S;
        return;
    }
    DevBuf<int64_t> npoints;
    npoints.alloc((size_t)L + 1);
    npoints.zero(st);
    hipLaunchKernelGGL(line_sizes, grS, bl, 0, st, S, (const int32_t*)flag.p, (const int32_t*)id.p,
                       (const int32_t*)a.count, (const uint8_t*)on.p, npoints.p, Pl.closed.p);
    MGB_HIP_CHECK(hipGetLastError());
    exclusive_scan(npoints.p, Pl.offsets.p, L + 1, tmp, st);
    int64_t P = 0;
    MGB_HIP_CHECK(hipMemcpyAsync(&P, Pl.offsets.p + L, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    Pl.P = P;
    Pl.ndropped = S - (P - L);             // every line of n edges has n + 1 points
    Pl.vertex.alloc((size_t)P); Pl.segment.alloc((size_t)P); Pl.arclength.alloc((size_t)P);
    hipLaunchKernelGGL(scatter_points, grH, bl, 0, st, H, (const int32_t*)cells.p, (const int32_t*)kept.p,
                       (const uint8_t*)on.p, a, (const int32_t*)id.p, (const int64_t*)Pl.offsets.p, Pl.vertex.p,
                       Pl.segment.p, Pl.arclength.p);
    MGB_HIP_CHECK(hipGetLastError());
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    // the mesh, the sorted keys, the lists and the doubling buffers are freed at scope exit
}

// ---- the sampler

// One lane per query.  The line's points are o0 .. o1 - 1 and its n = o1 - o0 - 1 edges run between neighbours; j is the
// last edge whose first point lies at or before s.
template <int E>
__global__ void __launch_bounds__(BLOCK) sample_lines(int64_t Q, int32_t C, const double* __restrict__ x,
                                                      const double* __restrict__ data,
                                                      const int64_t* __restrict__ offsets,
                                                      const double* __restrict__ arc, const int32_t* __restrict__ line,
                                                      const double* __restrict__ sq, double* __restrict__ out_x,
                                                      double* __restrict__ out_data) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const int64_t o0 = offsets[line[q]], o1 = offsets[line[q] + 1];
    const double* a = arc + o0;
    const int64_t n = o1 - o0 - 1;
    double s = sq[q];
    s = s < 0.0 ? 0.0 : s;
    s = s > a[n] ? a[n] : s;
    int64_t lo = 0, hi = n;                // first j in [0, n) with a[j] > s, or n
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= s) lo = mid + 1;
        else hi = mid;
    }
    const int64_t j = lo - 1;              // a[0] = 0 <= s, so lo >= 1
    const double d = a[j + 1] - a[j];
    const double t = d == 0.0 ? 0.0 : (s - a[j]) / d;
    const int64_t p = o0 + j;
    for (int c = 0; c < E; ++c) {
        const double u = x[p * E + c], v = x[(p + 1) * E + c];
        out_x[q * E + c] = u + t * (v - u);
    }
    for (int32_t c = 0; c < C; ++c) {
        const double u = data[p * C + c], v = data[(p + 1) * C + c];
        out_data[q * C + c] = u + t * (v - u);
    }
}

}  // namespace

void polyline_build(Polyline& Pl, const PolylineIn& in, hipStream_t st) {
    Pl.S = in.S;
    Pl.V = in.V;
    Pl.e = in.e;
    if (in.S == 0) {
        Pl.offsets.alloc(1);
        Pl.offsets.zero(st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        return;
    }
    if (in.e == 3) build<3>(Pl, in, st);
    else build<2>(Pl, in, st);
}

void polyline_fetch(const Polyline& Pl, int64_t* offsets, int32_t* vertex, int32_t* segment, uint8_t* closed,
                    double* arclength, double* length, hipStream_t st) {
    Pl.offsets.download(offsets, (size_t)Pl.L + 1, st);
    Pl.vertex.download(vertex, (size_t)Pl.P, st);
    Pl.segment.download(segment, (size_t)Pl.P, st);
    Pl.closed.download(closed, (size_t)Pl.L, st);
    Pl.arclength.download(arclength, (size_t)Pl.P, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t l = 0; l < Pl.L; ++l) length[l] = arclength[offsets[l + 1] - 1];
}

void polyline_sample(const PolylineSampleIn& in, double* out_points, double* out_data, hipStream_t st) {
    if (in.Q == 0) return;
    DevBuf<double> x, data, arc, s, ox, od;
    DevBuf<int64_t> offsets;
    DevBuf<int32_t> line;
    x.upload(in.points, (size_t)in.P * in.e, st);
    if (in.C) data.upload(in.data, (size_t)in.P * in.C, st);
    offsets.upload(in.offsets, (size_t)in.L + 1, st);
    arc.upload(in.arclength, (size_t)in.P, st);
    line.upload(in.line, (size_t)in.Q, st);
    s.upload(in.s, (size_t)in.Q, st);
    ox.alloc((size_t)in.Q * in.e);
    if (in.C) od.alloc((size_t)in.Q * in.C);
    const dim3 gr(grid_1d(in.Q)), bl(BLOCK);
    if (in.e == 3)
        hipLaunchKernelGGL(sample_lines<3>, gr, bl, 0, st, in.Q, in.C, (const double*)x.p, (const double*)data.p,
                           (const int64_t*)offsets.p, (const double*)arc.p, (const int32_t*)line.p, (const double*)s.p,
                           ox.p, od.p);
    else
        hipLaunchKernelGGL(sample_lines<2>, gr, bl, 0, st, in.Q, in.C, (const double*)x.p, (const double*)data.p,
                           (const int64_t*)offsets.p, (const double*)arc.p, (const int32_t*)line.p, (const double*)s.p,
                           ox.p, od.p);
    MGB_HIP_CHECK(hipGetLastError());
    ox.download(out_points, (size_t)in.Q * in.e, st);
    if (in.C) od.download(out_data, (size_t)in.Q * in.C, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
