// Level sets of an element-space function, cut straight from the elements: mgbhip_contour_* (include/mgbhip.h).
//
// The reference draws isosurfaces and slices by handing a VTK grid to PyVista on the CPU
// (ext/MultiGridBarrierPyPlotExt/plot3d.jl:85-150); it has no contouring code of its own.  Here every element is sampled
// on a uniform reference lattice with its own basis (value, physical position and carried fields), the lattice cells are
// split into simplices (two triangles per square along the (i, j)-(i+1, j+1) diagonal, the r^2 triangles of the uniform
// subdivision of a triangle, the six Kuhn tetrahedra of a cube around its (i, j, k)-(i+1, j+1, k+1) diagonal), and every
// simplex is cut linearly at every level.  There are no case tables: the vertices of a simplex are in ascending lattice
// order by construction, its edges are walked in ascending (a, b) order, and a crossing is always computed from the
// endpoint of lower lattice index, so the two simplices that share an edge compute the same bits.
//
// One workgroup (one wave when the element has few simplices) per element.  The lattice is formed once per element
// into LDS and every simplex reads it from there.  Two passes of the same kernel: the count pass forms the lattice of
// the contoured values only and writes one count per element; after an exclusive scan over the elements the emit pass
// forms the full lattice and writes the simplices.  Inside an element every thread owns a contiguous run of simplices
// and a block scan of the per-thread counts places the runs, so the output order (element, cell, simplex of the cell,
// level, triangle of a 2-2 split) does not depend on the launch: there are no atomics.
//
// A Q_k 2-D mesh may sit in R^3 (a surface): the lattice then has E = 3 position slots, each coordinate the same sum as
// the two of a flat mesh, and the level curves are segments in R^3.
//
// mgbhip_tessellate_* emits the lattice triangles themselves instead of their cuts (tessellate_kernel): the same lattice
// (form_lattice is the one copy of the sampling), the same enumeration, triangle i of element e at e * ntri + i.  The
// count is a function of N and refine alone, so there is no count pass, no scan and nothing to place.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "contour.hpp"
#include "device_prims.hpp"

// No fused multiply-adds in this file: a plain IEEE transcription of the algorithm (tests/contour_twin.py) then
// classifies every lattice value the same way and computes the same crossings.
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

constexpr int KIND_Q2 = 0, KIND_Q3 = 1, KIND_TRI = 2;
// what form_lattice samples: the contoured value alone; value, position, carried fields; position, fields
constexpr int MODE_COUNT = 0, MODE_EMIT = 1, MODE_TESS = 2;

struct ContourArgs {
    int64_t N, S;
    int32_t p, k, r, nfield, nlevels;
    int32_t npts, nsimp, chunk, table_len;
    const double* x;
    const double* table;       // Q_k: (r + 1) x (k + 1) basis values at the lattice coordinates; P1 / P2: p x 10
    const double* fields;
    const double* levels;
    const int64_t* off;        // emit pass: first simplex of each element
    int64_t* count;            // count pass: simplices of each element
    double* points;
    int32_t* level;
    int32_t* element;
    double* carried;
    double* values;            // tessellation: T x 3 x nfield
};

// first lattice index of row j of the barycentric lattice of the r-fold subdivision (row j holds r + 1 - j points)
__device__ inline int tri_row(int j, int r) { return j * (r + 1) - (j * (j - 1)) / 2; }

// lattice indices of the vertices of simplex s of an element, ascending
template <int KIND>
__device__ inline void simplex_vertices(int s, int r, int (&v)[KIND == KIND_Q3 ? 4 : 3]) {
    const int n1 = r + 1;
    if constexpr (KIND == KIND_Q2) {
        const int cell = s >> 1, w = s & 1;
        const int i = cell % r, j = cell / r;
        const int base = j * n1 + i;
        v[0] = base;
        v[1] = w ? base + n1 : base + 1;
        v[2] = base + n1 + 1;
    } else if constexpr (KIND == KIND_Q3) {
        const int cell = s / 6, w = s % 6;
        const int i = cell % r, j = (cell / r) % r, l = cell / (r * r);
        const int base = (l * n1 + j) * n1 + i;
        // Kuhn tetrahedron w: the axis permutation (a, b, c) in lexicographic order; its path is base, +e_a, +e_b, +e_c
        const int a = w >> 1;
        const int lo = a == 0 ? 1 : 0, hi = a == 2 ? 1 : 2;
        const int b = (w & 1) ? hi : lo;
        const int sa = a == 0 ? 1 : (a == 1 ? n1 : n1 * n1);
        const int sb = b == 0 ? 1 : (b == 1 ? n1 : n1 * n1);
        v[0] = base;
        v[1] = base + sa;
        v[2] = base + sa + sb;
        v[3] = base + 1 + n1 + n1 * n1;
    } else {
        // row j holds 2 (r - j) - 1 triangles: per cell i the upright one, then (but for the last cell) the inverted one
        int j = 0;
        while (j + 1 < r && 2 * r * (j + 1) - (j + 1) * (j + 1) <= s) ++j;
        const int q = s - (2 * r * j - j * j);
        const int i = q >> 1;
        const int r0 = tri_row(j, r) + i, r1 = tri_row(j + 1, r) + i;
        if (q & 1) {
            v[0] = r0 + 1;
            v[1] = r1;
            v[2] = r1 + 1;
        } else {
            v[0] = r0;
            v[1] = r0 + 1;
            v[2] = r1;
        }
    }
}

// The lattice of element e into LDS, slot-major, E position slots (E = 3 > D: a Q_k 2-D surface in R^3).
// MODE_COUNT: slot 0, the contoured value.  MODE_EMIT: slot 0 the contoured value, slots 1..E the position, slot E + c
// carried field c (field column c, c >= 1).  MODE_TESS: slots 0..E-1 the position, slot E + c field column c (c >= 0).
// Every slot is its own sum of p products in ascending node order.  The caller synchronises before and after.
template <int KIND, int E, int MODE>
__device__ __forceinline__ void form_lattice(const ContourArgs& a, int64_t e, double* lat, const double* tab, int tid,
                                             int nthr) {
    constexpr int NSLOT = MODE == MODE_COUNT ? 1 : E + CONTOUR_MAX_FIELDS;
    constexpr int P0 = MODE == MODE_EMIT ? 1 : 0;      // first position slot
    constexpr int F0 = MODE == MODE_EMIT ? 1 : 0;      // first field column that goes to slot E + column
    const int npts = a.npts, r = a.r, nf = a.nfield;
    const int nslot = MODE == MODE_COUNT ? 1 : E + nf;
    const double* fe = a.fields + e * a.p * nf;
    const double* xe = a.x + e * a.p * E;
    for (int pt = tid; pt < npts; pt += nthr) {
        double acc[NSLOT];
#pragma unroll
        for (int f = 0; f < NSLOT; ++f) acc[f] = 0.0;
        auto add = [&](double phi, int node) {
            if constexpr (MODE != MODE_TESS) acc[0] += phi * fe[node * nf];
            if constexpr (MODE != MODE_COUNT) {
#pragma unroll
                for (int c = 0; c < E; ++c) acc[P0 + c] += phi * xe[node * E + c];
#pragma unroll
                for (int c = F0; c < CONTOUR_MAX_FIELDS; ++c)
                    if (c < nf) acc[E + c] += phi * fe[node * nf + c];
            }
        };
        if constexpr (KIND == KIND_TRI) {
            int j = 0;
            while (j < r && tri_row(j + 1, r) <= pt) ++j;
            const int i = pt - tri_row(j, r);
            const double l1 = (double)i / (double)r, l2 = (double)j / (double)r;
            const double mono[10] = {1.0, l1, l2, l1 * l1, l1 * l2, l2 * l2, l1 * l1 * l1, l1 * l1 * l2, l1 * l2 * l2, l2 * l2 * l2};
            for (int node = 0; node < a.p; ++node) {
                double phi = 0.0;
#pragma unroll
                for (int m = 0; m < 10; ++m) phi += tab[node * 10 + m] * mono[m];
                add(phi, node);
            }
        } else {
            constexpr int D = KIND == KIND_Q3 ? 3 : 2;
            const int n1 = r + 1, S = a.k + 1;
            const double* b0 = tab + (pt % n1) * S;
            const double* b1 = tab + ((pt / n1) % n1) * S;
            const double* b2 = tab + (D == 3 ? pt / (n1 * n1) : 0) * S;
            const int n2 = D == 3 ? S : 1;
            int node = 0;
            for (int i2 = 0; i2 < n2; ++i2)
                for (int i1 = 0; i1 < S; ++i1)
                    for (int i0 = 0; i0 < S; ++i0, ++node) {
                        const double phi = D == 2 ? b0[i0] * b1[i1] : b0[i0] * b1[i1] * b2[i2];
                        add(phi, node);
                    }
        }
#pragma unroll
        for (int f = 0; f < NSLOT; ++f)
            if (f < nslot) lat[f * npts + pt] = acc[f];
    }
}

// EMIT = false: a.count[e] = simplices of element e.  EMIT = true: the simplices of element e from a.off[e] on.
// LDS: the lattice of form_lattice (MODE_COUNT / MODE_EMIT), then the table.  E = D but for a Q_k 2-D surface (E = 3).
template <int KIND, int E, bool EMIT>
__global__ void __launch_bounds__(BLOCK) contour_kernel(ContourArgs a) {
    constexpr int D = KIND == KIND_Q3 ? 3 : 2;
    constexpr int NSLOT = EMIT ? E + CONTOUR_MAX_FIELDS : 1;
    extern __shared__ double lds[];
    __shared__ int64_t sc[BLOCK];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int64_t e = blockIdx.x;
    const int npts = a.npts, r = a.r, nf = a.nfield;
    const int nslot = EMIT ? E + nf : 1;
    double* lat = lds;
    double* tab = lds + (size_t)nslot * npts;
    for (int i = tid; i < a.table_len; i += nthr) tab[i] = a.table[i];
    __syncthreads();

    // ---- the lattice of this element
    form_lattice<KIND, E, EMIT ? MODE_EMIT : MODE_COUNT>(a, e, lat, tab, tid, nthr);
    __syncthreads();

    // ---- the simplices of this thread: [s0, s1)
    const int s0 = min(tid * a.chunk, a.nsimp), s1 = min(s0 + a.chunk, a.nsimp);
    // pass 0 counts; pass 1 (EMIT only) walks the same simplices again and writes from the scanned offset on
    int64_t total = 0, o = 0;
    for (int pass = 0; pass < (EMIT ? 2 : 1); ++pass) {
        for (int s = s0; s < s1; ++s) {
            int v[D + 1];
            simplex_vertices<KIND>(s, r, v);
            double val[D + 1];
            bool finite = true;
#pragma unroll
            for (int q = 0; q <= D; ++q) {
                val[q] = lat[v[q]];
                finite = finite && isfinite(val[q]);
            }
            if (!finite) continue;
            double vmin = val[0], vmax = val[0];
#pragma unroll
            for (int q = 1; q <= D; ++q) {
                vmin = fmin(vmin, val[q]);
                vmax = fmax(vmax, val[q]);
            }
            for (int l = 0; l < a.nlevels; ++l) {
                const double c = a.levels[l];
                if (!(vmin < c && c <= vmax)) continue;       // all vertices on one side
                int above = 0;
#pragma unroll
                for (int q = 0; q <= D; ++q) above += val[q] >= c ? 1 : 0;
                const bool two = D == 3 && above == 2;        // a 2-2 split: a quadrilateral, two triangles
                const int ntri = two ? 2 : 1;
                if (pass == 0) {
                    total += ntri;
                    continue;
                }
                if constexpr (EMIT) {
                    if (o + ntri > a.S) return;               // cannot happen: both passes count alike
                    for (int t = 0; t < ntri; ++t) {
                        a.level[o + t] = l;
                        a.element[o + t] = (int32_t)e;
                    }
                    // cut edges in ascending (a, b) order: q0, q1, (q2, (q3)).  A quadrilateral q0 q1 q3 q2 is split
                    // along the diagonal through q0 into (q0, q1, q3) and (q0, q2, q3).
                    int n = 0;
#pragma unroll
                    for (int qa = 0; qa < D; ++qa)
#pragma unroll
                        for (int qb = qa + 1; qb <= D; ++qb) {
                            const double va = val[qa], vb = val[qb];
                            if ((va >= c) == (vb >= c)) continue;
                            const double t = (c - va) / (vb - va);
                            // where vertex n goes: (simplex, corner), and for a quadrilateral's q0 and q3 a second place
                            int64_t t0 = o, t1 = -1;
                            int c0 = n, c1 = 0;
                            if (two) {
                                if (n == 0) { t1 = o + 1; }
                                else if (n == 2) { t0 = o + 1; c0 = 1; }
                                else if (n == 3) { c0 = 2; t1 = o + 1; c1 = 2; }
                            }
#pragma unroll
                            for (int f = 1; f < NSLOT; ++f) {
                                if (f >= nslot) continue;
                                const double fa = lat[f * npts + v[qa]], fb = lat[f * npts + v[qb]];
                                const double w = fa + t * (fb - fa);
                                if (f <= E) {
                                    a.points[(t0 * D + c0) * E + (f - 1)] = w;
                                    if (t1 >= 0) a.points[(t1 * D + c1) * E + (f - 1)] = w;
                                } else {
                                    const int nc = nf - 1;
                                    a.carried[(t0 * D + c0) * nc + (f - E - 1)] = w;
                                    if (t1 >= 0) a.carried[(t1 * D + c1) * nc + (f - E - 1)] = w;
                                }
                            }
                            ++n;
                        }
                    o += ntri;
                }
            }
        }
        if (pass == 0) {
            // inclusive scan of the per-thread counts over the block
            sc[tid] = total;
            __syncthreads();
            for (int h = 1; h < nthr; h <<= 1) {
                const int64_t add = tid >= h ? sc[tid - h] : 0;
                __syncthreads();
                sc[tid] += add;
                __syncthreads();
            }
            if constexpr (EMIT) o = a.off[e] + sc[tid] - total;
            else if (tid == nthr - 1) a.count[e] = sc[tid];
        }
    }
}

// Every lattice triangle of element e: triangle s goes to e * a.nsimp + s, its vertices in ascending lattice index.
// LDS: the lattice of form_lattice (MODE_TESS), then the table.  KIND_Q2 (E = 2 or 3) and KIND_TRI.
template <int KIND, int E>
__global__ void __launch_bounds__(BLOCK) tessellate_kernel(ContourArgs a) {
    static_assert(KIND != KIND_Q3, "a tessellation is of 2-D elements");
    extern __shared__ double lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int64_t e = blockIdx.x;
    const int npts = a.npts, nf = a.nfield;
    double* lat = lds;
    double* tab = lds + (size_t)(E + nf) * npts;
    for (int i = tid; i < a.table_len; i += nthr) tab[i] = a.table[i];
    __syncthreads();
    form_lattice<KIND, E, MODE_TESS>(a, e, lat, tab, tid, nthr);
    __syncthreads();

    for (int s = tid; s < a.nsimp; s += nthr) {
        int v[3];
        simplex_vertices<KIND>(s, a.r, v);
        const int64_t t = e * a.nsimp + s;
        a.element[t] = (int32_t)e;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
#pragma unroll
            for (int c = 0; c < E; ++c) a.points[(t * 3 + q) * E + c] = lat[c * npts + v[q]];
            for (int c = 0; c < nf; ++c) a.values[(t * 3 + q) * nf + c] = lat[(E + c) * npts + v[q]];
        }
    }
}

// 1-D Lagrange basis on S nodes at xv, in the operation order of interpolate.hip's `lagrange`
void lagrange_host(int S, const double* nodes, double xv, double* L) {
    for (int i = 0; i < S; ++i) {
        double num = 1.0, den = 1.0;
        for (int j = 0; j < S; ++j)
            if (i != j) {
                num *= xv - nodes[j];
                den *= nodes[i] - nodes[j];
            }
        L[i] = num / den;
    }
}

template <int KIND, int E>
void launch(bool emit, unsigned block, size_t lds_bytes, const ContourArgs& a, hipStream_t st) {
    const dim3 gr((unsigned)a.N), bl(block);
    if (emit) hipLaunchKernelGGL((contour_kernel<KIND, E, true>), gr, bl, lds_bytes, st, a);
    else hipLaunchKernelGGL((contour_kernel<KIND, E, false>), gr, bl, lds_bytes, st, a);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_kind(int kind, int e, bool emit, unsigned block, size_t lds_bytes, const ContourArgs& a, hipStream_t st) {
    if (kind == KIND_Q2 && e == 3) launch<KIND_Q2, 3>(emit, block, lds_bytes, a, st);
    else if (kind == KIND_Q2) launch<KIND_Q2, 2>(emit, block, lds_bytes, a, st);
    else if (kind == KIND_Q3) launch<KIND_Q3, 3>(emit, block, lds_bytes, a, st);
    else launch<KIND_TRI, 2>(emit, block, lds_bytes, a, st);
}

template <int KIND, int E>
void launch_tess(unsigned block, size_t lds_bytes, const ContourArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((tessellate_kernel<KIND, E>), dim3((unsigned)a.N), dim3(block), lds_bytes, st, a);
    MGB_HIP_CHECK(hipGetLastError());
}

// the table the kernels read: the Q_k basis depends only on (k, r), so it is tabulated on the host, once per call
std::vector<double> lattice_table(const ContourIn& in) {
    std::vector<double> table;
    if (in.family == MGBHIP_INTERP_QK) {
        const int S = in.k + 1, r = in.refine;
        table.resize((size_t)(r + 1) * S);
        for (int i = 0; i <= r; ++i) lagrange_host(S, in.table, -1.0 + (2.0 * i) / r, table.data() + (size_t)i * S);
    } else {
        table.assign(in.table, in.table + (size_t)in.p * 10);
    }
    return table;
}

// lattice points and lattice simplices of one element
void lattice_sizes(int kind, int r, ContourArgs& a) {
    a.npts = kind == KIND_TRI ? (r + 1) * (r + 2) / 2 : (kind == KIND_Q2 ? (r + 1) * (r + 1) : (r + 1) * (r + 1) * (r + 1));
    a.nsimp = kind == KIND_TRI ? r * r : (kind == KIND_Q2 ? 2 * r * r : 6 * r * r * r);
}

}  // namespace

void contour_build_device(Contour& C, const ContourIn& in, const double* d_x, const double* d_table, int32_t table_len,
                          const double* d_fields, const double* d_levels, ContourWork& w, hipStream_t st) {
    C.d = in.d;
    C.e = in.e;
    C.ncarry = in.nfield - 1;
    C.S = 0;
    if (in.nlevels == 0) return;
    const int r = in.refine, d = in.d, e = in.e;
    const bool qk = in.family == MGBHIP_INTERP_QK;
    const int kind = qk ? (d == 3 ? KIND_Q3 : KIND_Q2) : KIND_TRI;
    w.count.ensure((size_t)in.N);
    w.off.ensure((size_t)in.N);

    ContourArgs a{};
    a.N = in.N;
    a.p = in.p; a.k = in.k; a.r = r; a.nfield = in.nfield; a.nlevels = in.nlevels;
    lattice_sizes(kind, r, a);
    a.table_len = table_len;
    // one wave for an element of few simplices, a workgroup of four otherwise
    const unsigned block = a.nsimp <= 128 ? 64 : BLOCK;
    a.chunk = (a.nsimp + (int)block - 1) / (int)block;
    a.x = d_x; a.table = d_table; a.fields = d_fields; a.levels = d_levels;
    a.count = w.count.p;
    launch_kind(kind, e, false, block, ((size_t)a.npts + (size_t)table_len) * sizeof(double), a, st);

    exclusive_scan(w.count.p, w.off.p, in.N, w.tmp, st);
    const int64_t S = scan_total(w.count.p, w.off.p, in.N, st);
    MGB_REQUIRE(S >= 0 && S < (int64_t)INT32_MAX, "contour: the number of simplices exceeds 32-bit indexing");
    if (S == 0) return;

    // grown to the largest soup seen and kept: a Contour that is built again (figure.hip) allocates nothing
    C.points.ensure((size_t)S * d * e);
    C.level.ensure((size_t)S);
    C.element.ensure((size_t)S);
    if (C.ncarry) C.carried.ensure((size_t)S * d * C.ncarry);
    a.S = S;
    a.off = w.off.p;
    a.points = C.points.p; a.level = C.level.p; a.element = C.element.p; a.carried = C.carried.p;
    launch_kind(kind, e, true, block, ((size_t)a.npts * (e + in.nfield) + (size_t)table_len) * sizeof(double), a, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    C.S = S;
}

std::vector<double> contour_lattice_table(const ContourIn& in) { return lattice_table(in); }

void contour_build(Contour& C, const ContourIn& in, hipStream_t st) {
    ContourWork w;
    if (in.nlevels == 0) {                     // nothing to cut: the core returns before it reads a pointer
        contour_build_device(C, in, nullptr, nullptr, 0, nullptr, nullptr, w, st);
        return;
    }
    const int64_t rows = (int64_t)in.p * in.N;
    const std::vector<double> table = lattice_table(in);
    DevBuf<double> d_x, d_table, d_fields, d_levels;
    d_x.upload(in.x, (size_t)rows * in.e, st);
    d_table.upload(table, st);
    d_fields.upload(in.fields, (size_t)rows * in.nfield, st);
    d_levels.upload(in.levels, (size_t)in.nlevels, st);
    contour_build_device(C, in, d_x.p, d_table.p, (int32_t)table.size(), d_fields.p, d_levels.p, w, st);
    // the inputs and the scan buffers are freed at scope exit; hipFree waits for the work that uses them
}

void contour_fetch(const Contour& C, double* points, int32_t* level, int32_t* element, double* carried, hipStream_t st) {
    if (C.S == 0) return;
    C.points.download(points, (size_t)C.S * C.d * C.e, st);
    C.level.download(level, (size_t)C.S, st);
    C.element.download(element, (size_t)C.S, st);
    if (carried && C.ncarry) C.carried.download(carried, (size_t)C.S * C.d * C.ncarry, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

int64_t tessellate_count(const ContourIn& in) {
    const int64_t r = in.refine;
    return in.N * (in.family == MGBHIP_INTERP_QK ? 2 * r * r : r * r);
}

void tessellate_build(Tessellation& T, const ContourIn& in, hipStream_t st) {
    T.e = in.e;
    T.nfield = in.nfield;
    T.T = tessellate_count(in);
    const int64_t rows = (int64_t)in.p * in.N;
    const int r = in.refine, e = in.e;
    const int kind = in.family == MGBHIP_INTERP_QK ? KIND_Q2 : KIND_TRI;
    const std::vector<double> table = lattice_table(in);

    DevBuf<double> d_x, d_table, d_fields;
    d_x.upload(in.x, (size_t)rows * e, st);
    d_table.upload(table, st);
    if (in.nfield) d_fields.upload(in.fields, (size_t)rows * in.nfield, st);
    T.points.alloc((size_t)T.T * 3 * e);
    T.element.alloc((size_t)T.T);
    if (in.nfield) T.values.alloc((size_t)T.T * 3 * in.nfield);

    ContourArgs a{};
    a.N = in.N;
    a.p = in.p; a.k = in.k; a.r = r; a.nfield = in.nfield;
    lattice_sizes(kind, r, a);
    a.table_len = (int32_t)table.size();
    a.x = d_x.p; a.table = d_table.p; a.fields = d_fields.p;
    a.points = T.points.p; a.element = T.element.p; a.values = T.values.p;
    // the launch shape of the contour kernels: one wave for an element of few triangles, a workgroup of four otherwise
    const unsigned block = a.nsimp <= 128 ? 64 : BLOCK;
    const size_t lds_bytes = ((size_t)a.npts * (e + in.nfield) + table.size()) * sizeof(double);
    if (kind == KIND_Q2 && e == 3) launch_tess<KIND_Q2, 3>(block, lds_bytes, a, st);
    else if (kind == KIND_Q2) launch_tess<KIND_Q2, 2>(block, lds_bytes, a, st);
    else launch_tess<KIND_TRI, 2>(block, lds_bytes, a, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    // the inputs are freed at scope exit; hipFree waits for the work that uses them
}

void tessellate_fetch(const Tessellation& T, double* points, int32_t* element, double* values, hipStream_t st) {
    if (T.T == 0) return;
    T.points.download(points, (size_t)T.T * 3 * T.e, st);
    T.element.download(element, (size_t)T.T, st);
    if (values && T.nfield) T.values.download(values, (size_t)T.T * 3 * T.nfield, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
