// Field lines of a vector field given by element-space functions: mgbhip_stream_* (include/mgbhip.h).
//
// interpolate.hip evaluates a field at points that are known before the kernel starts; here every point depends on the
// value at the previous one.  One lane owns one line and integrates it by the classical Runge-Kutta scheme with a fixed
// step; at every stage it locates its point in the resident location grid and evaluates the field there by the device
// functions of the fused query_* kernels (interp_device.hpp), so a stage velocity is bitwise what mgbhip_interpolate /
// mgbhip_interpolate_grad return at that point.  There is no warm start from the previous element: a point on a shared
// face takes the lowest-index element of its cell's candidate list, as everywhere else, and a warm start would change that.
//
// Every loop is bounded: max_steps steps of four stages, and inside a stage the Newton iterations and the candidate list
// of one cell.  A lane stores only into its own row of the stage buffers and of the results, so the results do not depend
// on the launch order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "interp_device.hpp"
#include "stream.hpp"

// No fused multiply-adds in this file: a step is a fixed sequence of IEEE operations (tests/streamlines_twin.py restates it).
#pragma clang fp contract(off)

namespace mgbhip {

namespace {

struct TraceArgs {
    int64_t S;
    int32_t max_steps, normalize;
    double h, min_speed;
    const double* seeds;       // S x D
    double* points;            // S x (max_steps + 1) x D
    int32_t* n;                // S
    int32_t* status;           // S
};

// The stage velocity of lane q at y.  The evaluators store through QueryArgs.out / QueryArgs.grad at row q, which the
// tracer points at its stage buffers (one row per lane); the lane reads its own row back.  VECTOR: the D components of
// z, value-only; GRADIENT: the gradient of the one component.  False: y is in no element (or, GRAD, the Jacobian there
// cannot be inverted: the fused kernel reports no element then, too).
template <int D_, int S, bool GRAD>
struct QkField {
    static constexpr int D = D_;
    __device__ static inline bool velocity(const QueryArgs& a, const Grid& g, int64_t q, const double (&y)[D],
                                           double (&v)[D]) {
        double nodes[S], L[D][S], xi[D];
        const int64_t found = qk_find<D, S>(a, g, y, nodes, L, xi);
        if (found < 0 || !qk_evaluate<D, S, GRAD>(a, q, found, nodes, L, xi)) return false;
        const double* r = GRAD ? a.grad : a.out;
        for (int d = 0; d < D; ++d) v[d] = r[q * D + d];
        return true;
    }
};

template <int FAM, bool GRAD>
struct SimplexField {
    static constexpr int D = 2;
    __device__ static inline bool velocity(const QueryArgs& a, const Grid& g, int64_t q, const double (&y)[2],
                                           double (&v)[2]) {
        double l1 = 0.0, l2 = 0.0;
        const int64_t found = simplex_find<FAM>(a, g, y, l1, l2);
        if (found < 0 || !simplex_evaluate<FAM, GRAD>(a, q, found, l1, l2)) return false;
        const double* r = GRAD ? a.grad : a.out;
        for (int d = 0; d < 2; ++d) v[d] = r[q * 2 + d];
        return true;
    }
};

// One lane per seed.  With k_s the stage velocities (divided by their length when normalize is set):
//   k1 = v(x);  k2 = v(x + (0.5 h) k1);  k3 = v(x + (0.5 h) k2);  k4 = v(x + h k3)
//   x <- x + (h / 6) (((k1 + 2 k2) + 2 k3) + k4)
// A stage point without an element ends the line at the current x (OUTSIDE if that is the seed itself, LEFT otherwise), a
// stage speed sqrt(v . v) that is not > min_speed ends it with STALLED (also NaN, and 0 / 0 under normalize).  The stage
// loop stays rolled: one inlined copy of locate and evaluate, whose registers the four stages share.
template <class F>
__global__ void __launch_bounds__(BLOCK) trace_lines(QueryArgs a, Grid g, TraceArgs t) {
    constexpr int D = F::D;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= t.S) return;
    double x[D], k[D], acc[D];
    for (int d = 0; d < D; ++d) {
        x[d] = t.seeds[q * D + d];
        k[d] = acc[d] = 0.0;
    }
    double* line = t.points + q * ((int64_t)t.max_steps + 1) * D;
    const double h6 = t.h / 6.0;
    int32_t n = 0, status = MGBHIP_STREAM_MAX_STEPS;
    bool go = true;
#pragma unroll 1
    for (int32_t step = 0; step < t.max_steps && go; ++step) {
#pragma unroll 1
        for (int s = 0; s < 4 && go; ++s) {
            const double c = s == 3 ? t.h : 0.5 * t.h;
            double y[D];
            for (int d = 0; d < D; ++d) y[d] = s == 0 ? x[d] : x[d] + c * k[d];
            if (!F::velocity(a, g, q, y, k)) {
                status = n == 0 ? MGBHIP_STREAM_OUTSIDE : MGBHIP_STREAM_LEFT;
                go = false;
                break;
            }
            if (n == 0) {                               // the seed has an element: it is the line's first point
                for (int d = 0; d < D; ++d) line[d] = x[d];
                n = 1;
            }
            double sq = k[0] * k[0];
            for (int d = 1; d < D; ++d) sq = sq + k[d] * k[d];
            const double speed = sqrt(sq);
            if (!(speed > t.min_speed)) {
                status = MGBHIP_STREAM_STALLED;
                go = false;
                break;
            }
            if (t.normalize)
                for (int d = 0; d < D; ++d) k[d] = k[d] / speed;
            for (int d = 0; d < D; ++d) acc[d] = s == 0 ? k[d] : acc[d] + (s == 3 ? 1.0 : 2.0) * k[d];
        }
        if (go) {
            for (int d = 0; d < D; ++d) {
                x[d] = x[d] + h6 * acc[d];
                line[(int64_t)n * D + d] = x[d];
            }
            ++n;
        }
    }
    for (int32_t i = n; i <= t.max_steps; ++i)
        for (int d = 0; d < D; ++d) line[(int64_t)i * D + d] = dnan();
    t.n[q] = n;
    t.status[q] = status;
}

template <class F>
void launch(const QueryArgs& a, const Grid& g, const TraceArgs& t, hipStream_t st) {
    hipLaunchKernelGGL((trace_lines<F>), dim3(grid_1d(t.S)), dim3(BLOCK), 0, st, a, g, t);
}

template <int D, int S>
void launch_qk(bool grad, const QueryArgs& a, const Grid& g, const TraceArgs& t, hipStream_t st) {
    if (grad) launch<QkField<D, S, true>>(a, g, t, st);
    else launch<QkField<D, S, false>>(a, g, t, st);
}

template <int D>
void launch_qk_d(int S, bool grad, const QueryArgs& a, const Grid& g, const TraceArgs& t, hipStream_t st) {
    switch (S) {
        case 2: launch_qk<D, 2>(grad, a, g, t, st); break;
        case 3: launch_qk<D, 3>(grad, a, g, t, st); break;
        case 4: launch_qk<D, 4>(grad, a, g, t, st); break;
        case 5: launch_qk<D, 5>(grad, a, g, t, st); break;
        case 6: launch_qk<D, 6>(grad, a, g, t, st); break;
        case 7: launch_qk<D, 7>(grad, a, g, t, st); break;
        case 8: launch_qk<D, 8>(grad, a, g, t, st); break;
        case 9: launch_qk<D, 9>(grad, a, g, t, st); break;
        default: throw InvalidArgument("stream: Q_k degree out of range");
    }
}

size_t field_len(const StreamTracer& T) {
    return (size_t)T.p * (size_t)T.N * (T.field == MGBHIP_STREAM_VECTOR ? (size_t)T.d : 1);
}

}  // namespace

void stream_build(StreamTracer& T, const InterpIn& geo, int32_t field, const double* z, hipStream_t st) {
    MGB_REQUIRE(interp_is_located(geo.family), "stream: only the Q_k (d = 2, 3), P1 and P2 families are traced");
    T.family = geo.family; T.d = geo.d; T.k = geo.k; T.p = geo.p; T.N = geo.N; T.field = field;
    T.x.upload(geo.x, (size_t)geo.p * geo.N * geo.d, st);
    T.table.upload(geo.table, (size_t)geo.table_len, st);
    T.z.upload(z, field_len(T), st);
    location_grid_build(T.grid, geo, T.x.p, st);
}

void stream_set_field(StreamTracer& T, const double* z, hipStream_t st) {
    T.z.upload(z, field_len(T), st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void stream_trace(StreamTracer& T, int64_t S, const double* seeds, double h, int32_t max_steps, bool normalize,
                  double min_speed, double* points, int32_t* n, int32_t* status, hipStream_t st) {
    if (S == 0) return;
    const bool grad = T.field == MGBHIP_STREAM_GRADIENT;
    const size_t D = (size_t)T.d, npts = (size_t)S * ((size_t)max_steps + 1) * D;
    T.seeds.upload(seeds, (size_t)S * D, st);
    T.points.ensure(npts);
    T.n.ensure((size_t)S);
    T.status.ensure((size_t)S);
    T.stage_out.ensure((size_t)S * (grad ? 1 : D));
    if (grad) T.stage_grad.ensure((size_t)S * D);
    QueryArgs a{};
    a.M = S;
    a.p = T.p;
    a.ncomp = grad ? 1 : T.d;
    a.x = T.x.p;
    a.table = T.table.p;
    a.z = T.z.p;
    a.start = T.grid.start.p;
    a.cand = T.grid.cand.p;
    a.box = T.grid.box.p;
    a.out = T.stage_out.p;
    a.grad = grad ? T.stage_grad.p : nullptr;
    const TraceArgs t{S, max_steps, normalize ? 1 : 0, h, min_speed, T.seeds.p, T.points.p, T.n.p, T.status.p};
    const Grid& g = T.grid.g;
    if (T.family == MGBHIP_INTERP_QK) {
        if (T.d == 2) launch_qk_d<2>(T.k + 1, grad, a, g, t, st);
        else launch_qk_d<3>(T.k + 1, grad, a, g, t, st);
    } else if (T.family == MGBHIP_INTERP_P1) {
        if (grad) launch<SimplexField<MGBHIP_INTERP_P1, true>>(a, g, t, st);
        else launch<SimplexField<MGBHIP_INTERP_P1, false>>(a, g, t, st);
    } else if (T.family == MGBHIP_INTERP_P2) {
        if (grad) launch<SimplexField<MGBHIP_INTERP_P2, true>>(a, g, t, st);
        else launch<SimplexField<MGBHIP_INTERP_P2, false>>(a, g, t, st);
    } else {
        if (grad) launch<SimplexField<MGBHIP_INTERP_P2C, true>>(a, g, t, st);
        else launch<SimplexField<MGBHIP_INTERP_P2C, false>>(a, g, t, st);
    }
    MGB_HIP_CHECK(hipGetLastError());
    T.points.download(points, npts, st);
    T.n.download(n, (size_t)S, st);
    T.status.download(status, (size_t)S, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mgbhip
