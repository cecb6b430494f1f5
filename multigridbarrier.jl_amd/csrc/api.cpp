// api.cpp -- extern "C" surface of libmgbhip.so (include/mgbhip.h).  Every entry point
// converts C++ exceptions to a status code + mgbhip_last_error(); nothing here computes on
// the CPU: a missing / failing GPU is an error, never a fallback.
#include <chrono>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <limits>
#include <memory>
#include <string>

#include "closest.hpp"
#include "contour.hpp"
#include "faces.hpp"
#include "figure.hpp"
#include "interpolate.hpp"
#include "polyline.hpp"
#include "problem.hpp"
#include "quadrature.hpp"
#include "residual.hpp"
#include "raycast.hpp"
#include "stream.hpp"
#include "surface.hpp"
#include "tubes.hpp"
#include "weld.hpp"

using namespace mgbhip;

mgbhip_problem* problem_create(mgbhip_ctx* ctx, const mgbhip_problem_desc* d, mgbhip_problem* share);
int core_run(mgbhip_problem* P, double* z, const double* c, const mgbhip_options* opt, mgbhip_core_result* res);
int matched_t_run(mgbhip_problem* P, const double* z, const double* c, double t_default, double* t_out);
void trial_values_run(mgbhip_problem* P, int level, double step, double* y, int32_t* moved, int32_t* finite, int32_t* path);

#ifdef MGB_STEP_PROBE
namespace mgbhip { void mf_debug_probe(long long* out64); }
#endif

static thread_local std::string g_last_error;

// Every entry point that takes a handle runs with the handle's device current on the calling
// thread (and restores the caller's device afterwards): a second context on another GPU, a call
// from another host thread or a torch.cuda.set_device between calls must not put buffers or
// launches on the wrong device for ctx->stream.
struct DeviceGuard {
    int prev = -1, dev = -1;
    explicit DeviceGuard(int d) : dev(d) {
        if (dev < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) MGB_HIP_CHECK(hipSetDevice(dev));
    }
    ~DeviceGuard() {
        if (dev >= 0 && prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};
static int dev_of(const mgbhip_ctx* c) { return c ? c->device : -1; }
// every other handle (problem, vector and the post-processing handles below) names its context
template <class H>
static int dev_of(const H* h) { return (h && h->ctx) ? h->ctx->device : -1; }

// A post-processing object and the context it lives in.  The opaque types of include/mgbhip.h are one line each.
template <class T>
struct Handle {
    mgbhip_ctx* ctx = nullptr;
    T obj;
};
struct mgbhip_locator : Handle<Locator> {};            // a point locator (interpolate.hpp)
struct mgbhip_closest : Handle<Closest> {};            // a closest-point locator (closest.hpp)
struct mgbhip_quadrature : Handle<Quadrature> {};      // a quadrature rule on a mesh (quadrature.hpp)
struct mgbhip_faces : Handle<Faces> {};                // the facets of a mesh (faces.hpp)
struct mgbhip_residual : Handle<Residual> {};          // a rule with second derivatives on a flat mesh (residual.hpp)
struct mgbhip_contour : Handle<Contour> {};            // a simplex soup (contour.hpp)
struct mgbhip_tessellation : Handle<Tessellation> {};  // the lattice triangles of a 2-D mesh (contour.hpp)
struct mgbhip_weld : Handle<Weld> {};                  // the index of a welded soup (weld.hpp)
struct mgbhip_polyline : Handle<Polyline> {};          // the lines of a segment mesh (polyline.hpp)
struct mgbhip_raycast : Handle<RayCaster> {};          // a ray caster (raycast.hpp)
struct mgbhip_surface : Handle<Surface> {};            // a triangle soup in its grid (surface.hpp)
struct mgbhip_tubes : Handle<Tubes> {};                // a capsule soup in its grid (tubes.hpp)
struct mgbhip_stream : Handle<StreamTracer> {};        // a field-line tracer (stream.hpp)
struct mgbhip_figure : Handle<Figure> {};              // a resident figure pipeline (figure.hpp)

#define MGB_API_BEGIN try {
#define MGB_API_BEGIN_ON(h) try { DeviceGuard _guard(dev_of(h));
#define MGB_API_END                                   \
    }                                                 \
    catch (const InvalidArgument& e) {                \
        g_last_error = e.what();                      \
        return MGBHIP_ERR_INVALID;                    \
    }                                                 \
    catch (const HipError& e) {                       \
        g_last_error = e.what();                      \
        return MGBHIP_ERR_HIP;                        \
    }                                                 \
    catch (const std::exception& e) {                 \
        g_last_error = e.what();                      \
        return MGBHIP_ERR_INVALID;                    \
    }

// a new handle in ctx, built by build(obj), released into *out only once it is complete
template <class H, class Build>
static void create_handle(mgbhip_ctx* ctx, H** out, Build build) {
    std::unique_ptr<H> h(new H());
    h->ctx = ctx;
    build(h->obj);
    *out = h.release();
}

// null is fine; else whatever is queued on the context's stream may still read the object's buffers
template <class H>
static int destroy_handle(H* h) {
    MGB_API_BEGIN_ON(h)
    if (!h) return MGBHIP_OK;
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return MGBHIP_OK;
    MGB_API_END
}

// The argument checks the rendering entry points share; `who` is the caller's prefix in the message.
static void check_window(const std::string& who, double t_min, double t_max) {
    MGB_REQUIRE(std::isfinite(t_min) && t_max > t_min, who + ": t_min must be finite and t_max > t_min");
}

// R rays of dimension dim: finite, directions of unit length within 1e-12
static void check_rays(const std::string& who, int64_t R, int dim, const double* origin, const double* dir) {
    for (int64_t i = 0; i < R * dim; ++i)
        MGB_REQUIRE(std::isfinite(origin[i]) && std::isfinite(dir[i]), who + ": origins and directions must be finite");
    for (int64_t r = 0; r < R; ++r) {
        double q = 0.0;
        for (int a = 0; a < dim; ++a) q += dir[r * dim + a] * dir[r * dim + a];
        MGB_REQUIRE(std::fabs(q - 1.0) <= 1e-12, who + ": directions must have unit length");
    }
}

static void check_clim(const std::string& who, double lo, double hi) {
    MGB_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && lo < hi, who + ": clim must be finite with lo < hi");
}

static void check_ambient(const std::string& who, double ambient) {
    MGB_REQUIRE(ambient >= 0.0 && ambient <= 1.0, who + ": ambient must be in [0, 1]");
}

// the Kt x 4 colour table of a shade call (r, g, b, alpha), then its colour limits and ambient term
static void check_table_clim_ambient(const std::string& who, int32_t Kt, const double* table, double lo, double hi,
                                     double ambient) {
    MGB_REQUIRE(Kt >= 2, who + ": the colour table needs at least two rows");
    for (int64_t i = 0; i < (int64_t)Kt * 4; ++i) MGB_REQUIRE(std::isfinite(table[i]), who + ": the colour table must be finite");
    check_clim(who, lo, hi);
    check_ambient(who, ambient);
}

// the K x 4 transfer table of a volume render (r, g, b, sigma), then its colour limits
static void check_transfer_clim(int32_t K, const double* transfer, double lo, double hi) {
    for (int64_t i = 0; i < (int64_t)K * 4; ++i)
        MGB_REQUIRE(std::isfinite(transfer[i]) && (i % 4 != 3 || transfer[i] >= 0.0),
                    "raycast: the transfer table must be finite with sigma >= 0");
    check_clim("raycast", lo, hi);
}

extern "C" {

const char* mgbhip_last_error(void) { return g_last_error.c_str(); }
const char* mgbhip_version(void) { return "mgbhip 0.1 (gfx950)"; }

int mgbhip_create(mgbhip_ctx** out, int device_id, void* hip_stream) {
    MGB_API_BEGIN
    MGB_REQUIRE(out != nullptr, "null output pointer");
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    const bool dbg2 = debug_level() >= 2;
    int count = 0;
    MGB_HIP_CHECK(hipGetDeviceCount(&count));
    MGB_REQUIRE(count > 0, "no HIP device visible: this library has no CPU fallback");
    MGB_REQUIRE(device_id >= 0 && device_id < count, "device id out of range");
    MGB_HIP_CHECK(hipSetDevice(device_id));
    if (dbg2) fprintf(stderr, "[mgbhip] create: device selected after %.3f s\n", since());
    mgbhip_ctx* c = new mgbhip_ctx();
    c->device = device_id;
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        MGB_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    c->timers.stream = c->stream;
    if (dbg2) fprintf(stderr, "[mgbhip] create: stream ready after %.3f s\n", since());
    *out = c;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_destroy(mgbhip_ctx* ctx) {
    MGB_API_BEGIN_ON(ctx)
    if (!ctx) return MGBHIP_OK;
    (void)hipStreamSynchronize(ctx->stream);
    ctx->timers.reset(false);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_problem_create(mgbhip_ctx* ctx, const mgbhip_problem_desc* desc, mgbhip_problem* share,
                          mgbhip_problem** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(out != nullptr, "null output pointer");
    *out = problem_create(ctx, desc, share);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_problem_destroy(mgbhip_problem* prob) {
    MGB_API_BEGIN_ON(prob)
    if (!prob) return MGBHIP_OK;
    (void)hipStreamSynchronize(prob->stream());
    delete prob;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_problem_set_box(mgbhip_problem* prob, double b, double R) {
    MGB_API_BEGIN
    MGB_REQUIRE(prob && prob->cone.feasibility, "set_box on a problem without the phase-I wrapper");
    prob->cone.box_b = b;
    prob->cone.box_R = R;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_problem_set_barrier_weights(mgbhip_problem* prob, const double* bw) {
    MGB_API_BEGIN_ON(prob)
    MGB_REQUIRE(prob, "null problem");
    if (bw) {
        prob->bw.upload(bw, (size_t)prob->n, prob->stream());
        MGB_HIP_CHECK(hipStreamSynchronize(prob->stream()));
        prob->has_bw = true;
    } else {
        prob->has_bw = false;
    }
    return MGBHIP_OK;
    MGB_API_END
}

int64_t mgbhip_level_size(const mgbhip_problem* prob, int32_t level) {
    if (!prob || level < 0 || level >= (int32_t)prob->levels.size()) return -1;
    return prob->levels[level].m;
}

static void check_level(mgbhip_problem* P, int32_t level) {
    MGB_REQUIRE(P != nullptr, "null problem");
    MGB_REQUIRE(level >= 0 && level < (int32_t)P->levels.size(), "level out of range");
}

int mgbhip_level_plan(mgbhip_problem* P, int32_t level, int32_t* out) {
    MGB_API_BEGIN
    check_level(P, level);
    MGB_REQUIRE(out != nullptr, "null argument");
    const Level& L = P->levels[level];
    out[0] = L.R_unit;
    out[1] = L.R_long;
    out[2] = L.T_long;
    out[3] = L.T_chunks;
    out[4] = (L.selection ? 1 : 0) | (L.direct ? 2 : 0);
    out[5] = L.acc;
    out[6] = L.acc_split;
    out[7] = L.long_lists;
    out[8] = L.gather_chunk;
    out[9] = L.gather_nchunk;
    out[10] = L.proj_kernel;
    out[11] = L.max_row;
    out[12] = L.max_col;
    out[13] = L.cmax;
    out[14] = L.nnz > 0 ? (int32_t)(L.list_total / L.nnz) : 0;
    out[15] = L.planned;
    return MGBHIP_OK;
    MGB_API_END
}

static_assert(MGBHIP_ELEM_F0 == MODE_F0 && MGBHIP_ELEM_F1 == MODE_F1 && MGBHIP_ELEM_F2 == MODE_F2 && MGBHIP_ELEM_NODE_F == MODE_NODE_F &&
              MGBHIP_ELEM_NODE_SLACK == MODE_NODE_SLACK && MGBHIP_ELEM_F01 == MODE_F01, "mgbhip.h mirrors ElemMode");
static_assert(MGBHIP_ELEM_KIND_DENSE == ELEM_DENSE && MGBHIP_ELEM_KIND_WIDE == ELEM_WIDE && MGBHIP_ELEM_KIND_FAST_DEFAULT == ELEM_FAST_DEFAULT &&
              MGBHIP_ELEM_KIND_FAST_RUNTIME == ELEM_FAST_RUNTIME && MGBHIP_ELEM_KIND_CONDENSE == ELEM_CONDENSE &&
              MGBHIP_ELEM_KIND_GENERIC == ELEM_GENERIC, "mgbhip.h mirrors ElemKind");

int mgbhip_elem_plan(mgbhip_problem* P, int32_t mode, int32_t* out) {
    MGB_API_BEGIN
    MGB_REQUIRE(P != nullptr && out != nullptr, "null argument");
    MGB_REQUIRE(mode >= MODE_F0 && mode <= MODE_F01, "elem_plan: bad mode");
    const ElemParams E = P->elem_params(nullptr);      // no evaluation point: nothing is launched or cached
    const ElemPlan plan = elem_plan_of(E, mode, false);
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[0] = plan.kind; out[1] = plan.NY; out[2] = plan.P; out[3] = plan.threads; out[4] = plan.G; out[5] = plan.EPB;
    out[6] = (int32_t)plan.grid; out[7] = (int32_t)plan.lds;
    out[8] = E.nstage; out[9] = elem_unstaged_rows(E); out[10] = E.ymask;
    out[11] = plan.kind;
    if (mode == MODE_F2 && !P->levels.empty() && P->levels.back().condense) out[11] = elem_plan_of(E, mode, true).kind;
    return MGBHIP_OK;
    MGB_API_END
}

static void stage_inputs(mgbhip_problem* P, int32_t level, const double* s, const double* c, const double* z0) {
    hipStream_t st = P->stream();
    P->d_x.upload(s, (size_t)P->levels[level].m, st);
    P->d_c.upload(c, (size_t)P->n * P->nD, st);
    P->d_z0.upload(z0, (size_t)P->nu * P->n, st);
    P->touch();
}

int mgbhip_f0(mgbhip_problem* P, int32_t level, const double* s, const double* c, const double* z0, double* value) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(s && c && z0 && value, "null argument");
    stage_inputs(P, level, s, c, z0);
    *value = P->eval_f0(level, P->d_x.p, P->d_z0.p, P->d_c.p);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_f1(mgbhip_problem* P, int32_t level, const double* s, const double* c, const double* z0, double* grad) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(s && c && z0 && grad, "null argument");
    stage_inputs(P, level, s, c, z0);
    P->eval_f1(level, P->d_x.p, P->d_z0.p, P->d_c.p, P->d_g.p);
    P->d_g.download(grad, (size_t)P->levels[level].m, P->stream());
    MGB_HIP_CHECK(hipStreamSynchronize(P->stream()));
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_f2(mgbhip_problem* P, int32_t level, const double* s, const double* c, const double* z0, double* values) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(s && c && z0, "null argument");
    stage_inputs(P, level, s, c, z0);
    P->eval_f2(level, P->d_x.p, P->d_z0.p, P->d_c.p);
    if (values) P->levels[level].Hval.download(values, (size_t)P->levels[level].nnz, P->stream());
    MGB_HIP_CHECK(hipStreamSynchronize(P->stream()));
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_hessian_pattern(mgbhip_problem* P, int32_t level, int64_t* nnz, const int32_t** rowptr,
                           const int32_t** colidx) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    P->ensure_plan(level);
    if (nnz) *nnz = P->levels[level].nnz;
    if (rowptr) *rowptr = P->levels[level].hHptr.data();
    if (colidx) *colidx = P->levels[level].hHcol.data();
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_solve(mgbhip_problem* P, int32_t level, const double* g, double* x) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(g && x, "null argument");
    hipStream_t st = P->stream();
    const size_t m = (size_t)P->levels[level].m;
    P->d_g.upload(g, m, st);
    P->factor(level);
    P->trisolve(level, P->d_g.p, P->d_nv.p);
    int status = P->levels[level].solver.status(st);
    if (status != MGBHIP_OK && P->lu_fallback(level, P->d_g.p, P->d_nv.p)) status = MGBHIP_OK;   // LDL' failed: pivoted LU (src/utils.jl:145)
    P->d_nv.download(x, m, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    if (status != MGBHIP_OK) g_last_error = "Cholesky met a non-positive pivot";
    return status;
    MGB_API_END
}

int mgbhip_set_hessian(mgbhip_problem* P, int32_t level, const double* values) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(values, "null argument");
    P->ensure_plan(level);
    mgbhip::Level& L = P->levels[level];
    MGB_REQUIRE(L.Hval.n >= (size_t)L.nnz, "this level keeps no CSR value array");
    L.Hval.upload(values, (size_t)L.nnz, P->stream());
    MGB_HIP_CHECK(hipStreamSynchronize(P->stream()));
    L.H.set_from_outside();
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_solve_newton(mgbhip_problem* P, int32_t level, const double* g, double* x, double* lambda2) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(g && x, "null argument");
    hipStream_t st = P->stream();
    const size_t m = (size_t)P->levels[level].m;
    P->d_g.upload(g, m, st);
    P->factor(level, P->d_g.p, P->d_nv.p);         // [H -g; -g' -1]: the forward substitution rides along
    P->trisolve_carried(level, P->d_nv.p);         // one backward sweep from x_n = 1
    int status = P->levels[level].solver.status(st);
    if (status != MGBHIP_OK && P->lu_fallback(level, P->d_g.p, P->d_nv.p)) status = MGBHIP_OK;   // LDL' failed: pivoted LU (src/utils.jl:145)
    P->d_nv.download(x, m, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    if (lambda2) {
        double acc = 0.0;
        for (size_t i = 0; i < m; ++i) acc += g[i] * x[i];
        *lambda2 = acc;
    }
    if (status != MGBHIP_OK) g_last_error = "Cholesky met a non-positive pivot";
    return status;
    MGB_API_END
}

int mgbhip_problem_set_sharding(mgbhip_problem* P, int32_t level, int64_t n_iface, const int32_t* iface_cols, const double* own_mask) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    mgbhip::Level& L = P->levels[level];
    MGB_REQUIRE(!L.solver.analyzed, "sharding must be set before the first solve of the level");
    MGB_REQUIRE(own_mask != nullptr && n_iface >= 0 && n_iface <= L.m && (n_iface == 0 || iface_cols), "bad sharding arguments");
    L.h_iface.assign(iface_cols, iface_cols + n_iface);
    for (int64_t i = 0; i < n_iface; ++i) {
        MGB_REQUIRE(L.h_iface[i] >= 0 && L.h_iface[i] < L.m, "interface column out of range");
        MGB_REQUIRE(i == 0 || L.h_iface[i] > L.h_iface[i - 1], "interface columns must be strictly increasing");
    }
    L.d_iface.upload(L.h_iface, P->stream());
    L.own.upload(own_mask, (size_t)L.m, P->stream());
    MGB_HIP_CHECK(hipStreamSynchronize(P->stream()));
    L.sharded = true;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_problem_set_collective(mgbhip_problem* P, mgbhip_allreduce_fn fn, void* user, int32_t accepts_device_ptr) {
    MGB_API_BEGIN_ON(P)
    P->coll_fn = fn;
    P->coll_user = user;
    P->coll_device = accepts_device_ptr != 0;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_newton_direction(mgbhip_problem* P, int32_t level, const double* s, const double* c, const double* z0, double* x,
                            double* lambda2, int32_t* condensed) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(s && c && z0 && x, "null argument");
    hipStream_t st = P->stream();
    const size_t m = (size_t)P->levels[level].m;
    stage_inputs(P, level, s, c, z0);
    P->eval_f1(level, P->d_x.p, P->d_z0.p, P->d_c.p, P->d_g.p);
    P->eval_f2(level, P->d_x.p, P->d_z0.p, P->d_c.p, false, P->d_g.p);      // exactly the Newton loop's sequence
    if (condensed) *condensed = P->levels[level].H.condensed() ? 1 : 0;
    P->factor(level, P->d_g.p, P->d_nv.p);
    P->trisolve_carried(level, P->d_nv.p);
    const int status = P->levels[level].solver.status(st);
    P->d_nv.download(x, m, st);
    if (lambda2) {
        std::vector<double> g(m);
        P->d_g.download(g.data(), m, st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        double acc = 0.0;
        for (size_t i = 0; i < m; ++i) acc += g[i] * x[i];
        *lambda2 = acc;
    }
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    if (status != MGBHIP_OK) g_last_error = "Cholesky met a non-positive pivot";
    return status;
    MGB_API_END
}

int mgbhip_trial_values(mgbhip_problem* P, int32_t level, const double* x, const double* dir, double step, const double* c,
                        const double* z0, double* y, double* g, double* xn, int32_t* moved, int32_t* finite, int32_t* path) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(x && dir && c && z0 && y && g && xn && moved && finite && path, "null argument");
    MGB_REQUIRE(!P->sharded(), "trial_values: not for sharded problems");
    hipStream_t st = P->stream();
    const size_t m = (size_t)P->levels[level].m;
    stage_inputs(P, level, x, c, z0);                  // d_x, d_c, d_z0 (the workspace of problem_create holds every level), touch()
    P->d_nv.upload(dir, m, st);
    trial_values_run(P, level, step, y, moved, finite, path);
    P->d_gn.download(g, m, st);
    P->d_xn.download(xn, m, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    return MGBHIP_OK;
    MGB_API_END
}


// ---- device-resident vectors --------------------------------------------------------------------
static double* vec_scratch(mgbhip_ctx* c, int64_t len) {
    c->vscratch.ensure((size_t)reduce_scratch_doubles(len));
    c->vscal.ensure(8);
    return c->vscratch.p;
}
static void same_ctx(const mgbhip_vec* a, const mgbhip_vec* b) {
    MGB_REQUIRE(a && b, "null vector");
    MGB_REQUIRE(a->ctx == b->ctx, "vectors belong to different contexts");
}

int mgbhip_vec_alloc(mgbhip_ctx* ctx, int64_t len, mgbhip_vec** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx && out && len >= 0, "bad argument");
    std::unique_ptr<mgbhip_vec> v(new mgbhip_vec());
    v->ctx = ctx;
    v->len = len;
    v->buf.alloc((size_t)std::max<int64_t>(len, 1));
    v->buf.zero(ctx->stream);
    *out = v.release();
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_vec_free(mgbhip_vec* v) {
    MGB_API_BEGIN_ON(v)
    if (!v) return MGBHIP_OK;
    (void)hipStreamSynchronize(v->ctx->stream);
    delete v;
    return MGBHIP_OK;
    MGB_API_END
}

int64_t mgbhip_vec_len(const mgbhip_vec* v) { return v ? v->len : -1; }

int mgbhip_vec_upload(mgbhip_vec* v, const double* host, int64_t len) {
    MGB_API_BEGIN_ON(v)
    MGB_REQUIRE(v && host && len == v->len, "upload: length mismatch");
    v->buf.upload(host, (size_t)len, v->ctx->stream);
    MGB_HIP_CHECK(hipStreamSynchronize(v->ctx->stream));     // the host buffer may go away
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_vec_download(const mgbhip_vec* v, double* host, int64_t len) {
    MGB_API_BEGIN_ON(v)
    MGB_REQUIRE(v && host && len == v->len, "download: length mismatch");
    v->buf.download(host, (size_t)len, v->ctx->stream);
    MGB_HIP_CHECK(hipStreamSynchronize(v->ctx->stream));
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_vec_fill(mgbhip_vec* v, double value) {
    MGB_API_BEGIN_ON(v)
    MGB_REQUIRE(v, "null vector");
    launch_fill(value, v->buf.p, v->len, v->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_vec_copy(mgbhip_vec* dst, const mgbhip_vec* src) {
    MGB_API_BEGIN_ON(dst)
    same_ctx(dst, src);
    MGB_REQUIRE(dst->len == src->len, "copy: length mismatch");
    if (dst->len) MGB_HIP_CHECK(hipMemcpyAsync(dst->buf.p, src->buf.p, (size_t)dst->len * sizeof(double),
                                               hipMemcpyDeviceToDevice, dst->ctx->stream));
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_vec_axpy(double alpha, const mgbhip_vec* x, mgbhip_vec* y) {
    MGB_API_BEGIN_ON(y)
    same_ctx(x, y);
    MGB_REQUIRE(x->len == y->len, "axpy: length mismatch");
    if (y->len) launch_axpy(alpha, x->buf.p, y->buf.p, y->len, y->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_vec_scale(double alpha, mgbhip_vec* x) {
    MGB_API_BEGIN_ON(x)
    MGB_REQUIRE(x, "null vector");
    if (x->len) launch_scale_copy(x->buf.p, alpha, x->buf.p, x->len, x->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_vec_dot(const mgbhip_vec* a, const mgbhip_vec* b, double* out) {
    MGB_API_BEGIN_ON(a)
    same_ctx(a, b);
    MGB_REQUIRE(out && a->len == b->len, "dot: bad argument");
    *out = 0.0;
    if (a->len == 0) return MGBHIP_OK;
    mgbhip_ctx* c = a->ctx;
    double* sc = vec_scratch(c, a->len);
    launch_dot(a->buf.p, b->buf.p, a->len, sc, c->vscal.p, 0, c->stream);
    c->vscal.download(out, 1, c->stream);
    MGB_HIP_CHECK(hipStreamSynchronize(c->stream));
    return MGBHIP_OK;
    MGB_API_END
}

static int vec_stats_host(const mgbhip_vec* a, double* two) {
    mgbhip_ctx* c = a->ctx;
    two[0] = two[1] = 0.0;
    if (a->len == 0) return MGBHIP_OK;
    double* sc = vec_scratch(c, a->len);
    launch_vec_stats(a->buf.p, a->len, sc, c->vscal.p, 0, c->stream);
    c->vscal.download(two, 2, c->stream);
    MGB_HIP_CHECK(hipStreamSynchronize(c->stream));
    return MGBHIP_OK;
}

int mgbhip_vec_norm(const mgbhip_vec* a, double* out) {
    MGB_API_BEGIN_ON(a)
    MGB_REQUIRE(a && out, "null argument");
    double two[2];
    vec_stats_host(a, two);
    *out = std::sqrt(two[0]);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_vec_isfinite(const mgbhip_vec* a, int32_t* all_finite) {
    MGB_API_BEGIN_ON(a)
    MGB_REQUIRE(a && all_finite, "null argument");
    double two[2];
    vec_stats_host(a, two);
    *all_finite = (two[1] == 0.0) ? 1 : 0;
    return MGBHIP_OK;
    MGB_API_END
}

static void check_closure_args(mgbhip_problem* P, int32_t level, const mgbhip_vec* s, const mgbhip_vec* c, const mgbhip_vec* z0) {
    check_level(P, level);
    MGB_REQUIRE(s && c && z0, "null vector");
    MGB_REQUIRE(s->ctx == P->ctx && c->ctx == P->ctx && z0->ctx == P->ctx, "vector and problem belong to different contexts");
    MGB_REQUIRE(s->len == P->levels[level].m, "s has the wrong length for this level");
    MGB_REQUIRE(c->len == P->n * P->nD, "c must hold n x nD entries");
    MGB_REQUIRE(z0->len == (int64_t)P->nu * P->n, "z0 must hold nu x n entries");
}

int mgbhip_f0_d(mgbhip_problem* P, int32_t level, const mgbhip_vec* s, const mgbhip_vec* c, const mgbhip_vec* z0, double* value) {
    MGB_API_BEGIN_ON(P)
    check_closure_args(P, level, s, c, z0);
    MGB_REQUIRE(value, "null argument");
    P->touch();                           // caller-owned vectors: no cached z0 + R*s can be trusted
    *value = P->eval_f0(level, s->buf.p, z0->buf.p, c->buf.p);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_f1_d(mgbhip_problem* P, int32_t level, const mgbhip_vec* s, const mgbhip_vec* c, const mgbhip_vec* z0, mgbhip_vec* grad) {
    MGB_API_BEGIN_ON(P)
    check_closure_args(P, level, s, c, z0);
    MGB_REQUIRE(grad && grad->ctx == P->ctx && grad->len == s->len, "grad has the wrong length");
    P->touch();
    P->eval_f1(level, s->buf.p, z0->buf.p, c->buf.p, grad->buf.p);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_f2_d(mgbhip_problem* P, int32_t level, const mgbhip_vec* s, const mgbhip_vec* c, const mgbhip_vec* z0) {
    MGB_API_BEGIN_ON(P)
    check_closure_args(P, level, s, c, z0);
    P->touch();
    P->eval_f2(level, s->buf.p, z0->buf.p, c->buf.p);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_solve_d(mgbhip_problem* P, int32_t level, const mgbhip_vec* g, mgbhip_vec* x) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(g && x && g->ctx == P->ctx && x->ctx == P->ctx, "bad vector");
    MGB_REQUIRE(g->len == P->levels[level].m && x->len == g->len, "solve: length mismatch");
    hipStream_t st = P->stream();
    P->factor(level);
    P->trisolve(level, g->buf.p, x->buf.p);
    const int status = P->levels[level].solver.status(st);
    if (status != MGBHIP_OK) g_last_error = "Cholesky met a non-positive pivot";
    return status;
    MGB_API_END
}

int mgbhip_prolong_add(mgbhip_problem* P, int32_t level, const mgbhip_vec* s, mgbhip_vec* z) {
    MGB_API_BEGIN_ON(P)
    check_level(P, level);
    MGB_REQUIRE(s && z && s->ctx == P->ctx && z->ctx == P->ctx, "bad vector");
    const Level& Lv = P->levels[level];
    MGB_REQUIRE(s->len == Lv.m && z->len == Lv.rows, "prolong_add: length mismatch");
    launch_csr_matvec(Lv.rows, Lv.Rptr.p, Lv.Rcol.p, Lv.Rval.p, s->buf.p, z->buf.p, true, false, P->stream());
    P->touch();
    return MGBHIP_OK;
    MGB_API_END
}

static int node_map(mgbhip_problem* P, const double* z, double* F, double* Dz, int mode) {
    MGB_REQUIRE(P && z && F, "null argument");
    hipStream_t st = P->stream();
    P->d_z0.upload(z, (size_t)P->nu * P->n, st);
    ElemParams E = P->elem_params(nullptr);
    E.z0 = P->d_z0.p;
    if (Dz) {
        P->d_nodeDz.ensure((size_t)P->n * P->nD);
        E.out_Dz = P->d_nodeDz.p;
    }
    launch_elem(E, mode, st);
    P->d_nodeF.download(F, (size_t)P->n, st);
    if (Dz) P->d_nodeDz.download(Dz, (size_t)P->n * P->nD, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    return MGBHIP_OK;
}

int mgbhip_node_barrier(mgbhip_problem* P, const double* z, double* F, double* Dz) {
    MGB_API_BEGIN_ON(P)
    return node_map(P, z, F, Dz, MODE_NODE_F);
    MGB_API_END
}

int mgbhip_node_slack(mgbhip_problem* P, const double* z, double* slack) {
    MGB_API_BEGIN_ON(P)
    return node_map(P, z, slack, nullptr, MODE_NODE_SLACK);
    MGB_API_END
}

void mgbhip_default_options(mgbhip_options* o, int64_t n_nodes) {
    const double eps = std::numeric_limits<double>::epsilon();
    o->tol = std::sqrt(eps);
    o->t = 0.1;
    o->kappa = 10.0;
    o->maxit = 10000;
    o->max_newton = (int32_t)std::ceil(std::log2(-std::log2(eps)) + 2);
    o->ls_beta = 0.5;
    o->ls_c1 = 0.1;
    o->line_search = 0;
    o->stop_lambda_tol = 0.25 / std::sqrt((double)n_nodes);
    o->stop_theta = 0.9;
    o->finalize = 1;
    o->finalize_theta = 0.9;
    o->early_stop = 0;
    o->stopping_criterion = nullptr;
    o->early_stop_fn = nullptr;
    o->user = nullptr;
}

int mgbhip_mgb_core(mgbhip_problem* P, double* z, const double* c, const mgbhip_options* opt, mgbhip_core_result* res) {
    MGB_API_BEGIN_ON(P)
    MGB_REQUIRE(P && z && c && opt && res, "null argument");
    MGB_REQUIRE(opt->tol > 0 && opt->t > 0 && opt->kappa > 1 && opt->maxit >= 1 && opt->max_newton >= 1, "bad options");
    int rc = core_run(P, z, c, opt, res);
    if (rc == MGBHIP_ERR_CONVERGENCE)
        g_last_error = res->failure_code == 2 ? "Convergence failure in mgb_solve: iteration_limit"
                                              : "Convergence failure in mgb_solve: stall";
    return rc;
    MGB_API_END
}

int mgbhip_matched_t(mgbhip_problem* P, const double* z, const double* c, double t_default, double* t_out) {
    MGB_API_BEGIN_ON(P)
    MGB_REQUIRE(P && z && c && t_out, "null argument");
    return matched_t_run(P, z, c, t_default, t_out);
    MGB_API_END
}

int mgbhip_stage_ms(mgbhip_problem* P, const char* stage, double* total_ms, int64_t* launches) {
    MGB_API_BEGIN_ON(P)
    MGB_REQUIRE(P && stage, "null argument");
    P->ctx->timers.collect();
    auto it = P->ctx->timers.recs.find(stage);
    if (total_ms) *total_ms = it == P->ctx->timers.recs.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == P->ctx->timers.recs.end() ? 0 : it->second.launches;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_solver_stats(mgbhip_problem* P, int32_t level, double* out) {
    MGB_API_BEGIN
    check_level(P, level);
    MGB_REQUIRE(out != nullptr, "null argument");
    const Level& L = P->levels[level];
    const MfPlan& pl = L.solver.plan;
    out[0] = (double)pl.fronts.size();
    out[1] = (double)pl.max_m;
    out[2] = (double)pl.arena_doubles;
    out[3] = (double)pl.factor_flops;
    out[4] = (double)pl.peeled;
    out[5] = pl.level_ptr.empty() ? 0.0 : (double)(pl.level_ptr.size() - 1);
    out[6] = (double)L.nnz;
    out[7] = (double)L.m;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_solver_chain(mgbhip_problem* P, int32_t level, double* out) {
    MGB_API_BEGIN
    check_level(P, level);
    MGB_REQUIRE(out != nullptr, "null argument");
    MGB_REQUIRE(P->levels[level].solver.analyzed, "mgbhip_solver_chain: the level has not been factored yet");
    P->levels[level].solver.chain_stats(out);
    return MGBHIP_OK;
    MGB_API_END
}

static_assert(MGBHIP_LAUNCH_ROW == mgbhip::MF_LAUNCH_ROW && MGBHIP_ASM_GATHER == mgbhip::MF_ASM_GATHER &&
              MGBHIP_ASM_COLUMNS == mgbhip::MF_ASM_COLS && MGBHIP_B0_GATHER == mgbhip::MF_B0_GATHER &&
              MGBHIP_B0_DIAG0 == mgbhip::MF_B0_DIAG0 && MGBHIP_B0_STEP0 == mgbhip::MF_B0_STEP0 && MGBHIP_BWD_K8 == mgbhip::MF_BWD_K8 &&
              MGBHIP_BWD_K16 == mgbhip::MF_BWD_K16 && MGBHIP_BWD_GENERAL == mgbhip::MF_BWD_GENERAL, "mgbhip.h and mf_launch_plan.hpp disagree");

int64_t mgbhip_solver_launches(mgbhip_problem* P, int32_t level, int32_t* out, int64_t cap) {
    int64_t count = 0;
    const int rc = [&]() -> int {
        MGB_API_BEGIN
        check_level(P, level);
        MGB_REQUIRE(cap >= 0 && (out != nullptr || cap == 0), "bad output buffer");
        MGB_REQUIRE(P->levels[level].solver.analyzed, "mgbhip_solver_launches: the level has not been factored yet");
        count = P->levels[level].solver.launches(out, cap);
        return MGBHIP_OK;
        MGB_API_END
    }();
    return rc == MGBHIP_OK ? count : -(int64_t)rc;
}

#ifdef MGB_STEP_PROBE
int mgbhip_debug_probe(long long* out64) { (void)hipDeviceSynchronize(); mgbhip::mf_debug_probe(out64); return 0; }
#endif

int mgbhip_reset_stage_timers(mgbhip_problem* P, int enable) {
    MGB_API_BEGIN_ON(P)
    MGB_REQUIRE(P, "null argument");
    P->ctx->timers.reset(enable != 0);
    return MGBHIP_OK;
    MGB_API_END
}

// the checks of the geometry arguments shared by mgbhip_interpolate, mgbhip_interpolate_grad and mgbhip_locator_create;
// fills in.table_len and in.sorted
static void interpolate_check_geometry(InterpIn& in) {
    const int32_t family = in.family, d = in.d, k = in.k, p = in.p;
    const int64_t N = in.N;
    const double* x = in.x;
    const bool fem = interp_is_fem(family);
    if (fem) {
        MGB_REQUIRE(x != nullptr && in.table != nullptr, "interpolate: FEM families need node coordinates and a table");
        MGB_REQUIRE(k >= 1 && k <= INTERP_MAX_DEGREE, "interpolate: element degree out of range");
    }
    switch (family) {
        case MGBHIP_INTERP_FEM1D:
            MGB_REQUIRE(d == 1 && p == k + 1, "interpolate: fem1d needs d = 1, p = k + 1");
            in.table_len = k + 1;
            for (int64_t e = 1; e < N && in.sorted; ++e) in.sorted = x[e * p] >= x[(e - 1) * p];
            break;
        case MGBHIP_INTERP_QK: {
            MGB_REQUIRE(d == 2 || d == 3, "interpolate: Q_k needs d = 2 or 3");
            int64_t s = 1;
            for (int a = 0; a < d; ++a) s *= k + 1;
            MGB_REQUIRE(p == s, "interpolate: Q_k needs p = (k + 1)^d");
            in.table_len = k + 1;
            break;
        }
        case MGBHIP_INTERP_P1:
        case MGBHIP_INTERP_P2:
        case MGBHIP_INTERP_P2C:
            MGB_REQUIRE(d == 2, "interpolate: triangles need d = 2");
            MGB_REQUIRE(family == MGBHIP_INTERP_P1 ? p == 3 : (p == 6 || p == 7), "interpolate: bad nodes per triangle");
            in.table_len = (int64_t)p * 10;
            break;
        case MGBHIP_INTERP_SPECTRAL1D:
            MGB_REQUIRE(d == 1 && N == 1 && k >= 0 && p == k + 1, "interpolate: spectral1d needs d = 1, N = 1, p = n");
            in.table = nullptr;
            break;
        case MGBHIP_INTERP_SPECTRAL2D:
            MGB_REQUIRE(d == 2 && N == 1 && k >= 0 && (int64_t)p == (int64_t)(k + 1) * (k + 1),
                        "interpolate: spectral2d needs d = 2, N = 1, p = n^2");
            in.table = nullptr;
            break;
        default:
            throw InvalidArgument("interpolate: unknown family");
    }
    MGB_REQUIRE((int64_t)p * N < (int64_t)INT32_MAX && in.M < (int64_t)INT32_MAX, "interpolate: sizes exceed 32-bit indexing");
}

// the argument checks and the run shared by mgbhip_interpolate (grad = NULL) and mgbhip_interpolate_grad
static void interpolate_checked(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N,
                                const double* x, const double* table, int32_t ncomp, const double* z, int64_t M,
                                const double* pts, double* out, double* grad, int32_t* elem) {
    const bool need_out = grad == nullptr;      // the gradient entry may leave the values out
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(N > 0, "interpolate: no elements (N = 0)");
    MGB_REQUIRE(M >= 0 && ncomp >= 1 && p >= 1, "interpolate: bad sizes");
    MGB_REQUIRE(z != nullptr && (M == 0 || (pts != nullptr && (out != nullptr || !need_out))), "null argument");
    InterpIn in;
    in.family = family; in.d = d; in.k = k; in.p = p; in.N = N; in.ncomp = ncomp; in.M = M;
    in.x = x; in.table = table; in.z = z; in.pts = pts; in.out = out; in.grad = grad; in.elem = elem;
    interpolate_check_geometry(in);
    MGB_REQUIRE(M * ncomp * (grad ? d : 1) < (int64_t)INT32_MAX, "interpolate: sizes exceed 32-bit indexing");
    interpolate_run(in, ctx->stream);
}

int mgbhip_interpolate(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N, const double* x,
                       const double* table, int32_t ncomp, const double* z, int64_t M, const double* pts, double* out,
                       int32_t* elem) {
    MGB_API_BEGIN_ON(ctx)
    interpolate_checked(ctx, family, d, k, p, N, x, table, ncomp, z, M, pts, out, nullptr, elem);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_interpolate_grad(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N,
                            const double* x, const double* table, int32_t ncomp, const double* z, int64_t M,
                            const double* pts, double* out, double* grad, int32_t* elem) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(grad != nullptr, "interpolate_grad: null gradient array");
    interpolate_checked(ctx, family, d, k, p, N, x, table, ncomp, z, M, pts, out, grad, elem);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_locator_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N, const double* x,
                          const double* table, int64_t M, const double* pts, mgbhip_locator** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr, "null output pointer");
    MGB_REQUIRE(N > 0, "interpolate: no elements (N = 0)");
    MGB_REQUIRE(M >= 0 && p >= 1, "interpolate: bad sizes");
    MGB_REQUIRE(M == 0 || pts != nullptr, "null argument");
    InterpIn in;
    in.family = family; in.d = d; in.k = k; in.p = p; in.N = N; in.M = M;
    in.x = x; in.table = table; in.pts = pts;
    interpolate_check_geometry(in);
    create_handle(ctx, out, [&](Locator& L) { locator_build(L, in, ctx->stream); });
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_locator_elements(const mgbhip_locator* loc, int32_t* elem) {
    MGB_API_BEGIN_ON(loc)
    MGB_REQUIRE(loc != nullptr, "null locator");
    MGB_REQUIRE(loc->obj.M == 0 || elem != nullptr, "null argument");
    locator_elements(loc->obj, elem, loc->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_locator_evaluate(mgbhip_locator* loc, int32_t ncomp, const double* z, double* out, double* grad) {
    MGB_API_BEGIN_ON(loc)
    MGB_REQUIRE(loc != nullptr, "null locator");
    const Locator& L = loc->obj;
    MGB_REQUIRE(ncomp >= 1, "interpolate: bad sizes");
    MGB_REQUIRE(z != nullptr && (L.M == 0 || out != nullptr || grad != nullptr), "null argument");
    MGB_REQUIRE(L.M * ncomp * (grad ? L.d : 1) < (int64_t)INT32_MAX, "interpolate: sizes exceed 32-bit indexing");
    locator_evaluate(loc->obj, ncomp, z, out, grad, loc->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_locator_destroy(mgbhip_locator* loc) { return destroy_handle(loc); }

int mgbhip_closest_create(mgbhip_ctx* ctx, int32_t d, int32_t e, int32_t k, int64_t N, const double* x,
                          const double* nodes, int64_t M, const double* pts, double max_distance,
                          mgbhip_closest** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr, "null output pointer");
    MGB_REQUIRE((d == 1 && (e == 2 || e == 3)) || (d == 2 && e == 3),
                "closest_point: (d, e) must be (1, 2), (1, 3) or (2, 3)");
    MGB_REQUIRE(k >= 1 && k <= INTERP_MAX_DEGREE, "closest_point: element degree out of range");
    MGB_REQUIRE(N > 0, "closest_point: no elements (N = 0)");
    MGB_REQUIRE(M >= 0, "closest_point: bad sizes");
    MGB_REQUIRE(x != nullptr && nodes != nullptr && (M == 0 || pts != nullptr), "null argument");
    MGB_REQUIRE(std::isfinite(max_distance) && max_distance >= 0.0, "closest_point: max_distance must be finite and >= 0");
    const int64_t p = d == 1 ? k + 1 : (int64_t)(k + 1) * (k + 1);
    MGB_REQUIRE(p * N * e < (int64_t)INT32_MAX && M * e < (int64_t)INT32_MAX, "closest_point: sizes exceed 32-bit indexing");
    create_handle(ctx, out, [&](Closest& Cl) { closest_build(Cl, d, e, k, N, x, nodes, M, pts, max_distance, ctx->stream); });
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_closest_fetch(const mgbhip_closest* cp, int32_t* elem, double* xi, double* foot, double* dist, int32_t* flag) {
    MGB_API_BEGIN_ON(cp)
    MGB_REQUIRE(cp != nullptr, "null closest-point locator");
    closest_fetch(cp->obj, elem, xi, foot, dist, flag, cp->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_closest_evaluate(mgbhip_closest* cp, int32_t ncomp, const double* z, double* out, double* grad) {
    MGB_API_BEGIN_ON(cp)
    MGB_REQUIRE(cp != nullptr, "null closest-point locator");
    const Closest& Cl = cp->obj;
    MGB_REQUIRE(ncomp >= 1, "closest_point: bad sizes");
    MGB_REQUIRE(z != nullptr && (Cl.M == 0 || out != nullptr || grad != nullptr), "null argument");
    MGB_REQUIRE(Cl.M * ncomp * (grad ? Cl.e : 1) < (int64_t)INT32_MAX && (int64_t)Cl.p * Cl.N * ncomp < (int64_t)INT32_MAX,
                "closest_point: sizes exceed 32-bit indexing");
    closest_evaluate(cp->obj, ncomp, z, out, grad, cp->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_closest_destroy(mgbhip_closest* cp) { return destroy_handle(cp); }

static_assert(MGBHIP_QUAD_VALUE == QUAD_VALUE && MGBHIP_QUAD_LP == QUAD_LP && MGBHIP_QUAD_W1P == QUAD_W1P &&
              MGBHIP_QUAD_ENERGY == QUAD_ENERGY, "mgbhip.h mirrors QuadKind");

static bool quad_dims_ok(int32_t d, int32_t e) { return d >= 1 && d <= 3 && e >= d && e <= 3; }

// the ten slots of mgbhip_quadrature_plan and mgbhip_faces_plan (16 are zeroed).  lds: slot 8 as each entry point has always
// reported plan.lds (the faces plan stops at INT32_MAX, the quadrature plan converts); the table bytes stop at INT32_MAX
static void quad_plan_out(const QuadPlan& plan, int32_t lds, size_t table_bytes, int32_t* out) {
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[0] = plan.threads; out[1] = plan.S; out[2] = plan.G; out[3] = plan.chunk; out[4] = plan.tables_lds;
    out[5] = plan.reduce_threads; out[6] = (int32_t)plan.groups; out[7] = (int32_t)plan.grid;
    out[8] = lds;
    out[9] = (int32_t)std::min<size_t>(table_bytes, (size_t)INT32_MAX);
}

int mgbhip_quadrature_create(mgbhip_ctx* ctx, int32_t d, int32_t e, int32_t p, int64_t N, const double* x, int32_t Q,
                             const double* wref, const double* phi, const double* dphi, mgbhip_quadrature** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr, "null output pointer");
    MGB_REQUIRE(quad_dims_ok(d, e), "quadrature: (d, e) must be (1, 1..3), (2, 2..3) or (3, 3)");
    MGB_REQUIRE(N > 0, "quadrature: no elements (N = 0)");
    MGB_REQUIRE(p >= 1 && Q >= 1, "quadrature: bad sizes");
    MGB_REQUIRE(x != nullptr && wref != nullptr && phi != nullptr && dphi != nullptr, "null argument");
    MGB_REQUIRE((int64_t)(1 + d) * Q * p < (int64_t)INT32_MAX && (int64_t)p * N * e < (int64_t)INT32_MAX &&
                    N * Q * e < (int64_t)INT32_MAX,
                "quadrature: sizes exceed 32-bit indexing");
    MGB_REQUIRE(quad_decide(d, e, p, Q, N).G >= 1, "quadrature: an element's nodes do not fit in LDS");
    for (int64_t i = 0; i < (int64_t)p * N * e; ++i) MGB_REQUIRE(std::isfinite(x[i]), "quadrature: the mesh has non-finite node coordinates");
    for (int32_t q = 0; q < Q; ++q) MGB_REQUIRE(std::isfinite(wref[q]), "quadrature: the rule must be finite");
    for (int64_t i = 0; i < (int64_t)Q * p; ++i) MGB_REQUIRE(std::isfinite(phi[i]), "quadrature: the basis tables must be finite");
    for (int64_t i = 0; i < (int64_t)Q * p * d; ++i) MGB_REQUIRE(std::isfinite(dphi[i]), "quadrature: the basis tables must be finite");
    create_handle(ctx, out, [&](Quadrature& Qd) { quadrature_build(Qd, d, e, p, N, x, Q, wref, phi, dphi, ctx->stream); });
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_quadrature_points(mgbhip_quadrature* h, double* points) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null quadrature");
    MGB_REQUIRE(points != nullptr, "null argument");
    quadrature_geometry(h->obj, points, nullptr, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_quadrature_weights(mgbhip_quadrature* h, double* weights) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null quadrature");
    MGB_REQUIRE(weights != nullptr, "null argument");
    quadrature_geometry(h->obj, nullptr, weights, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

// the size checks integrate and max share
static void quad_check_call(const Quadrature& Qd, int32_t kind, int32_t ncol, const double* z, const double* minus) {
    MGB_REQUIRE(kind >= QUAD_VALUE && kind <= QUAD_ENERGY, "quadrature: bad kind");
    MGB_REQUIRE(ncol >= 1, "quadrature: bad sizes");
    MGB_REQUIRE(z != nullptr, "null argument");
    MGB_REQUIRE(minus == nullptr || kind == QUAD_LP || kind == QUAD_W1P, "quadrature: minus goes with the lp and w1p kinds only");
    MGB_REQUIRE((int64_t)Qd.p * Qd.N * ncol < (int64_t)INT32_MAX && Qd.N * Qd.Q * ncol * (kind == QUAD_W1P ? Qd.e : 1) < (int64_t)INT32_MAX,
                "quadrature: sizes exceed 32-bit indexing");
}

int mgbhip_quadrature_integrate(mgbhip_quadrature* h, int32_t kind, double pexp, int32_t ncol, const double* z, const double* minus,
                                const double* source, double* per_element, double* totals) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null quadrature");
    quad_check_call(h->obj, kind, ncol, z, minus);
    MGB_REQUIRE(totals != nullptr, "null argument");
    MGB_REQUIRE(kind == QUAD_VALUE || (std::isfinite(pexp) && pexp > 0.0), "quadrature: p must be finite and > 0");
    MGB_REQUIRE((kind == QUAD_ENERGY) == (source != nullptr), "quadrature: source goes with the energy kind, and only with it");
    quadrature_integrate(h->obj, kind, kind == QUAD_VALUE ? 1.0 : pexp, false, ncol, z, minus, source, per_element, totals,
                         h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_quadrature_max(mgbhip_quadrature* h, int32_t kind, int32_t ncol, const double* z, const double* minus, double* maxima) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null quadrature");
    quad_check_call(h->obj, kind, ncol, z, minus);
    MGB_REQUIRE(kind == QUAD_LP || kind == QUAD_W1P, "quadrature: the maximum is defined for the lp and w1p kinds");
    MGB_REQUIRE(maxima != nullptr, "null argument");
    quadrature_integrate(h->obj, kind, 1.0, true, ncol, z, minus, nullptr, nullptr, maxima, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_quadrature_plan(int32_t d, int32_t e, int32_t p, int32_t Q, int64_t N, int32_t* out) {
    MGB_API_BEGIN
    MGB_REQUIRE(out != nullptr, "null argument");
    MGB_REQUIRE(quad_dims_ok(d, e) && p >= 1 && Q >= 1 && N >= 1, "quadrature: bad sizes");
    const QuadPlan plan = quad_decide(d, e, p, Q, N);
    quad_plan_out(plan, (int32_t)plan.lds, quad_lds_tables(1 + d, p, Q), out);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_quadrature_times(const mgbhip_quadrature* h, double* ms) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null quadrature");
    MGB_REQUIRE(ms != nullptr, "null argument");
    quadrature_times(h->obj, ms);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_quadrature_destroy(mgbhip_quadrature* h) { return destroy_handle(h); }

int mgbhip_residual_create(mgbhip_ctx* ctx, int32_t d, int32_t p, int64_t N, const double* x, int32_t Q, const double* wref,
                           const double* phi, const double* dphi, const double* d2phi, mgbhip_residual** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr, "null output pointer");
    MGB_REQUIRE(d == 2 || d == 3, "residual: d must be 2 or 3");
    MGB_REQUIRE(N > 0, "residual: no elements (N = 0)");
    MGB_REQUIRE(p >= 1 && Q >= 1, "residual: bad sizes");
    MGB_REQUIRE(x != nullptr && wref != nullptr && phi != nullptr && dphi != nullptr && d2phi != nullptr, "null argument");
    const int32_t M = d * (d + 1) / 2;
    MGB_REQUIRE((int64_t)residual_rows(d) * Q * p < (int64_t)INT32_MAX && (int64_t)p * N * d < (int64_t)INT32_MAX &&
                    N * Q * (d + 1) < (int64_t)INT32_MAX,
                "residual: sizes exceed 32-bit indexing");
    MGB_REQUIRE(residual_decide(d, p, Q, N).G >= 1, "residual: an element's nodes do not fit in LDS");
    for (int64_t i = 0; i < (int64_t)p * N * d; ++i) MGB_REQUIRE(std::isfinite(x[i]), "residual: the mesh has non-finite node coordinates");
    for (int32_t q = 0; q < Q; ++q) MGB_REQUIRE(std::isfinite(wref[q]) && wref[q] > 0.0, "residual: the rule's weights must be positive and finite");
    for (int64_t i = 0; i < (int64_t)Q * p; ++i) MGB_REQUIRE(std::isfinite(phi[i]), "residual: the basis tables must be finite");
    for (int64_t i = 0; i < (int64_t)Q * p * d; ++i) MGB_REQUIRE(std::isfinite(dphi[i]), "residual: the basis tables must be finite");
    for (int64_t i = 0; i < (int64_t)Q * p * M; ++i) MGB_REQUIRE(std::isfinite(d2phi[i]), "residual: the basis tables must be finite");
    create_handle(ctx, out, [&](Residual& Rd) { residual_build(Rd, d, p, N, x, Q, wref, phi, dphi, d2phi, ctx->stream); });
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_residual_geometry(mgbhip_residual* h, double* points, double* weights, double* sizes) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null residual");
    residual_geometry(h->obj, points, weights, sizes, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

// the checks pointwise and integrate share
static void residual_check_call(const Residual& Rd, double pexp, int32_t ncol, const double* z, const double* source, int32_t at_points) {
    MGB_REQUIRE(ncol >= 1, "residual: bad sizes");
    MGB_REQUIRE(z != nullptr && source != nullptr, "null argument");
    MGB_REQUIRE(at_points == 0 || at_points == 1, "residual: at_points must be 0 (p N nodal values) or 1 (N x Q values at the points)");
    MGB_REQUIRE(std::isfinite(pexp) && pexp >= 1.0, "residual: p must be finite and >= 1");
    MGB_REQUIRE((int64_t)Rd.p * Rd.N * ncol < (int64_t)INT32_MAX && Rd.N * Rd.Q * ncol < (int64_t)INT32_MAX,
                "residual: sizes exceed 32-bit indexing");
}

int mgbhip_residual_pointwise(mgbhip_residual* h, double pexp, int32_t ncol, const double* z, const double* source, int32_t at_points,
                              double* r) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null residual");
    residual_check_call(h->obj, pexp, ncol, z, source, at_points);
    MGB_REQUIRE(r != nullptr, "null argument");
    residual_pointwise(h->obj, pexp, ncol, z, source, at_points == 1, r, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_residual_integrate(mgbhip_residual* h, double pexp, int32_t ncol, const double* z, const double* source, int32_t at_points,
                              double* per_element, double* totals) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null residual");
    residual_check_call(h->obj, pexp, ncol, z, source, at_points);
    MGB_REQUIRE(totals != nullptr, "null argument");
    residual_integrate(h->obj, pexp, ncol, z, source, at_points == 1, per_element, totals, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_residual_plan(int32_t d, int32_t p, int32_t Q, int64_t N, int32_t* out) {
    MGB_API_BEGIN
    MGB_REQUIRE(out != nullptr, "null argument");
    MGB_REQUIRE((d == 2 || d == 3) && p >= 1 && Q >= 1 && N >= 1, "residual: bad sizes");
    const QuadPlan plan = residual_decide(d, p, Q, N);
    quad_plan_out(plan, (int32_t)plan.lds, quad_lds_tables(residual_rows(d), p, Q), out);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_residual_times(const mgbhip_residual* h, double* ms) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null residual");
    MGB_REQUIRE(ms != nullptr, "null argument");
    residual_times(h->obj, ms);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_residual_destroy(mgbhip_residual* h) { return destroy_handle(h); }

static_assert(MGBHIP_FACE_VALUE == FACE_VALUE && MGBHIP_FACE_FLUX == FACE_FLUX, "mgbhip.h mirrors FaceKind");

int mgbhip_faces_create(mgbhip_ctx* ctx, int32_t d, int32_t p, int64_t N, const double* x, const int32_t* t, int32_t F, int32_t Qf,
                        const double* wf, const double* phi, const double* dphi, const double* tangents, const double* normals,
                        const int32_t* corners, int32_t ncode, const int32_t* perm, mgbhip_faces** out, int64_t* nboundary,
                        int64_t* ninterior) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr && nboundary != nullptr && ninterior != nullptr, "null output pointer");
    MGB_REQUIRE(d == 2 || d == 3, "faces: d must be 2 or 3");
    MGB_REQUIRE(N > 0, "faces: no elements (N = 0)");
    MGB_REQUIRE(p >= 1 && F >= 1 && F <= 8 && Qf >= 1, "faces: bad sizes");
    MGB_REQUIRE(ncode == (d == 2 ? 2 : 8), "faces: the permutation table has 2 codes in 2-D and 8 in 3-D");
    MGB_REQUIRE(x != nullptr && t != nullptr && wf != nullptr && phi != nullptr && dphi != nullptr && tangents != nullptr &&
                    normals != nullptr && corners != nullptr && perm != nullptr, "null argument");
    MGB_REQUIRE(Qf <= FACE_MAX_QF, "faces: at most 100 points per face");
    MGB_REQUIRE((int64_t)F * (1 + d) * Qf * p < (int64_t)INT32_MAX && (int64_t)p * N * d < (int64_t)INT32_MAX &&
                    N * F * Qf * (2 * d + 1) < (int64_t)INT32_MAX,
                "faces: sizes exceed 32-bit indexing");
    MGB_REQUIRE(face_decide(d, p, Qf, F, 2, 1).G >= 1, "faces: the nodes of one face's elements do not fit in LDS");
    const int NC = 1 << (d - 1);
    for (int64_t i = 0; i < (int64_t)p * N * d; ++i) MGB_REQUIRE(std::isfinite(x[i]), "faces: the mesh has non-finite node coordinates");
    for (int64_t i = 0; i < (int64_t)p * N; ++i) MGB_REQUIRE(t[i] >= 0, "faces: node ids must lie in [0, 2^31)");
    for (int32_t q = 0; q < Qf; ++q) MGB_REQUIRE(std::isfinite(wf[q]), "faces: the rule must be finite");
    for (int64_t i = 0; i < (int64_t)F * Qf * p; ++i) MGB_REQUIRE(std::isfinite(phi[i]), "faces: the basis tables must be finite");
    for (int64_t i = 0; i < (int64_t)F * Qf * p * d; ++i) MGB_REQUIRE(std::isfinite(dphi[i]), "faces: the basis tables must be finite");
    for (int i = 0; i < F * (d - 1) * d; ++i) MGB_REQUIRE(std::isfinite(tangents[i]), "faces: the tangents must be finite");
    for (int i = 0; i < F * d; ++i) MGB_REQUIRE(std::isfinite(normals[i]), "faces: the normals must be finite");
    for (int i = 0; i < F * NC; ++i) MGB_REQUIRE(corners[i] >= 0 && corners[i] < p, "faces: a face corner is not a node of the element");
    for (int i = 0; i < ncode * Qf; ++i) MGB_REQUIRE(perm[i] >= 0 && perm[i] < Qf, "faces: a permutation entry is not a face point");
    FacesIn in;
    in.d = d; in.p = p; in.F = F; in.Qf = Qf; in.ncode = ncode; in.N = N; in.x = x; in.t = t; in.wf = wf; in.phi = phi; in.dphi = dphi;
    in.tangents = tangents; in.normals = normals; in.corners = corners; in.perm = perm;
    create_handle(ctx, out, [&](Faces& Fc) { faces_build(Fc, in, ctx->stream); });
    *nboundary = (*out)->obj.B;
    *ninterior = (*out)->obj.I;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_faces_topology(const mgbhip_faces* h, int32_t* boundary, int32_t* interior, int32_t* orientation, int32_t* element_faces) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null faces");
    faces_topology(h->obj, boundary, interior, orientation, element_faces, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_faces_geometry(mgbhip_faces* h, int32_t which, double* points, double* normals, double* measures) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null faces");
    MGB_REQUIRE(which == 0 || which == 1, "faces: which must be 0 (boundary) or 1 (interior)");
    faces_geometry(h->obj, which, points, normals, measures, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_faces_sizes(const mgbhip_faces* h, double* sizes) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null faces");
    MGB_REQUIRE(sizes != nullptr, "null argument");
    faces_sizes(h->obj, sizes, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

// the checks integrate, jumps and indicator share
static void faces_check_call(const Faces& Fc, int32_t kind, double pexp, int32_t ncol, const double* z) {
    MGB_REQUIRE(kind == FACE_VALUE || kind == FACE_FLUX, "faces: bad kind");
    MGB_REQUIRE(ncol >= 1, "faces: bad sizes");
    MGB_REQUIRE(z != nullptr, "null argument");
    MGB_REQUIRE(kind == FACE_VALUE || (std::isfinite(pexp) && pexp >= 1.0), "faces: p must be finite and >= 1");
    MGB_REQUIRE((int64_t)Fc.p * Fc.N * ncol < (int64_t)INT32_MAX && Fc.N * Fc.F * ncol < (int64_t)INT32_MAX,
                "faces: sizes exceed 32-bit indexing");
}

int mgbhip_faces_integrate(mgbhip_faces* h, int32_t kind, double pexp, int32_t ncol, const double* z, const double* weight,
                           double* per_face, double* totals) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null faces");
    faces_check_call(h->obj, kind, pexp, ncol, z);
    MGB_REQUIRE(totals != nullptr, "null argument");
    faces_integrate(h->obj, kind, kind == FACE_VALUE ? 2.0 : pexp, ncol, z, weight, per_face, totals, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_faces_jumps(mgbhip_faces* h, int32_t kind, double pexp, int32_t ncol, const double* z, double* jumps) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null faces");
    faces_check_call(h->obj, kind, pexp, ncol, z);
    MGB_REQUIRE(jumps != nullptr || h->obj.I == 0, "null argument");
    faces_jumps(h->obj, kind, kind == FACE_VALUE ? 2.0 : pexp, ncol, z, jumps, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_faces_indicator(mgbhip_faces* h, double pexp, int32_t ncol, const double* z, double* eta2, double* totals) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null faces");
    faces_check_call(h->obj, FACE_FLUX, pexp, ncol, z);
    MGB_REQUIRE(eta2 != nullptr && totals != nullptr, "null argument");
    faces_indicator(h->obj, pexp, ncol, z, eta2, totals, h->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_faces_plan(int32_t d, int32_t p, int32_t Qf, int32_t F, int32_t sides, int64_t nfaces, int32_t* out) {
    MGB_API_BEGIN
    MGB_REQUIRE(out != nullptr, "null argument");
    MGB_REQUIRE((d == 2 || d == 3) && p >= 1 && Qf >= 1 && F >= 1 && (sides == 1 || sides == 2) && nfaces >= 0, "faces: bad sizes");
    const QuadPlan plan = face_decide(d, p, Qf, F, sides, nfaces);
    quad_plan_out(plan, (int32_t)std::min<size_t>(plan.lds, (size_t)INT32_MAX), face_lds_tables(d, p, Qf, F), out);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_faces_times(const mgbhip_faces* h, double* ms) {
    MGB_API_BEGIN_ON(h)
    MGB_REQUIRE(h != nullptr, "null faces");
    MGB_REQUIRE(ms != nullptr, "null argument");
    faces_times(h->obj, ms);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_faces_destroy(mgbhip_faces* h) { return destroy_handle(h); }

int mgbhip_contour_create_embedded(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t e, int32_t k, int32_t p, int64_t N,
                                   const double* x, const double* table, int32_t nfield, const double* fields,
                                   int32_t nlevels, const double* levels, int32_t refine, mgbhip_contour** out,
                                   int64_t* nsimplices) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr && nsimplices != nullptr, "null output pointer");
    MGB_REQUIRE(interp_is_located(family), "contour: only the Q_k (d = 2, 3), P1 and P2 families have level sets");
    MGB_REQUIRE(N > 0, "contour: no elements (N = 0)");
    MGB_REQUIRE(p >= 1 && nlevels >= 0, "contour: bad sizes");
    MGB_REQUIRE(nfield >= 1 && nfield <= CONTOUR_MAX_FIELDS, "contour: nfield must be 1..5 (at most four carried fields)");
    MGB_REQUIRE(fields != nullptr && (nlevels == 0 || levels != nullptr), "null argument");
    InterpIn geo;
    geo.family = family; geo.d = d; geo.k = k; geo.p = p; geo.N = N; geo.x = x; geo.table = table;
    interpolate_check_geometry(geo);
    MGB_REQUIRE(e == d || (family == MGBHIP_INTERP_QK && d == 2 && e == 3),
                "contour_create_embedded: e must be d, or 3 for Q_k with d = 2 (a surface in R^3)");
    MGB_REQUIRE(refine >= 1 && refine <= (d == 3 ? CONTOUR_MAX_REFINE_3D : CONTOUR_MAX_REFINE_2D),
                d == 3 ? "contour: refine must be 1..8 for d = 3" : "contour: refine must be 1..16 for d = 2");
    for (int32_t l = 0; l < nlevels; ++l) MGB_REQUIRE(std::isfinite(levels[l]), "contour: a level is not finite");
    ContourIn in;
    in.family = family; in.d = d; in.e = e; in.k = k; in.p = p; in.N = N; in.nfield = nfield; in.nlevels = nlevels;
    in.refine = refine; in.x = x; in.table = table; in.fields = fields; in.levels = levels;
    create_handle(ctx, out, [&](Contour& C) { contour_build(C, in, ctx->stream); });
    *nsimplices = (*out)->obj.S;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_contour_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N, const double* x,
                          const double* table, int32_t nfield, const double* fields, int32_t nlevels,
                          const double* levels, int32_t refine, mgbhip_contour** out, int64_t* nsimplices) {
    return mgbhip_contour_create_embedded(ctx, family, d, d, k, p, N, x, table, nfield, fields, nlevels, levels, refine, out,
                                          nsimplices);
}

int mgbhip_contour_fetch(const mgbhip_contour* c, double* points, int32_t* level, int32_t* element, double* carried) {
    MGB_API_BEGIN_ON(c)
    MGB_REQUIRE(c != nullptr, "null contour");
    MGB_REQUIRE(c->obj.S == 0 || (points != nullptr && level != nullptr && element != nullptr), "null argument");
    contour_fetch(c->obj, points, level, element, carried, c->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_contour_destroy(mgbhip_contour* c) { return destroy_handle(c); }

int mgbhip_tessellate_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t e, int32_t k, int32_t p, int64_t N,
                             const double* x, const double* table, int32_t nfield, const double* fields, int32_t refine,
                             mgbhip_tessellation** out, int64_t* ntriangles) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr && ntriangles != nullptr, "null output pointer");
    MGB_REQUIRE(interp_is_located(family),
                "tessellate: only the Q_k (d = 2), P1 and P2 families are tessellated");
    MGB_REQUIRE(d == 2, "tessellate: d must be 2 (the lattice triangles of 2-D elements)");
    MGB_REQUIRE(N > 0, "tessellate: no elements (N = 0)");
    MGB_REQUIRE(p >= 1, "tessellate: bad sizes");
    MGB_REQUIRE(nfield >= 0 && nfield <= CONTOUR_MAX_FIELDS, "tessellate: nfield must be 0..5");
    MGB_REQUIRE(nfield == 0 || fields != nullptr, "tessellate: null fields");
    InterpIn geo;
    geo.family = family; geo.d = d; geo.k = k; geo.p = p; geo.N = N; geo.x = x; geo.table = table;
    interpolate_check_geometry(geo);
    MGB_REQUIRE(e == 2 || (family == MGBHIP_INTERP_QK && e == 3),
                "tessellate: e must be 2, or 3 for Q_k (a surface in R^3)");
    MGB_REQUIRE(refine >= 1 && refine <= CONTOUR_MAX_REFINE_2D, "tessellate: refine must be 1..16");
    ContourIn in;
    in.family = family; in.d = d; in.e = e; in.k = k; in.p = p; in.N = N; in.nfield = nfield; in.refine = refine;
    in.x = x; in.table = table; in.fields = fields;
    const int64_t T = tessellate_count(in);      // N < 2^31 / p and refine <= 16: no overflow
    if (T > (int64_t)INT32_MAX / 3)
        throw InvalidArgument("tessellate: T = " + std::to_string(T) + " triangles have more than 2^31 - 1 vertices: use a "
                              "smaller refine");
    create_handle(ctx, out, [&](Tessellation& Ts) { tessellate_build(Ts, in, ctx->stream); });
    *ntriangles = (*out)->obj.T;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_tessellate_fetch(const mgbhip_tessellation* t, double* points, int32_t* element, double* values) {
    MGB_API_BEGIN_ON(t)
    MGB_REQUIRE(t != nullptr, "tessellate_fetch: null tessellation");
    MGB_REQUIRE(points != nullptr && element != nullptr, "tessellate_fetch: null argument");
    tessellate_fetch(t->obj, points, element, values, t->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_tessellate_destroy(mgbhip_tessellation* t) { return destroy_handle(t); }

int mgbhip_weld_create(mgbhip_ctx* ctx, int64_t S, int32_t nv, int32_t e, const double* points, const int32_t* group,
                       double tol, int32_t want_normals, mgbhip_weld** out, int64_t* V, int64_t* ncomponents) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr && V != nullptr && ncomponents != nullptr, "null output pointer");
    MGB_REQUIRE(S > 0, "weld: no simplices (S <= 0)");
    MGB_REQUIRE(nv == 2 || nv == 3, "weld: nv must be 2 (segments) or 3 (triangles)");
    MGB_REQUIRE(e == 2 || e == 3, "weld: e must be 2 or 3");
    MGB_REQUIRE(S < ((int64_t)INT32_MAX + 1) / nv, "weld: S x nv corners exceed 32-bit indexing (M >= 2^31)");
    MGB_REQUIRE(std::isfinite(tol) && tol >= 0.0, "weld: tol must be finite and >= 0");
    MGB_REQUIRE(!want_normals || (nv == 3 && e == 3), "weld: normals need triangles in R^3 (nv = 3, e = 3)");
    MGB_REQUIRE(points != nullptr, "weld: null points");
    WeldIn in;
    in.S = S; in.nv = nv; in.e = e; in.points = points; in.group = group; in.tol = tol; in.want_normals = want_normals != 0;
    create_handle(ctx, out, [&](Weld& W) { weld_build(W, in, ctx->stream); });
    *V = (*out)->obj.V;
    *ncomponents = (*out)->obj.ncomp;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_weld_fetch(const mgbhip_weld* w, int32_t* cells, int32_t* first_corner, int32_t* component, double* normals) {
    MGB_API_BEGIN_ON(w)
    MGB_REQUIRE(w != nullptr, "weld_fetch: null weld");
    MGB_REQUIRE(cells != nullptr && first_corner != nullptr && component != nullptr, "weld_fetch: null argument");
    weld_fetch(w->obj, cells, first_corner, component, normals, w->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_weld_rounds(const mgbhip_weld* w, int32_t* vertex_rounds, int32_t* component_rounds) {
    MGB_API_BEGIN
    MGB_REQUIRE(w != nullptr && vertex_rounds != nullptr && component_rounds != nullptr, "weld_rounds: null argument");
    *vertex_rounds = w->obj.vertex_rounds;
    *component_rounds = w->obj.component_rounds;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_weld_destroy(mgbhip_weld* w) { return destroy_handle(w); }

int mgbhip_polyline_create(mgbhip_ctx* ctx, int64_t V, int32_t e, const double* vertices, int64_t S, const int32_t* cells,
                           mgbhip_polyline** out, int64_t* L, int64_t* P, int64_t* ndropped) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr && L != nullptr && P != nullptr && ndropped != nullptr, "polylines: null output pointer");
    MGB_REQUIRE(e == 2 || e == 3, "polylines: e must be 2 or 3");
    MGB_REQUIRE(V >= 0 && V <= (int64_t)INT32_MAX, "polylines: V must be in [0, 2^31)");
    MGB_REQUIRE(S >= 0, "polylines: S must be >= 0");
    MGB_REQUIRE(S < ((int64_t)INT32_MAX + 1) / 2, "polylines: S x 2 half-edges exceed 32-bit indexing (2 S >= 2^31)");
    MGB_REQUIRE(V == 0 || vertices != nullptr, "polylines: null vertices");
    MGB_REQUIRE(S == 0 || cells != nullptr, "polylines: null cells");
    for (int64_t i = 0; i < 2 * S; ++i)
        MGB_REQUIRE(cells[i] >= 0 && cells[i] < V, "polylines: an entry of cells lies outside [0, V)");
    for (int64_t i = 0; i < V * e; ++i) MGB_REQUIRE(std::isfinite(vertices[i]), "polylines: vertices has a non-finite coordinate");
    PolylineIn in;
    in.V = V; in.S = S; in.e = e; in.vertices = vertices; in.cells = cells;
    create_handle(ctx, out, [&](Polyline& Pl) { polyline_build(Pl, in, ctx->stream); });
    *L = (*out)->obj.L;
    *P = (*out)->obj.P;
    *ndropped = (*out)->obj.ndropped;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_polyline_fetch(const mgbhip_polyline* pl, int64_t* offsets, int32_t* vertex, int32_t* segment, uint8_t* closed,
                          double* arclength, double* length) {
    MGB_API_BEGIN_ON(pl)
    MGB_REQUIRE(pl != nullptr, "polyline_fetch: null polyline");
    MGB_REQUIRE(offsets != nullptr, "polyline_fetch: null offsets");
    MGB_REQUIRE(pl->obj.P == 0 || (vertex != nullptr && segment != nullptr && arclength != nullptr),
                "polyline_fetch: null vertex, segment or arclength");
    MGB_REQUIRE(pl->obj.L == 0 || (closed != nullptr && length != nullptr), "polyline_fetch: null closed or length");
    polyline_fetch(pl->obj, offsets, vertex, segment, closed, arclength, length, pl->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_polyline_rounds(const mgbhip_polyline* pl, int32_t* rounds, int32_t* nphases) {
    MGB_API_BEGIN
    MGB_REQUIRE(pl != nullptr && rounds != nullptr && nphases != nullptr, "polyline_rounds: null argument");
    rounds[0] = pl->obj.rounds[0];
    rounds[1] = pl->obj.rounds[1];
    *nphases = 2;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_polyline_destroy(mgbhip_polyline* pl) { return destroy_handle(pl); }

int mgbhip_polyline_sample(mgbhip_ctx* ctx, int32_t e, int64_t P, const double* points, int32_t C, const double* data,
                           int64_t L, const int64_t* offsets, const double* arclength, int64_t Q, const int32_t* line,
                           const double* s, double* out_points, double* out_data) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(e == 2 || e == 3, "polyline_sample: e must be 2 or 3");
    MGB_REQUIRE(P >= 0 && P <= (int64_t)INT32_MAX && L >= 0 && Q >= 0 && C >= 0, "polyline_sample: bad sizes");
    MGB_REQUIRE(Q * (int64_t)(e > C ? e : C) <= (int64_t)INT32_MAX, "polyline_sample: sizes exceed 32-bit indexing");
    MGB_REQUIRE(offsets != nullptr, "polyline_sample: null offsets");
    MGB_REQUIRE(P == 0 || (points != nullptr && arclength != nullptr), "polyline_sample: null points or arclength");
    MGB_REQUIRE(C == 0 || P == 0 || data != nullptr, "polyline_sample: null data with C > 0");
    MGB_REQUIRE(Q == 0 || (line != nullptr && s != nullptr && out_points != nullptr), "polyline_sample: null line, s or out_points");
    MGB_REQUIRE(C == 0 || Q == 0 || out_data != nullptr, "polyline_sample: null out_data with C > 0");
    MGB_REQUIRE(offsets[0] == 0 && offsets[L] == P, "polyline_sample: offsets must run from 0 to P");
    for (int64_t l = 0; l < L; ++l)
        MGB_REQUIRE(offsets[l + 1] - offsets[l] >= 2, "polyline_sample: offsets must give every line at least two points");
    for (int64_t i = 0; i < P; ++i) MGB_REQUIRE(std::isfinite(arclength[i]), "polyline_sample: arclength must be finite");
    for (int64_t q = 0; q < Q; ++q) {
        MGB_REQUIRE(line[q] >= 0 && line[q] < L, "polyline_sample: an entry of line lies outside [0, L)");
        MGB_REQUIRE(std::isfinite(s[q]), "polyline_sample: s must be finite");
    }
    PolylineSampleIn in;
    in.e = e; in.C = C; in.P = P; in.L = L; in.Q = Q; in.points = points; in.data = C ? data : nullptr; in.offsets = offsets;
    in.arclength = arclength; in.line = line; in.s = s;
    polyline_sample(in, out_points, out_data, ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_raycast_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N, const double* x,
                          const double* table, int64_t R, const double* origin, const double* dir, const double* box,
                          double step, double t_min, double t_max, mgbhip_raycast** out, int64_t* nsamples) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr && nsamples != nullptr, "null output pointer");
    MGB_REQUIRE(family == MGBHIP_INTERP_QK || family == MGBHIP_INTERP_P1 || family == MGBHIP_INTERP_P2,
                "raycast: only the Q_k (d = 2, 3), P1 and P2 families are ray cast");
    MGB_REQUIRE(N > 0, "raycast: no elements (N = 0)");
    MGB_REQUIRE(p >= 1 && R >= 0 && R < (int64_t)INT32_MAX, "raycast: bad sizes");
    MGB_REQUIRE(R == 0 || (origin != nullptr && dir != nullptr && box != nullptr), "null argument");
    RayIn in;
    in.geo.family = family; in.geo.d = d; in.geo.k = k; in.geo.p = p; in.geo.N = N; in.geo.x = x; in.geo.table = table;
    interpolate_check_geometry(in.geo);
    MGB_REQUIRE(std::isfinite(step) && step > 0.0, "raycast: step must be finite and positive");
    check_window("raycast", t_min, t_max);
    check_rays("raycast", R, d, origin, dir);
    for (int a = 0; a < d && R > 0; ++a)
        MGB_REQUIRE(std::isfinite(box[a]) && std::isfinite(box[d + a]) && box[a] <= box[d + a], "raycast: bad clip box");
    in.R = R; in.origin = origin; in.dir = dir; in.box = box; in.step = step; in.t_min = t_min; in.t_max = t_max;
    create_handle(ctx, out, [&](RayCaster& RC) { raycast_build(RC, in, ctx->stream); });
    *nsamples = (*out)->obj.S;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_raycast_offsets(const mgbhip_raycast* rc, int64_t* offsets) {
    MGB_API_BEGIN_ON(rc)
    MGB_REQUIRE(rc != nullptr, "null ray caster");
    MGB_REQUIRE(offsets != nullptr, "null argument");
    raycast_offsets(rc->obj, offsets, rc->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_raycast_samples(const mgbhip_raycast* rc, double* pts) {
    MGB_API_BEGIN_ON(rc)
    MGB_REQUIRE(rc != nullptr, "null ray caster");
    MGB_REQUIRE(rc->obj.S == 0 || pts != nullptr, "null argument");
    raycast_samples(rc->obj, pts, rc->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_raycast_lengths(const mgbhip_raycast* rc, double* step, double* length) {
    MGB_API_BEGIN_ON(rc)
    MGB_REQUIRE(rc != nullptr, "null ray caster");
    raycast_lengths(rc->obj, step, length, rc->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_raycast_integrate(mgbhip_raycast* rc, int32_t ncomp, const double* z, double* out) {
    MGB_API_BEGIN_ON(rc)
    MGB_REQUIRE(rc != nullptr, "null ray caster");
    MGB_REQUIRE(ncomp >= 1, "raycast: bad sizes");
    MGB_REQUIRE(z != nullptr && (rc->obj.R == 0 || out != nullptr), "null argument");
    raycast_integrate(rc->obj, ncomp, z, out, rc->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_raycast_render(mgbhip_raycast* rc, const double* u, int32_t K, const double* transfer, double lo, double hi,
                          double* out) {
    MGB_API_BEGIN_ON(rc)
    MGB_REQUIRE(rc != nullptr, "null ray caster");
    MGB_REQUIRE(u != nullptr && transfer != nullptr && (rc->obj.R == 0 || out != nullptr), "null argument");
    MGB_REQUIRE(K >= 2, "raycast: the transfer table needs at least two rows");
    check_transfer_clim(K, transfer, lo, hi);
    raycast_render(rc->obj, u, K, transfer, lo, hi, out, rc->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_raycast_destroy(mgbhip_raycast* rc) { return destroy_handle(rc); }

int mgbhip_raycast_render_layers(mgbhip_raycast* rc, const double* u, int32_t K, const double* transfer, double lo,
                                 double hi, int32_t nhits, const double* t_hit, const double* layer, double* out) {
    MGB_API_BEGIN_ON(rc)
    MGB_REQUIRE(rc != nullptr, "null ray caster");
    MGB_REQUIRE(u != nullptr && transfer != nullptr && (rc->obj.R == 0 || (out != nullptr && t_hit != nullptr && layer != nullptr)),
                "null argument");
    MGB_REQUIRE(K >= 2, "raycast: the transfer table needs at least two rows");
    MGB_REQUIRE(nhits >= 1 && nhits <= SURFACE_MAX_HITS, "raycast: the number of layers per ray must be 1..8");
    check_transfer_clim(K, transfer, lo, hi);
    for (int64_t r = 0; r < rc->obj.R; ++r)
        for (int32_t k = 0; k < nhits; ++k) {
            const double th = t_hit[r * nhits + k];
            MGB_REQUIRE(!std::isnan(th) && (k == 0 || t_hit[r * nhits + k - 1] <= th),
                        "raycast: the layer depths of a ray must ascend (+inf for a missing layer)");
            for (int c = 0; c < 4; ++c)
                MGB_REQUIRE(std::isfinite(layer[(r * nhits + k) * 4 + c]), "raycast: every layer entry must be finite");
        }
    raycast_render_layers(rc->obj, u, K, transfer, lo, hi, nhits, t_hit, layer, out, rc->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_stream_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N, const double* x,
                         const double* table, int32_t field, const double* z, mgbhip_stream** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr, "null output pointer");
    MGB_REQUIRE(interp_is_located(family),
                "stream: only the Q_k (d = 2, 3), P1 and P2 families are traced");
    MGB_REQUIRE(N > 0, "stream: no elements (N = 0)");
    MGB_REQUIRE(p >= 1 && (int64_t)p * N * 3 < (int64_t)INT32_MAX, "stream: bad sizes");
    MGB_REQUIRE(field == MGBHIP_STREAM_VECTOR || field == MGBHIP_STREAM_GRADIENT, "stream: unknown field kind");
    MGB_REQUIRE(z != nullptr, "null argument");
    InterpIn geo;
    geo.family = family; geo.d = d; geo.k = k; geo.p = p; geo.N = N; geo.x = x; geo.table = table;
    interpolate_check_geometry(geo);
    for (int64_t i = 0; i < (int64_t)p * N * d; ++i) MGB_REQUIRE(std::isfinite(x[i]), "stream: non-finite node coordinates");
    create_handle(ctx, out, [&](StreamTracer& Tr) { stream_build(Tr, geo, field, z, ctx->stream); });
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_stream_set_field(mgbhip_stream* s, const double* z) {
    MGB_API_BEGIN_ON(s)
    MGB_REQUIRE(s != nullptr, "null stream tracer");
    MGB_REQUIRE(z != nullptr, "null argument");
    stream_set_field(s->obj, z, s->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_stream_trace(mgbhip_stream* s, int64_t S, const double* seeds, double h, int32_t max_steps, int32_t normalize,
                        double min_speed, double* points, int32_t* n, int32_t* status) {
    MGB_API_BEGIN_ON(s)
    MGB_REQUIRE(s != nullptr, "null stream tracer");
    MGB_REQUIRE(S >= 0 && max_steps >= 1, "stream: bad sizes (S >= 0, max_steps >= 1)");
    MGB_REQUIRE(std::isfinite(h) && h != 0.0, "stream: the step must be finite and non-zero");
    MGB_REQUIRE(std::isfinite(min_speed) && min_speed >= 0.0, "stream: min_speed must be finite and >= 0");
    // by count, in a type that cannot overflow: S (max_steps + 1) d < 2^31
    MGB_REQUIRE((long double)S * ((long double)max_steps + 1.0L) * (long double)s->obj.d < 2147483648.0L,
                "stream: S * (max_steps + 1) * d exceeds 32-bit indexing");
    MGB_REQUIRE(S == 0 || (seeds != nullptr && points != nullptr && n != nullptr && status != nullptr), "null argument");
    stream_trace(s->obj, S, seeds, h, max_steps, normalize != 0, min_speed, points, n, status, s->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_stream_destroy(mgbhip_stream* s) { return destroy_handle(s); }

int mgbhip_surface_create(mgbhip_ctx* ctx, int64_t T, const double* points, mgbhip_surface** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr, "null output pointer");
    MGB_REQUIRE(T >= 0 && T < (int64_t)INT32_MAX / 9, "surface: bad sizes");
    MGB_REQUIRE(T == 0 || points != nullptr, "null argument");
    for (int64_t i = 0; i < T * 9; ++i) MGB_REQUIRE(std::isfinite(points[i]), "surface: every vertex must be finite");
    create_handle(ctx, out, [&](Surface& Sf) { surface_build(Sf, T, points, ctx->stream); });
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_surface_trace(mgbhip_surface* s, int64_t R, const double* origin, const double* dir, double t_min,
                         double t_max, int32_t K, double* t, int32_t* tri, double* u, double* v) {
    MGB_API_BEGIN_ON(s)
    MGB_REQUIRE(s != nullptr, "null surface");
    MGB_REQUIRE(K >= 1 && K <= SURFACE_MAX_HITS, "surface: K must be 1..8");
    MGB_REQUIRE(R >= 0 && R < (int64_t)INT32_MAX / (4 * SURFACE_MAX_HITS), "surface: bad sizes");
    MGB_REQUIRE(R == 0 || (origin != nullptr && dir != nullptr && t != nullptr && tri != nullptr && u != nullptr && v != nullptr),
                "null argument");
    check_window("surface", t_min, t_max);
    check_rays("surface", R, 3, origin, dir);
    surface_trace(s->obj, R, origin, dir, t_min, t_max, K, t, tri, u, v, s->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_surface_shade(mgbhip_surface* s, int64_t R, int32_t K, const double* dir, const int32_t* tri, const double* u,
                         const double* v, const double* values, int32_t Kt, const double* table, double lo, double hi,
                         double ambient, double* layer) {
    MGB_API_BEGIN_ON(s)
    MGB_REQUIRE(s != nullptr, "null surface");
    MGB_REQUIRE(K >= 1 && K <= SURFACE_MAX_HITS, "surface: K must be 1..8");
    MGB_REQUIRE(R >= 0 && R < (int64_t)INT32_MAX / (4 * SURFACE_MAX_HITS), "surface: bad sizes");
    MGB_REQUIRE(R == 0 || (dir != nullptr && tri != nullptr && u != nullptr && v != nullptr && layer != nullptr),
                "null argument");
    MGB_REQUIRE(table != nullptr && (s->obj.n == 0 || values != nullptr), "null argument");
    check_table_clim_ambient("surface", Kt, table, lo, hi, ambient);
    for (int64_t i = 0; i < R * 3; ++i) MGB_REQUIRE(std::isfinite(dir[i]), "surface: directions must be finite");
    for (int64_t i = 0; i < R * K; ++i)
        MGB_REQUIRE(tri[i] >= -1 && (int64_t)tri[i] < s->obj.n, "surface: a triangle index is out of range");
    surface_shade(s->obj, R, K, dir, tri, u, v, values, Kt, table, lo, hi, ambient, layer, s->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_surface_destroy(mgbhip_surface* s) { return destroy_handle(s); }

int mgbhip_tubes_create(mgbhip_ctx* ctx, int64_t S, const double* points, const double* radii, mgbhip_tubes** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr, "null output pointer");
    MGB_REQUIRE(S >= 0 && S < (int64_t)INT32_MAX / 6, "tubes: bad sizes");
    MGB_REQUIRE(S == 0 || (points != nullptr && radii != nullptr), "null argument");
    for (int64_t i = 0; i < S * 6; ++i) MGB_REQUIRE(std::isfinite(points[i]), "tubes: every end point must be finite");
    for (int64_t i = 0; i < S; ++i)
        MGB_REQUIRE(std::isfinite(radii[i]) && radii[i] > 0.0, "tubes: every radius must be finite and positive");
    create_handle(ctx, out, [&](Tubes& Tb) { tubes_build(Tb, S, points, radii, ctx->stream); });
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_tubes_trace(mgbhip_tubes* s, int64_t R, const double* origin, const double* dir, double t_min, double t_max,
                       int32_t K, double* t, int32_t* segment, double* sp) {
    MGB_API_BEGIN_ON(s)
    MGB_REQUIRE(s != nullptr, "null tubes");
    MGB_REQUIRE(K >= 1 && K <= TUBES_MAX_HITS, "tubes: K must be 1..8");
    MGB_REQUIRE(R >= 0 && R < (int64_t)INT32_MAX / (4 * TUBES_MAX_HITS), "tubes: bad sizes");
    MGB_REQUIRE(R == 0 || (origin != nullptr && dir != nullptr && t != nullptr && segment != nullptr && sp != nullptr),
                "null argument");
    check_window("tubes", t_min, t_max);
    check_rays("tubes", R, 3, origin, dir);
    tubes_trace(s->obj, R, origin, dir, t_min, t_max, K, t, segment, sp, s->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_tubes_shade(mgbhip_tubes* s, int64_t R, int32_t K, const double* origin, const double* dir, const double* t,
                       const int32_t* segment, const double* sp, const double* values, int32_t Kt, const double* table,
                       double lo, double hi, double ambient, double* layer) {
    MGB_API_BEGIN_ON(s)
    MGB_REQUIRE(s != nullptr, "null tubes");
    MGB_REQUIRE(K >= 1 && K <= TUBES_MAX_HITS, "tubes: K must be 1..8");
    MGB_REQUIRE(R >= 0 && R < (int64_t)INT32_MAX / (4 * TUBES_MAX_HITS), "tubes: bad sizes");
    MGB_REQUIRE(R == 0 || (origin != nullptr && dir != nullptr && t != nullptr && segment != nullptr && sp != nullptr &&
                           layer != nullptr),
                "null argument");
    MGB_REQUIRE(table != nullptr && (s->obj.n == 0 || values != nullptr), "null argument");
    check_table_clim_ambient("tubes", Kt, table, lo, hi, ambient);
    for (int64_t i = 0; i < R * 3; ++i)
        MGB_REQUIRE(std::isfinite(origin[i]) && std::isfinite(dir[i]), "tubes: origins and directions must be finite");
    for (int64_t i = 0; i < R * K; ++i) {
        MGB_REQUIRE(segment[i] >= -1 && (int64_t)segment[i] < s->obj.n, "tubes: a segment index is out of range");
        MGB_REQUIRE(segment[i] < 0 || (std::isfinite(t[i]) && sp[i] >= 0.0 && sp[i] <= 1.0),
                    "tubes: a hit needs a finite t and s in [0, 1]");
    }
    tubes_shade(s->obj, R, K, origin, dir, t, segment, sp, values, Kt, table, lo, hi, ambient, layer, s->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_tubes_destroy(mgbhip_tubes* s) { return destroy_handle(s); }

int mgbhip_figure_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N, const double* x,
                         const double* table, int64_t R, const double* origin, const double* dir, const double* box,
                         double step, int32_t volume, int32_t nlevels, const double* levels, int32_t nslices,
                         const int32_t* axes, const double* coords, int32_t ntable, const double* vtable,
                         const double* stable, double lo, double hi, double ambient, int32_t K, mgbhip_figure** out) {
    MGB_API_BEGIN_ON(ctx)
    MGB_REQUIRE(ctx != nullptr, "null context");
    MGB_REQUIRE(out != nullptr, "null output pointer");
    MGB_REQUIRE(family == MGBHIP_INTERP_QK && d == 3, "figure: only the Q_k family with d = 3 (fem3d) has a figure");
    MGB_REQUIRE(N > 0, "figure: no elements (N = 0)");
    MGB_REQUIRE(K >= 1 && K <= SURFACE_MAX_HITS, "figure: K must be 1..8");
    MGB_REQUIRE(p >= 1 && R >= 1 && R < (int64_t)INT32_MAX / (4 * SURFACE_MAX_HITS), "figure: bad sizes");
    MGB_REQUIRE(nlevels >= 0 && nlevels <= FIGURE_MAX_LEVELS, "figure: nlevels must be 0..64");
    MGB_REQUIRE(nslices >= 0 && nslices <= FIGURE_MAX_SLICES, "figure: nslices must be 0..16");
    MGB_REQUIRE(ntable >= 2, "figure: the colour tables need at least two rows");
    MGB_REQUIRE(origin != nullptr && dir != nullptr && box != nullptr && vtable != nullptr && stable != nullptr,
                "null argument");
    MGB_REQUIRE((nlevels == 0 || levels != nullptr) && (nslices == 0 || (axes != nullptr && coords != nullptr)),
                "null argument");
    FigureIn in;
    InterpIn& geo = in.rays.geo;
    geo.family = family; geo.d = d; geo.k = k; geo.p = p; geo.N = N; geo.x = x; geo.table = table;
    interpolate_check_geometry(geo);
    MGB_REQUIRE(k <= CONTOUR_MAX_REFINE_3D, "figure: the contour lattice of a frame is refine = k, at most 8");
    MGB_REQUIRE(std::isfinite(step) && step > 0.0, "figure: step must be finite and positive");
    for (int32_t l = 0; l < nlevels; ++l) MGB_REQUIRE(std::isfinite(levels[l]), "figure: a level is not finite");
    for (int32_t i = 0; i < nslices; ++i)
        MGB_REQUIRE(axes[i] >= 0 && axes[i] <= 2 && std::isfinite(coords[i]),
                    "figure: a slice needs an axis in 0..2 and a finite coordinate");
    for (int64_t i = 0; i < (int64_t)ntable * 4; ++i) {
        MGB_REQUIRE(std::isfinite(vtable[i]) && (i % 4 != 3 || vtable[i] >= 0.0),
                    "figure: the volume table must be finite with sigma >= 0");
        MGB_REQUIRE(std::isfinite(stable[i]), "figure: the surface table must be finite");
    }
    check_clim("figure", lo, hi);
    check_ambient("figure", ambient);
    check_rays("figure", R, 3, origin, dir);
    for (int a = 0; a < 3; ++a)
        MGB_REQUIRE(std::isfinite(box[a]) && std::isfinite(box[3 + a]) && box[a] <= box[3 + a], "figure: bad clip box");
    for (int64_t i = 0; i < (int64_t)p * N * 3; ++i) MGB_REQUIRE(std::isfinite(x[i]), "figure: the mesh must be finite");
    in.rays.R = R; in.rays.origin = origin; in.rays.dir = dir; in.rays.box = box; in.rays.step = step;
    in.rays.t_min = 0.0; in.rays.t_max = std::numeric_limits<double>::infinity();
    in.volume = volume ? 1 : 0;
    in.nlevels = nlevels; in.levels = levels; in.nslices = nslices; in.axes = axes; in.coords = coords;
    in.ntable = ntable; in.vtable = vtable; in.stable = stable; in.lo = lo; in.hi = hi; in.ambient = ambient; in.K = K;
    create_handle(ctx, out, [&](Figure& F) { figure_build(F, in, ctx->stream); });
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_figure_render(mgbhip_figure* f, const double* u, double* out) {
    MGB_API_BEGIN_ON(f)
    MGB_REQUIRE(f != nullptr, "null figure");
    MGB_REQUIRE(u != nullptr && out != nullptr, "null argument");
    figure_render(f->obj, u, out, f->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_figure_render_rgba8(mgbhip_figure* f, const double* u, const double* background, uint8_t* out) {
    MGB_API_BEGIN_ON(f)
    MGB_REQUIRE(f != nullptr, "null figure");
    MGB_REQUIRE(u != nullptr && background != nullptr && out != nullptr, "null argument");
    for (int a = 0; a < 3; ++a) MGB_REQUIRE(std::isfinite(background[a]), "figure: the background must be finite");
    figure_render_rgba8(f->obj, u, background, out, f->ctx->stream);
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_figure_counts(const mgbhip_figure* f, int64_t* ntriangles, int64_t* npairs) {
    MGB_API_BEGIN_ON(f)
    MGB_REQUIRE(f != nullptr, "null figure");
    if (ntriangles) *ntriangles = f->obj.T;
    if (npairs) *npairs = f->obj.P;
    return MGBHIP_OK;
    MGB_API_END
}

int mgbhip_figure_destroy(mgbhip_figure* f) { return destroy_handle(f); }

}  // extern "C"
