/*
 * mgbhip.h -- C ABI of libmgbhip.so, the MI355X (gfx950) backend for the inner
 * Newton hot path of MultiGridBarrier.jl.
 *
 * Boundary: the reference moves a CPU `MGBProblem` through
 * `native_to_device(D, prob)`, runs the barrier Newton loops on the device types,
 * and moves the `MGBSOL` back (reference: src/mgb.jl:798-842, src/device.jl:40-60).
 * This library is what a `HIPDevice <: Device` package extension binds by `ccall`:
 * plain pointers and sizes only, an opaque handle that owns all device memory,
 * assembly plans and factorizations (the reference keeps those in two process-global
 * caches flushed by `mgb_cleanup`, src/BlockMatrices.jl:320,737-751; here they die
 * with the handle).  INTEGRATION.md shows the Julia side.
 *
 * Conventions
 *  - every entry point returns an `int` status (MGBHIP_OK = 0); numerical
 *    infeasibility is NOT an error: barrier values come back as +Inf/NaN exactly
 *    like the reference's `Log` protocol (src/utils.jl:14, src/newton.jl:35-50);
 *  - all floating point is IEEE double; index arrays are 32-bit, 0-based;
 *  - host pointers unless a parameter is named `d_*`;
 *  - a handle is not thread-safe; distinct handles are independent; all work of a
 *    handle is issued on the stream given at creation (never the NULL stream
 *    implicitly), mirroring the stream discipline the reference's CUDA backend
 *    is tested for (test/test_cuda.jl:118-130).
 */
#ifndef MGBHIP_H
#define MGBHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGBHIP_OK 0
#define MGBHIP_ERR_INVALID 1      /* bad argument / unsupported functor family or size */
#define MGBHIP_ERR_HIP 2          /* a HIP runtime call failed (see mgbhip_last_error) */
#define MGBHIP_ERR_NOT_SPD 3      /* Cholesky met a non-positive pivot (reference: the
                                     Symmetric `\` would fall back / throw, src/utils.jl:145) */
#define MGBHIP_ERR_NONFINITE 4    /* a Newton precondition failed (src/newton.jl:238-254) */
#define MGBHIP_ERR_CONVERGENCE 5  /* MGBConvergenceFailure (src/utils.jl:178-184); code in diagnostics */

#define MGBHIP_MAX_PIECES 4
#define MGBHIP_MAX_IDX 10  /* Euclidean-power piece width nz (3-D p_harmonic / norton_hoff: d^2 + 1)      */
#define MGBHIP_MAX_LIN 4   /* linear pieces: at most 4 constraint rows (nc) on at most 4 indexed rows (ni)  */
#define MGBHIP_MAX_ND 13   /* 3-D vector problems: d (1 + d) + 1 rows                                      */
#define MGBHIP_MAX_NU 4
#define MGBHIP_MAX_OPS 8

#define MGBHIP_KIND_EP 1          /* convex_Euclidian_power (src/convex_euclidian_power.jl:352-453) */
#define MGBHIP_KIND_LINEAR 2      /* convex_linear          (src/convex_linear.jl:78-223)           */

typedef struct mgbhip_ctx mgbhip_ctx;          /* device + stream + workspace            */
typedef struct mgbhip_problem mgbhip_problem;  /* one AMG (src/multigrid.jl:278-288) + one Convex */

/* One piece of a Convex (src/convex.jl:80-86).  Grids are n x K, column-major, as the
 * reference's `Q.args`; NULL selects the documented default without reading memory. */
typedef struct {
    int32_t kind;                 /* MGBHIP_KIND_*                                        */
    int32_t ni;                   /* length of idx (EP: nz)                               */
    int32_t nc;                   /* LINEAR: constraint rows; EP: ignored (= ni)          */
    int32_t idx[MGBHIP_MAX_IDX];  /* 0-based positions into y                             */
    const double* A;              /* n x (nc*ni), per-node matrix column-major; NULL = I  */
    const double* b;              /* n x nc; NULL = 0                                     */
    const double* p;              /* EP: n; NULL = use p_const / mu_const                 */
    const double* mu;             /* EP: n (src/convex_euclidian_power.jl:380-381)        */
    double p_const, mu_const;
    const double* select;         /* n: non-zero = piece active at the node; NULL = all   */
} mgbhip_piece;

typedef struct {
    int32_t npieces;
    mgbhip_piece pieces[MGBHIP_MAX_PIECES];
    /* phase-I wrapper `_feasibility_convex` (src/mgb.jl:217-287): when `feasibility`
     * is non-zero the node barrier is cobarrier(y[0:NC]) plus the box terms, with
     * NC = nD_main + 1; b and R are set per box round by mgbhip_problem_set_box.   */
    int32_t feasibility;
    int32_t NC;
} mgbhip_cone;

/* CSR image of one prolongation R_fine[l] (src/multigrid.jl:491): (nu*n) x m. */
typedef struct {
    int64_t rows, cols;
    const int32_t* rowptr;        /* rows + 1 */
    const int32_t* colidx;
    const double* values;
} mgbhip_csr;

typedef struct {
    int32_t p;                    /* nodes per element (block size)                       */
    int64_t N;                    /* elements; n = p*N broken nodes                       */
    int32_t nu;                   /* state components                                     */
    int32_t nD;                   /* rows of D                                            */
    int32_t n_ops;                /* distinct operator arrays                             */
    const double* ops[MGBHIP_MAX_OPS]; /* each p x p x N, Julia Array{T,3} layout; NULL = identity
                                     (BlockDiag, src/BlockMatrices.jl:17-22)              */
    int32_t D_state[MGBHIP_MAX_ND];    /* state component of D row k (BlockColumn.active_col) */
    int32_t D_op[MGBHIP_MAX_ND];       /* operator index of D row k                        */
    const double* w;              /* n quadrature weights                                 */
    int32_t L;                    /* hierarchy depth                                      */
    const mgbhip_csr* R;          /* L prolongations, coarsest first                      */
    mgbhip_cone cone;
    const double* barrier_weights;/* n, or NULL for the flat (1/n) average (src/convex.jl:279-304) */
    /* Node coordinates `AMG.x` (src/multigrid.jl:280), n x dim column-major, or NULL.  Used only as an
     * ordering hint by the sparse direct solve (geometric nested dissection on the centroids of the
     * level-J basis functions); NULL falls back to a graph-only dissection.  Results do not depend
     * on it beyond rounding. */
    const double* x;
    int32_t dim;
} mgbhip_problem_desc;

/* Solver controls (reference defaults: src/mgb.jl:95-101, :360-363, src/newton.jl:139). */
typedef struct {
    double tol;                   /* sqrt(eps)            */
    double t;                     /* 0.1                  */
    double kappa;                 /* 10                   */
    int32_t maxit;                /* 10000                */
    int32_t max_newton;           /* ceil(log2(-log2 eps)) + 2 = 8 */
    double ls_beta, ls_c1;        /* backtracking 0.5, 0.1 */
    int32_t line_search;          /* 0 backtracking, 1 illinois */
    double stop_lambda_tol;       /* stopping_inexact(0.25/sqrt(n), 0.9); <0 => stopping_exact(stop_theta) */
    double stop_theta;
    int32_t finalize;             /* 1: stopping_exact(finalize_theta); 0: NoFinalize */
    double finalize_theta;        /* 0.9 */
    int32_t early_stop;           /* 0 none; 1 phase-I margin rule (src/mgb.jl:486-491)   */
    /* Optional user callables, NULL = the built-in rule selected above.  They receive only what the
     * reference hands to the corresponding Julia callable:
     *   stopping_criterion(ymin, ynext, gmin, |gnext|, sqrt(incmin), sqrt(inc)): the reference's
     *   `stop(ymin, ynext, gmin, gnext, n, ndecmin, ndec)` (src/newton.jl:187,222-225,279; kwarg of mgb_solve,
     *   src/mgb.jl:360) with the vectors gnext, n reduced to the norm both built-in rules use -> non-zero = converged;
     *   early_stop(z, t): z is the current fine iterate copied to the host (nu*n doubles), called
     *   between completed t-steps like `early_stop(z)` (src/mgb.jl:85-89,138) -> non-zero = stop.  */
    int (*stopping_criterion)(double ymin, double ynext, double gmin, double gnorm_next, double ndecmin, double ndec,
                              void* user);
    int (*early_stop_fn)(const double* z, double t, void* user);
    void* user;
} mgbhip_options;

/* Diagnostics of one mgb_core run (the fields of SOL_main, src/mgb.jl:176-182). */
typedef struct {
    int32_t k;                    /* t-steps taken                                         */
    int32_t L;
    int32_t failure_code;         /* 0 ok, 1 :stall, 2 :iteration_limit                    */
    double t_final, t_elapsed;
    double solve_seconds;         /* wall time inside factor+solve (reported separately)   */
    int64_t newton_iterations;    /* sum(its)                                              */
    int64_t f0_evals, f1_evals, f2_evals, factorizations;
    /* caller-provided, capacity in cap_steps: its is L x cap_steps column-major */
    int32_t cap_steps;
    int64_t* its;
    double* ts;
    double* kappas;
    double* times;
    double* c_dot_Dz;
} mgbhip_core_result;

/* ---- lifecycle --------------------------------------------------------------------- */
int mgbhip_create(mgbhip_ctx** ctx, int device_id, void* hip_stream /* NULL: private stream */);
int mgbhip_destroy(mgbhip_ctx* ctx);
const char* mgbhip_last_error(void);
const char* mgbhip_version(void);

/* native_to_device for one (AMG, Convex) pair (ext/MultiGridBarrierCUDAExt/conversion.jl:152-159).
 * `share` may name an existing problem of the same ctx whose operator arrays and weights
 * are identical (the (main, feasibility) pair shares them; test/test_cuda.jl:80-99). */
int mgbhip_problem_create(mgbhip_ctx* ctx, const mgbhip_problem_desc* desc,
                          mgbhip_problem* share, mgbhip_problem** out);
int mgbhip_problem_destroy(mgbhip_problem* prob);      /* also flushes plans + factorizations */
int mgbhip_problem_set_box(mgbhip_problem* prob, double b, double R);
int mgbhip_problem_set_barrier_weights(mgbhip_problem* prob, const double* bw /* n or NULL */);
int64_t mgbhip_level_size(const mgbhip_problem* prob, int32_t level);   /* m_J = ncols R_fine[J] */

/* ---- the Barrier closures (src/convex.jl:155-202) at level J (0-based), host vectors ----
 * s: m_J, c: n x nD column-major (= t * f_grid), z0: nu*n.                              */
int mgbhip_f0(mgbhip_problem* prob, int32_t level, const double* s, const double* c,
              const double* z0, double* value);
int mgbhip_f1(mgbhip_problem* prob, int32_t level, const double* s, const double* c,
              const double* z0, double* grad /* m_J */);
/* f2 assembles H = R' H_blk R on the device and optionally copies it out as CSR
 * (pattern fixed per level: query with mgbhip_hessian_pattern).                          */
int mgbhip_f2(mgbhip_problem* prob, int32_t level, const double* s, const double* c,
              const double* z0, double* values /* nnz or NULL */);
int mgbhip_hessian_pattern(mgbhip_problem* prob, int32_t level, int64_t* nnz,
                           const int32_t** rowptr, const int32_t** colidx);
/* n = solve(symmetric(H), g) with the H of the last mgbhip_f2 at this level
 * (src/newton.jl:253, src/utils.jl:142-145): sparse Cholesky on the device.              */
int mgbhip_solve(mgbhip_problem* prob, int32_t level, const double* g, double* x);
/* The reference's `solve(A, b)` hook (src/utils.jl:142-145; cuDSS twin cudss_solver.jl:396-408) takes any
 * matrix with the level's sparsity pattern: replace the values of H (CSR order of mgbhip_hessian_pattern);
 * the next mgbhip_solve / mgbhip_solve_newton factors them.                                                */
int mgbhip_set_hessian(mgbhip_problem* prob, int32_t level, const double* values /* nnz */);
/* The solve exactly as the resident Newton loop performs it (src/newton.jl:253-255): the bordered matrix
 * [H -g; -g' -1] is factored, so the forward substitution rides along the factorization, and one backward
 * sweep returns x = H^{-1} g; lambda2 (optional) = <g, x>.                                                  */
int mgbhip_solve_newton(mgbhip_problem* prob, int32_t level, const double* g, double* x, double* lambda2);
/* ---- one process per GPU: domain decomposition of the resident loop ----
 * The problem handed to mgbhip_problem_create is then this rank's SLICE: its elements, and per level the columns of
 * R restricted to the unknowns its elements touch plus the interface unknowns (those whose support meets more than
 * one rank), both in an order common to all ranks.  Per level: the interface columns (local indices, ascending) and
 * an ownership mask (1 where this rank counts an unknown in dot products and norms, 0 elsewhere; interface unknowns
 * are owned by exactly one rank).  The library then keeps s distributed with a replicated interface: f0 and the
 * scalars of the Newton loop are summed over ranks, f1 sums its interface entries, every rank eliminates its
 * interior unknowns and the assembled interface front of the factorization is summed over ranks before each rank
 * factors it.  `allreduce` sums (op 0) or maximises (op 1) `count` doubles in place over all ranks and returns 0;
 * the buffer is host memory unless accepts_device_ptr was set, in which case large buffers are passed as device
 * pointers that are ready on the handle's stream when the call is made (the callee must complete before it returns).
 * Must be set before the first evaluation; mgbhip_mgb_core then runs the same control flow on every rank.       */
typedef int (*mgbhip_allreduce_fn)(void* user, double* buf, int64_t count, int32_t op, int32_t on_device);
int mgbhip_problem_set_sharding(mgbhip_problem* prob, int32_t level, int64_t n_iface,
                                const int32_t* iface_cols, const double* own_mask /* m_J */);
int mgbhip_problem_set_collective(mgbhip_problem* prob, mgbhip_allreduce_fn allreduce, void* user,
                                  int32_t accepts_device_ptr);
/* One Newton direction exactly as the resident loop forms it at (s, c, z0): g = f1, H = f2 left in the
 * element-block slab (fine levels: leaf fronts condensed inside the element kernel from the second call on),
 * bordered factorization, backward sweep.  x = H^{-1} g, lambda2 = <g, x>; *condensed (optional) reports
 * whether the element kernel wrote the leaf fronts.  Test / measurement hook.                               */
int mgbhip_newton_direction(mgbhip_problem* prob, int32_t level, const double* s, const double* c,
                            const double* z0, double* x, double* lambda2, int32_t* condensed);
/* Per-node barrier value map_rows_gpu(F0, args..., Dz(z)) (src/mgb.jl:410-420) and the
 * slack initialiser (src/mgb.jl:437-440); y is n x nD column-major.                      */
int mgbhip_node_barrier(mgbhip_problem* prob, const double* z, double* F /* n */, double* Dz /* n*nD or NULL */);
int mgbhip_node_slack(mgbhip_problem* prob, const double* z, double* slack /* n */);

/* ---- the loops (src/newton.jl:227-287, src/mgb.jl:16-183), resident on the device ---- */
int mgbhip_mgb_core(mgbhip_problem* prob, double* z /* nu*n in/out */, const double* c /* n x nD */,
                    const mgbhip_options* opt, mgbhip_core_result* res);
/* _matched_t (src/mgb.jl:307-330) */
int mgbhip_matched_t(mgbhip_problem* prob, const double* z, const double* c, double t_default,
                     double* t_out);
void mgbhip_default_options(mgbhip_options* opt, int64_t n_nodes);

/* ---- device-resident vectors and closures ------------------------------------------------------
 * The "fine" integration style of SURVEY.md section 8b: a binding that keeps the reference's generic
 * `newton` / `mgb_step` (src/newton.jl:227-287, src/mgb.jl:16-82) wraps `mgbhip_vec` in its device
 * vector type; nothing crosses PCIe per call except scalars.  A vector belongs to one context and is
 * used on that context's stream.  (The CUDA extension gets these from CuArray broadcasting:
 * ext/MultiGridBarrierCUDAExt/mgb_interface.jl:14-41.)                                           */
typedef struct mgbhip_vec mgbhip_vec;
int mgbhip_vec_alloc(mgbhip_ctx* ctx, int64_t len, mgbhip_vec** out);      /* mgb_zeros: zero-filled  */
int mgbhip_vec_free(mgbhip_vec* v);
int64_t mgbhip_vec_len(const mgbhip_vec* v);
int mgbhip_vec_upload(mgbhip_vec* v, const double* host, int64_t len);
int mgbhip_vec_download(const mgbhip_vec* v, double* host, int64_t len);
int mgbhip_vec_fill(mgbhip_vec* v, double value);
int mgbhip_vec_copy(mgbhip_vec* dst, const mgbhip_vec* src);
int mgbhip_vec_axpy(double alpha, const mgbhip_vec* x, mgbhip_vec* y);      /* y += alpha x            */
int mgbhip_vec_scale(double alpha, mgbhip_vec* x);                          /* x *= alpha              */
int mgbhip_vec_dot(const mgbhip_vec* a, const mgbhip_vec* b, double* out);
int mgbhip_vec_norm(const mgbhip_vec* a, double* out);                      /* 2-norm                  */
int mgbhip_vec_isfinite(const mgbhip_vec* a, int32_t* all_finite);          /* mgb_all_isfinite        */
/* The Barrier closures and the direct solve on device vectors (s: m_J, c: n*nD column-major,
 * z0: nu*n, grad/x: m_J); f2_d leaves H assembled on the device for solve_d.                     */
int mgbhip_f0_d(mgbhip_problem* prob, int32_t level, const mgbhip_vec* s, const mgbhip_vec* c,
                const mgbhip_vec* z0, double* value);
int mgbhip_f1_d(mgbhip_problem* prob, int32_t level, const mgbhip_vec* s, const mgbhip_vec* c,
                const mgbhip_vec* z0, mgbhip_vec* grad);
int mgbhip_f2_d(mgbhip_problem* prob, int32_t level, const mgbhip_vec* s, const mgbhip_vec* c,
                const mgbhip_vec* z0);
int mgbhip_solve_d(mgbhip_problem* prob, int32_t level, const mgbhip_vec* g, mgbhip_vec* x);
/* z += R_J s  (src/mgb.jl:60) */
int mgbhip_prolong_add(mgbhip_problem* prob, int32_t level, const mgbhip_vec* s, mgbhip_vec* z);

/* ---- measurement hooks (bench.py): device-time of the named stage of the last call,
 * from hipEvents on the handle's stream.                                               */
int mgbhip_stage_ms(mgbhip_problem* prob, const char* stage, double* total_ms, int64_t* launches);
int mgbhip_reset_stage_timers(mgbhip_problem* prob, int enable);
/* Factorization statistics of a level (after its first solve): out[0] fronts, [1] largest
 * front, [2] arena doubles, [3] factor flops, [4] peeled unknowns, [5] tree levels,
 * [6] nnz(H), [7] unknowns.                                                             */
int mgbhip_solver_stats(mgbhip_problem* prob, int32_t level, double* out8);
/* Shape of one factorization + backward sweep of a level as the device runs it (bench.py: roofline_solver): out[0]
 * sequential 32-column pivot blocks on the critical path of the large fronts, [1] tree levels on the large-front
 * path, [2] kernel launches per factorization, [3] per backward sweep, [4] arena doubles, [5] factor flops,
 * [6] doubles the trailing updates move beyond one pass over the arena, [7] reserved.  The reference's counterpart is
 * opaque (cuDSS FACTORIZATION + SOLVE per Newton iteration, ext/MultiGridBarrierCUDAExt/cudss_solver.jl:279-288). */
int mgbhip_solver_chain(mgbhip_problem* prob, int32_t level, double* out8);
/* Which kernels the shape gates of a level selected (inspection only; nothing is computed or built).  out[0] R_unit
 * (prolongation fused into the element kernel), [1] R_long (a row of R longer than 64: wave per row), [2] T_long (a column
 * of R longer than 64: wave per row of R'), [3] T_chunks (> 0: chunked restriction, chunks per row of R'), [4] bit 0: selection
 * level, bit 1: direct values, [5] acc (LDS accumulation), [6] acc_split, [7] long_lists (wave per contribution list),
 * [8] gather_chunk, [9] gather_nchunk (> 1: two-stage gather), [10] projection kernel of the last f2 (MGBHIP_PROJ_*),
 * [11] longest row of R, [12] longest column of R, [13] cmax (widest per-state column set of an element), [14] mean
 * contribution-list length (integer quotient), [15] 1 once the assembly plan exists (the first f2 of the level builds it;
 * [4]..[10], [13] and [14] describe it and are zero / defaults before).                                                   */
enum { MGBHIP_PROJ_NONE = 0, MGBHIP_PROJ_LOOP = 1, MGBHIP_PROJ_STAGED = 2, MGBHIP_PROJ_MFMA = 3, MGBHIP_PROJ_ACCUMULATE = 4 };
int mgbhip_level_plan(mgbhip_problem* prob, int32_t level, int32_t* out16);
/* Which element kernel a launch of `mode` (MGBHIP_ELEM_F0 .. MGBHIP_ELEM_F01) runs on this problem (inspection only; nothing is
 * launched).  The decision is the launchers' own (csrc/elem_layout.hpp, elem_decide).  out[0] kernel kind (MGBHIP_ELEM_KIND_*) of
 * the plain launch, [1] NY and [2] P of the instantiation (fast kernels: the compile-time pair; generic: NY = nD, P = 0; wide and
 * dense: 0, 0), [3] threads per workgroup, [4] lanes per element G, [5] elements per workgroup, [6] workgroups, [7] dynamic LDS
 * bytes ([3]..[7] are 0 on the dense path, which sizes its own launches), [8] operators staged through LDS, [9] D rows whose
 * operator is read from HBM, [10] ymask (bit k: row k of D z enters a barrier term), [11] kind of the Hessian launch of the
 * Newton loop on the finest level: MGBHIP_ELEM_KIND_CONDENSE once that level has condensed leaves and mode is MGBHIP_ELEM_F2,
 * otherwise [0]; [12]..[15] reserved (0).                                                                              */
enum { MGBHIP_ELEM_F0 = 0, MGBHIP_ELEM_F1 = 1, MGBHIP_ELEM_F2 = 2, MGBHIP_ELEM_NODE_F = 3, MGBHIP_ELEM_NODE_SLACK = 4, MGBHIP_ELEM_F01 = 5 };
enum { MGBHIP_ELEM_KIND_DENSE = 0, MGBHIP_ELEM_KIND_WIDE = 1, MGBHIP_ELEM_KIND_FAST_DEFAULT = 2, MGBHIP_ELEM_KIND_FAST_RUNTIME = 3,
       MGBHIP_ELEM_KIND_CONDENSE = 4, MGBHIP_ELEM_KIND_GENERIC = 5 };
int mgbhip_elem_plan(mgbhip_problem* prob, int32_t mode, int32_t* out16);
/* Test and diagnostic entry point: ONE line-search trial of the Newton loop at level `level`, run by the loop's own code.
 * x and dir (m_level each) are the iterate and the direction, the trial point is x - step * dir; c (n x nD, column-major) and
 * z0 (nu * n) as in mgbhip_f0.  y: the objective at the trial point, g (m_level): its gradient, xn (m_level): the trial point as
 * the device formed it, moved: 0 when no entry of x changed, finite: 0 when the loop would reject the trial (non-finite value or
 * gradient; y, g are then whatever the kernels left), path: bit 0 the element kernel formed the trial point on the fly, bit 1 the
 * restriction, the |g|^2 partial sums and the step ran in one launch.  Valid without any earlier solve.  Not for sharded problems. */
int mgbhip_trial_values(mgbhip_problem* prob, int32_t level, const double* x, const double* dir, double step, const double* c,
                        const double* z0, double* y, double* g, double* xn, int32_t* moved, int32_t* finite, int32_t* path);
/* The factorization launches of a level's sparse LDL', leaves first (inspection only, valid after the level's first solve;
 * nothing is computed or changed).  Returns the number of launches, or -status on an error, and writes at most `cap` rows of
 * MGBHIP_LAUNCH_ROW int32 to out (out may be NULL with cap = 0):  [0] tree level, [1] first front, [2] fronts, [3] LDS class
 * (0: large-front path), [4] largest front m, [5] largest pivot block k, [6] most children of a front, [7] tiny (16 lanes per
 * leaf front), [8] wave (one wave per front), [9] inverse-based large-front kernels, [10] interface front, [11] fronts stored
 * as packed triangles, [12] assembly kernel of a large-front launch (MGBHIP_ASM_*), [13] where block 0 of the pivot chain is
 * factored (MGBHIP_B0_*), [14] backward sweep of an LDS launch (MGBHIP_BWD_*), [15] reserved.                                */
enum { MGBHIP_LAUNCH_ROW = 16 };
enum { MGBHIP_ASM_NONE = 0, MGBHIP_ASM_GATHER = 1, MGBHIP_ASM_COLUMNS = 2 };
enum { MGBHIP_B0_NA = 0, MGBHIP_B0_GATHER = 1, MGBHIP_B0_DIAG0 = 2, MGBHIP_B0_STEP0 = 3 };
enum { MGBHIP_BWD_NA = 0, MGBHIP_BWD_K8 = 1, MGBHIP_BWD_K16 = 2, MGBHIP_BWD_GENERAL = 3 };
int64_t mgbhip_solver_launches(mgbhip_problem* prob, int32_t level, int32_t* out, int64_t cap);

/* ---- point evaluation (reference: `interpolate`, src/utils.jl:16-58) ---------------------------------------------
 * out[q, c] = the element-space function with broken-basis values z[:, c] at point q, for M points pts (M x d,
 * row-major); out is M x ncomp row-major, z is (p*N) x ncomp row-major (row e*p + i: local node i of element e).
 *  - FEM1D       d = 1, k = degree, p = k + 1; x = the p*N node coordinates, table = the k + 1 reference nodes.
 *                The reference's algorithm (src/TensorFEM.jl:967-1014): clamped outside [x[0], x[p*N-1]].
 *  - QK          d = 2 or 3, p = (k + 1)^d, x (p*N) x d, table = the k + 1 reference nodes; Newton from xi = 0.
 *  - P1 / P2     d = 2, p = 3 / 6 / 7, x (p*N) x 2, table = p x 10 coefficients of the basis over the monomials
 *                1, l1, l2, l1^2, l1 l2, l2^2, l1^3, l1^2 l2, l1 l2^2, l2^3 (l1 = 1 at corner slot 0, l2 = 1 at the
 *                next corner slot, the third corner is the origin).  P2 needs straight elements (every edge node at
 *                its edge's midpoint, the bubble node at the centroid).
 *  - P2C         P2 with curved elements: the element map sum_j phi_j(l1, l2) x_j over all p nodes is inverted by
 *                Newton from the affine pair of the three corners, with Q_k's stopping and containment rule.
 *  - SPECTRAL1D  d = 1, k = n - 1, p = n, N = 1, z = Chebyshev coefficients (n x ncomp), x and table unused.
 *  - SPECTRAL2D  d = 2, k = n - 1, p = n*n, N = 1, z row i*n + j = C[i, j] (value = bx' C by), x and table unused.
 * 2-D / 3-D FEM: a point outside every element (or with a non-finite coordinate) gives NaN and elem -1; a point in
 * several elements takes the lowest element index.  elem (M, may be NULL) receives the element used.  M = 0 is a
 * no-op; N = 0 is MGBHIP_ERR_INVALID.  Host pointers; the work runs on ctx's stream and is complete on return.   */
#define MGBHIP_INTERP_FEM1D 1
#define MGBHIP_INTERP_QK 2
#define MGBHIP_INTERP_P1 3
#define MGBHIP_INTERP_P2 4
#define MGBHIP_INTERP_SPECTRAL1D 5
#define MGBHIP_INTERP_SPECTRAL2D 6
#define MGBHIP_INTERP_P2C 7 /* P2 with curved (isoparametric) elements; arguments, table and layouts are those of P2 */
int mgbhip_interpolate(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N,
                       const double* x, const double* table, int32_t ncomp, const double* z, int64_t M,
                       const double* pts, double* out, int32_t* elem);
/* The same evaluation with the gradient with respect to x: grad[q, c, a] = d/dx_a of component c at point q (M x ncomp
 * x d, row-major; d = 1: M x ncomp).  Arguments, layouts and checks are those of mgbhip_interpolate; out (M x ncomp)
 * may be NULL, and where given it is bitwise what mgbhip_interpolate returns; grad == NULL is MGBHIP_ERR_INVALID.
 *  - QK          grad = J^{-T} sum_i grad_xi phi_i(xi) z_i at the located xi, J the Jacobian of the element map there
 *                (curved elements included).
 *  - P1 / P2     the monomial table differentiated in (l1, l2), mapped by the inverse transpose of the two edge vectors.
 *  - P2C         grad = J^{-T} (du/dl1, du/dl2) with J[a][b] = sum_j dphi_j/dl_b x_j[a] at the located (l1, l2).
 *  - FEM1D       the derivative of the element's Lagrange interpolant over dx/dxi.  Values are clamped outside
 *                [x[0], x[p*N-1]], so the derivative there is 0.0 (also at +-Inf); at the two end points it is the
 *                one-sided derivative of the end element; NaN gives NaN.
 *  - SPECTRAL*   the derivative of the Chebyshev sums by the recurrence for T_n' (finite at +-1); 2-D: both partials.
 * A point that gets NaN for its value gets NaN in every gradient entry.  The gradient is discontinuous across element
 * faces: a point on a shared face reports the gradient of the lowest-index element, the one its value comes from. */
int mgbhip_interpolate_grad(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N,
                            const double* x, const double* table, int32_t ncomp, const double* z, int64_t M,
                            const double* pts, double* out /* M x ncomp, may be NULL */,
                            double* grad /* M x ncomp x d */, int32_t* elem /* M or NULL */);

/* ---- point locator: locate the points once, evaluate many z at them ---------------------------------------------
 * mgbhip_locator_create does the part of mgbhip_interpolate that does not depend on z (grid of element boxes, points
 * sorted by cell, element map inverted per point) and keeps per point the element and the reference coordinates on the
 * device; mgbhip_locator_evaluate uploads one z, runs the evaluation half of the query and copies the result back.
 * What it returns is bitwise what mgbhip_interpolate / mgbhip_interpolate_grad return for the same arguments (values,
 * gradients, elements, NaN positions).  Argument meaning, layouts, checks and error codes are those of
 * mgbhip_interpolate; x, table and pts are copied (the caller's arrays may change or go away afterwards).  A locator
 * belongs to the context it was created from and must be destroyed before it.  M = 0 is allowed: every call is then a
 * no-op.  ncomp may differ from call to call.                                                                      */
typedef struct mgbhip_locator mgbhip_locator;
int mgbhip_locator_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N,
                          const double* x, const double* table, int64_t M, const double* pts,
                          mgbhip_locator** out);
/* elem[q] = the element point q was located in (-1: none; the spectral families report 0 for a finite point) */
int mgbhip_locator_elements(const mgbhip_locator* loc, int32_t* elem /* M */);
int mgbhip_locator_evaluate(mgbhip_locator* loc, int32_t ncomp, const double* z /* (p*N) x ncomp */,
                            double* out /* M x ncomp, may be NULL when grad is given */,
                            double* grad /* M x ncomp x d, or NULL: values only */);
int mgbhip_locator_destroy(mgbhip_locator* loc); /* NULL is a no-op */

/* ---- closest point: evaluate element-space functions on embedded curves and surfaces ----------------------------
 * N Q_k elements of dimension d in e > d coordinates [(d, e) = (1, 2), (1, 3) or (2, 3); 1 <= k <= 8; x: (p N) x e with
 * p = (k + 1)^d nodes per element, axis 0 fastest; nodes: the k + 1 reference nodes in [-1, 1]].  create projects the M
 * points [pts: M x e] once: per point, among the elements that come within max_distance [finite, >= 0] of it, the point
 * of least distance [the foot], found per candidate element by a projected Newton iteration on |x(xi) - pt|^2 over
 * [-1, 1]^d from the element's node nearest to the point [at most 64 iterations; a candidate that does not converge
 * competes with the distance at its last iterate].  Candidates are visited in ascending element index and a later one
 * wins only on a strictly smaller distance.  A point with no foot within max_distance, outside the padded box of the
 * mesh or with a non-finite coordinate has element -1.  x, nodes and pts are copied.  M = 0 is allowed: every call is
 * then a no-op.  A handle belongs to the context it was created from and must be destroyed before it.
 *  - fetch [any output may be NULL], by point: elem [M], xi [M x d, the reference coordinates of the foot], foot [M x e],
 *    dist [M], flag [M: 1 where the winning candidate's iteration met its stopping test]; NaN where elem is -1.
 *  - evaluate: out[q][c] = sum_i phi_i(xi_q) z[i][c] over the nodes of point q's element; grad [M x ncomp x e, or NULL:
 *    values only] the tangential gradient J (J^T J)^-1 grad_xi u with J = dx/dxi at the foot [a curve: (du/dxi) x' /
 *    |x'|^2].  The values are bitwise the same with and without grad; a point without an element has NaN everywhere.
 *    ncomp may differ from call to call.                                                                            */
typedef struct mgbhip_closest mgbhip_closest;
int mgbhip_closest_create(mgbhip_ctx* ctx, int32_t d, int32_t e, int32_t k, int64_t N, const double* x,
                          const double* nodes, int64_t M, const double* pts, double max_distance,
                          mgbhip_closest** out);
int mgbhip_closest_fetch(const mgbhip_closest* cp, int32_t* elem /* M */, double* xi /* M x d */,
                         double* foot /* M x e */, double* dist /* M */, int32_t* flag /* M */);
int mgbhip_closest_evaluate(mgbhip_closest* cp, int32_t ncomp, const double* z /* (p*N) x ncomp */,
                            double* out /* M x ncomp, may be NULL when grad is given */,
                            double* grad /* M x ncomp x e, or NULL: values only */);
int mgbhip_closest_destroy(mgbhip_closest* cp); /* NULL is a no-op */

/* ---- quadrature: integrals and norms of element-space functions over the mesh ------------------------------------
 * N elements of p nodes and dimension d in e >= d coordinates [(d, e) = (1, 1..3), (2, 2..3) or (3, 3); x: (p N) x e,
 * element-major] and a rule of Q points per element, given by its reference weights wref [Q] and by the element basis
 * at its points: phi [Q x p], dphi [Q x p x d, the derivatives in reference coordinates].  Nothing else tells the
 * library the element family.  At point q of an element with nodes x_i and values z_i
 *     x_q = sum_i phi[q][i] x_i,   J = sum_i x_i dphi[q][i]^T [e x d],   measure_q = wref[q] sqrt(det J^T J),
 *     u_q = sum_i phi[q][i] z_i,   grad u = J (J^T J)^-1 sum_i dphi[q][i] z_i   [tangential when e > d].
 * x, wref, phi and dphi are copied.  A handle belongs to the context it was created from and must be destroyed before it.
 *  - points [N x Q x e] and weights [N x Q, the measures: they sum to the measure of the mesh].
 *  - integrate: z [(p N) x ncol]; per column the sum over all points of measure_q F_q with F = u [VALUE], |u - g|^pexp
 *    [LP], |grad u - G|^pexp [W1P, Euclidean norm in R^e] or |grad u|^pexp / pexp - f u [ENERGY; source: f as p N nodal
 *    values].  minus: g [N x Q x ncol] or G [N x Q x ncol x e] at the points, or NULL for zero; pexp finite and > 0
 *    [ignored by VALUE].  totals [ncol]; per_element [N x ncol] or NULL.  An element's value is the sum of its Q terms
 *    in an order fixed by Q alone, the totals are compensated sums over the elements in a fixed order: results are
 *    reproducible bit for bit, do not depend on per_element, and a column's do not depend on the other columns.
 *  - max: per column the largest |u_q - g_q| [LP] or |grad u - G| [W1P] over all points, into maxima [ncol].
 *  - plan [no handle, no device]: out16 = { threads, lanes per element S = min(Q, threads), elements per workgroup G,
 *    columns per pass, 1 if phi / dphi are staged in LDS [0: read through L2], threads of the reduction over the
 *    elements, element groups, workgroups, dynamic LDS bytes, bytes of the tables, 0... } for that shape.
 *  - times: device milliseconds of the last integrate or max call, taken with events on the context's stream:
 *    ms2 = { the element kernel, the reduction over the elements }; invalid before the first call.                  */
enum { MGBHIP_QUAD_VALUE = 0, MGBHIP_QUAD_LP = 1, MGBHIP_QUAD_W1P = 2, MGBHIP_QUAD_ENERGY = 3 };
typedef struct mgbhip_quadrature mgbhip_quadrature;
int mgbhip_quadrature_create(mgbhip_ctx* ctx, int32_t d, int32_t e, int32_t p, int64_t N, const double* x, int32_t Q,
                             const double* wref, const double* phi, const double* dphi, mgbhip_quadrature** out);
int mgbhip_quadrature_points(mgbhip_quadrature* quad, double* points /* N x Q x e */);
int mgbhip_quadrature_weights(mgbhip_quadrature* quad, double* weights /* N x Q */);
int mgbhip_quadrature_integrate(mgbhip_quadrature* quad, int32_t kind, double pexp, int32_t ncol,
                                const double* z /* (p*N) x ncol */, const double* minus /* or NULL */,
                                const double* source /* p*N: ENERGY; else NULL */,
                                double* per_element /* N x ncol, or NULL */, double* totals /* ncol */);
int mgbhip_quadrature_max(mgbhip_quadrature* quad, int32_t kind, int32_t ncol, const double* z /* (p*N) x ncol */,
                          const double* minus /* or NULL */, double* maxima /* ncol */);
int mgbhip_quadrature_plan(int32_t d, int32_t e, int32_t p, int32_t Q, int64_t N, int32_t* out16);
int mgbhip_quadrature_times(const mgbhip_quadrature* quad, double* ms2);
int mgbhip_quadrature_destroy(mgbhip_quadrature* quad); /* NULL is a no-op */

/* ---- residual: the element-interior residual of the p-Laplace equation ---------------------------------------------
 * The half of the residual a-posteriori estimator that the face jumps below leave out: with the sign convention of the
 * ENERGY kind above [-div a(grad u) = f, a(g) = |g|^(pexp-2) g] the strong residual r = f + div a(grad u) at the points
 * of a rule and, per element, h_K^2 times the integral of r^2.  N elements of p nodes in d = e = 2 or 3 coordinates
 * [x: (p N) x d, element-major] and a rule of Q points per element with positive weights wref [Q], given with the
 * element basis at its points: phi [Q x p], dphi [Q x p x d] and d2phi [Q x p x d(d+1)/2, the second derivatives in
 * reference coordinates in the order (0,0), (0,1), (1,1) for d = 2 and (0,0), (0,1), (0,2), (1,1), (1,2), (2,2) for
 * d = 3].  Nothing else tells the library the element family.  At point q of an element with nodes x_i and values z_i
 *     J = sum_i x_i dphi[q][i]^T,   measure_q = wref[q] det J,   g = grad u = J^-T sum_i dphi[q][i] z_i,
 *     H_xi(v) = sum_i v_i d2phi[q][i],   H = J^-T [H_xi(z) - sum_a g_a H_xi(x_a)] J^-1   [the Hessian of u in x; exact on
 *     curved elements],   div a = |g|^(pexp-2) [tr H + (pexp - 2) g^T H g / |g|^2];   pexp = 2: tr H;   g = 0: 0.
 * Everything is copied.  A handle belongs to the context it was created from and must be destroyed before it.
 *  - create: MGBHIP_ERR_INVALID if det J is not positive and finite at a point of the rule.
 *  - geometry [any pointer may be NULL]: points [N x Q x d], weights [N x Q, the measures], sizes [N: h_K = |K|^(1/d),
 *    |K| the sum of an element's measures in point order].
 *  - source: f as p N nodal values carried to the points by phi [at_points = 0] or as N x Q values at the points
 *    [at_points = 1]; one source serves every column.  z [(p N) x ncol]; pexp finite and >= 1.
 *  - pointwise: r [N x Q x ncol], no reduction.
 *  - integrate: per column and element h_K^2 times the sum over its points of measure_q r_q^2, into per_element
 *    [N x ncol] or NULL, and their sum into totals [ncol].  An element's value is the sum of its Q terms in an order
 *    fixed by Q alone, the totals are compensated sums over the elements in a fixed order: results are reproducible bit
 *    for bit, do not depend on per_element, and a column's do not depend on the other columns.
 *  - plan [no handle, no device]: the ten slots of mgbhip_quadrature_plan for that shape; S, G and the LDS base are those
 *    of a quadrature of the same shape, the tables have 1 + d + d(d+1)/2 rows per node.
 *  - times: device milliseconds of the last pointwise or integrate call, taken with events on the context's stream:
 *    ms2 = { the element kernel, the reduction over the elements [0 after pointwise] }; invalid before the first call. */
typedef struct mgbhip_residual mgbhip_residual;
int mgbhip_residual_create(mgbhip_ctx* ctx, int32_t d, int32_t p, int64_t N, const double* x, int32_t Q, const double* wref,
                           const double* phi, const double* dphi, const double* d2phi, mgbhip_residual** out);
int mgbhip_residual_geometry(mgbhip_residual* res, double* points /* N x Q x d */, double* weights /* N x Q */,
                             double* sizes /* N */);
int mgbhip_residual_pointwise(mgbhip_residual* res, double pexp, int32_t ncol, const double* z /* (p*N) x ncol */,
                              const double* source /* p*N, or N x Q */, int32_t at_points, double* r /* N x Q x ncol */);
int mgbhip_residual_integrate(mgbhip_residual* res, double pexp, int32_t ncol, const double* z /* (p*N) x ncol */,
                              const double* source /* p*N, or N x Q */, int32_t at_points,
                              double* per_element /* N x ncol, or NULL */, double* totals /* ncol */);
int mgbhip_residual_plan(int32_t d, int32_t p, int32_t Q, int64_t N, int32_t* out16);
int mgbhip_residual_times(const mgbhip_residual* res, double* ms2);
int mgbhip_residual_destroy(mgbhip_residual* res); /* NULL is a no-op */

/* ---- faces: the facets of a mesh, fluxes through its boundary and jumps across its interior faces ------------------
 * N elements of p nodes in d = e = 2 or 3 coordinates [x: (p N) x d, element-major; t: N x p global node ids in
 * [0, 2^31)], F local faces per element with 2^(d-1) corner nodes each [corners: F x 2^(d-1) local node indices] and a
 * rule of Qf <= 100 points per face: weights wf [Qf] and, per local face, the element basis at the face's points
 * [phi: F x Qf x p; dphi: F x Qf x p x d, the derivatives in reference coordinates], the reference tangents d xi / d s_j
 * [tangents: F x (d-1) x d] and the reference outward normal [normals: F x d].  perm [ncode x Qf, ncode = 2 in 2-D and 8
 * in 3-D]: point q of a face seen from its L side is point perm[code][q] seen from its R side.  Nothing else tells the
 * library the element family.  Everything is copied.
 *  - create builds the topology on the device: an (element, face) pair whose sorted corner ids [2-D: both; 3-D: the
 *    three smallest] occur once is a boundary face, twice an interior face; more often is MGBHIP_ERR_INVALID, as is a
 *    det J that is not positive and finite at a face point.  Boundary faces are numbered in ascending element * F +
 *    face, interior faces in ascending lower incidence [the L side].  The code of an interior face: with i0, i1 the
 *    places of L's first two face corners among R's face corners, i0 in 2-D and 2 i0 + [(i0 xor i1) == 2] in 3-D.
 *  - topology [any pointer may be NULL]: boundary [B x 2: element, face], interior [I x 4: eL, fL, eR, fR], orientation
 *    [I], element_faces [N x F: an interior face index, or -1 - b for boundary face b].
 *  - geometry [which = 0: boundary faces, 1: interior faces from their L side; any pointer may be NULL]: points
 *    [nf x Qf x d], unit outward normals [nf x Qf x d], measures ds [nf x Qf].  sizes [I]: |F|^(1/(d-1)), |F| the sum of
 *    an interior face's measures in point order.
 *  - At point q of local face f of an element with nodes x_i and values z_i:  J = sum_i x_i dphi[f][q][i]^T,
 *    grad u = J^-T sum_i z_i dphi[f][q][i],  n = J^-T n_ref / |J^-T n_ref|,  ds = wf[q] |J t| [2-D] or
 *    wf[q] |J t1 x J t2| [3-D],  a = |grad u|^(pexp-2) grad u  [pexp >= 1; the zero vector where grad u = 0].
 *  - integrate: z [(p N) x ncol]; per column the sum over the boundary of ds weight F with F = u [VALUE] or a . n
 *    [FLUX]; weight [B x Qf] or NULL for 1; per_face [B x ncol] or NULL; totals [ncol].
 *  - jumps [I x ncol]: per interior face the sum of ds_L (u_L - u_R)^2 [VALUE] or ds_L (a_L . n_L + a_R . n_R)^2 [FLUX],
 *    each side evaluated through its own element at the matched point.
 *  - indicator: eta2 [N x ncol], per element the sum over its interior faces in local face order of (size / 2) times
 *    the FLUX jump; totals [ncol].
 *    A face's value is the sum of its Qf terms in an order fixed by Qf alone, totals are compensated sums in face or
 *    element order: results are reproducible bit for bit, a column's do not depend on the other columns, a face's do
 *    not depend on the weights of other faces, and totals do not depend on per_face.
 *  - plan [no handle, no device]: out16 = { threads, lanes per face, faces per workgroup G [0: a face does not fit],
 *    columns per pass, 1 if the tables are staged in LDS [0: read through L2], threads of the reduction, face groups,
 *    workgroups, dynamic LDS bytes, bytes of the tables, 0... } for sides = 1 [boundary] or 2 [interior].
 *  - times: device milliseconds taken with events on the context's stream: ms3 = { the face kernel and the reduction
 *    of the last integrate / jumps / indicator call [0 before the first], the topology build of create }.            */
enum { MGBHIP_FACE_VALUE = 0, MGBHIP_FACE_FLUX = 1 };
typedef struct mgbhip_faces mgbhip_faces;
int mgbhip_faces_create(mgbhip_ctx* ctx, int32_t d, int32_t p, int64_t N, const double* x, const int32_t* t, int32_t F,
                        int32_t Qf, const double* wf, const double* phi, const double* dphi, const double* tangents,
                        const double* normals, const int32_t* corners, int32_t ncode, const int32_t* perm,
                        mgbhip_faces** out, int64_t* nboundary, int64_t* ninterior);
int mgbhip_faces_topology(const mgbhip_faces* faces, int32_t* boundary, int32_t* interior, int32_t* orientation,
                          int32_t* element_faces);
int mgbhip_faces_geometry(mgbhip_faces* faces, int32_t which, double* points, double* normals, double* measures);
int mgbhip_faces_sizes(const mgbhip_faces* faces, double* sizes /* I */);
int mgbhip_faces_integrate(mgbhip_faces* faces, int32_t kind, double pexp, int32_t ncol, const double* z /* (p*N) x ncol */,
                           const double* weight /* B x Qf, or NULL */, double* per_face /* B x ncol, or NULL */,
                           double* totals /* ncol */);
int mgbhip_faces_jumps(mgbhip_faces* faces, int32_t kind, double pexp, int32_t ncol, const double* z /* (p*N) x ncol */,
                       double* jumps /* I x ncol */);
int mgbhip_faces_indicator(mgbhip_faces* faces, double pexp, int32_t ncol, const double* z /* (p*N) x ncol */,
                           double* eta2 /* N x ncol */, double* totals /* ncol */);
int mgbhip_faces_plan(int32_t d, int32_t p, int32_t Qf, int32_t F, int32_t sides, int64_t nfaces, int32_t* out16);
int mgbhip_faces_times(const mgbhip_faces* faces, double* ms3);
int mgbhip_faces_destroy(mgbhip_faces* faces); /* NULL is a no-op */

/* ---- level sets: level curves (d = 2) and isosurfaces (d = 3) of an element-space function ------------------------
 * Every element is sampled on a uniform reference lattice of refine + 1 points per axis (Q_k; axis 0 fastest) or on
 * the barycentric lattice of the refine-fold uniform subdivision (P1 / P2) with its own basis; a lattice square is
 * split into two triangles along the diagonal from corner [i, j] to [i+1, j+1], a lattice cube into the six Kuhn
 * tetrahedra around the diagonal from [i, j, k] to [i+1, j+1, k+1]; every simplex is cut linearly at every level
 * [a vertex with value >= level is above; a simplex with a non-finite vertex value emits nothing].  The result is an
 * unindexed list of S simplices of d vertices each: segments [d = 2] or triangles [d = 3].
 *  - family, d, k, p, N, x, table are those of the interpolate entry point above; only QK [d = 2 or 3], P1, P2
 *    [straight elements] and P2C are accepted.
 *  - fields is (p*N) x nfield row-major, 1 <= nfield <= 5: column 0 is contoured, the others are carried along and
 *    interpolated linearly to every vertex of the result.
 *  - levels: nlevels finite values [nlevels = 0 gives S = 0]; duplicates are separate levels.
 *  - refine: 1..16 for d = 2, 1..8 for d = 3.
 * Order of the simplices: element, lattice cell, simplex of the cell, level index, triangle of a 2-2 split of a
 * tetrahedron.  It is produced by a count pass, an exclusive scan and an emit pass, without atomics: two calls return
 * bitwise equal arrays.  create leaves the result on the device and reports S; fetch copies it out: points S x d x d
 * [simplex, vertex, coordinate; S x d x e after mgbhip_contour_create_embedded], level S [index into levels],
 * element S, carried S x d x (nfield - 1) or NULL.  The handle belongs to the context it was created from and must be
 * destroyed before it.  Host pointers; the work runs on ctx's stream and is complete on return.                     */
typedef struct mgbhip_contour mgbhip_contour;
int mgbhip_contour_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N,
                          const double* x, const double* table, int32_t nfield /* 1 + ncarry */, const double* fields,
                          int32_t nlevels, const double* levels, int32_t refine,
                          mgbhip_contour** out, int64_t* nsimplices);
int mgbhip_contour_fetch(const mgbhip_contour* c, double* points, int32_t* level, int32_t* element,
                         double* carried /* or NULL */);
int mgbhip_contour_destroy(mgbhip_contour* c); /* NULL is a no-op */

/* ---- level curves on a surface: the same cut for a Q_k 2-D mesh embedded in R^3 ------------------------------------
 * mgbhip_contour_create_embedded is mgbhip_contour_create with the ambient dimension e of the node coordinates given:
 * x is (p*N) x e.  It accepts what mgbhip_contour_create accepts, with e == d, and family = QK, d = 2, e = 3 [a surface:
 * the elements are the images of the reference square in R^3].  mgbhip_contour_create is this entry with e = d.  The
 * lattice, the triangles, the classification and the one t = (c - v_a) / (v_b - v_a) of a crossing are those of the
 * block above; the lattice carries e position coordinates, each its own sum of p products in ascending node order, and
 * a crossing is x[c] = x_a[c] + t (x_b[c] - x_a[c]) per coordinate.  So a surface whose third coordinate is 0.0
 * everywhere returns in the first two coordinates the bits of the d = e = 2 call, and 0.0 in the third.
 * mgbhip_contour_fetch writes points as S x d x e [simplex, vertex, coordinate]; order, level, element and carried are
 * unchanged.                                                                                                         */
int mgbhip_contour_create_embedded(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t e, int32_t k, int32_t p,
                                   int64_t N, const double* x /* (p*N) x e */, const double* table,
                                   int32_t nfield /* 1 + ncarry */, const double* fields, int32_t nlevels,
                                   const double* levels, int32_t refine, mgbhip_contour** out, int64_t* nsimplices);

/* ---- tessellation: the lattice triangles of a 2-D mesh, flat or a surface in R^3 -----------------------------------
 * Every element is sampled on the lattice of the level-set block above [the same device code: positions and fields are
 * the sums the contour kernel forms] and every lattice triangle is emitted instead of its cuts: per lattice square the
 * triangles ([i, j], [i+1, j], [i+1, j+1]) and ([i, j], [i, j+1], [i+1, j+1]), i fastest [Q_k: 2 refine^2 per element];
 * per row j and cell i of the barycentric lattice the upright triangle ([i, j], [i+1, j], [i, j+1]) and then, unless
 * the cell is the last of its row, the inverted one ([i+1, j], [i, j+1], [i+1, j+1]) [P1 / P2: refine^2 per element].
 * The vertices of a triangle are in ascending lattice index.  Triangle i of element n is triangle n * ntri + i of the
 * result: T = N * ntri is known from N and refine, there is no count pass, no scan and there are no atomics; two calls
 * return bitwise equal arrays.
 *  - family, d, k, p, N, table are those of the interpolate entry point above; only QK [d = 2; e = 2 or 3], P1, P2
 *    [d = e = 2, straight elements] and P2C [d = e = 2] are accepted.  x is (p*N) x e.
 *  - fields is (p*N) x nfield row-major, 0 <= nfield <= 5 [NULL when nfield = 0]: every column is interpolated to every
 *    lattice point like the position.
 *  - refine: 1..16.  T x 3 > 2^31 - 1 vertices is MGBHIP_ERR_INVALID before anything is allocated.
 * create leaves the result on the device and reports T; fetch copies it out: points T x 3 x e [triangle, vertex,
 * coordinate], element T, values T x 3 x nfield or NULL.  The handle belongs to the context it was created from and
 * must be destroyed before it.  Host pointers; the work runs on ctx's stream and is complete on return.            */
typedef struct mgbhip_tessellation mgbhip_tessellation;
int mgbhip_tessellate_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t e, int32_t k, int32_t p, int64_t N,
                             const double* x /* (p*N) x e */, const double* table, int32_t nfield /* 0..5 */,
                             const double* fields, int32_t refine, mgbhip_tessellation** out, int64_t* ntriangles);
int mgbhip_tessellate_fetch(const mgbhip_tessellation* t, double* points, int32_t* element,
                            double* values /* or NULL */);
int mgbhip_tessellate_destroy(mgbhip_tessellation* t); /* NULL is a no-op */

/* ---- welding: an indexed mesh, its components and vertex normals from a simplex soup ------------------------------
 * points is S x nv x e [simplex, corner, coordinate], nv in {2, 3} [segments, triangles], e in {2, 3}; the M = S nv
 * corners are numbered simplex-major.  group is S int32, or NULL [all zeros].  Two corners are linked iff their simplices
 * have the same group and fabs(x_a - y_a) <= tol on every axis a [one IEEE subtraction and one compare per axis].  A
 * vertex is a connected component of the link graph [chains weld]; vertices are numbered by their lowest corner,
 * first_corner[v], and the position of vertex v is that corner's: nothing is averaged.  cells [S x nv] holds the vertex of
 * every corner; a simplex with two corners in one vertex is kept.  The component of a vertex is its connected component
 * in the graph of the simplex edges, numbered by lowest vertex.  With want_normals [nv = e = 3 only] the normal of a
 * vertex is the sum of cross(p1 - p0, p2 - p0) over the triangles of its corners in ascending corner order, divided by
 * sqrt((nx nx + ny ny) + nz nz), or all zeros when that root is 0 or not finite [no fused multiply-add].
 * The corners are put into a uniform grid of cell side max(tol, largest extent / 2^20) and sorted by cell once; more than
 * 1024 corners in one cell is MGBHIP_ERR_INVALID [the count and tol are named] before any pair is tested, as are a
 * non-finite coordinate, S <= 0, nv or e outside its set, S nv >= 2^31, a negative or non-finite tol and want_normals
 * with (nv, e) != (3, 3).  Classes and components are labelled by hooking and shortcutting with integer atomicMin; the
 * results do not depend on the order of the atomics and two calls return bitwise equal arrays.  create leaves the index
 * on the device, frees its work buffers and reports V and the number of components; fetch copies it out [normals V x 3,
 * or NULL]; rounds reports how many labelling rounds the vertex classes and the components took.  The handle belongs to
 * the context it was created from and must be destroyed before it.  Host pointers; the work runs on ctx's stream and is
 * complete on return.                                                                                                */
typedef struct mgbhip_weld mgbhip_weld;
int mgbhip_weld_create(mgbhip_ctx* ctx, int64_t S, int32_t nv, int32_t e, const double* points,
                       const int32_t* group /* S, or NULL */, double tol, int32_t want_normals,
                       mgbhip_weld** out, int64_t* V, int64_t* ncomponents);
int mgbhip_weld_fetch(const mgbhip_weld* w, int32_t* cells /* S x nv */, int32_t* first_corner /* V */,
                      int32_t* component /* V */, double* normals /* V x 3, or NULL */);
int mgbhip_weld_rounds(const mgbhip_weld* w, int32_t* vertex_rounds, int32_t* component_rounds);
int mgbhip_weld_destroy(mgbhip_weld* w); /* NULL is a no-op */

/* ---- polylines: the segments of an indexed curve mesh ordered into lines -------------------------------------------
 * vertices is V x e, e in {2, 3}; cells is S x 2 int32 with entries in [0, V), 2 S < 2^31.  Segment s is dropped if its two
 * vertices are equal, or if a lower-numbered segment that is not dropped has the same unordered pair; the others are
 * edges.  A vertex with two edges is interior, one with one edge [an end] or three and more [a junction] is a node.  Two
 * edges that share an interior vertex belong to the same line: a line is an open path between two nodes [which may be
 * the same junction] or a cycle of interior vertices [closed].  Lines are numbered by their lowest segment.  An open line
 * starts at the end node with the smaller vertex number, or with equal ends along the end edge with the lower segment
 * number; a closed line starts at its lowest vertex and goes on to the smaller of that vertex's two neighbours.
 * Line l of n edges owns the n + 1 points offsets[l] .. offsets[l + 1] - 1 [offsets is L + 1 int64]; a closed line repeats
 * its first vertex as its last point.  vertex [P] is the vertex of every point, segment [P] the segment from point j to
 * j + 1 and -1 at the last point of a line, closed [L] is 0 or 1.  arclength [P] is 0 at the first point of a line and then
 * the sum of the lengths sqrt((dx dx + dy dy) [+ dz dz]) of the edges before the point [no fused multiply-add], added
 * within the line alone in the order of a balanced tree; length [L] is the arc length at the last point of every line.
 * The lines are ranked by pointer doubling, one lane per directed half-edge, in two passes of ceil(log2(2 S)) + 1 rounds
 * each [the lowest vertex of every cycle; then rank, ends, lowest segment and length]; rounds reports the rounds of each
 * pass [nphases = 2 entries].  No atomics are used and two calls return bitwise equal arrays.  A NULL pointer, e outside
 * {2, 3}, 2 S >= 2^31, an entry of cells outside [0, V) and a non-finite coordinate are MGBHIP_ERR_INVALID with a message
 * that names the argument; S = 0 gives L = P = 0.  create leaves the lines on the device, frees its work buffers and
 * reports L, P and the number of dropped segments; fetch copies them out.  The handle belongs to the context it was
 * created from and must be destroyed before it.
 * sample is stateless: for Q queries [line, s] on lines given by points [P x e], data [P x C, or NULL with C = 0],
 * offsets and arclength as above, s is clamped to [0, length of the line], j is the largest edge of the line whose first
 * point has arclength a[j] <= s, t = (s - a[j]) / (a[j + 1] - a[j]) or 0 when that difference is 0, and out_points
 * [Q x e] and out_data [Q x C] are x_j + t (x_{j+1} - x_j) per column [no fused multiply-add].  A line outside [0, L), a
 * non-finite s or arclength and offsets that do not give every line two points within P are MGBHIP_ERR_INVALID.
 * Host pointers; the work runs on ctx's stream and is complete on return.                                            */
typedef struct mgbhip_polyline mgbhip_polyline;
int mgbhip_polyline_create(mgbhip_ctx* ctx, int64_t V, int32_t e, const double* vertices /* V x e */, int64_t S,
                           const int32_t* cells /* S x 2 */, mgbhip_polyline** out, int64_t* L, int64_t* P,
                           int64_t* ndropped);
int mgbhip_polyline_fetch(const mgbhip_polyline* pl, int64_t* offsets /* L + 1 */, int32_t* vertex /* P */,
                          int32_t* segment /* P */, uint8_t* closed /* L */, double* arclength /* P */,
                          double* length /* L */);
int mgbhip_polyline_rounds(const mgbhip_polyline* pl, int32_t* rounds /* one per iterated phase */, int32_t* nphases);
int mgbhip_polyline_destroy(mgbhip_polyline* pl); /* NULL is a no-op */
int mgbhip_polyline_sample(mgbhip_ctx* ctx, int32_t e, int64_t P, const double* points, int32_t C,
                           const double* data /* P x C, or NULL */, int64_t L, const int64_t* offsets,
                           const double* arclength, int64_t Q, const int32_t* line, const double* s,
                           double* out_points, double* out_data /* Q x C, or NULL */);

/* ---- ray casting: line integrals and volume rendering of an element-space function --------------------------------
 * R rays x = origin + t dir [R x d each, row-major; dir of unit length, so t is arc length] are clipped to
 * [t_min, t_max] and against the axis-parallel box [box: 2 d doubles, lo then hi] by the slab test: for an axis a with
 * dir[a] != 0, t1 = (lo[a] - o[a]) / dir[a], t2 = (hi[a] - o[a]) / dir[a], tmin = max(tmin, min(t1, t2)), tmax =
 * min(tmax, max(t1, t2)); an axis with dir[a] == 0 misses unless lo[a] <= o[a] <= hi[a]; a ray with !(tmax > tmin) has
 * no samples.  Otherwise it has n = max(1, floor((tmax - tmin) / step + 0.5)) samples of step h = (tmax - tmin) / n, sample
 * i at t = tmin + (i + 0.5) h, x[a] = o[a] + t dir[a] [no fused multiply-add].  create lays the samples out ray by ray
 * [count pass, exclusive scan, emit pass; no atomics], locates them like mgbhip_locator_create and keeps per sample the
 * element and the reference coordinates on the device; it reports the number of samples S, and S > 2^31 - 1 is
 * MGBHIP_ERR_INVALID before the sample arrays are allocated.
 *  - family, d, k, p, N, x, table are those of the interpolate entry point above; only QK [d = 2 or 3], P1 and P2
 *    [straight elements] are accepted (not P2C: rays are clipped against the unpadded node box).  R = 0 is allowed.
 *  - offsets [R + 1]: ray r owns samples offsets[r] .. offsets[r + 1] - 1.  samples [S x d]: the positions, regenerated.
 *  - lengths: step[r] = h of ray r [0 without samples], length[r] = h x the number of its samples that lie in an
 *    element; either pointer may be NULL.
 *  - integrate: z is (p*N) x ncomp; out[r, c] = h x the sum, in sample order, of the finite values of column c at the
 *    samples of ray r [a sample outside the mesh has the value NaN].
 *  - render: u is p*N values, transfer K x 4 rows of (r, g, b, sigma), K >= 2, finite, sigma >= 0 per unit length;
 *    lo < hi finite.  Front to back from T = 1, C = 0, per sample with a finite value v: s = min(1, max(0, (v - lo) /
 *    (hi - lo))), f = s (K - 1), j = min(floor(f), K - 2), w = f - j, row = T[j] + w (T[j+1] - T[j]), e = exp(-(sigma h)),
 *    C += (T (1 - e)) row_rgb, T = T e.  out [R x 4] = (C_r, C_g, C_b, 1 - T): premultiplied colour and alpha.
 * The handle belongs to the context it was created from and must be destroyed before it.  Host pointers; the work runs
 * on ctx's stream and is complete on return.                                                                        */
typedef struct mgbhip_raycast mgbhip_raycast;
int mgbhip_raycast_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N,
                          const double* x, const double* table, int64_t R, const double* origin, const double* dir,
                          const double* box, double step, double t_min, double t_max,
                          mgbhip_raycast** out, int64_t* nsamples);
int mgbhip_raycast_offsets(const mgbhip_raycast* rc, int64_t* offsets /* R + 1 */);
int mgbhip_raycast_samples(const mgbhip_raycast* rc, double* pts /* S x d */);
int mgbhip_raycast_lengths(const mgbhip_raycast* rc, double* step /* R or NULL */, double* length /* R or NULL */);
int mgbhip_raycast_integrate(mgbhip_raycast* rc, int32_t ncomp, const double* z /* (p*N) x ncomp */,
                             double* out /* R x ncomp */);
int mgbhip_raycast_render(mgbhip_raycast* rc, const double* u /* p*N */, int32_t K, const double* transfer /* K x 4 */,
                          double lo, double hi, double* out /* R x 4 */);
int mgbhip_raycast_destroy(mgbhip_raycast* rc); /* NULL is a no-op */
/* render with nhits [1..8] layers per ray merged into the samples by depth: t_hit [R x nhits] ascends along every ray
 * [+inf: no layer], layer [R x nhits x 4] holds finite premultiplied colour and alpha.  From T = 1, C = 0 the layers
 * with t_hit <= t_i are applied before sample i [t_i = tmin + (i + 0.5) h], the finite ones that remain after the last
 * sample; a layer does C += T layer_rgb, T = T (1 - layer_alpha); a sample does what render does.  A ray without
 * samples composites its layers alone.                                                                              */
int mgbhip_raycast_render_layers(mgbhip_raycast* rc, const double* u /* p*N */, int32_t K,
                                 const double* transfer /* K x 4 */, double lo, double hi, int32_t nhits,
                                 const double* t_hit /* R x nhits */, const double* layer /* R x nhits x 4 */,
                                 double* out /* R x 4 */);

/* ---- rays against a triangle soup: nearest hits and their shading ---------------------------------------------------
 * create uploads T triangles [points: T x 3 x 3, triangle, vertex, coordinate; finite; T = 0 is allowed] and sorts them
 * into a uniform grid of cells [boxes, union, count pass, exclusive scan, emit pass, stable radix sort by cell; no
 * atomics].  The grid decides only which triangles a ray is tested against, never the result.
 *  - trace: R rays x = origin + t dir [dir of unit length].  With v0, v1, v2 the vertices of a triangle, a x b the cross
 *    product [(a x b)[0] = a1 b2 - a2 b1, cyclically] and a . b = (a0 b0 + a1 b1) + a2 b2, without fused multiply-add:
 *      e1 = v1 - v0, e2 = v2 - v0, p = dir x e2, det = e1 . p, s = origin - v0, u = (s . p) / det, q = s x e1,
 *      v = (dir . q) / det, t = (e2 . q) / det.
 *    The triangle is hit iff det is finite and non-zero, u >= 0, v >= 0, u + v <= 1 and t_min <= t <= t_max [two-sided].
 *    Per ray the K [1..8] nearest hits in the order of (t, triangle index) are written to t, tri, u, v [R x K each];
 *    a missing entry is t = +inf, tri = -1, u = v = NaN.
 *  - shade: tri, u, v as trace returned them; values [T x 3] is a value per triangle vertex, table [Kt x 4] rows of
 *    (r, g, b, alpha) looked up as render looks up its table: c = ((1 - u - v) c0 + u c1) + v c2, s = min(1, max(0, (c -
 *    lo) / (hi - lo))), f = s (Kt - 1), j = min(floor(f), Kt - 2), w = f - j, row = table[j] + w (table[j+1] - table[j]);
 *    n = e1 x e2, nn = n / sqrt(n . n), shade = ambient + (1 - ambient) |nn . dir|, alpha = min(1, max(0, row[3]));
 *    layer [R x K x 4] = ((alpha shade) r, (alpha shade) g, (alpha shade) b, alpha); a missing hit or a non-finite c
 *    gives a zero layer.
 * The handle belongs to the context it was created from and must be destroyed before it.  Host pointers; the work runs
 * on ctx's stream and is complete on return.                                                                        */
typedef struct mgbhip_surface mgbhip_surface;
int mgbhip_surface_create(mgbhip_ctx* ctx, int64_t T, const double* points /* T x 3 x 3 */, mgbhip_surface** out);
int mgbhip_surface_trace(mgbhip_surface* s, int64_t R, const double* origin, const double* dir, double t_min,
                         double t_max, int32_t K, double* t, int32_t* tri, double* u, double* v /* R x K each */);
int mgbhip_surface_shade(mgbhip_surface* s, int64_t R, int32_t K, const double* dir, const int32_t* tri,
                         const double* u, const double* v, const double* values /* T x 3 */, int32_t Kt,
                         const double* table /* Kt x 4 */, double lo, double hi, double ambient,
                         double* layer /* R x K x 4 */);
int mgbhip_surface_destroy(mgbhip_surface* s); /* NULL is a no-op */

/* ---- rays against a soup of capsules: curves drawn as tubes ---------------------------------------------------------
 * create uploads S segments [points: S x 2 x 3, segment, end point, coordinate; finite; S = 0 is allowed] with a radius
 * each [finite, > 0] and sorts the boxes of their capsules [the end points' box widened by the radius] into the grid of
 * the triangle block above, by the same kernels.  A capsule is the set of points within r of the segment [a, b].
 *  - trace: R rays x = origin + t dir [dir of unit length].  With a . b = (a0 b0 + a1 b1) + a2 b2, without fused
 *    multiply-add:
 *      ba = b - a, oa = origin - a, ob = origin - b,
 *      baba = ba . ba, bard = ba . dir, baoa = ba . oa, rdoa = dir . oa, oaoa = oa . oa,
 *      A = baba - bard bard, B = baba rdoa - baoa bard, Cq = (baba oaoa - baoa baoa) - (r r) baba, h = B B - A Cq;
 *      side:  valid iff A > 0, h >= 0 and 0 <= y <= baba, with ts = (-B - sqrt(h)) / A, y = baoa + ts bard; s = y / baba;
 *      cap a: b2 = dir . oa, c2 = oaoa - r r, h2 = b2 b2 - c2; valid iff h2 >= 0; ta = -b2 - sqrt(h2); s = 0;
 *      cap b: the same with ob; s = 1.
 *    The entry parameter is the smallest valid one of ts, ta, tb [compared with < in that order: a tie keeps the earlier
 *    piece; exact for the union because a capsule is convex].  The capsule is hit iff a piece is valid and
 *    t_min <= t <= t_max for that entry parameter: a ray that starts inside a capsule does not hit it, exit points are
 *    never reported, a capsule gives at most one hit.  Per ray the K [1..8] nearest hits in the order of (t, segment
 *    index) are written to t, segment, s [R x K each]; a missing entry is t = +inf, segment = -1, s = NaN.
 *  - shade: t, segment, s as trace returned them; values [S x 2] is a value per end point, table [Kt x 4] rows of
 *    (r, g, b, alpha) looked up as mgbhip_surface_shade looks up its table with c = (1 - s) c0 + s c1;
 *    x = origin + t dir, q = a + s ba, n = x - q, nn = n / sqrt(n . n), shade = ambient + (1 - ambient) |nn . dir|,
 *    alpha = min(1, max(0, row[3])); layer [R x K x 4] = ((alpha shade) r, (alpha shade) g, (alpha shade) b, alpha); a
 *    missing hit or a non-finite c gives a zero layer.
 * The handle belongs to the context it was created from and must be destroyed before it.  Host pointers; the work runs
 * on ctx's stream and is complete on return.                                                                        */
typedef struct mgbhip_tubes mgbhip_tubes;
int mgbhip_tubes_create(mgbhip_ctx* ctx, int64_t S, const double* points /* S x 2 x 3 */, const double* radii /* S */,
                        mgbhip_tubes** out);
int mgbhip_tubes_trace(mgbhip_tubes* s, int64_t R, const double* origin, const double* dir, double t_min, double t_max,
                       int32_t K, double* t, int32_t* segment, double* sp /* R x K each */);
int mgbhip_tubes_shade(mgbhip_tubes* s, int64_t R, int32_t K, const double* origin, const double* dir, const double* t,
                       const int32_t* segment, const double* sp, const double* values /* S x 2 */, int32_t Kt,
                       const double* table /* Kt x 4 */, double lo, double hi, double ambient,
                       double* layer /* R x K x 4 */);
int mgbhip_tubes_destroy(mgbhip_tubes* s); /* NULL is a no-op */

/* ---- field lines: the lines of a vector field traced through the mesh ----------------------------------------------
 * The field is v = (z[:, 0], .., z[:, d-1]) [field = VECTOR: z is (p*N) x d row-major, the element-space functions of
 * the components] or v = grad u [field = GRADIENT: z is the p*N values of u].  v(y) is evaluated as
 * mgbhip_interpolate [VECTOR] / mgbhip_interpolate_grad [GRADIENT] evaluate it and is bitwise what they return: the
 * lowest-index element of the candidate list of y's cell that contains y, never a warm start from the previous element.
 * create uploads the mesh, builds the location grid and keeps both on the device with z; set_field replaces z alone [the
 * same shape].  trace follows S lines from seeds [S x d; a non-finite seed is outside the mesh] by the classical
 * Runge-Kutta scheme with the signed step h [finite, != 0], without fused multiply-add:
 *     k1 = v(x);  k2 = v(x + (0.5 h) k1);  k3 = v(x + (0.5 h) k2);  k4 = v(x + h k3);
 *     x <- x + (h / 6) (((k1 + 2 k2) + 2 k3) + k4).
 * Every stage forms speed = sqrt(v . v) [squares added in axis order]; with normalize != 0 the stage velocity is
 * v / speed, so |h| is arc length.  A stage point without an element ends the line at the current x with LEFT [OUTSIDE
 * when it is the seed itself: the line then has no point]; !(speed > min_speed) ends it with STALLED [also for NaN, and
 * for 0 / 0 under normalize]; otherwise it ends after max_steps [>= 1] steps.  min_speed is finite and >= 0.
 *  - points [S x (max_steps + 1) x d]: row 0 of a line is its seed, row i the point after i steps, NaN from row n on.
 *  - n [S]: the number of points of the line, 0 for a seed in no element.  status [S]: MGBHIP_STREAM_*.
 *  - family, d, k, p, N, x, table are those of the interpolate entry point above; only QK [d = 2 or 3], P1, P2
 *    [straight elements] and P2C are accepted.  S = 0 is a no-op; S (max_steps + 1) d >= 2^31 is MGBHIP_ERR_INVALID before
 *    anything is allocated.
 * One lane traces one line and stores by seed index: two calls return bitwise equal arrays.  The handle belongs to the
 * context it was created from and must be destroyed before it.  Host pointers; the work runs on ctx's stream and is
 * complete on return.                                                                                               */
#define MGBHIP_STREAM_VECTOR 0
#define MGBHIP_STREAM_GRADIENT 1
#define MGBHIP_STREAM_MAX_STEPS 0
#define MGBHIP_STREAM_LEFT 1
#define MGBHIP_STREAM_STALLED 2
#define MGBHIP_STREAM_OUTSIDE 3
typedef struct mgbhip_stream mgbhip_stream;
int mgbhip_stream_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N,
                         const double* x, const double* table, int32_t field, const double* z,
                         mgbhip_stream** out);
int mgbhip_stream_set_field(mgbhip_stream* s, const double* z /* (p*N) x d or p*N */);
int mgbhip_stream_trace(mgbhip_stream* s, int64_t S, const double* seeds /* S x d */, double h, int32_t max_steps,
                        int32_t normalize, double min_speed, double* points /* S x (max_steps + 1) x d */,
                        int32_t* n /* S */, int32_t* status /* S */);
int mgbhip_stream_destroy(mgbhip_stream* s); /* NULL is a no-op */

/* ---- the default figure of a fem3d solution, frame after frame -------------------------------------------------------
 * One handle chains the stages above on the device for a fixed camera, fixed isosurface levels, fixed slices and fixed
 * colour limits, and renders one field after another; a frame is bitwise what the host gets by chaining
 * mgbhip_contour_create, mgbhip_surface_create / _trace / _shade and mgbhip_raycast_create / _render_layers with the same
 * arguments, because the same kernels run on the same inputs.
 *  - create: family, d, k, p, N, x, table are those of mgbhip_raycast_create, restricted to QK with d = 3 and k <= 8.
 *    R >= 1 rays [origin, dir: R x 3, dir of unit length], box [2 x 3: the clip box, lo then hi] and step are those of
 *    mgbhip_raycast_create with t_min = 0, t_max = +inf.  volume != 0 samples and locates the rays once; volume = 0
 *    draws the surfaces alone.  levels [nlevels, 0..64, finite] are the isosurfaces of u, each coloured by its level
 *    value; slice i [nslices, 0..16] is the plane x[axes[i]] = coords[i] [axis 0..2, finite], cut as the level set of
 *    the coordinate function with u carried and coloured by u.  vtable [ntable x 4: r, g, b, sigma >= 0] is the
 *    volume's table, stable [ntable x 4: r, g, b, alpha] the surfaces', both finite, ntable >= 2; lo < hi finite are
 *    the colour limits of both; ambient in [0, 1] is that of mgbhip_surface_shade; K [1..8] hits are kept per ray.
 *    Everything is checked, and refused by count, before anything is allocated.  Resident from here on: the mesh, the
 *    rays, the levels, the slices' coordinate functions, both tables and, with the volume, the located samples.
 *  - render: u is p*N values.  The contours are cut with the lattice refine = k; the soup is the isosurface triangles
 *    followed by the slices in the order given [T = 0 is allowed: every ray misses]; it is put into its grid, traced
 *    [K nearest hits] and shaded on the device.  With the volume the layers are merged into the samples as
 *    mgbhip_raycast_render_layers merges them; without it they are composited alone, front to back from T = 1, C = 0 by
 *    C = C + T layer_rgb, T = T (1 - layer_alpha), giving (C, 1 - T).  out [R x 4] is premultiplied colour and alpha.
 *    The transfers of a frame are u going in and out coming back, besides the scalar read-backs of the stages.
 *  - render_rgba8: the same frame over background [3 doubles, finite] as bytes: per colour channel c = C + (1 - alpha) b,
 *    q = floor(255 min(1, max(0, c)) + 0.5), 0 for a c that is not finite; the fourth byte is that rule applied to
 *    alpha.  out is R x 4 bytes.  No fused multiply-add.
 *  - counts: the triangles of the last frame's soup and the (cell, triangle) pairs of its grid [0, 0 before the first
 *    frame]; either pointer may be NULL.
 * Per-frame buffers grow to the largest frame seen and are kept.  The handle belongs to the context it was created from
 * and must be destroyed before it.  Host pointers; the work runs on ctx's stream and is complete on return.          */
typedef struct mgbhip_figure mgbhip_figure;
int mgbhip_figure_create(mgbhip_ctx* ctx, int32_t family, int32_t d, int32_t k, int32_t p, int64_t N,
                         const double* x, const double* table, int64_t R, const double* origin, const double* dir,
                         const double* box, double step, int32_t volume, int32_t nlevels, const double* levels,
                         int32_t nslices, const int32_t* axes, const double* coords, int32_t ntable,
                         const double* vtable /* ntable x 4 */, const double* stable /* ntable x 4 */, double lo,
                         double hi, double ambient, int32_t K, mgbhip_figure** out);
int mgbhip_figure_render(mgbhip_figure* f, const double* u /* p*N */, double* out /* R x 4 */);
int mgbhip_figure_render_rgba8(mgbhip_figure* f, const double* u /* p*N */, const double* background /* 3 */,
                               uint8_t* out /* R x 4 */);
int mgbhip_figure_counts(const mgbhip_figure* f, int64_t* ntriangles, int64_t* npairs);
int mgbhip_figure_destroy(mgbhip_figure* f); /* NULL is a no-op */

#ifdef __cplusplus
}
#endif
#endif /* MGBHIP_H */
