// elem_kernels.hpp -- element evaluation kernels and launch_elem (included by kernels.hip).
#pragma once
#include <mutex>
#include <utility>

#include "dense.hpp"
#include "elem_device.hpp"

namespace mgbhip {

namespace {

template <int NY, int MODE>
__global__ __launch_bounds__(256) void elem_kernel(const ElemParams P, const int lgG) {
    extern __shared__ double sh[];
    const int tid = threadIdx.x;
    const int G = 1 << lgG;
    const int EPB = 256 >> lgG;
    const int el = tid >> lgG;
    const int r = tid & (G - 1);
    const int p = P.p;
    const int pp = p * p;
    const int nu = P.nu;
    const int64_t e = (int64_t)blockIdx.x * EPB + el;
    const bool active = (e < P.N) && (r < p);
    const int64_t n = P.n;
    const int64_t node = e * p + r;

    double* zl = sh;                                    // [EPB][nu][G]
    double* opL = zl + elem_lds_z(256, nu);     // [nstage][EPB][pp]
    double* YL = opL + elem_lds_ops(P.nstage, EPB, pp);     // MODE_F1: [EPB][NY][G]; MODE_F2: [EPB][tri][G]

    // 1. stage the operator blocks of this workgroup's elements (flat, coalesced)
    {
        const int64_t e0 = (int64_t)blockIdx.x * EPB;
        int64_t lim = (P.N - e0) * pp;
        if (lim > (int64_t)EPB * pp) lim = (int64_t)EPB * pp;
        for (int o = 0; o < P.nstage; ++o) {
            const double* src = P.stage_ptr[o] + e0 * pp;
            double* dst = opL + (size_t)o * EPB * pp;
            for (int i = tid; i < lim; i += 256) dst[i] = src[i];
        }
    }
    // 2. fine broken-basis values of this element: z0 + R*s  (src/convex.jl:156)
    if (active) stage_z(P, zl, el, nu, G, r, n, node);
    __syncthreads();

    auto OP = [&](int k, int rr, int cc) -> double {    // D_k block entry (rr, cc) of this element
        const int so = P.D_stage[k];
        if (so >= 0) return opL[((size_t)so * EPB + el) * pp + cc * p + rr];
        return P.ops[P.D_op[k]][e * pp + cc * p + rr];
    };

    // 3. Dz at this node (src/convex.jl:125)
    double y[NY];
#pragma unroll
    for (int k = 0; k < NY; ++k) {
        double v = 0.0;
        if (active) {
            const int a = P.D_state[k];
            if (P.D_stage[k] == -1) {
                v = zl[(el * nu + a) * G + r];
            } else {
                for (int cc = 0; cc < p; ++cc) v += OP(k, r, cc) * zl[(el * nu + a) * G + cc];
            }
        }
        y[k] = v;
    }

    double F = 0.0;
    double g[NY];
    double H[NY * NY];
    (void)g;
    (void)H;

    if (MODE == MODE_F0 || MODE == MODE_NODE_F) {
        if (active) cone_eval<NY, 0>(P.cone, node, n, y, F, g, H);
        if (MODE == MODE_NODE_F) {
            if (active) {
                P.out_F[node] = F;
                if (P.out_Dz != nullptr) {
#pragma unroll
                    for (int k = 0; k < NY; ++k) P.out_Dz[node + n * k] = y[k];
                }
            }
            return;
        }
        double val = 0.0;
        if (active) {
            const double bar = barrier_f0(P, node, F);
            double lin = 0.0;
#pragma unroll
            for (int k = 0; k < NY; ++k) lin += P.c[node + n * k] * y[k];
            val = bar + P.w[node] * lin;
        }
        __syncthreads();            // zl / opL no longer needed: reuse LDS for the reduction
        const double tot = block_sum_256(val, sh);
        if (tid == 0) P.out_partial[blockIdx.x] = tot;
        return;
    }
    if (MODE == MODE_NODE_SLACK) {
        if (active) P.out_F[node] = cone_slack<NY>(P.cone, node, n, y);
        return;
    }
    if (MODE == MODE_F01) {
        // One line-search trial (src/newton.jl:35-50 evaluates F0 then F1 at the same point): the operator
        // blocks, z and c are streamed once instead of twice.
        double val = 0.0;
        if (active) {
            double F0v;
            cone_eval<NY, 0>(P.cone, node, n, y, F0v, g, H);
            cone_eval<NY, 1>(P.cone, node, n, y, F, g, H);
            const double wv = P.w[node];
            const double bwv = P.bw ? P.bw[node] : 0.0;
            const double bar = P.bw ? ((bwv == 0.0) ? 0.0 : bwv * F0v) : P.invn * F0v;
            double lin = 0.0;
#pragma unroll
            for (int k = 0; k < NY; ++k) {
                const double ck = P.c[node + n * k];
                lin += ck * y[k];
                const double sc = P.bw ? ((bwv == 0.0) ? 0.0 : bwv * g[k]) : P.invn * g[k];
                YL[(el * NY + k) * G + r] = sc + wv * ck;
            }
            val = bar + wv * lin;
        }
        __syncthreads();
        if (active) {
            const int i = r;
            for (int a = 0; a < nu; ++a) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < NY; ++k) {
                    if (P.D_state[k] != a) continue;
                    const double* Yk = YL + (el * NY + k) * G;
                    if (P.D_stage[k] == -1) {
                        acc += Yk[i];
                    } else {
                        for (int rr = 0; rr < p; ++rr) acc += OP(k, rr, i) * Yk[rr];
                    }
                }
                P.out_ret[(int64_t)a * n + node] = acc;
            }
        }
        __syncthreads();            // zl / opL / YL no longer needed: reuse LDS for the reduction
        const double tot = block_sum_256(val, sh);
        if (tid == 0) P.out_partial[blockIdx.x] = tot;
        return;
    }
    if (MODE == MODE_F1) {
        // Y = scale(grad F) + w .* c   (src/convex.jl:170-173), then sum_k D_k' Y_k per element
        if (active) {
            cone_eval<NY, 1>(P.cone, node, n, y, F, g, H);
            const double wv = P.w[node];
            const double bwv = P.bw ? P.bw[node] : 0.0;
#pragma unroll
            for (int k = 0; k < NY; ++k) {
                double sc = P.bw ? ((bwv == 0.0) ? 0.0 : bwv * g[k]) : P.invn * g[k];
                YL[(el * NY + k) * G + r] = sc + wv * P.c[node + n * k];
            }
        }
        __syncthreads();
        if (active) {
            const int i = r;
            for (int a = 0; a < nu; ++a) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < NY; ++k) {
                    if (P.D_state[k] != a) continue;
                    const double* Yk = YL + (el * NY + k) * G;
                    if (P.D_stage[k] == -1) {
                        acc += Yk[i];
                    } else {
                        for (int rr = 0; rr < p; ++rr) acc += OP(k, rr, i) * Yk[rr];
                    }
                }
                P.out_ret[(int64_t)a * n + node] = acc;
            }
        }
        return;
    }
    if (MODE == MODE_F2) {
        constexpr int NT = NY * (NY + 1) / 2;
        if (active) {
            cone_eval<NY, 2>(P.cone, node, n, y, F, g, H);
            const double bwv = P.bw ? P.bw[node] : 0.0;
#pragma unroll
            for (int k = 0; k < NY; ++k)
#pragma unroll
                for (int k2 = k; k2 < NY; ++k2) {
                    const double h = H[k * NY + k2];
                    const double sc = P.bw ? ((bwv == 0.0) ? 0.0 : bwv * h) : P.invn * h;   // written out: scale_by changes the NY = 1 stream
                    YL[((size_t)el * NT + tri_index(k, k2, NY)) * G + r] = sc;
                }
        }
        __syncthreads();
        if (active) {
            // lane j = r owns column j of every block (a,b), a <= b, of the element Hessian
            //   Hel_ab[i,j] = sum_rr sum_{k in K_a} sum_{k2 in K_b} D_k[rr,i] Y[rr][k,k2] D_k2[rr,j]
            // (src/convex.jl:191-200 with the 16 temporaries fused away)
            const int j = r;
            const int NB = nu * (nu + 1) / 2;
            for (int a = 0; a < nu; ++a)
                for (int b = a; b < nu; ++b) {
                    const int blk = a * nu - (a * (a - 1)) / 2 + (b - a);
                    const bool dblk = (P.diag_mask >> blk) & 1;
                    double* out = P.out_hel + P.blk_off[blk] + (dblk ? (e * p + j) - j : (e * p + j) * (int64_t)p);
                    for (int i = dblk ? j : 0; i < (dblk ? j + 1 : p); ++i) {
                        double val = 0.0;
#pragma unroll
                        for (int k = 0; k < NY; ++k) {
                            if (P.D_state[k] != a) continue;
                            const bool idk = P.D_stage[k] == -1;
#pragma unroll
                            for (int k2 = 0; k2 < NY; ++k2) {
                                if (P.D_state[k2] != b) continue;
                                const bool idk2 = P.D_stage[k2] == -1;
                                const int t = (k <= k2) ? tri_index(k, k2, NY) : tri_index(k2, k, NY);
                                const double* Yt = YL + ((size_t)el * NT + t) * G;
                                if (idk && idk2) {
                                    val += (i == j) ? Yt[i] : 0.0;
                                } else if (idk) {
                                    val += Yt[i] * OP(k2, i, j);
                                } else if (idk2) {
                                    val += OP(k, j, i) * Yt[j];
                                } else {
                                    double acc = 0.0;
                                    for (int rr = 0; rr < p; ++rr) acc += OP(k, rr, i) * Yt[rr] * OP(k2, rr, j);
                                    val += acc;
                                }
                            }
                        }
                        out[i] = val;
                    }
                }
        }
        return;
    }
}

// Wide path (problems with more than 10 D rows or a power cone wider than NARROW_W; cone.hpp: cone_eval_wide): the same
// contract as elem_kernel -- z_at with the selection map, the on-the-fly trial point, barrier weights / invn, diag_mask
// and blk_off of the slab, the phase-I cobarrier and box terms -- for a runtime nD <= WIDE_NY.  y and the gradient live
// in registers (WIDE_NY doubles each); the node Hessian is written entry by entry into its LDS triangle [EPB][tri][G]
// and never held in registers, and the block products run as runtime loops over the D rows.  MODE_F2 runs
// WIDE_F2_THREADS threads per workgroup (the triangle of 128 lanes at nD = 13 is 93 KB), every other mode 256.
template <int MODE>
__global__ __launch_bounds__(256) void elem_wide_kernel(const ElemParams P, const int lgG) {
    extern __shared__ double sh[];
    const int tid = threadIdx.x;
    const int NT_ = blockDim.x;
    const int G = 1 << lgG;
    const int EPB = NT_ >> lgG;
    const int el = tid >> lgG;
    const int r = tid & (G - 1);
    const int p = P.p;
    const int pp = p * p;
    const int nu = P.nu;
    const int nD = P.nD;
    const int64_t e = (int64_t)blockIdx.x * EPB + el;
    const bool active = (e < P.N) && (r < p);
    const int64_t n = P.n;
    const int64_t node = e * p + r;

    double* zl = sh;                                    // [EPB][nu][G]
    double* opL = zl + elem_lds_z((size_t)NT_, nu);     // [nstage][EPB][pp]
    double* YL = opL + elem_lds_ops(P.nstage, EPB, pp);     // MODE_F1 / F01: [EPB][nD][G]; MODE_F2: [EPB][tri][G]
    {
        const int64_t e0 = (int64_t)blockIdx.x * EPB;
        int64_t lim = (P.N - e0) * pp;
        if (lim > (int64_t)EPB * pp) lim = (int64_t)EPB * pp;
        for (int o = 0; o < P.nstage; ++o) {
            const double* src = P.stage_ptr[o] + e0 * pp;
            double* dst = opL + (size_t)o * EPB * pp;
            for (int i = tid; i < lim; i += NT_) dst[i] = src[i];
        }
    }
    if (active) stage_z(P, zl, el, nu, G, r, n, node);
    __syncthreads();

    auto OP = [&](int k, int rr, int cc) -> double {
        const int so = P.D_stage[k];
        if (so >= 0) return opL[((size_t)so * EPB + el) * pp + cc * p + rr];
        return P.ops[P.D_op[k]][e * pp + cc * p + rr];
    };

    double y[WIDE_NY];
#pragma unroll
    for (int k = 0; k < WIDE_NY; ++k) {
        double v = 0.0;
        if (active && k < nD) {
            const int a = P.D_state[k];
            if (P.D_stage[k] == -1) {
                v = zl[(el * nu + a) * G + r];
            } else {
                for (int cc = 0; cc < p; ++cc) v += OP(k, r, cc) * zl[(el * nu + a) * G + cc];
            }
        }
        y[k] = v;
    }
    double F = 0.0;
    double g[WIDE_NY];

    if (MODE == MODE_F0 || MODE == MODE_NODE_F) {
        if (active) cone_eval_wide<0>(P.cone, node, n, nD, y, F, g, nullptr, 0);
        if (MODE == MODE_NODE_F) {
            if (active) {
                P.out_F[node] = F;
                if (P.out_Dz != nullptr)
                    for (int k = 0; k < nD; ++k) P.out_Dz[node + n * k] = y[k];
            }
            return;
        }
        double val = 0.0;
        if (active) {
            const double bar = barrier_f0(P, node, F);
            double lin = 0.0;
#pragma unroll
            for (int k = 0; k < WIDE_NY; ++k) lin += (k < nD) ? P.c[node + n * k] * y[k] : 0.0;
            val = bar + P.w[node] * lin;
        }
        __syncthreads();
        const double tot = block_sum_256(val, sh);
        if (tid == 0) P.out_partial[blockIdx.x] = tot;
        return;
    }
    if (MODE == MODE_NODE_SLACK) {
        if (active) P.out_F[node] = cone_slack<WIDE_NY, WIDE_W>(P.cone, node, n, y);
        return;
    }
    if (MODE == MODE_F1 || MODE == MODE_F01) {
        double val = 0.0;
        if (active) {
            double F0v = 0.0;
            if (MODE == MODE_F01) cone_eval_wide<0>(P.cone, node, n, nD, y, F0v, g, nullptr, 0);
            cone_eval_wide<1>(P.cone, node, n, nD, y, F, g, nullptr, 0);
            const double wv = P.w[node];
            const double bwv = P.bw ? P.bw[node] : 0.0;
            double lin = 0.0;
#pragma unroll
            for (int k = 0; k < WIDE_NY; ++k) {
                if (k >= nD) continue;
                const double ck = P.c[node + n * k];
                lin += ck * y[k];
                const double sc = P.bw ? ((bwv == 0.0) ? 0.0 : bwv * g[k]) : P.invn * g[k];
                YL[(el * nD + k) * G + r] = sc + wv * ck;
            }
            if (MODE == MODE_F01) {
                const double bar = P.bw ? ((bwv == 0.0) ? 0.0 : bwv * F0v) : P.invn * F0v;
                val = bar + wv * lin;
            }
        }
        __syncthreads();
        if (active) {
            const int i = r;
            for (int a = 0; a < nu; ++a) {
                double acc = 0.0;
                for (int k = 0; k < nD; ++k) {
                    if (P.D_state[k] != a) continue;
                    const double* Yk = YL + (el * nD + k) * G;
                    if (P.D_stage[k] == -1) {
                        acc += Yk[i];
                    } else {
                        for (int rr = 0; rr < p; ++rr) acc += OP(k, rr, i) * Yk[rr];
                    }
                }
                P.out_ret[(int64_t)a * n + node] = acc;
            }
        }
        if (MODE == MODE_F01) {
            __syncthreads();
            const double tot = block_sum_256(val, sh);
            if (tid == 0) P.out_partial[blockIdx.x] = tot;
        }
        return;
    }
    if (MODE == MODE_F2) {
        const int NT = nD * (nD + 1) / 2;
        double* Tn = YL + (size_t)el * NT * G + r;      // this node's triangle, stride G
        for (int t = 0; t < NT; ++t) Tn[(size_t)t * G] = 0.0;
        if (active) {
            cone_eval_wide<2>(P.cone, node, n, nD, y, F, g, Tn, G);
            const double bwv = P.bw ? P.bw[node] : 0.0;
            for (int t = 0; t < NT; ++t) {
                const double h = Tn[(size_t)t * G];
                Tn[(size_t)t * G] = scale_by(P, bwv, h);
            }
        }
        __syncthreads();
        if (active) {
            const int j = r;
            for (int a = 0; a < nu; ++a)
                for (int b = a; b < nu; ++b) {
                    const int blk = a * nu - (a * (a - 1)) / 2 + (b - a);
                    const bool dblk = (P.diag_mask >> blk) & 1;
                    double* out = P.out_hel + P.blk_off[blk] + (dblk ? (e * p + j) - j : (e * p + j) * (int64_t)p);
                    for (int i = dblk ? j : 0; i < (dblk ? j + 1 : p); ++i) {
                        double val = 0.0;
                        for (int k = 0; k < nD; ++k) {
                            if (P.D_state[k] != a) continue;
                            const bool idk = P.D_stage[k] == -1;
                            for (int k2 = 0; k2 < nD; ++k2) {
                                if (P.D_state[k2] != b) continue;
                                const bool idk2 = P.D_stage[k2] == -1;
                                const int t = (k <= k2) ? tri_index(k, k2, nD) : tri_index(k2, k, nD);
                                const double* Yt = YL + ((size_t)el * NT + t) * G;
                                if (idk && idk2) {
                                    val += (i == j) ? Yt[i] : 0.0;
                                } else if (idk) {
                                    val += Yt[i] * OP(k2, i, j);
                                } else if (idk2) {
                                    val += OP(k, j, i) * Yt[j];
                                } else {
                                    double acc = 0.0;
                                    for (int rr = 0; rr < p; ++rr) acc += OP(k, rr, i) * Yt[rr] * OP(k2, rr, j);
                                    val += acc;
                                }
                            }
                        }
                        out[i] = val;
                    }
                }
        }
        return;
    }
}

// Specialised element Hessian kernel for compile-time (NY, P): same arithmetic as MODE_F2 of the
// generic kernel, restructured so that lane j first forms C_k[r] = sum_k' Y_r[k,k'] D_k'[r,j] in
// registers and then out[i] = sum_k sum_r D_k[r,i] C_k[r]  (|K_a| * P * (|K_b| + P) multiply-adds
// per block instead of |K_a| |K_b| P^2), all loops unrolled, operators and Y in LDS, the
// finished blocks staged through LDS and written with a flat coalesced copy (the slab is
// block-major: [block][element][P*P]).
// D-table signatures.  SigRuntime reads the (state, operator slot) rows from the kernel
// arguments; SigDefault<NY> is the reference's default_D layout (src/mgb.jl:595-607)
//   [u id; u dx; (u dy; (u dz;)) s id]  with the default cone idx = 2:dim+2,
// i.e. rows 1..NY-1 enter the barrier, row 0 (u itself) does not.  With a compile-time
// signature every set-membership test below folds away and the block products shrink to the
// structurally non-zero terms.
struct SigRuntime {
    static constexpr bool rt = true;
    static __device__ __forceinline__ constexpr int state(int) { return 0; }
    static __device__ __forceinline__ constexpr int stage(int) { return 0; }
    static __device__ __forceinline__ constexpr int mask() { return 0; }
};
template <int NY>
struct SigDefault {
    static constexpr bool rt = false;
    static __device__ __forceinline__ constexpr int state(int k) { return k == NY - 1 ? 1 : 0; }
    static __device__ __forceinline__ constexpr int stage(int k) { return (k == 0 || k == NY - 1) ? -1 : k - 1; }
    static __device__ __forceinline__ constexpr int mask() { return ((1 << NY) - 1) & ~1; }
};

template <int NY, int P, class Sig, bool CONDENSE = false>
__global__ __launch_bounds__(256) void elem_f2_fast(const ElemParams Pm) {
    constexpr int G = elem_group(P);
    constexpr int EPB = 256 / G;
    constexpr int PP = P * P;
    constexpr int NT = NY * (NY + 1) / 2;
    extern __shared__ double sh[];
    const int tid = threadIdx.x;
    const int el = tid / G;
    const int r = tid % G;
    const int nu = Sig::rt ? Pm.nu : 2;
    auto DST = [&](int k) -> int { return Sig::rt ? Pm.D_state[k] : Sig::state(k); };
    auto DSG = [&](int k) -> int { return Sig::rt ? Pm.D_stage[k] : Sig::stage(k); };
    const int ymask = Sig::rt ? Pm.ymask : Sig::mask();
    const int64_t e0 = (int64_t)blockIdx.x * EPB;
    const int64_t e = e0 + el;
    const bool active = (e < Pm.N) && (r < P);
    const int64_t n = Pm.n;
    const int64_t node = e * P + r;

    double* zl = sh;                                    // [EPB][nu][G]
    double* opL = zl + elem_lds_z(256, nu);     // [nstage][EPB][PP]
    double* YL = opL + elem_lds_ops(Pm.nstage, EPB, PP);     // [EPB][NT][G]

    // z0 + R s of this lane's node: requested first (selection levels chain two loads: column, then s)
    double zr[MGBHIP_MAX_NU];
#pragma unroll
    for (int a = 0; a < MGBHIP_MAX_NU; ++a) zr[a] = (active && a < nu) ? z_at(Pm, (int64_t)a * n + node) : 0.0;
    {   // operator blocks of this workgroup's elements -> LDS.  All loads of a stage are issued before the first
        // LDS store (a rolled copy loop waits one memory latency per iteration)
        int64_t lim = (Pm.N - e0) * PP;
        if (lim > (int64_t)EPB * PP) lim = (int64_t)EPB * PP;
        constexpr int NIT = (EPB * PP + 255) / 256;
        for (int o = 0; o < Pm.nstage; ++o) {
            const double* src = Pm.stage_ptr[o] + e0 * PP;
            double* dst = opL + (size_t)o * EPB * PP;
            copy_unrolled<NIT>(src, dst, lim, tid);
        }
    }
    if (active) {
#pragma unroll
        for (int a = 0; a < MGBHIP_MAX_NU; ++a)
            if (a < nu) zl[(el * nu + a) * G + r] = zr[a];
    }
    __syncthreads();
    const double* opE = opL + (size_t)el * PP;           // + slot * EPB * PP
    auto OP = [&](int k, int rr, int cc) -> double { return opE[(size_t)DSG(k) * EPB * PP + cc * P + rr]; };

    double y[NY];
#pragma unroll
    for (int k = 0; k < NY; ++k) {
        double v = 0.0;
        if (active) {
            const double* za = zl + (el * nu + DST(k)) * G;
            if (DSG(k) < 0) v = za[r];
            else {
#pragma unroll
                for (int cc = 0; cc < P; ++cc) v += OP(k, r, cc) * za[cc];
            }
        }
        y[k] = v;
    }
    if (active) {
        double F, g[NY], H[NY * NY];
        cone_eval<NY, 2>(Pm.cone, node, n, y, F, g, H);
        const double bwv = Pm.bw ? Pm.bw[node] : 0.0;
#pragma unroll
        for (int k = 0; k < NY; ++k)
#pragma unroll
            for (int k2 = k; k2 < NY; ++k2) {
                const double h = H[k * NY + k2];
                YL[((size_t)el * NT + tri_index(k, k2, NY)) * G + r] = scale_by(Pm, bwv, h);
            }
    }
    __syncthreads();
    const int j = r;
    const double* Ye = YL + (size_t)el * NT * G;
    int blk = 0;
    double cblk[CONDENSE ? 3 : 1][P];      // CONDENSE: column j of the uu / us blocks and ss_j stay in registers
#pragma unroll
    for (int a = 0; a < nu; ++a)
#pragma unroll
        for (int b = a; b < nu; ++b, ++blk) {
            // lane j owns column j of the block: P contiguous doubles of the block-major slab; a wave
            // covers 64/G whole blocks, so every cache line is completed within the wave's stores
            const bool dblk = CONDENSE ? (blk == 2) : ((Pm.diag_mask >> blk) & 1);      // diagonal block, stored compactly
            double* dst = CONDENSE ? &cblk[blk < 3 ? blk : 0][0]
                                   : Pm.out_hel + Pm.blk_off[blk] + (dblk ? (e * P + j) : (e * P + j) * (int64_t)P);
            bool b_all_id = true;
#pragma unroll
            for (int k2 = 0; k2 < NY; ++k2)
                if (DST(k2) == b && ((ymask >> k2) & 1) && DSG(k2) >= 0) b_all_id = false;
            if (active && b_all_id) {
                // every operator of state b is the identity: C_k[r] = delta(r, j) * sum_k' Y_j[k,k']
                double Cd[NY];
#pragma unroll
                for (int k = 0; k < NY; ++k) {
                    double acc = 0.0;
                    if (DST(k) == a && ((ymask >> k) & 1)) {
#pragma unroll
                        for (int k2 = 0; k2 < NY; ++k2) {
                            if (DST(k2) != b || !((ymask >> k2) & 1)) continue;
                            const int t = (k <= k2) ? tri_index(k, k2, NY) : tri_index(k2, k, NY);
                            acc += Ye[t * G + j];
                        }
                    }
                    Cd[k] = acc;
                }
                if (dblk) {          // state a carries identity operators only as well
                    double val = 0.0;
#pragma unroll
                    for (int k = 0; k < NY; ++k)
                        if (DST(k) == a && ((ymask >> k) & 1)) val += Cd[k];
                    dst[0] = val;
                } else {
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        double val = 0.0;
#pragma unroll
                        for (int k = 0; k < NY; ++k) {
                            if (DST(k) != a || !((ymask >> k) & 1)) continue;
                            if (DSG(k) < 0) val += (i == j) ? Cd[k] : 0.0;
                            else val += OP(k, j, i) * Cd[k];
                        }
                        dst[i] = val;
                    }
                }
            } else if (active) {
                double C[NY][P];
#pragma unroll
                for (int k = 0; k < NY; ++k) {
                    if (DST(k) != a || !((ymask >> k) & 1)) continue;
#pragma unroll
                    for (int rr = 0; rr < P; ++rr) {
                        double acc = 0.0;
#pragma unroll
                        for (int k2 = 0; k2 < NY; ++k2) {
                            if (DST(k2) != b || !((ymask >> k2) & 1)) continue;
                            const int t = (k <= k2) ? tri_index(k, k2, NY) : tri_index(k2, k, NY);
                            const double yv = Ye[t * G + rr];
                            if (DSG(k2) < 0) acc += (rr == j) ? yv : 0.0;
                            else acc += yv * OP(k2, rr, j);
                        }
                        C[k][rr] = acc;
                    }
                }
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    double val = 0.0;
#pragma unroll
                    for (int k = 0; k < NY; ++k) {
                        if (DST(k) != a || !((ymask >> k) & 1)) continue;
                        if (DSG(k) < 0) val += C[k][i];
                        else {
#pragma unroll
                            for (int rr = 0; rr < P; ++rr) val += OP(k, rr, i) * C[k][rr];
                        }
                    }
                    dst[i] = val;
                }
            }
        }
    if constexpr (CONDENSE) {
        // ---- partial factorization of the element's leaf front (kernels.hpp: launch_elem_f2_condense) --------------
        // Leaf index list: [slack of node 0..P-1 | interior u node (element node P-1) | the other element nodes that
        // are unknowns, in the front's order | border].  Lane j holds uu(:, j), us(:, j) (u_i against slack j), ss_j.
        static_assert(!Sig::rt && P <= 8, "condensation: default two-state signature only");
        constexpr int PB = P - 1;                     // the interior node
        __syncthreads();                              // every lane is done with the staged operators: reuse their LDS
        double* X = opL + (size_t)el * (2 * PP);      // per-element scratch (nstage == 2: 2 * PP doubles per element)
        double* Xus = X;                              // [P][P]: Xus[q * P + i] = us(i, q)
        double* Xinv = X + PP;                        // [P] 1 / ss_q
        double* Xbeta = Xinv + P;                     // [P] border entries -g of the slacks
        double* Xc = Xbeta + P;                       // [P] uu'(:, PB) after the slack elimination
        double* Xs = Xc + P;                          // [0] border entry of the interior node after the slacks, [1] its pivot
        const double* uuc = cblk[0];
        const double* usc = cblk[1];
        const double ssj = cblk[2][0];
        LeafDesc ld{0, 0, 0};
        double inv = 0.0, beta = 0.0;
        bool bad = false;
        if (active) {
            ld = Pm.leaf_desc[e];
            beta = -Pm.leaf_g[Pm.leaf_slack0 + node];
            bad = (ssj == 0.0) || !isfinite(ssj);
            inv = 1.0 / ssj;
#pragma unroll
            for (int i = 0; i < P; ++i) Xus[j * P + i] = usc[i];
            Xinv[j] = inv;
            Xbeta[j] = beta;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double up[P];                                 // uu'(i, j) = uu(i, j) - sum_q us(i, q) us(j, q) / ss_q
        double bj = 0.0, corner = 0.0;
        if (active) {
            double t[P];
#pragma unroll
            for (int q = 0; q < P; ++q) t[q] = Xus[q * P + j] * Xinv[q];
#pragma unroll
            for (int i = 0; i < P; ++i) {
                double acc = uuc[i];
#pragma unroll
                for (int q = 0; q < P; ++q) acc -= Xus[q * P + i] * t[q];
                up[i] = acc;
            }
#pragma unroll
            for (int q = 0; q < P; ++q) bj -= Xbeta[q] * t[q];                 // border row entry of u_j after the slacks
            if (j == PB) {
                bj -= Pm.leaf_g[ld.interior];                                   // the interior node is a pivot of this leaf
#pragma unroll
                for (int q = 0; q < P; ++q) corner -= Xbeta[q] * Xbeta[q] * Xinv[q];
#pragma unroll
                for (int i = 0; i < P; ++i) Xc[i] = up[i];
                Xs[0] = bj;
                Xs[1] = up[PB];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            // The finished leaf front: square column-major (entry (r, c) at r + c*m) straight to the arena, or -- packed
            // leaves -- the lower triangle (column c at c*m - c(c-1)/2) staged in LDS and copied out in one coalesced
            // run of m(m+1)/2 doubles per element.
            const int m = (int)(ld.packed & 15u);
            const bool pk = Pm.leaf_packed != 0;
            int pos[P];
#pragma unroll
            for (int i = 0; i < P; ++i) pos[i] = (int)((ld.packed >> (4 + 4 * i)) & 15u);
            double d7 = 1.0, bb = 0.0, inv7 = 1.0, f = 0.0, xc[P];
#pragma unroll
            for (int i = 0; i < P; ++i) xc[i] = 0.0;
            if (active) {
                d7 = Xs[1];
                bb = Xs[0];
                inv7 = 1.0 / d7;
#pragma unroll
                for (int i = 0; i < P; ++i) xc[i] = Xc[i];
                f = (j < PB) ? xc[j] * inv7 : 0.0;
                bad = bad || (j == PB && ((d7 == 0.0) || !isfinite(d7)));
            }
            double* Fg = Pm.leaf_arena + ld.F_off;
            double* S = Fg;                               // destination of the scattered writes
            if (pk) {
                __syncthreads();                          // every lane has read its scratch: the staging area may overlap it
                S = sh + (size_t)el * 120;
            }
            auto at = [&](int rr, int cc) -> int { return pk ? cc * m - (cc * (cc - 1)) / 2 + (rr - cc) : rr + cc * m; };
            if (active) {
                // slack column j: pivot, zeros against the later slacks, the u rows, the border row
                S[at(j, j)] = ssj;
#pragma unroll
                for (int rr = 0; rr < P; ++rr)
                    if (rr > j) S[at(rr, j)] = 0.0;
                S[at(P, j)] = usc[PB] * inv;
#pragma unroll
                for (int i = 0; i < PB; ++i)
                    if (pos[i] != 15) S[at(pos[i], j)] = usc[i] * inv;
                S[at(m - 1, j)] = beta * inv;
                if (j == PB) {                             // column of the interior node
                    S[at(P, P)] = d7;
#pragma unroll
                    for (int i = 0; i < PB; ++i)
                        if (pos[i] != 15) S[at(pos[i], P)] = xc[i] * inv7;
                    S[at(m - 1, P)] = bb * inv7;
                    S[at(m - 1, m - 1)] = corner - bb * bb * inv7;
                } else if (pos[j] != 15) {                 // update column of element node j
#pragma unroll
                    for (int i = 0; i < PB; ++i)
                        if (pos[i] != 15 && pos[i] >= pos[j]) S[at(pos[i], pos[j])] = up[i] - xc[i] * f;
                    S[at(m - 1, pos[j])] = bj - bb * f;
                }
            }
            if (pk) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (e < Pm.N) {
                    const LeafDesc l2 = Pm.leaf_desc[e];       // lane G-1 of the group takes part in the copy
                    const int mm = (int)(l2.packed & 15u);
                    double* dstF = Pm.leaf_arena + l2.F_off;
                    for (int t = r; t < mm * (mm + 1) / 2; t += G) dstF[t] = S[t];
                }
            }
        }
        if (bad) atomicOr(Pm.leaf_status, 1);
    }
}

// Specialised line-search trial (MODE_F01 of the generic kernel: value and gradient at one point from one
// pass over the operator blocks) for compile-time (NY, P) and D-table signature: every loop unrolled, the
// set-membership tests of the D table folded away.  Same arithmetic, same summation order.
template <int NY, int P, class Sig>
__global__ __launch_bounds__(256) void elem_f01_fast(const ElemParams Pm) {
    constexpr int G = elem_group(P);
    constexpr int EPB = 256 / G;
    constexpr int PP = P * P;
    extern __shared__ double sh[];
    const int tid = threadIdx.x;
    const int el = tid / G;
    const int r = tid % G;
    const int nu = Sig::rt ? Pm.nu : 2;
    auto DST = [&](int k) -> int { return Sig::rt ? Pm.D_state[k] : Sig::state(k); };
    auto DSG = [&](int k) -> int { return Sig::rt ? Pm.D_stage[k] : Sig::stage(k); };
    const int64_t e0 = (int64_t)blockIdx.x * EPB;
    const int64_t e = e0 + el;
    const bool active = (e < Pm.N) && (r < P);
    const int64_t n = Pm.n;
    const int64_t node = e * P + r;

    double* zl = sh;                                    // [EPB][nu][G]
    double* opL = zl + elem_lds_z(256, nu);     // [nstage][EPB][PP]
    double* YL = opL + elem_lds_ops(Pm.nstage, EPB, PP);     // [EPB][NY][G]
    {   // operator blocks of this workgroup's elements -> LDS.  All loads of a stage are issued before the first
        // LDS store (a rolled copy loop waits one memory latency per iteration)
        int64_t lim = (Pm.N - e0) * PP;
        if (lim > (int64_t)EPB * PP) lim = (int64_t)EPB * PP;
        constexpr int NIT = (EPB * PP + 255) / 256;
        for (int o = 0; o < Pm.nstage; ++o) {
            const double* src = Pm.stage_ptr[o] + e0 * PP;
            double* dst = opL + (size_t)o * EPB * PP;
            copy_unrolled<NIT>(src, dst, lim, tid);
        }
    }
    // the node's cost row and weights do not depend on anything staged: request them with the operators
    double ck[NY];
    double wv = 0.0, bwv = 0.0;
    if (active) {
        for (int a = 0; a < nu; ++a) zl[(el * nu + a) * G + r] = z_at(Pm, (int64_t)a * n + node);
#pragma unroll
        for (int k = 0; k < NY; ++k) ck[k] = Pm.c[node + n * k];
        wv = Pm.w[node];
        bwv = Pm.bw ? Pm.bw[node] : 0.0;
    }
    __syncthreads();
    const double* opE = opL + (size_t)el * PP;
    auto OP = [&](int k, int rr, int cc) -> double { return opE[(size_t)DSG(k) * EPB * PP + cc * P + rr]; };
    double y[NY];
#pragma unroll
    for (int k = 0; k < NY; ++k) {
        double v = 0.0;
        if (active) {
            const double* za = zl + (el * nu + DST(k)) * G;
            if (DSG(k) < 0) v = za[r];
            else {
#pragma unroll
                for (int cc = 0; cc < P; ++cc) v += OP(k, r, cc) * za[cc];
            }
        }
        y[k] = v;
    }
    double val = 0.0;
    if (active) {
        double F0v, F, g[NY], H[NY * NY];
        cone_eval<NY, 0>(Pm.cone, node, n, y, F0v, g, H);
        cone_eval<NY, 1>(Pm.cone, node, n, y, F, g, H);
        const double bar = Pm.bw ? ((bwv == 0.0) ? 0.0 : bwv * F0v) : Pm.invn * F0v;
        double lin = 0.0;
#pragma unroll
        for (int k = 0; k < NY; ++k) {
            lin += ck[k] * y[k];
            const double sc = Pm.bw ? ((bwv == 0.0) ? 0.0 : bwv * g[k]) : Pm.invn * g[k];
            YL[(el * NY + k) * G + r] = sc + wv * ck[k];
        }
        val = bar + wv * lin;
    }
    __syncthreads();
    if (active) {
        const int i = r;
        for (int a = 0; a < nu; ++a) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < NY; ++k) {
                if (DST(k) != a) continue;
                const double* Yk = YL + (el * NY + k) * G;
                if (DSG(k) < 0) {
                    acc += Yk[i];
                } else {
#pragma unroll
                    for (int rr = 0; rr < P; ++rr) acc += OP(k, rr, i) * Yk[rr];
                }
            }
            Pm.out_ret[(int64_t)a * n + node] = acc;
        }
    }
    __syncthreads();            // operators / Y no longer needed: reuse LDS for the reduction
    const double tot = block_sum_256(val, sh);
    if (tid == 0) Pm.out_partial[blockIdx.x] = tot;
}

// Opt-in to more than 64 KB of dynamic LDS, up to the launch cap.
template <class K>
void allow_big_lds(K kernel) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ELEM_LDS_MAX);
}

}  // namespace

int64_t elem_grid(int p, int64_t N) {
    if (p > 64) return dense_grid((int64_t)p * N);
    const int epb = 256 / elem_group(p);
    return (N + epb - 1) / epb;
}

// The fast kernels of entry I of ELEM_FAST_TABLE for one mode: KD / KR are the default- and the runtime-signature
// instantiation.  Launches when the plan names this entry.
template <int I, auto KD, auto KR>
static bool launch_fast_entry(const ElemParams& P, const ElemPlan& plan, hipStream_t st) {
    if (plan.NY != ELEM_FAST_TABLE[I][0] || plan.P != ELEM_FAST_TABLE[I][1]) return false;
    static bool attr = [] {
        allow_big_lds(KR);
        allow_big_lds(KD);
        (void)hipGetLastError();
        return true;
    }();
    (void)attr;
    hipLaunchKernelGGL(plan.kind == ELEM_FAST_DEFAULT ? KD : KR, dim3((unsigned)plan.grid), dim3((unsigned)plan.threads), plan.lds, st, P);
    return true;
}
template <int I>
static bool launch_f2_fast_entry(const ElemParams& P, const ElemPlan& plan, hipStream_t st) {
    constexpr int NY = ELEM_FAST_TABLE[I][0], PN = ELEM_FAST_TABLE[I][1];
    return launch_fast_entry<I, &elem_f2_fast<NY, PN, SigDefault<NY>>, &elem_f2_fast<NY, PN, SigRuntime>>(P, plan, st);
}
template <int I>
static bool launch_f01_fast_entry(const ElemParams& P, const ElemPlan& plan, hipStream_t st) {
    constexpr int NY = ELEM_FAST_TABLE[I][0], PN = ELEM_FAST_TABLE[I][1];
    return launch_fast_entry<I, &elem_f01_fast<NY, PN, SigDefault<NY>>, &elem_f01_fast<NY, PN, SigRuntime>>(P, plan, st);
}
template <int... I>
static bool launch_fast(const ElemParams& P, int mode, const ElemPlan& plan, hipStream_t st, std::integer_sequence<int, I...>) {
    return mode == MODE_F2 ? (launch_f2_fast_entry<I>(P, plan, st) || ...) : (launch_f01_fast_entry<I>(P, plan, st) || ...);
}

bool launch_elem_f2_condense(const ElemParams& P, hipStream_t st) {
    // fem2d_P2 with bubble, default D table: 7 nodes per element, node 6 interior (the only family specialised so far)
    constexpr int NY = ELEM_CONDENSE_NY, PN = ELEM_CONDENSE_P;
    const ElemPlan plan = elem_plan_of(P, MODE_F2, true);
    if (plan.kind != ELEM_CONDENSE) return false;
    MGB_REQUIRE(P.leaf_desc && P.leaf_arena && P.leaf_g && P.leaf_status, "condensing f2: leaf arguments missing");
    static bool attr = [] {
        allow_big_lds(elem_f2_fast<NY, PN, SigDefault<NY>, true>);
        (void)hipGetLastError();
        return true;
    }();
    (void)attr;
    hipLaunchKernelGGL((elem_f2_fast<NY, PN, SigDefault<NY>, true>), dim3((unsigned)plan.grid), dim3((unsigned)plan.threads), plan.lds, st, P);
    MGB_HIP_CHECK(hipGetLastError());
    return true;
}

// Generic kernels, narrow and wide: kernel_of(M) is the MODE instantiation of the kernel template for
// M = std::integral_constant<int, MODE_*> -- the one list of modes serves the launch and the LDS opt-in.
template <class K>
static void launch_elem_generic(const ElemParams& P, int mode, const ElemPlan& plan, K kernel_of, hipStream_t st) {
    static std::once_flag once;
    std::call_once(once, [&] {
        for (int m = MODE_F0; m <= MODE_F01; ++m) dispatch_mode(m, [&](auto M) { allow_big_lds(kernel_of(M)); });
        (void)hipGetLastError();
    });
    int lgG = 0;
    while ((1 << lgG) < plan.G) ++lgG;
    const dim3 grid((unsigned)plan.grid), blk((unsigned)plan.threads);
    const size_t lds = plan.lds;
    MGB_REQUIRE(lds <= ELEM_LDS_MAX, "element kernel LDS budget exceeded");
    if (!dispatch_mode(mode, [&](auto M) { hipLaunchKernelGGL(kernel_of(M), grid, blk, lds, st, P, lgG); }))
        throw InvalidArgument("launch_elem: bad mode");
    MGB_HIP_CHECK(hipGetLastError());
}
template <int NY>
static void launch_elem_ny(const ElemParams& P, int mode, const ElemPlan& plan, hipStream_t st) {
    launch_elem_generic(P, mode, plan, [](auto M) { return &elem_kernel<NY, decltype(M)::value>; }, st);
}

void launch_elem(const ElemParams& P, int mode, hipStream_t st) {
    const ElemPlan plan = elem_plan_of(P, mode, false);
    if (plan.kind == ELEM_DENSE) {      // one dense spectral element: GEMV + node kernel path (dense.hip)
        launch_dense_eval(P, mode, st);
        return;
    }
    MGB_REQUIRE(P.p >= 1 && P.p <= 64, "element kernels support 1 <= p <= 64 nodes per element");
    MGB_REQUIRE(P.nD >= 1 && P.nD <= MGBHIP_MAX_ND, "nD out of range");
    if (plan.kind == ELEM_WIDE) {
        launch_elem_generic(P, mode, plan, [](auto M) { return &elem_wide_kernel<decltype(M)::value>; }, st);
        return;
    }
    MGB_REQUIRE(P.nD <= 10, "narrow element kernels: nD out of range");
    if (plan.kind == ELEM_FAST_DEFAULT || plan.kind == ELEM_FAST_RUNTIME) {
        // compile-time specialisations (elem_layout.hpp: ELEM_FAST_TABLE)
        const bool launched = launch_fast(P, mode, plan, st, std::make_integer_sequence<int, ELEM_FAST_COUNT>{});
        MGB_REQUIRE(launched, "launch_elem: no fast kernel for the planned (NY, P)");
        MGB_HIP_CHECK(hipGetLastError());
        return;
    }
    switch (plan.NY) {
        case 1: launch_elem_ny<1>(P, mode, plan, st); break;
        case 2: launch_elem_ny<2>(P, mode, plan, st); break;
        case 3: launch_elem_ny<3>(P, mode, plan, st); break;
        case 4: launch_elem_ny<4>(P, mode, plan, st); break;
        case 5: launch_elem_ny<5>(P, mode, plan, st); break;
        case 6: launch_elem_ny<6>(P, mode, plan, st); break;
        case 7: launch_elem_ny<7>(P, mode, plan, st); break;
        case 8: launch_elem_ny<8>(P, mode, plan, st); break;
        case 9: launch_elem_ny<9>(P, mode, plan, st); break;
        case 10: launch_elem_ny<10>(P, mode, plan, st); break;
    }
}

}  // namespace mgbhip
