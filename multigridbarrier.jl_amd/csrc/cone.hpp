// cone.hpp -- per-node barrier functors on the device.
//
// The reference compiles arbitrary Julia functors into its map_rows kernel
// (ext/MultiGridBarrierCUDAExt/map_rows_gpu.jl:20-28); a C-ABI backend enumerates the
// functor families instead: Euclidean-power cones
// (src/convex_euclidian_power.jl:71-253, :387-433), linear inequalities
// (src/convex_linear.jl:119-214), their piecewise sums (src/convex_piecewise.jl:15-75)
// and the phase-I wrapper (src/mgb.jl:217-287).  Everything is evaluated in registers:
// index scatters are written as compile-time-unrolled selects so that no array is
// dynamically indexed (no scratch memory).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mgbhip.h"

namespace mgbhip {

struct PieceDev {
    int32_t kind, ni, nc;
    int32_t idx[MGBHIP_MAX_IDX];
    const double* A;
    const double* b;
    const double* p;
    const double* mu;
    const double* select;
    double p_const, mu_const;
};

struct ConeDev {
    int32_t npieces;
    int32_t feasibility;
    int32_t NC;
    double box_b, box_R;
    PieceDev pc[MGBHIP_MAX_PIECES];
};

// Piece width of the register-resident functors below: every kernel that existed before the wide path instantiates them
// at this width (cone_eval<NY, ORDER> with the default W).  Wider Euclidean-power pieces (up to MGBHIP_MAX_IDX) and D
// tables of more than 10 rows take the wide path (cone_eval_wide below).
constexpr int NARROW_W = 4;
constexpr int WIDE_W = MGBHIP_MAX_IDX;
constexpr int WIDE_NY = MGBHIP_MAX_ND;
static_assert(MGBHIP_MAX_LIN <= NARROW_W, "linear pieces must fit the narrow functors");

// "Convex programmer's log" (src/utils.jl:14): -Inf off the domain instead of a throw.
__device__ __forceinline__ double mgb_Log(double x) { return x <= 0.0 ? -INFINITY : log(x); }
// src/convex_linear.jl:388-390
__device__ __forceinline__ double mgb_safe_pow(double s, double a) { return exp(a * mgb_Log(s)); }

// select y[i] for a runtime i without dynamic register indexing
template <int NY>
__device__ __forceinline__ double pick(const double (&y)[NY], int i) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < NY; ++j) v = (i == j) ? y[j] : v;
    return v;
}

// Accumulate one piece's barrier (or cobarrier when slack_pos >= 0: y[slack_pos] is the
// slack, added to s for EP and to every row for LINEAR) into F / g / H.
// ORDER: 0 value, 1 gradient, 2 Hessian.  H is row-major NY x NY (symmetric anyway).
template <int NY, int ORDER, int W = NARROW_W>
__device__ __forceinline__ void piece_accumulate(const PieceDev& P, int64_t node, int64_t n,
                                                 const double (&y)[NY], int slack_pos, double& F,
                                                 double (&g)[NY], double (&H)[NY * NY]) {
    constexpr int MI = W;
    const int ni = P.ni;
    double yk[MI];
#pragma unroll
    for (int c = 0; c < MI; ++c) yk[c] = (c < ni) ? pick<NY>(y, P.idx[c]) : 0.0;
    const double slack = (slack_pos >= 0) ? pick<NY>(y, slack_pos) : 0.0;

    // local gradient / Hessian in the idx coordinates (+ slack row/col)
    double gl[MI], Hl[MI * MI], cross[MI];
    double g_sl = 0.0, H_sl = 0.0;
#pragma unroll
    for (int i = 0; i < MI; ++i) { gl[i] = 0.0; cross[i] = 0.0; }
#pragma unroll
    for (int i = 0; i < MI * MI; ++i) Hl[i] = 0.0;

    if (P.kind == MGBHIP_KIND_EP) {
        const int nz = ni;
        // z = A yk + b ; A column-major nz x nz per node (NULL = identity)
        double z[MI];
        double Am[MI * MI];
        const bool hasA = P.A != nullptr;
#pragma unroll
        for (int r = 0; r < MI; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < MI; ++c) {
                double a = 0.0;
                if (r < nz && c < nz) a = hasA ? P.A[node + n * (int64_t)(r + nz * c)] : (r == c ? 1.0 : 0.0);
                Am[r + MI * c] = a;
                acc += a * yk[c];
            }
            z[r] = acc + ((P.b != nullptr && r < nz) ? P.b[node + n * (int64_t)r] : 0.0);
        }
        const double p0 = P.p ? P.p[node] : P.p_const;
        const double mu = P.mu ? P.mu[node] : P.mu_const;
        double qsq = 0.0;
#pragma unroll
        for (int r = 0; r < MI; ++r) qsq += (r < nz - 1) ? z[r] * z[r] : 0.0;
        const double s = pick<MI>(z, nz - 1) + slack;
        const double alpha = 2.0 / p0;
        const double s_a = mgb_safe_pow(s, alpha);
        const double rr = s_a - qsq;
        if (ORDER == 0) {
            F += -mgb_Log(rr) - mu * mgb_Log(s);
            return;
        }
        const double inv_r = 1.0 / rr;
        const double s_am1 = mgb_safe_pow(s, alpha - 1.0);
        double gz[MI], Hz[MI * MI];
        if (ORDER == 1) {
#pragma unroll
            for (int r = 0; r < MI; ++r)
                gz[r] = (r < nz - 1) ? 2.0 * inv_r * z[r] : ((r == nz - 1) ? (-alpha * s_am1 * inv_r - mu / s) : 0.0);
            // g_idx = A' gz
#pragma unroll
            for (int c = 0; c < MI; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int r = 0; r < MI; ++r) acc += Am[r + MI * c] * gz[r];
                gl[c] = acc;
            }
            g_sl = pick<MI>(gz, nz - 1);
        } else {
            const double inv_r2 = inv_r * inv_r;
            const double coef_qs = -2.0 * alpha * s_am1 * inv_r2;
            const double s_am2 = mgb_safe_pow(s, alpha - 2.0);
            const double s_2am2 = mgb_safe_pow(s, 2.0 * alpha - 2.0);
            const double H_ss = -alpha * (alpha - 1.0) * s_am2 * inv_r + alpha * alpha * s_2am2 * inv_r2 + mu / (s * s);
#pragma unroll
            for (int j = 0; j < MI; ++j)
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    double v = 0.0;
                    const bool iq = i < nz - 1, jq = j < nz - 1;
                    const bool is = i == nz - 1, js = j == nz - 1;
                    if (iq && jq) v = 4.0 * z[i] * z[j] * inv_r2 + (i == j ? 2.0 * inv_r : 0.0);
                    else if (iq && js) v = coef_qs * z[i];
                    else if (is && jq) v = coef_qs * z[j];
                    else if (is && js) v = H_ss;
                    Hz[i + MI * j] = v;
                }
            // Hl = A' Hz A ; cross = A' Hz[:, nz-1] ; H_sl = Hz[nz-1, nz-1]
            double T[MI * MI];   // T = Hz A
#pragma unroll
            for (int c = 0; c < MI; ++c)
#pragma unroll
                for (int r = 0; r < MI; ++r) {
                    double acc = 0.0;
#pragma unroll
                    for (int q = 0; q < MI; ++q) acc += Hz[r + MI * q] * Am[q + MI * c];
                    T[r + MI * c] = acc;
                }
#pragma unroll
            for (int c = 0; c < MI; ++c)
#pragma unroll
                for (int r = 0; r < MI; ++r) {
                    double acc = 0.0;
#pragma unroll
                    for (int q = 0; q < MI; ++q) acc += Am[q + MI * r] * T[q + MI * c];
                    Hl[r + MI * c] = acc;
                }
            double hcol[MI];
#pragma unroll
            for (int r = 0; r < MI; ++r) {
                double v = 0.0;
#pragma unroll
                for (int q = 0; q < MI; ++q) v = (q == nz - 1) ? Hz[r + MI * q] : v;
                hcol[r] = v;
            }
#pragma unroll
            for (int c = 0; c < MI; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int r = 0; r < MI; ++r) acc += Am[r + MI * c] * hcol[r];
                cross[c] = acc;
            }
            H_sl = H_ss;
        }
    } else {
        // linear inequalities: Fv = A yk + b (+ slack); A column-major nc x ni per node
        const int nc = P.nc;
        constexpr int MC = MGBHIP_MAX_LIN;
        double Am[MC * MI], Fv[MC];
        const bool hasA = P.A != nullptr;
#pragma unroll
        for (int r = 0; r < MC; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < MI; ++c) {
                double a = 0.0;
                if (r < nc && c < ni) a = hasA ? P.A[node + n * (int64_t)(r + nc * c)] : (r == c ? 1.0 : 0.0);
                Am[r + MC * c] = a;
                acc += a * yk[c];
            }
            Fv[r] = acc + ((P.b != nullptr && r < nc) ? P.b[node + n * (int64_t)r] : 0.0) + slack;
        }
        if (ORDER == 0) {
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < MC; ++r) acc += (r < nc) ? mgb_Log(Fv[r]) : 0.0;
            F += -acc;
            return;
        }
        if (ORDER == 1) {
            double invF[MC];
#pragma unroll
            for (int r = 0; r < MC; ++r) invF[r] = (r < nc) ? 1.0 / Fv[r] : 0.0;
#pragma unroll
            for (int c = 0; c < MI; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int r = 0; r < MC; ++r) acc += Am[r + MC * c] * invF[r];
                gl[c] = -acc;
            }
#pragma unroll
            for (int r = 0; r < MC; ++r) g_sl -= invF[r];
        } else {
            double invF2[MC];
#pragma unroll
            for (int r = 0; r < MC; ++r) invF2[r] = (r < nc) ? 1.0 / (Fv[r] * Fv[r]) : 0.0;
#pragma unroll
            for (int c = 0; c < MI; ++c)
#pragma unroll
                for (int a = 0; a < MI; ++a) {
                    double acc = 0.0;
#pragma unroll
                    for (int r = 0; r < MC; ++r) acc += Am[r + MC * a] * invF2[r] * Am[r + MC * c];
                    Hl[a + MI * c] = acc;
                }
#pragma unroll
            for (int c = 0; c < MI; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int r = 0; r < MC; ++r) acc += Am[r + MC * c] * invF2[r];
                cross[c] = acc;
            }
#pragma unroll
            for (int r = 0; r < MC; ++r) H_sl += invF2[r];
        }
    }

    // scatter into the y layout (src/convex_linear.jl:237-366)
    if (ORDER == 1) {
#pragma unroll
        for (int i = 0; i < NY; ++i) {
            double add = 0.0;
#pragma unroll
            for (int c = 0; c < MI; ++c) add = (c < ni && P.idx[c] == i) ? gl[c] : add;
            if (i == slack_pos) add = g_sl;
            g[i] += add;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NY; ++i) {
            int ki = -1;
#pragma unroll
            for (int c = 0; c < MI; ++c) ki = (c < ni && P.idx[c] == i) ? c : ki;
#pragma unroll
            for (int j = 0; j < NY; ++j) {
                int kj = -1;
#pragma unroll
                for (int c = 0; c < MI; ++c) kj = (c < ni && P.idx[c] == j) ? c : kj;
                double add = 0.0;
                if (i == slack_pos && j == slack_pos) add = H_sl;
                else if (i == slack_pos && kj >= 0) add = pick<MI>(cross, kj);
                else if (j == slack_pos && ki >= 0) add = pick<MI>(cross, ki);
                else if (ki >= 0 && kj >= 0) {
                    double v = 0.0;
#pragma unroll
                    for (int q = 0; q < MI * MI; ++q) v = (q == ki + MI * kj) ? Hl[q] : v;
                    add = v;
                }
                H[i * NY + j] += add;
            }
        }
    }
}

// Fast path of the most common Convex: a single Euclidean-power piece with A = I, b = 0, no
// select grid (the reference's default p-Laplace cone, src/mgb.jl:722).  Same formulas as
// core_grad / core_hess (src/convex_euclidian_power.jl:387-433) with the four powers of s
// derived from one exp/log pair: s^(a-1) = s^a / s, s^(a-2) = s^a / s^2, s^(2a-2) = (s^a / s)^2.
template <int NY, int ORDER, int W = NARROW_W>
__device__ __forceinline__ void ep_identity_eval(const PieceDev& P, int64_t node, const double (&y)[NY],
                                                 double& F, double (&g)[NY], double (&H)[NY * NY]) {
    constexpr int MI = W;
    const int nz = P.ni;
    double z[MI];
#pragma unroll
    for (int c = 0; c < MI; ++c) z[c] = (c < nz) ? pick<NY>(y, P.idx[c]) : 0.0;
    const double p0 = P.p ? P.p[node] : P.p_const;
    const double mu = P.mu ? P.mu[node] : P.mu_const;
    double qsq = 0.0;
#pragma unroll
    for (int c = 0; c < MI; ++c) qsq += (c < nz - 1) ? z[c] * z[c] : 0.0;
    const double s = pick<MI>(z, nz - 1);
    const double alpha = 2.0 / p0;
    const double ls = mgb_Log(s);
    const double s_a = exp(alpha * ls);
    const double rr = s_a - qsq;
    if (ORDER == 0) {
        F = -mgb_Log(rr) - mu * ls;
        return;
    }
    const double inv_r = 1.0 / rr;
    const double inv_s = 1.0 / s;
    const double s_am1 = s_a * inv_s;
    double gz[MI], Hz[MI * MI];
    if (ORDER == 1) {
#pragma unroll
        for (int c = 0; c < MI; ++c)
            gz[c] = (c < nz - 1) ? 2.0 * inv_r * z[c] : ((c == nz - 1) ? (-alpha * s_am1 * inv_r - mu * inv_s) : 0.0);
#pragma unroll
        for (int i = 0; i < NY; ++i) {
            double add = 0.0;
#pragma unroll
            for (int c = 0; c < MI; ++c) add = (c < nz && P.idx[c] == i) ? gz[c] : add;
            g[i] = add;
        }
        return;
    }
    const double inv_r2 = inv_r * inv_r;
    const double coef_qs = -2.0 * alpha * s_am1 * inv_r2;
    const double s_am2 = s_am1 * inv_s;
    const double H_ss = -alpha * (alpha - 1.0) * s_am2 * inv_r + alpha * alpha * (s_am1 * s_am1) * inv_r2 + mu * inv_s * inv_s;
#pragma unroll
    for (int j = 0; j < MI; ++j)
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            double v = 0.0;
            const bool iq = i < nz - 1, jq = j < nz - 1;
            const bool is = i == nz - 1, js = j == nz - 1;
            if (iq && jq) v = 4.0 * z[i] * z[j] * inv_r2 + (i == j ? 2.0 * inv_r : 0.0);
            else if (iq && js) v = coef_qs * z[i];
            else if (is && jq) v = coef_qs * z[j];
            else if (is && js) v = H_ss;
            Hz[i + MI * j] = v;
        }
#pragma unroll
    for (int i = 0; i < NY; ++i) {
        int ki = -1;
#pragma unroll
        for (int c = 0; c < MI; ++c) ki = (c < nz && P.idx[c] == i) ? c : ki;
#pragma unroll
        for (int j = 0; j < NY; ++j) {
            int kj = -1;
#pragma unroll
            for (int c = 0; c < MI; ++c) kj = (c < nz && P.idx[c] == j) ? c : kj;
            double v = 0.0;
            if (ki >= 0 && kj >= 0) {
#pragma unroll
                for (int q = 0; q < MI * MI; ++q) v = (q == ki + MI * kj) ? Hz[q] : v;
            }
            H[i * NY + j] = v;
        }
    }
}

// Full node barrier: value F, gradient g, Hessian H for the Convex or its phase-I wrapper.
template <int NY, int ORDER, int W = NARROW_W>
__device__ __forceinline__ void cone_eval(const ConeDev& C, int64_t node, int64_t n, const double (&y)[NY],
                                          double& F, double (&g)[NY], double (&H)[NY * NY]) {
    if (C.npieces == 1 && !C.feasibility && C.pc[0].kind == MGBHIP_KIND_EP && C.pc[0].A == nullptr &&
        C.pc[0].b == nullptr && C.pc[0].select == nullptr) {
        ep_identity_eval<NY, ORDER, W>(C.pc[0], node, y, F, g, H);
        return;
    }
    F = 0.0;
    if (ORDER == 1) {
#pragma unroll
        for (int i = 0; i < NY; ++i) g[i] = 0.0;
    }
    if (ORDER == 2) {
#pragma unroll
        for (int i = 0; i < NY * NY; ++i) H[i] = 0.0;
    }
    const int slack_pos = C.feasibility ? C.NC - 1 : -1;
    for (int k = 0; k < C.npieces; ++k) {
        const PieceDev& P = C.pc[k];
        if (P.select != nullptr && P.select[node] == 0.0) continue;   // exact zero, never 0 * Inf
        piece_accumulate<NY, ORDER, W>(P, node, n, y, slack_pos, F, g, H);
    }
    if (C.feasibility) {
        const int NC = C.NC;
        const double bb = C.box_b, RR = C.box_R;
        const double u = pick<NY>(y, NC - 1);
        if (ORDER == 0) {
            F += -mgb_Log(bb - u) - mgb_Log(bb + u);
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < NY; ++i) acc += (i >= NC) ? (-mgb_Log(RR - y[i]) - mgb_Log(RR + y[i])) : 0.0;
            F += acc;
        } else if (ORDER == 1) {
#pragma unroll
            for (int i = 0; i < NY; ++i) {
                if (i == NC - 1) g[i] += 1.0 / (bb - u) - 1.0 / (bb + u);
                else if (i >= NC) g[i] = 1.0 / (RR - y[i]) - 1.0 / (RR + y[i]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NY; ++i) {
                if (i == NC - 1) H[i * NY + i] += 1.0 / ((bb - u) * (bb - u)) + 1.0 / ((bb + u) * (bb + u));
                else if (i >= NC) H[i * NY + i] = 1.0 / ((RR - y[i]) * (RR - y[i])) + 1.0 / ((RR + y[i]) * (RR + y[i]));
            }
        }
    }
}

// Slack initialiser (src/convex_euclidian_power.jl:243-253, src/convex_linear.jl:205-214,
// src/convex_piecewise.jl:62-75): max over active pieces.
template <int NY, int W = NARROW_W>
__device__ __forceinline__ double cone_slack(const ConeDev& C, int64_t node, int64_t n, const double (&y)[NY]) {
    constexpr int MI = W;
    double out = -INFINITY;
    bool any = false;
    for (int k = 0; k < C.npieces; ++k) {
        const PieceDev& P = C.pc[k];
        if (P.select != nullptr && P.select[node] == 0.0) continue;
        const int ni = P.ni;
        double yk[MI];
#pragma unroll
        for (int c = 0; c < MI; ++c) yk[c] = (c < ni) ? pick<NY>(y, P.idx[c]) : 0.0;
        double val;
        const int nr = (P.kind == MGBHIP_KIND_EP) ? ni : P.nc;
        double z[MI];
#pragma unroll
        for (int r = 0; r < MI; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < MI; ++c) {
                double a = 0.0;
                if (r < nr && c < ni) a = P.A ? P.A[node + n * (int64_t)(r + nr * c)] : (r == c ? 1.0 : 0.0);
                acc += a * yk[c];
            }
            z[r] = acc + ((P.b != nullptr && r < nr) ? P.b[node + n * (int64_t)r] : 0.0);
        }
        if (P.kind == MGBHIP_KIND_EP) {
            const double p0 = P.p ? P.p[node] : P.p_const;
            double qsq = 0.0;
#pragma unroll
            for (int r = 0; r < MI; ++r) qsq += (r < ni - 1) ? z[r] * z[r] : 0.0;
            const double s = pick<MI>(z, ni - 1);
            val = -fmin(s - mgb_safe_pow(qsq, p0 / 2.0), s);
        } else {
            double mn = INFINITY;
#pragma unroll
            for (int r = 0; r < MI; ++r) mn = (r < nr) ? fmin(mn, z[r]) : mn;
            val = -mn;
        }
        out = any ? fmax(out, val) : val;
        any = true;
    }
    return out;
}

// ---- wide path ------------------------------------------------------------------------------------------------------
// Problems with more than 10 D rows or a Euclidean-power piece wider than NARROW_W (the vector-valued Zoo problems:
// nz = d^2 + 1, nD = d (1 + d) + 1) are evaluated here.  The node Hessian is never held in registers: for a power cone
// in the coordinates z = A y[idx] + b = (q, s) it is a scaled projector plus rank-two terms,
//     A' H_z A = (2/r) A_q'A_q + (4/r^2) v v' + c_qs (v a_s' + a_s v') + H_ss a_s a_s',   v = A_q' q,  a_s = last row of A,
// so every entry of the upper triangle is formed from O(nz) values and added straight into a triangle the caller owns
// (LDS in the element kernel, HBM in the dense node kernel).  A is read from its grid where it is needed.

__device__ __forceinline__ int wide_tri(int k, int k2, int nD) {    // k <= k2
    return k * nD - (k * (k - 1)) / 2 + (k2 - k);
}
__device__ __forceinline__ double piece_A(const PieceDev& P, int64_t node, int64_t n, int nr, int r, int c) {
    return P.A ? P.A[node + n * (int64_t)(r + nr * c)] : (r == c ? 1.0 : 0.0);
}

// One piece.  ORDER 0: F += value; ORDER 1: F unchanged, g += gradient; ORDER 2: T[wide_tri(k, k2) * ld] += H[k][k2]
// for k <= k2.  slack_pos >= 0: phase-I cobarrier with y[slack_pos] as the slack (as piece_accumulate).
template <int ORDER>
__device__ __forceinline__ void wide_piece(const PieceDev& P, int64_t node, int64_t n, int nD, const double (&y)[WIDE_NY],
                                           int slack_pos, double& F, double (&g)[WIDE_NY], double* T, int ld) {
    constexpr int W = WIDE_W;
    const int ni = P.ni;
    double yk[W];
#pragma unroll
    for (int c = 0; c < W; ++c) yk[c] = (c < ni) ? pick<WIDE_NY>(y, P.idx[c]) : 0.0;
    const double slack = (slack_pos >= 0) ? pick<WIDE_NY>(y, slack_pos) : 0.0;
    double gl[W], cross[W];
    double g_sl = 0.0, H_sl = 0.0;
#pragma unroll
    for (int c = 0; c < W; ++c) { gl[c] = 0.0; cross[c] = 0.0; }

    if (P.kind == MGBHIP_KIND_EP) {
        const int nz = ni;
        double z[W];
#pragma unroll
        for (int r = 0; r < W; ++r) {
            double acc = 0.0;
            if (r < nz) {
#pragma unroll
                for (int c = 0; c < W; ++c)
                    if (c < nz) acc += piece_A(P, node, n, nz, r, c) * yk[c];
                if (P.b != nullptr) acc += P.b[node + n * (int64_t)r];
            }
            z[r] = acc;
        }
        const double p0 = P.p ? P.p[node] : P.p_const;
        const double mu = P.mu ? P.mu[node] : P.mu_const;
        double qsq = 0.0;
#pragma unroll
        for (int r = 0; r < W; ++r) qsq += (r < nz - 1) ? z[r] * z[r] : 0.0;
        const double s = pick<W>(z, nz - 1) + slack;
        const double alpha = 2.0 / p0;
        const double rr = mgb_safe_pow(s, alpha) - qsq;
        if (ORDER == 0) {
            F += -mgb_Log(rr) - mu * mgb_Log(s);
            return;
        }
        const double inv_r = 1.0 / rr;
        const double s_am1 = mgb_safe_pow(s, alpha - 1.0);
        if (ORDER == 1) {
            const double gs = -alpha * s_am1 * inv_r - mu / s;
            // g_idx = A' gz with gz = (2 q / r, gs)
#pragma unroll
            for (int c = 0; c < W; ++c) {
                double acc = 0.0;
                if (c < nz) {
#pragma unroll
                    for (int r = 0; r < W; ++r)
                        if (r < nz) acc += piece_A(P, node, n, nz, r, c) * ((r < nz - 1) ? 2.0 * inv_r * z[r] : gs);
                }
                gl[c] = acc;
            }
            g_sl = gs;
        } else {
            const double inv_r2 = inv_r * inv_r;
            const double coef_qs = -2.0 * alpha * s_am1 * inv_r2;
            const double s_am2 = mgb_safe_pow(s, alpha - 2.0);
            const double s_2am2 = mgb_safe_pow(s, 2.0 * alpha - 2.0);
            const double H_ss = -alpha * (alpha - 1.0) * s_am2 * inv_r + alpha * alpha * s_2am2 * inv_r2 + mu / (s * s);
            double v[W], as[W];
#pragma unroll
            for (int c = 0; c < W; ++c) {
                double acc = 0.0, a_last = 0.0;
                if (c < nz) {
#pragma unroll
                    for (int r = 0; r < W; ++r)
                        if (r < nz - 1) acc += piece_A(P, node, n, nz, r, c) * z[r];
                    a_last = piece_A(P, node, n, nz, nz - 1, c);
                }
                v[c] = acc;
                as[c] = a_last;
            }
#pragma unroll
            for (int c1 = 0; c1 < W; ++c1) {
                if (c1 >= nz) continue;
                const int k = P.idx[c1];
#pragma unroll
                for (int c2 = 0; c2 < W; ++c2) {
                    if (c2 >= nz) continue;
                    const int k2 = P.idx[c2];
                    if (k > k2) continue;
                    double gram = 0.0;     // (A_q' A_q)[c1, c2]
                    if (P.A) {
                        for (int r = 0; r < nz - 1; ++r)
                            gram += P.A[node + n * (int64_t)(r + nz * c1)] * P.A[node + n * (int64_t)(r + nz * c2)];
                    } else {
                        gram = (c1 == c2 && c1 < nz - 1) ? 1.0 : 0.0;
                    }
                    const double h = 2.0 * inv_r * gram + 4.0 * inv_r2 * v[c1] * v[c2] +
                                     coef_qs * (v[c1] * as[c2] + as[c1] * v[c2]) + H_ss * as[c1] * as[c2];
                    T[(size_t)wide_tri(k, k2, nD) * ld] += h;
                }
                cross[c1] = coef_qs * v[c1] + H_ss * as[c1];     // (A' H_z)[c1, nz - 1]
            }
            H_sl = H_ss;
        }
    } else {
        // linear inequalities (at most MGBHIP_MAX_LIN rows on MGBHIP_MAX_LIN indexed rows): Fv = A yk + b (+ slack)
        constexpr int MC = MGBHIP_MAX_LIN;
        const int nc = P.nc;
        double Fv[MC];
#pragma unroll
        for (int r = 0; r < MC; ++r) {
            double acc = 0.0;
            if (r < nc) {
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    if (c < ni) acc += piece_A(P, node, n, nc, r, c) * yk[c];
                if (P.b != nullptr) acc += P.b[node + n * (int64_t)r];
                acc += slack;
            }
            Fv[r] = acc;
        }
        if (ORDER == 0) {
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < MC; ++r) acc += (r < nc) ? mgb_Log(Fv[r]) : 0.0;
            F += -acc;
            return;
        }
        double inv[MC];
#pragma unroll
        for (int r = 0; r < MC; ++r) inv[r] = (r < nc) ? ((ORDER == 1) ? 1.0 / Fv[r] : 1.0 / (Fv[r] * Fv[r])) : 0.0;
#pragma unroll
        for (int c = 0; c < MC; ++c) {
            double acc = 0.0;
            if (c < ni) {
#pragma unroll
                for (int r = 0; r < MC; ++r)
                    if (r < nc) acc += piece_A(P, node, n, nc, r, c) * inv[r];
            }
            if (ORDER == 1) gl[c] = -acc;
            else cross[c] = acc;
        }
#pragma unroll
        for (int r = 0; r < MC; ++r) {
            if (ORDER == 1) g_sl -= inv[r];
            else H_sl += inv[r];
        }
        if (ORDER == 2) {
#pragma unroll
            for (int c1 = 0; c1 < MC; ++c1) {
                if (c1 >= ni) continue;
                const int k = P.idx[c1];
#pragma unroll
                for (int c2 = 0; c2 < MC; ++c2) {
                    if (c2 >= ni) continue;
                    const int k2 = P.idx[c2];
                    if (k > k2) continue;
                    double acc = 0.0;
#pragma unroll
                    for (int r = 0; r < MC; ++r)
                        if (r < nc) acc += piece_A(P, node, n, nc, r, c1) * inv[r] * piece_A(P, node, n, nc, r, c2);
                    T[(size_t)wide_tri(k, k2, nD) * ld] += acc;
                }
            }
        }
    }

    if (ORDER == 1) {
#pragma unroll
        for (int i = 0; i < WIDE_NY; ++i) {
            double add = 0.0;
#pragma unroll
            for (int c = 0; c < W; ++c) add += (c < ni && P.idx[c] == i) ? gl[c] : 0.0;
            if (i == slack_pos) add += g_sl;
            g[i] += add;
        }
    } else if (slack_pos >= 0) {
        // slack row / column: pieces index the user rows, all below slack_pos
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c < ni) T[(size_t)wide_tri(P.idx[c], slack_pos, nD) * ld] += cross[c];
        T[(size_t)wide_tri(slack_pos, slack_pos, nD) * ld] += H_sl;
    }
}

// Node barrier on the wide path: ORDER 0 value F; ORDER 1 F = 0 and gradient g[0 .. nD); ORDER 2 the unscaled upper
// triangle ADDED into T (the caller zeroes it), entry (k, k2) at T[wide_tri(k, k2, nD) * ld].
template <int ORDER>
__device__ __forceinline__ void cone_eval_wide(const ConeDev& C, int64_t node, int64_t n, int nD, const double (&y)[WIDE_NY],
                                               double& F, double (&g)[WIDE_NY], double* T, int ld) {
    F = 0.0;
    if (ORDER == 1) {
#pragma unroll
        for (int i = 0; i < WIDE_NY; ++i) g[i] = 0.0;
    }
    const int slack_pos = C.feasibility ? C.NC - 1 : -1;
    for (int k = 0; k < C.npieces; ++k) {
        const PieceDev& P = C.pc[k];
        if (P.select != nullptr && P.select[node] == 0.0) continue;   // exact zero, never 0 * Inf
        wide_piece<ORDER>(P, node, n, nD, y, slack_pos, F, g, T, ld);
    }
    if (C.feasibility) {
        const int NC = C.NC;
        const double bb = C.box_b, RR = C.box_R;
        const double u = pick<WIDE_NY>(y, NC - 1);
        if (ORDER == 0) {
            F += -mgb_Log(bb - u) - mgb_Log(bb + u);
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < WIDE_NY; ++i) acc += (i >= NC && i < nD) ? (-mgb_Log(RR - y[i]) - mgb_Log(RR + y[i])) : 0.0;
            F += acc;
        } else if (ORDER == 1) {
#pragma unroll
            for (int i = 0; i < WIDE_NY; ++i) {
                if (i == NC - 1) g[i] += 1.0 / (bb - u) - 1.0 / (bb + u);
                else if (i >= NC && i < nD) g[i] = 1.0 / (RR - y[i]) - 1.0 / (RR + y[i]);
            }
        } else {
            T[(size_t)wide_tri(NC - 1, NC - 1, nD) * ld] += 1.0 / ((bb - u) * (bb - u)) + 1.0 / ((bb + u) * (bb + u));
#pragma unroll
            for (int i = 0; i < WIDE_NY; ++i)
                if (i >= NC && i < nD) T[(size_t)wide_tri(i, i, nD) * ld] += 1.0 / ((RR - y[i]) * (RR - y[i])) + 1.0 / ((RR + y[i]) * (RR + y[i]));
        }
    }
}

}  // namespace mgbhip
