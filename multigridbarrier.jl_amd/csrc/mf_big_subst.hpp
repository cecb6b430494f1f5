// mf_big_subst.hpp -- large fronts (m > lds_cap), substitution generation: a batch of multi-workgroup kernels per tree
// level (grid.y = front within the batch).  After the assembly (mf_big_assemble.hpp, shared with the inverse-based
// generation), per 32-column panel a (redundant diagonal
// LDL' + row-tile triangular solve) kernel and a 64x64-tiled symmetric rank-32 update kernel; triangular solves
// either one launch per 32-column block step or, while the work vector fits in LDS, one workgroup per front (big1).
// This is the path of fronts beyond BIG_INV_MAX_M, of MGBHIP_OLD_BIG=1 and of MfSolver::robust.
#pragma once
#include "mf_device.hpp"

namespace mgbhip {
namespace {

// Panel step.  Every workgroup of a front loads the (fully updated, still unfactored)
// diagonal block, wave 0 factors it redundantly in LDS, then the workgroup solves its TR
// rows of the panel: L21 = A21 L11^{-T} D^{-1}.  The factored diagonal block goes to a
// scratch slot (`dscr`), never in place, because sibling workgroups are still reading the
// unfactored block; the update kernel copies it home.  A front without rows below the block
// has a single active workgroup, which writes in place.
__global__ __launch_bounds__(256) void mf_big_panel(const FrontDev* __restrict__ fr, int32_t first, int j0,
                                                    double* __restrict__ arena, double* __restrict__ dscr,
                                                    int32_t* __restrict__ status, int do_diag) {
    __shared__ double Dk[NB][NB + 1];
    __shared__ double rinv[NB];
    const FrontDev F = fr[first + blockIdx.y];
    const int m = F.m, k = F.k;
    if (j0 >= k) return;
    const int nb = min(NB, k - j0);
    const int r0 = j0 + nb + blockIdx.x * TR;
    if (blockIdx.x > 0 && r0 >= m) return;
    double* W = arena + F.F_off;
    double* slot = dscr + ((int64_t)blockIdx.y * 2 + ((j0 / NB) & 1)) * (NB * NB);
    const int tid = threadIdx.x;
    const bool last = (j0 + nb >= m);              // no panel rows, no trailing block: write home
    // this thread's panel row: issue the loads before the diagonal block is ready
    const int r = r0 + tid;
    double a[NB];
    if (r < m) {
#pragma unroll
        for (int c = 0; c < NB; ++c) a[c] = (c < nb) ? W[r + (int64_t)(j0 + c) * m] : 0.0;
    }
    if (do_diag) {
        for (int i = tid; i < NB * NB; i += 256) {
            const int rr = i % NB, c = i / NB;
            Dk[rr][c] = (rr >= c && rr < nb) ? W[(j0 + rr) + (int64_t)(j0 + c) * m] : 0.0;
        }
        __syncthreads();
        if (tid < 64) {
            double d[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) d[c] = (tid < nb && c <= tid) ? Dk[tid][c] : 0.0;
            const bool bad = wave_ldlt_regs<NB>(d, nb, tid);
#pragma unroll
            for (int c = 0; c < NB; ++c)
                if (tid < nb && c <= tid) Dk[tid][c] = d[c];
            if (bad && tid == 0 && blockIdx.x == 0) atomicOr(status, 1);
        }
        __syncthreads();
        if (blockIdx.x == 0 && !last) {
            for (int i = tid; i < NB * NB; i += 256) {
                const int rr = i % NB, c = i / NB;
                if (rr >= c && rr < nb) slot[rr + NB * c] = Dk[rr][c];
            }
        }
    } else {
        // factored by the previous step's update kernel (look-ahead)
        for (int i = tid; i < NB * NB; i += 256) {
            const int rr = i % NB, c = i / NB;
            Dk[rr][c] = (rr >= c && rr < nb) ? slot[rr + NB * c] : 0.0;
        }
        __syncthreads();
    }
    if (tid < nb) rinv[tid] = 1.0 / Dk[tid][tid];
    if (blockIdx.x == 0 && last) {
        for (int i = tid; i < NB * NB; i += 256) {
            const int rr = i % NB, c = i / NB;
            if (rr >= c && rr < nb) W[(j0 + rr) + (int64_t)(j0 + c) * m] = Dk[rr][c];
        }
    }
    __syncthreads();
    if (r < m) {
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            if (c < nb) {
                double v = a[c];
#pragma unroll
                for (int q = 0; q < NB; ++q)
                    if (q < c) v -= a[q] * Dk[c][q];
                a[c] = v;
            }
        }
#pragma unroll
        for (int c = 0; c < NB; ++c)
            if (c < nb) W[r + (int64_t)(j0 + c) * m] = a[c] * rinv[c];
    }
}

// Symmetric update of the trailing block with the finished panel:
// C[r, c] -= sum_q L[r, q] d_q L[c, q], 64 x 64 tiles of the lower triangle, 4 x 4 per thread.
// Tile 0 also copies the factored diagonal block from the scratch slot to its home.
__global__ __launch_bounds__(256) void mf_big_update(const FrontDev* __restrict__ fr, int32_t first, int j0,
                                                     double* __restrict__ arena, double* __restrict__ dscr,
                                                     int32_t* __restrict__ status) {
    __shared__ double Pi[NB][ST + 1];
    __shared__ double Qj[NB][ST + 1];
    __shared__ double dq[NB];
    __shared__ double Dn[NB][NB + 1];      // look-ahead: the next diagonal block (tile 0 only)
    const FrontDev F = fr[first + blockIdx.y];
    const int m = F.m, k = F.k;
    if (j0 >= k) return;
    const int nb = min(NB, k - j0);
    const int j1 = j0 + nb;
    const int T = (m - j1 + ST - 1) / ST;
    const int tid = threadIdx.x;
    double* W = arena + F.F_off;
    const double* src = dscr + ((int64_t)blockIdx.y * 2 + ((j0 / NB) & 1)) * (NB * NB);
    const bool look = j1 < k;                  // a next panel exists: its diagonal block is factored here
    if (blockIdx.x == gridDim.x - 1) {
        // Look-ahead workgroup: update only the next diagonal block (nbn x nbn corner of tile 0)
        // and factor it, concurrently with the trailing tiles, so the next panel kernel starts
        // with its row solves at once.  Tile 0 leaves that corner alone (it is rewritten from
        // the scratch slot when the factored block goes home), so there is no race on W.
        if (!look) return;
        const int nbn = min(NB, k - j1);
        double* nslot = dscr + ((int64_t)blockIdx.y * 2 + ((j1 / NB) & 1)) * (NB * NB);
        if (tid < NB) dq[tid] = (tid < nb) ? src[tid + NB * tid] : 0.0;
        double w0[NB * NB / 256];                // corner entries, loaded while the panel rows arrive
#pragma unroll
        for (int t = 0; t < NB * NB / 256; ++t) {
            const int i = tid + 256 * t, rr = i % NB, c = i / NB;
            w0[t] = (rr >= c && rr < nbn) ? W[(j1 + rr) + (int64_t)(j1 + c) * m] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < NB * NB / 256; ++t) {
            const int i = tid + 256 * t, rr = i % NB, q = i / NB;
            Pi[q][rr] = (rr < nbn && q < nb) ? W[(j1 + rr) + (int64_t)(j0 + q) * m] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NB * NB / 256; ++t) {
            const int i = tid + 256 * t, rr = i % NB, c = i / NB;
            double acc = 0.0;
#pragma unroll 8
            for (int q = 0; q < NB; ++q) acc += Pi[q][rr] * (Pi[q][c] * dq[q]);
            Dn[rr][c] = w0[t] - acc;
        }
        __syncthreads();
        if (tid < 64) {
            double d[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) d[c] = (tid < nbn && c <= tid) ? Dn[tid][c] : 0.0;
            const bool bad = wave_ldlt_regs<NB>(d, nbn, tid);
#pragma unroll
            for (int c = 0; c < NB; ++c)
                if (tid < nbn && c <= tid) nslot[tid + NB * c] = d[c];
            if (bad && tid == 0) atomicOr(status, 1);
        }
        return;
    }
    const int lin = blockIdx.x;
    int ti = (int)((sqrt(8.0 * lin + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= lin) ++ti;
    while (ti * (ti + 1) / 2 > lin) --ti;
    const int tj = lin - ti * (ti + 1) / 2;
    if (ti >= T) return;
    // One round of global loads: the pivots d_q, the two 64 x 32 panel slices and this thread's
    // 4 x 4 micro-tile of the trailing block are all requested before anything waits (the
    // scaling by d_q happens on the LDS side, the micro-tile is consumed after the products).
    if (tid < NB) dq[tid] = (tid < nb) ? src[tid + NB * tid] : 0.0;
    const int rbase = j1 + ti * ST, cbase = j1 + tj * ST;
    const int tx = tid % 16, ty = tid / 16;
    double wt[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c = cbase + ty + 16 * b;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int r = rbase + tx + 16 * a;
            wt[a][b] = (c < m && r < m && r >= c) ? W[r + (int64_t)c * m] : 0.0;
        }
    }
    for (int i = tid; i < NB * ST; i += 256) {
        const int rr = i % ST, q = i / ST;
        const int r = rbase + rr, c = cbase + rr;
        Pi[q][rr] = (q < nb && r < m) ? W[r + (int64_t)(j0 + q) * m] : 0.0;
        Qj[q][rr] = (q < nb && c < m) ? W[c + (int64_t)(j0 + q) * m] : 0.0;
    }
    if (lin == 0) {
        for (int i = tid; i < nb * nb; i += 256) {
            const int r = i % nb, c = i / nb;
            if (r >= c) W[(j0 + r) + (int64_t)(j0 + c) * m] = src[r + NB * c];
        }
    }
    __syncthreads();
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
#pragma unroll 4
    for (int q = 0; q < NB; ++q) {              // rows q >= nb of Pi/Qj and dq hold zeros
        double pr[4], qc[4];
        const double d = dq[q];
#pragma unroll
        for (int a = 0; a < 4; ++a) pr[a] = Pi[q][tx + 16 * a] * d;
#pragma unroll
        for (int b = 0; b < 4; ++b) qc[b] = Qj[q][ty + 16 * b];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] += pr[a] * qc[b];
    }
    const int nskip = (lin == 0 && look) ? min(NB, k - j1) : 0;     // corner owned by the look-ahead workgroup
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int c = cbase + ty + 16 * b;
        if (c >= m) continue;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int r = rbase + tx + 16 * a;
            if (r < m && r >= c && !(r - j1 < nskip && c - j1 < nskip)) W[r + (int64_t)c * m] = wt[a][b] - acc[a][b];
        }
    }
}

// ---- large-front triangular solves: multi-workgroup, one launch per 32-column block step ----
// Work vectors live in `tg` (indexed like front_idx); solved pivot blocks go to `ts` (forward)
// or straight to x (backward), never in place, because sibling workgroups still read them.

// t = [b(piv); 0] + children's update vectors; each workgroup owns 256 destination entries.
__global__ __launch_bounds__(256) void mf_fwd_big_init(const FrontDev* __restrict__ fr, int32_t first,
                                                       const int32_t* __restrict__ front_idx,
                                                       const int32_t* __restrict__ children,
                                                       const int32_t* __restrict__ rel,
                                                       const double* __restrict__ b,
                                                       const double* __restrict__ uvec, double* __restrict__ tg) {
    const FrontDev F = fr[first + blockIdx.y];
    const int m = F.m, k = F.k;
    const int d0 = blockIdx.x * 256;
    if (d0 >= m) return;
    const int d1 = min(d0 + 256, m);
    const int tid = threadIdx.x;
    double* t = tg + F.idx_off;
    const int32_t* idx = front_idx + F.idx_off;
    const int jme = d0 + tid;
    double v = 0.0;
    if (jme < d1 && jme < k) v = b[idx[jme]];
    __shared__ double tl[256];
    tl[tid] = v;
    __syncthreads();
    for (int c = 0; c < F.nchild; ++c) {
        const FrontDev C = fr[children[F.child_off + c]];
        const int32_t* rl = rel + C.rel_off;
        const double* uc = uvec + C.u_off;
        const int bc = C.m - C.k;
        int lo = 0, hi = bc;
        while (lo < hi) { int mid = (lo + hi) >> 1; if (rl[mid] < d0) lo = mid + 1; else hi = mid; }
        const int jb = lo;
        hi = bc;
        while (lo < hi) { int mid = (lo + hi) >> 1; if (rl[mid] < d1) lo = mid + 1; else hi = mid; }
        for (int j = jb + tid; j < lo; j += 256) tl[rl[j] - d0] += uc[j];
        __syncthreads();
    }
    if (jme < d1) t[jme] = tl[tid];
}

__global__ __launch_bounds__(256) void mf_fwd_big_step(const FrontDev* __restrict__ fr, int32_t first, int j0,
                                                       const double* __restrict__ arena, double* __restrict__ tg,
                                                       double* __restrict__ ts) {
    __shared__ double Dk[NB][NB + 1];
    __shared__ double yb[NB];
    const FrontDev F = fr[first + blockIdx.y];
    const int m = F.m, k = F.k;
    if (j0 >= k) return;
    const int nb = min(NB, k - j0);
    const int r0 = j0 + nb + blockIdx.x * 256;
    if (blockIdx.x > 0 && r0 >= m) return;
    const double* Fm = arena + F.F_off;
    double* t = tg + F.idx_off;
    const int tid = threadIdx.x;
    for (int i = tid; i < nb * nb; i += 256) {
        const int r = i % nb, c = i / nb;
        Dk[r][c] = (r > c) ? Fm[(j0 + r) + (int64_t)(j0 + c) * m] : 0.0;
    }
    __syncthreads();
    if (tid < 64) {
        double v = (tid < nb) ? t[j0 + tid] : 0.0;
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            if (c < nb) {
                const double tc = readlane_f64(v, c);
                if (tid > c && tid < nb) v -= Dk[tid][c] * tc;
            }
        }
        if (tid < nb) {
            yb[tid] = v;
            if (blockIdx.x == 0) ts[F.idx_off + j0 + tid] = v;
        }
    }
    __syncthreads();
    const int r = r0 + tid;
    if (r < m) {
        double v = t[r];
        for (int c = 0; c < nb; ++c) v -= Fm[r + (int64_t)(j0 + c) * m] * yb[c];
        t[r] = v;
    }
}

__global__ __launch_bounds__(256) void mf_fwd_big_fin(const FrontDev* __restrict__ fr, int32_t first,
                                                      const int32_t* __restrict__ front_idx,
                                                      const double* __restrict__ arena,
                                                      const double* __restrict__ tg, const double* __restrict__ ts,
                                                      double* __restrict__ y, double* __restrict__ uvec) {
    const FrontDev F = fr[first + blockIdx.y];
    const int m = F.m, k = F.k;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const double* Fm = arena + F.F_off;
    if (j < k) y[front_idx[F.idx_off + j]] = ts[F.idx_off + j] / Fm[j + (int64_t)j * m];
    else uvec[F.u_off + j - k] = tg[F.idx_off + j];
}

// v[q] = y[piv q] - sum_{r >= k} L[r, q] x[bnd r]: one wave per pivot column.
__global__ __launch_bounds__(256) void mf_bwd_big_init(const FrontDev* __restrict__ fr, int32_t first,
                                                       const int32_t* __restrict__ front_idx,
                                                       const double* __restrict__ arena,
                                                       const double* __restrict__ y, const double* __restrict__ x,
                                                       double* __restrict__ tg) {
    const FrontDev F = fr[first + blockIdx.y];
    const int m = F.m, k = F.k;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= k) return;
    const int32_t* idx = front_idx + F.idx_off;
    const double* Lq = arena + F.F_off + (int64_t)q * m;
    double s = 0.0;
    for (int r = k + lane; r < m; r += 64) s += Lq[r] * x[idx[r]];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) tg[F.idx_off + q] = y[idx[q]] - s;
}

// Block step (descending j0): solve the unit-upper diagonal block, publish x, and update the
// entries q < j0 with rows j0..j0+nb of L (32 contiguous doubles per column).
__global__ __launch_bounds__(256) void mf_bwd_big_step(const FrontDev* __restrict__ fr, int32_t first, int j0,
                                                       const int32_t* __restrict__ front_idx,
                                                       const double* __restrict__ arena, double* __restrict__ tg,
                                                       double* __restrict__ x) {
    __shared__ double Dk[NB][NB + 1];
    __shared__ double xb[NB];
    const FrontDev F = fr[first + blockIdx.y];
    const int m = F.m, k = F.k;
    if (j0 >= k) return;
    const int nb = min(NB, k - j0);
    const int q0 = blockIdx.x * 256;
    if (blockIdx.x > 0 && q0 >= j0) return;
    const double* Fm = arena + F.F_off;
    double* t = tg + F.idx_off;
    const int tid = threadIdx.x;
    for (int i = tid; i < nb * nb; i += 256) {
        const int r = i % nb, c = i / nb;
        Dk[r][c] = (r > c) ? Fm[(j0 + r) + (int64_t)(j0 + c) * m] : 0.0;
    }
    __syncthreads();
    if (tid < 64) {
        double v = (tid < nb) ? t[j0 + tid] : 0.0;
#pragma unroll
        for (int c = NB - 1; c >= 0; --c) {
            if (c < nb) {
                const double xc = readlane_f64(v, c);
                if (tid < c) v -= Dk[c][tid] * xc;
            }
        }
        if (tid < nb) {
            xb[tid] = v;
            if (blockIdx.x == 0) x[front_idx[F.idx_off + j0 + tid]] = v;
        }
    }
    __syncthreads();
    const int q = q0 + tid;
    if (q < j0) {
        const double* Lq = Fm + (int64_t)q * m + j0;
        double v = t[q];
        for (int c = 0; c < nb; ++c) v -= Lq[c] * xb[c];
        t[q] = v;
    }
}

// ---- large-front triangular solves, one workgroup per front -----------------------------------
// The block steps of a triangular solve are a chain of dependent latencies (diagonal block ->
// row update -> next diagonal block); the arithmetic is tiny.  One 1024-thread workgroup per
// front keeps the whole work vector in LDS and turns every kernel boundary of the multi-launch
// path into a workgroup barrier; fronts of a level run side by side on their own CUs.  L is
// streamed once (coalesced along rows in the forward sweep).  Used while the vector fits in LDS.
constexpr int BIG1_THREADS = 1024;
constexpr int BIG1_MAX_M = 6000;       // work vector + diagonal block within the 64 KB static LDS budget

__global__ __launch_bounds__(BIG1_THREADS) void mf_fwd_big1(const FrontDev* __restrict__ fr, int32_t first,
                                                            const int32_t* __restrict__ front_idx,
                                                            const int32_t* __restrict__ children,
                                                            const int32_t* __restrict__ rel,
                                                            const double* __restrict__ arena,
                                                            const double* __restrict__ b, double* __restrict__ y,
                                                            double* __restrict__ uvec) {
    extern __shared__ double sh[];
    const FrontDev F = fr[first + blockIdx.x];
    const int m = F.m, k = F.k;
    const int tid = threadIdx.x, nt = BIG1_THREADS;
    double* tl = sh;                         // [m]
    double* Dk = sh + ((m + 1) & ~1);        // [NB][NB + 1]
    const int32_t* idx = front_idx + F.idx_off;
    const double* Fm = arena + F.F_off;
    for (int j = tid; j < m; j += nt) tl[j] = (j < k) ? b[idx[j]] : 0.0;
    __syncthreads();
    for (int c = 0; c < F.nchild; ++c) {
        const FrontDev C = fr[children[F.child_off + c]];
        const int32_t* rl = rel + C.rel_off;
        const double* uc = uvec + C.u_off;
        const int bc = C.m - C.k;
        for (int j = tid; j < bc; j += nt) tl[rl[j]] += uc[j];
        __syncthreads();
    }
    // strictly-lower entry (r, c) of the first diagonal block, one per thread
    const int dr = tid % NB, dc = tid / NB;
    double dnext = (dr > dc && dr < k && dc < k) ? Fm[dr + (int64_t)dc * m] : 0.0;
    for (int j0 = 0; j0 < k; j0 += NB) {
        const int nb = min(NB, k - j0);
        Dk[dr * (NB + 1) + dc] = dnext;
        __syncthreads();
        {   // prefetch the next diagonal block while this one is used
            const int jn = j0 + NB;
            dnext = (dr > dc && jn + dr < k && jn + dc < k) ? Fm[(jn + dr) + (int64_t)(jn + dc) * m] : 0.0;
        }
        if (tid < 64) {
            double v = (tid < nb) ? tl[j0 + tid] : 0.0;
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const double tc = readlane_f64(v, c);
                if (tid > c && tid < NB) v -= Dk[tid * (NB + 1) + c] * tc;      // rows/columns >= nb hold zeros
            }
            if (tid < nb) tl[j0 + tid] = v;
        }
        __syncthreads();
        for (int r = j0 + nb + tid; r < m; r += nt) {
            const double* Lr = Fm + r + (int64_t)j0 * m;
            double v = tl[r];
            if (nb == NB) {
#pragma unroll
                for (int c = 0; c < NB; ++c) v -= Lr[(int64_t)c * m] * tl[j0 + c];
            } else {
                for (int c = 0; c < nb; ++c) v -= Lr[(int64_t)c * m] * tl[j0 + c];
            }
            tl[r] = v;
        }
        __syncthreads();
    }
    for (int j = tid; j < m; j += nt) {
        if (j < k) y[idx[j]] = tl[j] / Fm[j + (int64_t)j * m];
        else uvec[F.u_off + j - k] = tl[j];
    }
}

__global__ __launch_bounds__(BIG1_THREADS) void mf_bwd_big1(const FrontDev* __restrict__ fr, int32_t first,
                                                            const int32_t* __restrict__ front_idx,
                                                            const double* __restrict__ arena,
                                                            const double* __restrict__ y, double* __restrict__ x) {
    extern __shared__ double sh[];
    const FrontDev F = fr[first + blockIdx.x];
    const int m = F.m, k = F.k;
    const int tid = threadIdx.x, nt = BIG1_THREADS;
    const int lane = tid & 63, wave = tid >> 6;
    double* tl = sh;                         // [m]: pivots hold the running right-hand side, the rest x(boundary)
    double* Dk = sh + ((m + 1) & ~1);        // [NB][NB + 1]
    const int32_t* idx = front_idx + F.idx_off;
    const double* Fm = arena + F.F_off;
    for (int j = tid; j < m; j += nt) tl[j] = (j < k) ? y[idx[j]] : x[idx[j]];
    __syncthreads();
    // v[q] = y[q] - sum_{r >= k} L[r, q] x[r]: one wave per pivot column
    for (int q = wave; q < k; q += nt / 64) {
        const double* Lq = Fm + (int64_t)q * m;
        double s = 0.0;
        for (int r = k + lane; r < m; r += 64) s += Lq[r] * tl[r];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) tl[q] -= s;
    }
    __syncthreads();
    const int dr = tid % NB, dc = tid / NB;
    const int last = ((k - 1) / NB) * NB;
    double dnext = (dr > dc && last + dr < k) ? Fm[(last + dr) + (int64_t)(last + dc) * m] : 0.0;
    for (int j0 = last; j0 >= 0; j0 -= NB) {
        const int nb = min(NB, k - j0);
        Dk[dr * (NB + 1) + dc] = dnext;
        __syncthreads();
        if (j0 >= NB) {
            const int jn = j0 - NB;          // full block
            dnext = (dr > dc) ? Fm[(jn + dr) + (int64_t)(jn + dc) * m] : 0.0;
        }
        if (tid < 64) {
            double v = (tid < nb) ? tl[j0 + tid] : 0.0;
#pragma unroll
            for (int c = NB - 1; c >= 0; --c) {
                const double xc = readlane_f64(v, c);
                if (tid < c) v -= Dk[c * (NB + 1) + tid] * xc;      // rows/columns >= nb hold zeros
            }
            if (tid < nb) {
                tl[j0 + tid] = v;
                x[idx[j0 + tid]] = v;
            }
        }
        __syncthreads();
        for (int q = tid; q < j0; q += nt) {
            const double* Lq = Fm + (int64_t)q * m + j0;
            double v = tl[q];
            if (nb == NB) {
#pragma unroll
                for (int c = 0; c < NB; ++c) v -= Lq[c] * tl[j0 + c];
            } else {
                for (int c = 0; c < nb; ++c) v -= Lq[c] * tl[j0 + c];
            }
            tl[q] = v;
        }
        __syncthreads();
    }
}

// ---- host launchers ------------------------------------------------------------------------------------------
// The pivot chain of `nfronts` assembled fronts: per 32-column step the panel solve (which factors the diagonal block
// of step 0 itself) and the trailing update with its look-ahead workgroup.
inline void launch_subst_steps(const FactorArgs& a, const MfLaunch& L, int nfronts) {
    for (int j0 = 0; j0 < L.max_k; j0 += NB) {
        const int rem = L.max_m - j0;                // rows from the panel start, at most
        const dim3 gp(std::max(1, (rem - 1 + TR - 1) / TR), nfronts);
        hipLaunchKernelGGL(mf_big_panel, gp, dim3(256), 0, a.st, a.fr, L.first, j0, a.arena, a.dscr, a.status, j0 == 0 ? 1 : 0);
        const int T = (rem - 1 + ST - 1) / ST;       // trailing tiles (upper bound)
        if (T > 0) {
            const dim3 gu(T * (T + 1) / 2 + 1, nfronts);     // + the look-ahead workgroup
            hipLaunchKernelGGL(mf_big_update, gu, dim3(256), 0, a.st, a.fr, L.first, j0, a.arena, a.dscr, a.status);
        }
    }
}

inline void launch_fwd_big_steps(const SolveArgs& a, const MfLaunch& L) {
    const dim3 gi((L.max_m + 255) / 256, L.count);
    hipLaunchKernelGGL(mf_fwd_big_init, gi, dim3(256), 0, a.st, a.fr, L.first, a.front_idx, a.children, a.rel, a.b, a.uvec, a.tbig);
    for (int j0 = 0; j0 < L.max_k; j0 += NB) {
        const int rem = L.max_m - j0;
        const dim3 gs(std::max(1, (rem - 1 + 255) / 256), L.count);
        hipLaunchKernelGGL(mf_fwd_big_step, gs, dim3(256), 0, a.st, a.fr, L.first, j0, a.arena, a.tbig, a.tsol);
    }
    hipLaunchKernelGGL(mf_fwd_big_fin, gi, dim3(256), 0, a.st, a.fr, L.first, a.front_idx, a.arena, a.tbig, a.tsol, a.y, a.uvec);
}
inline void launch_bwd_big_steps(const SolveArgs& a, const MfLaunch& L) {
    const dim3 gi((L.max_k + 3) / 4, L.count);
    hipLaunchKernelGGL(mf_bwd_big_init, gi, dim3(256), 0, a.st, a.fr, L.first, a.front_idx, a.arena, a.y, a.x, a.tbig);
    const int last = ((L.max_k - 1) / NB) * NB;
    for (int j0 = last; j0 >= 0; j0 -= NB) {
        const dim3 gs(std::max(1, (j0 + 255) / 256), L.count);
        hipLaunchKernelGGL(mf_bwd_big_step, gs, dim3(256), 0, a.st, a.fr, L.first, j0, a.front_idx, a.arena, a.tbig, a.x);
    }
}

// mf_fwd_big1 / mf_bwd_big1: the work vector + the diagonal block
inline size_t big1_lds(int max_m) { return (size_t)(((max_m + 1) & ~1) + NB * (NB + 1)) * sizeof(double); }
inline void launch_fwd_big1(const SolveArgs& a, const MfLaunch& L) {
    hipLaunchKernelGGL(mf_fwd_big1, dim3(L.count), dim3(BIG1_THREADS), big1_lds(L.max_m), a.st, a.fr, L.first, a.front_idx,
                       a.children, a.rel, a.arena, a.b, a.y, a.uvec);
}
inline void launch_bwd_big1(const SolveArgs& a, const MfLaunch& L) {
    hipLaunchKernelGGL(mf_bwd_big1, dim3(L.count), dim3(BIG1_THREADS), big1_lds(L.max_m), a.st, a.fr, L.first, a.front_idx,
                       a.arena, a.y, a.x);
}

}  // namespace
}  // namespace mgbhip
