// mf_small.hpp -- fronts that are factored out of LDS or registers (m <= lds_cap): the workgroup-per-front kernel
// mf_factor_small, the wave-per-front kernel mf_factor_wave (m <= 48, small children), the 16-lanes-per-front kernels
// of the leaves (m <= 16), and the triangular solves of all of them.  Every front is assembled, factored and written
// back by its owner in one launch; all fronts of one tree level and size class share the launch.
#pragma once
#include "mf_device.hpp"

namespace mgbhip {
namespace {

// One workgroup per front.  Right-looking LDL' blocked by NB = 32 columns: wave 0 factors the
// diagonal block in registers (shuffles only), every thread then solves one panel row in
// registers, and all threads apply the rank-32 update -- 3 workgroup barriers per 32 columns.
template <int NBT, bool PACKED>
__global__ void mf_factor_small(const FrontDev* __restrict__ fr, int32_t first,
                                const int32_t* __restrict__ children, const int32_t* __restrict__ rel,
                                const int32_t* __restrict__ a_src, const int32_t* __restrict__ a_dst,
                                const double* __restrict__ Hval, double* __restrict__ arena,
                                int32_t* __restrict__ status) {
    extern __shared__ double W[];
    const FrontDev F = fr[first + blockIdx.x];
    double* Fg = arena + F.F_off;
    const int m = F.m, k = F.k;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int tx = tid % TX, ty = tid / TX, TYn = nt / TX;
    // PACKED (classes 88 and 128, whose square arrays leave room for one or two workgroups per compute unit): the
    // front lives in LDS as a packed lower triangle, column c at W + co(c) (entry (r, c), r >= c, at co(c) + r) --
    // half the LDS, twice the resident fronts; analyze() remaps a_dst.  The smaller classes keep the square array
    // (their occupancy is not LDS-bound and the plain column offset c * m is cheaper to form).
    const int mm = PACKED ? m * (m + 1) / 2 : m * m;
    auto co = [m](int c) { return PACKED ? c * (m - 1) - c * (c - 1) / 2 : c * m; };
    double* S = W + mm;                        // [NBT][m] scaled multipliers of the current panel

    SP(0);
    // the first batch of A entries and the first chunk of child descriptors are requested before the LDS front is
    // zeroed: two dependent-load chains (a_src -> Hval, children -> fr) run under the fill instead of after it
    int a_d0 = -1;
    double a_v0 = 0.0;
    if (tid < F.a_cnt) {
        a_d0 = a_dst[F.a_off + tid];
        a_v0 = Hval[a_src[F.a_off + tid]];
    }
    int64_t pU = 0, pR = 0;
    int32_t pM = 0, pB = 0;
    if (tid < min(CHILD_CHUNK, F.nchild)) {
        const FrontDev C = fr[children[F.child_off + tid]];
        child_update_desc(C, pU, pM);
        pR = C.rel_off;
        pB = C.m - C.k;
    }
    for (int i = tid; i < mm; i += nt) W[i] = 0.0;
    __syncthreads();
    if (a_d0 >= 0) W[a_d0] = a_v0;
    for (int t = tid + nt; t < F.a_cnt; t += nt) W[a_dst[F.a_off + t]] = Hval[a_src[F.a_off + t]];
    __syncthreads();
    SP(1);
    // Extend-add of the children.  The additions of different children may hit the same slot, so
    // children stay ordered (deterministic sums) with a barrier between them -- but their global
    // loads do not have to: the child descriptors are fetched once into LDS, and the entries of
    // four children at a time are staged in registers before the first of them is applied, so a
    // front with many small children (static-condensation leaves under an element patch) pays one
    // memory latency per four children instead of three dependent ones per child.
    __shared__ int64_t cU[CHILD_CHUNK];        // arena offset of the child's update block (kc, kc)
    __shared__ int64_t cR[CHILD_CHUNK];        // rel offset
    __shared__ int32_t cM[CHILD_CHUNK], cB[CHILD_CHUNK];
    __shared__ int32_t crl[128];               // relative indices of one larger child (b <= m <= 128)
    __shared__ double prinv[32];               // reciprocal pivots of the current panel
    for (int cbase = 0; cbase < F.nchild; cbase += CHILD_CHUNK) {
        const int nc = min(CHILD_CHUNK, F.nchild - cbase);
        __syncthreads();
        if (tid < nc) {
            if (cbase == 0) {
                cU[tid] = pU; cR[tid] = pR; cM[tid] = pM; cB[tid] = pB;
            } else {
                const FrontDev C = fr[children[F.child_off + cbase + tid]];
                int64_t u_; int32_t m_;
                child_update_desc(C, u_, m_);
                cU[tid] = u_;
                cR[tid] = C.rel_off;
                cM[tid] = m_;
                cB[tid] = C.m - C.k;
            }
        }
        __syncthreads();
        for (int c0 = 0; c0 < nc; c0 += 4) {
            if (nt >= 256 && (c0 & 15) == 0) {
                // Sixteen small children (update block <= 8 x 8) at once: wave w takes children 4w .. 4w+3, one entry
                // per lane, so ALL their loads are in flight together (one memory latency for the group instead
                // of four).  The additions keep child order: a wave applies its four children in program order
                // (LDS operations of one wave stay ordered) and the waves take turns, four barriers in all.
                // Written for four waves: in a wider workgroup (factor_small_threads) waves 4 and up own no child
                // (4 w >= 16 >= ng) and only join the barriers.
                const int ng = min(16, nc - c0);
                bool small16 = true;
                for (int u = 0; u < ng; ++u) small16 = small16 && cB[c0 + u] * cB[c0 + u] <= 64;
                if (small16) {
                    const int w = tid >> 6, e = tid & 63;
                    int dst[4];
                    double val[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        dst[u] = -1;
                        val[u] = 0.0;
                        const int c = c0 + 4 * w + u;
                        if (4 * w + u < ng) {
                            const int b = cB[c];
                            if (e < b * b) {
                                const int j = e / b, r = e - j * b;
                                if (r >= j) {
                                    const int32_t* rl = rel + cR[c];
                                    dst[u] = rl[r] + co(rl[j]);
                                    val[u] = arena[child_entry(cU[c], cM[c], j, r)];
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int ph = 0; ph < 4; ++ph) {
                        if (4 * ph < ng) {
                            if (ph == w) {
#pragma unroll
                                for (int u = 0; u < 4; ++u) {
                                    if (dst[u] >= 0) W[dst[u]] += val[u];
                                    wave_sync();            // child u's stores before child u+1's loads
                                }
                            }
                            __syncthreads();
                        }
                    }
                    c0 += 12;          // the loop increment adds the other 4
                    continue;
                }
            }
            int dst[4];
            double val[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                dst[u] = -1;
                val[u] = 0.0;
                const int c = c0 + u;
                if (c < nc) {
                    const int b = cB[c];
                    if (b * b <= nt && tid < b * b) {
                        const int j = tid / b, r = tid - j * b;
                        if (r >= j) {
                            const int32_t* rl = rel + cR[c];
                            dst[u] = rl[r] + co(rl[j]);
                            val[u] = arena[child_entry(cU[c], cM[c], j, r)];
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u;
                if (c >= nc) break;
                if (dst[u] >= 0) W[dst[u]] += val[u];
                const int b = cB[c];
                if (b * b > nt) {               // larger child: 2-D sweep, relative indices from LDS
                    const int32_t* rlg = rel + cR[c];
                    for (int j = tid; j < b; j += nt) crl[j] = rlg[j];
                    __syncthreads();
                    const int mc = cM[c];
                    for (int j = ty; j < b; j += TYn) {
                        const int dcol = co(crl[j]);
                        const double* Uc = arena + child_entry(cU[c], mc, j, 0);     // (r, j) at Uc[r]; packed children shift by j
                        for (int r = j + tx; r < b; r += 4 * TX) {      // four rows per lane in flight
                            const int r1 = r + TX, r2 = r + 2 * TX, r3 = r + 3 * TX;
                            const double u0 = Uc[r];
                            const double u1 = r1 < b ? Uc[r1] : 0.0;
                            const double u2 = r2 < b ? Uc[r2] : 0.0;
                            const double u3 = r3 < b ? Uc[r3] : 0.0;
                            W[crl[r] + dcol] += u0;
                            if (r1 < b) W[crl[r1] + dcol] += u1;
                            if (r2 < b) W[crl[r2] + dcol] += u2;
                            if (r3 < b) W[crl[r3] + dcol] += u3;
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
    SP(2);
    bool bad = false;
    for (int j0 = 0; j0 < k; j0 += NBT) {
        const int nb = min(NBT, k - j0);
        SPL(0);
        if (tid < 64) {                       // diagonal block in registers
            double a[NBT];
#pragma unroll
            for (int c = 0; c < NBT; ++c) a[c] = (tid < nb && c <= tid) ? W[(j0 + tid) + co(j0 + c)] : 0.0;
            bad |= wave_ldlt_regs<NBT>(a, nb, tid);
#pragma unroll
            for (int c = 0; c < NBT; ++c)
                if (tid < nb && c <= tid) {
                    W[(j0 + tid) + co(j0 + c)] = a[c];
                    if (c == tid) prinv[c] = 1.0 / a[c];      // pivot reciprocals for the row solves
                }
        }
        SPL(1);
        __syncthreads();
        SPL(2);
        {                                     // panel rows: l = (a L11^{-T}) D^{-1}, one row per thread
            const int r = j0 + nb + tid;
            if (r < m) {
                double a[NBT];
#pragma unroll
                for (int c = 0; c < NBT; ++c) a[c] = (c < nb) ? W[r + co(j0 + c)] : 0.0;
#pragma unroll
                for (int c = 0; c < NBT; ++c) {
                    if (c < nb) {
                        double v = a[c];
#pragma unroll
                        for (int q = 0; q < NBT; ++q)
                            if (q < c) v -= a[q] * W[(j0 + c) + co(j0 + q)];
                        a[c] = v;
                    }
                }
                // a[c] is still l(r, c) * d_c here: exactly the scaled multiplier the update needs
#pragma unroll
                for (int c = 0; c < NBT; ++c) {
                    S[c * m + r] = (c < nb) ? a[c] : 0.0;
                    if (c < nb) W[r + co(j0 + c)] = a[c] * prinv[c];
                }
            }
        }
        SPL(3);
        __syncthreads();
        SPL(4);
        // rank-nb update of the trailing lower triangle on the matrix cores, one 16 x 16 tile per wave and pass:
        //   W[r, c] -= sum_q l(r, q) * S(q, c),   S(q, c) = l(c, q) d_q from the row solve above.
        // v_mfma_f64_16x16x4: lane (fr16, fk) feeds A[m = fr16][k = fk] = S(q, cc0 + fr16) and B[k = fk][n = fr16] =
        // l(r0 + fr16, q), and holds D[m = fk + 4 i][n = fr16], i = 0..3 -- rows run along the 16 lanes, so every
        // LDS access of a tile is 16 consecutive doubles.  The scalar form read 16 LDS operands per 2 FMAs and kept
        // the LDS pipeline of the compute unit saturated (three fronts per unit: 17 us for a rank-15 update of 65 rows).
        {
            const int c0 = j0 + nb;
            const int T = (m - c0 + 15) >> 4;
            const int lane = tid & 63, fr16 = lane & 15, fk = lane >> 4;
            for (int tile = tid >> 6; tile < T * (T + 1) / 2; tile += nt >> 6) {
                int I = (int)((sqrtf(8.0f * (float)tile + 1.0f) - 1.0f) * 0.5f);
                while ((I + 1) * (I + 2) / 2 <= tile) ++I;
                while (I * (I + 1) / 2 > tile) --I;
                const int J = tile - I * (I + 1) / 2;
                const int r0 = c0 + 16 * I, cc0 = c0 + 16 * J;
                const int rr = min(r0 + fr16, m - 1), cc = min(cc0 + fr16, m - 1);       // tiles overhang the front: clamp, never stored
                double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = 0; kk < NBT / 4; ++kk) {
                    const int q = 4 * kk + fk;
                    const double sa = S[q * m + cc];                                   // rows q >= nb of S are zero
                    const double lb = (q < nb) ? W[rr + co(j0 + q)] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, lb, acc, 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int col = cc0 + fk + 4 * i, row = r0 + fr16;
                    if (row < m && col < m && row >= col) W[row + co(col)] -= acc[i];
                }
            }
        }
        SPL(5);
        __syncthreads();
        SPL(6);
    }
    SP(3);
    if (bad && tid == 0) atomicOr(status, 1);
    // write the lower triangle back to the (square, column-major) frontal matrix: a 2-D sweep, rows fastest
    if (PACKED) {
        for (int c = ty; c < m; c += TYn) {
            const int cc = co(c);
            for (int r = c + tx; r < m; r += TX) Fg[r + (int64_t)c * m] = W[cc + r];
        }
    } else {
        for (int i = tid; i < mm; i += nt) Fg[i] = W[i];
    }
    SP(4);
}

// Fronts with m <= MW (32 or 48): ONE WAVE per front, no workgroup barriers.  The front is assembled in a packed
// LDS triangle (column stride MW; analyze() remaps a_dst for these fronts), lane r then takes row r into
// registers and the whole partial factorization -- k pivots and the Schur complement of the boundary rows -- is
// wave_ldlt_regs: v_readlane broadcasts and FMAs only.  A 46-row front with 21 pivots and 16 leaf children takes
// about half the time of the workgroup-per-front kernel, and twice as many fronts are resident per compute unit.
template <int MW>
__global__ __launch_bounds__(256) void mf_factor_wave(const FrontDev* __restrict__ fr, int32_t first, int32_t count,
                                                      const int32_t* __restrict__ children, const int32_t* __restrict__ rel,
                                                      const int32_t* __restrict__ a_src, const int32_t* __restrict__ a_dst,
                                                      const double* __restrict__ Hval, double* __restrict__ arena,
                                                      int32_t* __restrict__ status) {
    constexpr int PK = MW * (MW + 1) / 2;
    extern __shared__ double sh[];
#ifdef MGB_STEP_PROBE      // one wave of the level-1 launch at L = 9: phase timestamps (tools/gpu_probe_wave.py)
#define WP(i) do { if (threadIdx.x == 0 && gridDim.x == 2048 && blockIdx.x == 1500) g_probe[8 + (i)] = wall_clock64(); } while (0)
#else
#define WP(i) do { } while (0)
#endif
    WP(0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fi = blockIdx.x * 4 + wave;
    if (fi >= count) return;                       // waves are independent: no workgroup barrier below
    const FrontDev F = fr[first + fi];
    const int m = F.m, k = F.k;
    double* W = sh + (size_t)wave * PK;
    // child descriptors of this wave (chunks of WCH), behind the four fronts: 4 x 48-row triangles + the descriptors
    // stay under 40 KB, so four workgroups share a compute unit
    constexpr int WCH = 32;
    int64_t* cU = reinterpret_cast<int64_t*>(sh + (size_t)4 * PK) + wave * 2 * WCH;
    int64_t* cR = cU + WCH;
    int32_t* cM = reinterpret_cast<int32_t*>(reinterpret_cast<int64_t*>(sh + (size_t)4 * PK) + 4 * 2 * WCH) + wave * 2 * WCH;
    int32_t* cB = cM + WCH;
    auto pidx = [](int r, int c) { return c * MW - c * (c - 1) / 2 + (r - c); };
    // first batch of A entries and the first chunk of child descriptors are requested before the triangle is zeroed
    int a_d0 = -1;
    double a_v0 = 0.0;
    if (lane < F.a_cnt) {
        a_d0 = a_dst[F.a_off + lane];
        a_v0 = Hval[a_src[F.a_off + lane]];
    }
    int64_t pU = 0, pR = 0;
    int32_t pM = 0, pB = 0;
    if (lane < min(WCH, F.nchild)) {
        const FrontDev C = fr[children[F.child_off + lane]];
        child_update_desc(C, pU, pM);
        pR = C.rel_off;
        pB = C.m - C.k;
    }
    for (int i = lane; i < PK; i += 64) W[i] = 0.0;
    wave_sync();
    WP(1);
    if (a_d0 >= 0) W[a_d0] = a_v0;
    for (int t = lane + 64; t < F.a_cnt; t += 64) W[a_dst[F.a_off + t]] = Hval[a_src[F.a_off + t]];
    wave_sync();
    WP(2);
    for (int cbase = 0; cbase < F.nchild; cbase += WCH) {
        const int nc = min(WCH, F.nchild - cbase);
        if (lane < nc) {
            if (cbase == 0) {
                cU[lane] = pU; cR[lane] = pR; cM[lane] = pM; cB[lane] = pB;
            } else {
                const FrontDev C = fr[children[F.child_off + cbase + lane]];
                int64_t u_; int32_t m_;
                child_update_desc(C, u_, m_);
                cU[lane] = u_;
                cR[lane] = C.rel_off;
                cM[lane] = m_;
                cB[lane] = C.m - C.k;
            }
        }
        wave_sync();
        for (int c0 = 0; c0 < nc; c0 += 16) {
            const int ng = min(16, nc - c0);
            bool small16 = true;
            for (int u = 0; u < ng; ++u) small16 = small16 && cB[c0 + u] * cB[c0 + u] <= 64;
            if (small16) {
                // sixteen small children (the element leaves under a level-1 front): one entry per lane and child, all
                // loads in flight at once, then added in child order.  j = lane / b by a float reciprocal: exact for
                // lane < 64, b <= 8 ((lane + 1/2) / b stays 1/16 away from every integer).
                int dst[16];
                double val[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    dst[u] = -1;
                    val[u] = 0.0;
                    if (u < ng) {
                        const int c = c0 + u, b = cB[c];
                        if (lane < b * b) {
                            const int j = (int)(((float)lane + 0.5f) * __builtin_amdgcn_rcpf((float)b)), r = lane - j * b;
                            if (r >= j) {
                                const int32_t* rl = rel + cR[c];
                                dst[u] = pidx(rl[r], rl[j]);
                                val[u] = arena[child_entry(cU[c], cM[c], j, r)];
                            }
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    if (u < ng) {
                        if (dst[u] >= 0) W[dst[u]] += val[u];
                        wave_sync();                    // child u's stores before child u+1's loads
                    }
                }
            } else {
                for (int u = 0; u < ng; ++u) {
                    const int c = c0 + u, b = cB[c], mc = cM[c];
                    const int32_t* rl = rel + cR[c];
                    for (int e = lane; e < b * b; e += 256) {       // four entries per lane in flight
                        int dd[4];
                        double vv[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int ee = e + 64 * q;
                            dd[q] = -1;
                            vv[q] = 0.0;
                            if (ee < b * b) {
                                const int j = ee / b, r = ee - j * b;
                                if (r >= j) {
                                    dd[q] = pidx(rl[r], rl[j]);
                                    vv[q] = arena[child_entry(cU[c], mc, j, r)];
                                }
                            }
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (dd[q] >= 0) W[dd[q]] += vv[q];         // distinct slots within one child
                    }
                    wave_sync();
                }
            }
        }
        wave_sync();
    }
    WP(3);
    double a[MW];
#pragma unroll
    for (int c = 0; c < MW; ++c) a[c] = (lane < m && c <= lane) ? W[pidx(lane, c)] : 0.0;
    WP(4);
    const bool bad = wave_ldlt_regs<MW>(a, k, lane);
    WP(5);
    if (bad) atomicOr(status, 1);
    if (lane < m) {
        double* Fg = arena + F.F_off;
#pragma unroll
        for (int c = 0; c < MW; ++c)
            if (c <= lane) Fg[lane + (int64_t)c * m] = a[c];
    }
    WP(6);
}

// Triangular solves of small fronts: one wave per front (4 fronts per workgroup), the work
// vector lives in registers (rows lane and lane + 64), no workgroup barriers.
__global__ __launch_bounds__(256) void mf_forward_small(const FrontDev* __restrict__ fr, int32_t first,
                                                        int32_t count, int32_t ts,
                                                        const int32_t* __restrict__ front_idx,
                                                        const int32_t* __restrict__ children,
                                                        const int32_t* __restrict__ rel,
                                                        const double* __restrict__ arena,
                                                        const double* __restrict__ b, double* __restrict__ y,
                                                        double* __restrict__ uvec) {
    extern __shared__ double sh[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fi = blockIdx.x * 4 + wave;
    if (fi >= count) return;
    const FrontDev F = fr[first + fi];
    const int m = F.m, k = F.k;
    double* t = sh + wave * ts;
    const int32_t* idx = front_idx + F.idx_off;
    const double* Fm = arena + F.F_off;
    for (int j = lane; j < m; j += 64) t[j] = (j < k) ? b[idx[j]] : 0.0;
    wave_sync();
    // children's update vectors: descriptors of up to 64 children are fetched by the lanes in
    // parallel and broadcast from registers; the loads of four children are in flight together,
    // the additions stay in child order (deterministic sums)
    for (int cbase = 0; cbase < F.nchild; cbase += 64) {
        const int nc = min(64, F.nchild - cbase);
        int64_t my_u = 0, my_r = 0;
        int my_b = 0;
        if (lane < nc) {
            const FrontDev C = fr[children[F.child_off + cbase + lane]];
            my_u = C.u_off;
            my_r = C.rel_off;
            my_b = C.m - C.k;
        }
        for (int c0 = 0; c0 < nc; c0 += 4) {
            int dst[4];
            double val[4];
            int bb[4];
            int64_t ru[4], rr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = min(c0 + u, nc - 1);
                bb[u] = (c0 + u < nc) ? __shfl(my_b, c, 64) : 0;
                ru[u] = __shfl(my_u, c, 64);
                rr[u] = __shfl(my_r, c, 64);
                dst[u] = -1;
                val[u] = 0.0;
                if (lane < bb[u]) {
                    dst[u] = rel[rr[u] + lane];
                    val[u] = uvec[ru[u] + lane];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u >= nc) break;
                if (dst[u] >= 0) t[dst[u]] += val[u];
                for (int j = lane + 64; j < bb[u]; j += 64) t[rel[rr[u] + j]] += uvec[ru[u] + j];
                wave_sync();
            }
        }
    }
    const int r1 = lane + 64;
    double t0 = (lane < m) ? t[lane] : 0.0;
    double t1 = (r1 < m) ? t[r1] : 0.0;
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
        const double* Lj = Fm + (int64_t)j * m;
        const double l0 = (lane > j && lane < m) ? Lj[lane] : 0.0;
        const double l1 = (r1 > j && r1 < m) ? Lj[r1] : 0.0;
        const double tj = (j < 64) ? readlane_f64(t0, j) : readlane_f64(t1, j - 64);   // j is wave-uniform
        t0 -= l0 * tj;
        t1 -= l1 * tj;
    }
    if (lane < m) {
        if (lane < k) y[idx[lane]] = t0 / Fm[lane + (int64_t)lane * m];
        else uvec[F.u_off + lane - k] = t0;
    }
    if (r1 < m) {
        if (r1 < k) y[idx[r1]] = t1 / Fm[r1 + (int64_t)r1 * m];
        else uvec[F.u_off + r1 - k] = t1;
    }
}

// KMAX > 0: every front of the launch has k <= KMAX pivots and the lane's entries of all pivot columns are requested
// before the first elimination step (the steps are a dependent chain; with the loads inside it every step paid a
// memory latency).  KMAX == 0: the rolled form.
template <int KMAX>
__global__ __launch_bounds__(256) void mf_backward_small(const FrontDev* __restrict__ fr, int32_t first,
                                                         int32_t count,
                                                         const int32_t* __restrict__ front_idx,
                                                         const double* __restrict__ arena,
                                                         const double* __restrict__ y, double* __restrict__ x) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fi = blockIdx.x * 4 + wave;
    if (fi >= count) return;
    const FrontDev F = fr[first + fi];
    const int m = F.m, k = F.k;
    const int32_t* idx = front_idx + F.idx_off;
    const double* Fm = arena + F.F_off;
    const int r1 = lane + 64;
    double t0 = 0.0, t1 = 0.0;
    if constexpr (KMAX > 0) {
        double l0[KMAX], l1[KMAX];
        const bool two = m > 64;                     // wave-uniform
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            l0[j] = (j < k && lane > j && lane < m) ? Fm[(int64_t)j * m + lane] : 0.0;
            l1[j] = (two && j < k && r1 < m) ? Fm[(int64_t)j * m + r1] : 0.0;        // r1 > j always (k <= KMAX <= 64)
        }
        if (lane < m) t0 = (lane < k) ? y[idx[lane]] : x[idx[lane]];
        if (r1 < m) t1 = (r1 < k) ? y[idx[r1]] : x[idx[r1]];
#pragma unroll
        for (int j = KMAX - 1; j >= 0; --j) {
            if (j < k) {
                double s = l0[j] * t0;
                if (two) s += l1[j] * t1;
                s = wave_sum_f64(s);
                if (lane == j) t0 -= s;
            }
        }
    } else {
        if (lane < m) t0 = (lane < k) ? y[idx[lane]] : x[idx[lane]];
        if (r1 < m) t1 = (r1 < k) ? y[idx[r1]] : x[idx[r1]];
#pragma unroll 2
        for (int j = k - 1; j >= 0; --j) {
            const double* Lj = Fm + (int64_t)j * m;
            double s = 0.0;
            if (lane > j && lane < m) s += Lj[lane] * t0;
            if (r1 > j && r1 < m) s += Lj[r1] * t1;
            s = wave_sum_f64(s);
            if (lane == j) t0 -= s;
            if (r1 == j) t1 -= s;
        }
    }
    if (lane < k) x[idx[lane]] = t0;
    if (r1 < k) x[idx[r1]] = t1;
}

// ---- leaf fronts with m <= 16 (the static-condensation leaves: one per element) -----------------
// A wave-per-front kernel leaves 3/4 of its lanes idle on these and pays a full LDS instruction
// per handful of entries.  Here 16 lanes own one front (4 fronts per wave, 16 per workgroup):
// lane r keeps row r of the front in registers, the column of multipliers is exchanged through a
// 16-double LDS line per front, and the triangular solves use width-16 shuffles.
__global__ __launch_bounds__(256) void mf_factor_tiny(const FrontDev* __restrict__ fr, int32_t first, int32_t count,
                                                      const int32_t* __restrict__ a_src,
                                                      const int32_t* __restrict__ a_dst,
                                                      const double* __restrict__ Hval, double* __restrict__ arena,
                                                      int32_t* __restrict__ status) {
    __shared__ double Wt[16][136];          // packed lower triangle, column stride 16 (a_dst is remapped by analyze())
    __shared__ double colb[16][16];
    const int g = threadIdx.x >> 4, r = threadIdx.x & 15;
    const int fi = blockIdx.x * 16 + g;
    const bool on = fi < count;
    const FrontDev F = fr[first + (on ? fi : 0)];
    const int m = F.m, k = on ? F.k : 0;
    double* W = Wt[g];
    for (int i = r; i < 136; i += 16) W[i] = 0.0;
    wave_sync();
    if (on)
        for (int t = r; t < F.a_cnt; t += 16) W[a_dst[F.a_off + t]] = Hval[a_src[F.a_off + t]];
    wave_sync();
    double a[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = (on && r < m && c <= r) ? W[c * 16 - c * (c - 1) / 2 + (r - c)] : 0.0;
    int kmax = k;
    kmax = max(kmax, __shfl_xor(kmax, 16, 64));
    kmax = max(kmax, __shfl_xor(kmax, 32, 64));
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j >= kmax) break;
        colb[g][r] = a[j];
        wave_sync();
        const bool act = j < k;
        const double d = colb[g][j];
        if (act && (d == 0.0 || !isfinite(d))) bad = true;
        const double lr = a[j] * fast_recip(act ? d : 1.0);
#pragma unroll
        for (int c = j + 1; c < 16; ++c) {
            const double v = colb[g][c];          // entry (c, j); rows >= m hold zeros
            if (act) a[c] -= lr * v;
        }
        if (act && r > j) a[j] = lr;
        wave_sync();
    }
    if (bad) atomicOr(status, 1);
    if (on && r < m) {
        double* Fg = arena + F.F_off;
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c <= r) Fg[tiny_entry(F, r, c)] = a[c];
    }
}

__global__ __launch_bounds__(256) void mf_forward_tiny(const FrontDev* __restrict__ fr, int32_t first, int32_t count,
                                                       const int32_t* __restrict__ front_idx,
                                                       const double* __restrict__ arena,
                                                       const double* __restrict__ b, double* __restrict__ y,
                                                       double* __restrict__ uvec) {
    const int g = threadIdx.x >> 4, r = threadIdx.x & 15;
    const int fi = blockIdx.x * 16 + g;
    const bool on = fi < count;
    const FrontDev F = fr[first + (on ? fi : 0)];
    const int m = F.m, k = on ? F.k : 0;
    const int32_t* idx = front_idx + F.idx_off;
    const double* Fm = arena + F.F_off;
    const bool row = on && r < m;
    const int myidx = row ? idx[r] : 0;
    double t = (row && r < k) ? b[myidx] : 0.0;
    double l[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) l[j] = (row && j < k && r > j) ? Fm[tiny_entry(F, r, j)] : 0.0;
    const double dr = (row && r < k) ? Fm[tiny_entry(F, r, r)] : 1.0;
    int kmax = k;
    kmax = max(kmax, __shfl_xor(kmax, 16, 64));
    kmax = max(kmax, __shfl_xor(kmax, 32, 64));
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j >= kmax) break;
        const double tj = __shfl(t, j, 16);
        t -= l[j] * tj;                            // l[j] = 0 outside (j < k, r > j)
    }
    if (row) {
        if (r < k) y[myidx] = t / dr;
        else uvec[F.u_off + r - k] = t;
    }
}

__global__ __launch_bounds__(256) void mf_backward_tiny(const FrontDev* __restrict__ fr, int32_t first, int32_t count,
                                                        const int32_t* __restrict__ front_idx,
                                                        const double* __restrict__ arena,
                                                        const double* __restrict__ y, double* __restrict__ x) {
    const int g = threadIdx.x >> 4, r = threadIdx.x & 15;
    const int fi = blockIdx.x * 16 + g;
    const bool on = fi < count;
    const FrontDev F = fr[first + (on ? fi : 0)];
    const int m = F.m, k = on ? F.k : 0;
    const int32_t* idx = front_idx + F.idx_off;
    const double* Fm = arena + F.F_off;
    const bool row = on && r < m;
    const int myidx = row ? idx[r] : 0;
    double t = row ? ((r < k) ? y[myidx] : x[myidx]) : 0.0;
    double l[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) l[j] = (row && j < k && r > j) ? Fm[tiny_entry(F, r, j)] : 0.0;
    int kmax = k;
    kmax = max(kmax, __shfl_xor(kmax, 16, 64));
    kmax = max(kmax, __shfl_xor(kmax, 32, 64));
#pragma unroll
    for (int j = 15; j >= 0; --j) {
        if (j >= kmax) continue;
        double s = l[j] * t;                       // rows r > j of column j (zero elsewhere)
        s = row16_sum_f64(s);
        if (r == j && j < k) t -= s;
    }
    if (row && r < k) x[myidx] = t;
}

// ---- host launchers ------------------------------------------------------------------------------------------
// mf_factor_small: LDS by factor_small_lds, threads per front by factor_small_threads (mf_launch_plan.hpp)
inline void launch_factor_small(const FactorArgs& a, const MfLaunch& L) {
    // 8-column LDS panels (16- and 32-column ones were measured slower in round 3 and removed in round 4)
    const int threads = factor_small_threads(L, a.compute_units, a.small_threads);
    MGB_REQUIRE(threads >= L.max_m - 1, "mf_factor_small: fewer threads than panel rows");      // one row per thread in the panel solve
    if (L.cls >= 88)
        hipLaunchKernelGGL((mf_factor_small<8, true>), dim3(L.count), dim3(threads), factor_small_lds(L.cls), a.st, a.fr, L.first,
                           a.children, a.rel, a.a_src, a.a_dst, a.values, a.arena, a.status);
    else
        hipLaunchKernelGGL((mf_factor_small<8, false>), dim3(L.count), dim3(threads), factor_small_lds(L.cls), a.st, a.fr, L.first,
                           a.children, a.rel, a.a_src, a.a_dst, a.values, a.arena, a.status);
}

// mf_factor_wave: four packed triangles + the staged child descriptors of four waves
template <int MW>
inline size_t factor_wave_lds() {
    return (size_t)4 * (MW * (MW + 1) / 2) * sizeof(double) + 4 * 64 * (sizeof(int64_t) + sizeof(int32_t));
}
template <int MW>
inline void launch_factor_wave(const FactorArgs& a, const MfLaunch& L) {
    hipLaunchKernelGGL(mf_factor_wave<MW>, dim3((L.count + 3) / 4), dim3(256), factor_wave_lds<MW>(), a.st, a.fr, L.first, L.count,
                       a.children, a.rel, a.a_src, a.a_dst, a.values, a.arena, a.status);
}

inline void launch_factor_tiny(const FactorArgs& a, const MfLaunch& L) {
    hipLaunchKernelGGL(mf_factor_tiny, dim3((L.count + 15) / 16), dim3(256), 0, a.st, a.fr, L.first, L.count, a.a_src, a.a_dst,
                       a.values, a.arena, a.status);
}

inline void launch_forward_tiny(const SolveArgs& a, const MfLaunch& L) {
    hipLaunchKernelGGL(mf_forward_tiny, dim3((L.count + 15) / 16), dim3(256), 0, a.st, a.fr, L.first, L.count, a.front_idx,
                       a.arena, a.b, a.y, a.uvec);
}
inline void launch_backward_tiny(const SolveArgs& a, const MfLaunch& L) {
    hipLaunchKernelGGL(mf_backward_tiny, dim3((L.count + 15) / 16), dim3(256), 0, a.st, a.fr, L.first, L.count, a.front_idx,
                       a.arena, a.y, a.x);
}

inline size_t forward_small_lds(int ts) { return (size_t)4 * ts * sizeof(double); }     // one work vector per wave
inline void launch_forward_small(const SolveArgs& a, const MfLaunch& L) {
    const int ts = (L.max_m + 1) & ~1;
    hipLaunchKernelGGL(mf_forward_small, dim3((L.count + 3) / 4), dim3(256), forward_small_lds(ts), a.st, a.fr, L.first, L.count,
                       ts, a.front_idx, a.children, a.rel, a.arena, a.b, a.y, a.uvec);
}
template <int KMAX>
inline void launch_backward_small_k(const SolveArgs& a, const MfLaunch& L) {
    hipLaunchKernelGGL(mf_backward_small<KMAX>, dim3((L.count + 3) / 4), dim3(256), 0, a.st, a.fr, L.first, L.count, a.front_idx,
                       a.arena, a.y, a.x);
}
inline void launch_backward_small(const SolveArgs& a, const MfLaunch& L) {
    const int kmax = backward_small_kmax(L);        // mf_launch_plan.hpp
    if (kmax == 8) launch_backward_small_k<8>(a, L);
    else if (kmax == 16) launch_backward_small_k<16>(a, L);
    else launch_backward_small_k<0>(a, L);
}

}  // namespace
}  // namespace mgbhip
