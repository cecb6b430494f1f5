// panel_kernels.hpp -- coarse-level panel projection and accumulation (included by kernels.hip).
#pragma once
#include <algorithm>

#include "reduce_kernels.hpp"

namespace mgbhip {

namespace {

// General (coarse) levels: one wave per element computes the projected block
// [panel_0 .. panel_{nu-1}]' * Hel_e * [panel_0 .. panel_{nu-1}] in two steps per block pair
// (tmp = Hel_ab * panel_b in LDS, then panel_a' * tmp) into the element's slab; the structural
// nonzeros of H gather from the slab afterwards (deterministic, no atomics).
__global__ __launch_bounds__(256) void panel_project_kernel(const PanelParams P) {
    extern __shared__ double sh[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wave;
    if (e >= P.N) return;
    const int p = P.p, nu = P.nu;
    const int NB2 = nu * (nu + 1) / 2;
    double* tmp = sh + (size_t)wave * p * P.cmax;
    const int32_t base = P.ecol_ptr[e * nu];
    const int32_t ct = P.ecol_ptr[(e + 1) * nu] - base;
    for (int a = 0; a < nu; ++a) {
        const int32_t oa = P.ecol_ptr[e * nu + a], ca = P.ecol_ptr[e * nu + a + 1] - oa;
        const double* pa = P.panels + (int64_t)p * oa;
        for (int b = P.upper_only ? a : 0; b < nu; ++b) {        // upper_only: block pairs below the diagonal are never read
            const int32_t ob = P.ecol_ptr[e * nu + b], cb = P.ecol_ptr[e * nu + b + 1] - ob;
            const double* pb = P.panels + (int64_t)p * ob;
            const bool tr = a > b;
            const int blk = tr ? (b * nu - (b * (b - 1)) / 2 + (a - b)) : (a * nu - (a * (a - 1)) / 2 + (b - a));
            const double* Hb = P.hel + ((int64_t)blk * P.N + e) * (int64_t)p * p;
            for (int t = lane; t < p * cb; t += 64) {
                const int rr = t % p, ib = t / p;
                double acc = 0.0;
                for (int ss = 0; ss < p; ++ss) acc += (tr ? Hb[ss + p * rr] : Hb[rr + p * ss]) * pb[ss + p * ib];
                tmp[t] = acc;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int t = lane; t < ca * cb; t += 64) {
                const int ia = t % ca, ib = t / ca;
                if (P.upper_only && a == b && ia > ib) continue;
                double acc = 0.0;
                for (int rr = 0; rr < p; ++rr) acc += pa[rr + p * ia] * tmp[rr + p * ib];
                const int64_t o = P.eoff[e] + (oa - base + ia) + (int64_t)ct * (ob - base + ib);
                P.slab[P.spos ? P.spos[o] : o] = acc;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

// Small coarse levels whose basis functions overlap almost everywhere (3-D hierarchies): a per-element
// slab would hold sum_e ct_e^2 doubles for an m x m system of a few hundred unknowns, and the gather
// behind it reads them back at random.  Instead a workgroup owns a stream of elements and a chunk of the
// packed upper triangle of H as an LDS accumulator: per element the panels, blocks and T = Hel * P are
// staged in LDS, the projected entries that fall into the chunk are added in place (no global
// read-modify-write, no atomics), and at the end the chunk goes to the stream's partial result.  A
// second kernel sums the streams in order.  Deterministic; traffic = inputs + nstream * m^2 / 2 doubles.
__global__ __launch_bounds__(256) void panel_accumulate_kernel(const PanelParams P, const int32_t* __restrict__ ecols,
                                                               int32_t m, int32_t ctmax, int32_t chunk,
                                                               double* __restrict__ partial) {
    extern __shared__ double sh[];
    const int tid = threadIdx.x;
    const int nstream = gridDim.x, stream = blockIdx.x;
    const int p = P.p, nu = P.nu;
    const int nblk = nu * (nu + 1) / 2;
    const int64_t mt = (int64_t)m * (m + 1) / 2;       // packed upper triangle: (gi <= gj) at gi + gj (gj + 1) / 2
    const int64_t lo = (int64_t)blockIdx.y * chunk;
    const int64_t hi = lo + chunk < mt ? lo + chunk : mt;
    double* acc = sh;                                  // [chunk]
    double* Pl = acc + chunk;                          // Pl[rr + p*j]
    double* Hl = Pl + (size_t)p * ctmax;               // Hl[blk*p*p + rr + p*ss]
    double* Tl = Hl + (size_t)nblk * p * p;            // Tl[(a*p + rr) + nu*p*j]
    int32_t* cl = reinterpret_cast<int32_t*>(Tl + (size_t)nu * p * ctmax);   // cl[j] column, cl[ctmax + j] state
    for (int t = tid; t < chunk; t += 256) acc[t] = 0.0;
    const int nrow = nu * p;
    // The staging data of the NEXT element travel in registers while the current one is processed
    // (launch_panel_accumulate guarantees p*ctmax <= 4*256, nblk*p*p <= 3*256, ctmax <= 256).
    double rP[4], rH[3];
    int32_t rC = 0, rS = 0, nbase = 0, nct = 0;
    auto prefetch = [&](int64_t e) {
        nbase = P.ecol_ptr[e * nu];
        nct = P.ecol_ptr[(e + 1) * nu] - nbase;
        if (tid < nct) {
            rC = ecols[nbase + tid];
            int st = 0;
            for (int a = 1; a < nu; ++a)
                if (nbase + tid >= P.ecol_ptr[e * nu + a]) st = a;
            rS = st;
        }
        const double* pan = P.panels + (int64_t)p * nbase;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = tid + 256 * k;
            rP[k] = t < p * nct ? pan[t] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = tid + 256 * k;
            if (t < nblk * p * p) {
                const int blk = t / (p * p), q = t - blk * (p * p);
                rH[k] = P.hel[((int64_t)blk * P.N + e) * (int64_t)(p * p) + q];
            }
        }
    };
    if (stream < P.N) prefetch(stream);
    for (int64_t e = stream; e < P.N; e += nstream) {
        const int32_t ct = nct;
        __syncthreads();                               // previous element's LDS operands are no longer read
        if (tid < ct) { cl[tid] = rC; cl[ctmax + tid] = rS; }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = tid + 256 * k;
            if (t < p * ct) Pl[t] = rP[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = tid + 256 * k;
            if (t < nblk * p * p) Hl[t] = rH[k];
        }
        __syncthreads();
        if (e + nstream < P.N) prefetch(e + nstream);  // in flight during the two product phases below
        // columns whose packed positions can fall into this workgroup's chunk [lo, hi)
        int jlo, jhi;
        {
            int a0 = 0, a1 = ct;                       // first column whose largest position reaches lo
            while (a0 < a1) {
                const int mid = (a0 + a1) >> 1;
                const int64_t g = cl[mid];
                if (g + g * (g + 1) / 2 < lo) a0 = mid + 1; else a1 = mid;
            }
            jlo = a0;
            a0 = jlo; a1 = ct;                         // first column whose smallest position is >= hi
            const int64_t g0 = cl[0];
            while (a0 < a1) {
                const int mid = (a0 + a1) >> 1;
                const int64_t g = cl[mid];
                if (g0 + g * (g + 1) / 2 < hi) a0 = mid + 1; else a1 = mid;
            }
            jhi = a0;
        }
        const float inv_nrow = 1.0f / (float)nrow;
        for (int t = tid + nrow * jlo; t < nrow * jhi; t += 256) {   // T[a][rr][j] = sum_ss Hel_{a, b(j)}[rr][ss] * P[ss][j], j in [jlo, jhi)
            int j = (int)(((float)t + 0.5f) * inv_nrow);
            if (j * nrow > t) --j;
            if ((j + 1) * nrow <= t) ++j;
            const int row = t - j * nrow;
            const int a = row / p, rr = row - a * p;
            const int b = cl[ctmax + j];
            const bool tr = a > b;
            const int blk = tr ? (b * nu - (b * (b - 1)) / 2 + (a - b)) : (a * nu - (a * (a - 1)) / 2 + (b - a));
            const double* Hb = Hl + (size_t)blk * p * p;
            double v = 0.0;
            for (int ss = 0; ss < p; ++ss) v += (tr ? Hb[ss + p * rr] : Hb[rr + p * ss]) * Pl[ss + p * j];
            Tl[row + nrow * j] = v;
        }
        __syncthreads();
        // B[i][j] for the pairs i <= j (the element's columns are sorted, so gi <= gj) whose packed
        // position falls into this workgroup's chunk.  Positions grow with t = i + j (j + 1) / 2, so
        // the chunk is a contiguous t range: bracket it by columns, then enumerate only that range.
        const int tbeg = jlo * (jlo + 1) / 2, tend = jhi * (jhi + 1) / 2;
        for (int t = tbeg + tid; t < tend; t += 256) {
            int j = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
            while ((j + 1) * (j + 2) / 2 <= t) ++j;
            while (j * (j + 1) / 2 > t) --j;
            const int i = t - j * (j + 1) / 2;
            const int64_t gi = cl[i], gj = cl[j];
            const int64_t pos = gi + gj * (gj + 1) / 2;
            if (pos < lo || pos >= hi) continue;
            const int a = cl[ctmax + i];
            double v = 0.0;
            for (int rr = 0; rr < p; ++rr) v += Pl[rr + p * i] * Tl[(a * p + rr) + nrow * j];
            acc[pos - lo] += v;                        // distinct (gi, gj) per thread within an element
        }
    }
    __syncthreads();
    double* out = partial + (int64_t)stream * mt + lo;
    for (int t = tid; t < (int)(hi - lo); t += 256) out[t] = acc[t];
}

// H[i, j] = H[j, i] = sum over the streams' partial results, in stream order (i <= j)
__global__ __launch_bounds__(256) void accumulate_reduce_kernel(int32_t m, int32_t nstream, const double* __restrict__ partial,
                                                                double* __restrict__ H) {
    const int64_t mt = (int64_t)m * (m + 1) / 2;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)m * m) return;
    const int i = (int)(q % m), j = (int)(q / m);
    if (i > j) return;
    const double* src = partial + (int64_t)i + ((int64_t)j * (j + 1)) / 2;
    double s = 0.0;
    int w = 0;
    for (; w + 8 <= nstream; w += 8) {          // eight independent loads in flight, fixed summation order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(w + u) * mt];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; w < nstream; ++w) s += src[(int64_t)w * mt];
    H[(int64_t)i * m + j] = s;
    H[(int64_t)j * m + i] = s;
}

// Slab variant of the same staging (levels that keep the slab + gather path): the element's
// panels, blocks and T = Hel * P live in LDS, the ct x ct projected block is written with flat
// coalesced stores.  Replaces the per-block-pair loops of panel_project_kernel, which re-read the
// panels from L2 for every output entry.
__global__ __launch_bounds__(256) void panel_project_staged_kernel(const PanelParams P, int32_t ctmax) {
    extern __shared__ double sh[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wave;
    if (e >= P.N) return;
    const int p = P.p, nu = P.nu;
    const int nblk = nu * (nu + 1) / 2;
    const size_t per_wave = (size_t)p * ctmax + (size_t)nblk * p * p + (size_t)nu * p * ctmax + ctmax;
    double* Pl = sh + (size_t)wave * per_wave;
    double* Hl = Pl + (size_t)p * ctmax;
    double* Tl = Hl + (size_t)nblk * p * p;
    int32_t* sl = reinterpret_cast<int32_t*>(Tl + (size_t)nu * p * ctmax);   // sl[j]: state of column j
    const int32_t base = P.ecol_ptr[e * nu];
    const int32_t ct = P.ecol_ptr[(e + 1) * nu] - base;
    for (int j = lane; j < ct; j += 64) {
        int st = 0;
        for (int a = 1; a < nu; ++a)
            if (base + j >= P.ecol_ptr[e * nu + a]) st = a;
        sl[j] = st;
    }
    const double* pan = P.panels + (int64_t)p * base;
    for (int t = lane; t < p * ct; t += 64) Pl[t] = pan[t];
    for (int blk = 0; blk < nblk; ++blk) {
        const double* hb = P.hel + ((int64_t)blk * P.N + e) * (int64_t)(p * p);
        for (int q = lane; q < p * p; q += 64) Hl[blk * p * p + q] = hb[q];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int nrow = nu * p;
    const float inv_nrow = 1.0f / (float)nrow, inv_ct = 1.0f / (float)ct;
    for (int t = lane; t < nrow * ct; t += 64) {
        int j = (int)(((float)t + 0.5f) * inv_nrow);
        if (j * nrow > t) --j;
        if ((j + 1) * nrow <= t) ++j;
        const int row = t - j * nrow;
        const int a = row / p, rr = row - a * p;
        const int b = sl[j];
        const bool tr = a > b;
        const int blk = tr ? (b * nu - (b * (b - 1)) / 2 + (a - b)) : (a * nu - (a * (a - 1)) / 2 + (b - a));
        const double* Hb = Hl + (size_t)blk * p * p;
        double acc = 0.0;
        for (int ss = 0; ss < p; ++ss) acc += (tr ? Hb[ss + p * rr] : Hb[rr + p * ss]) * Pl[ss + p * j];
        Tl[row + nrow * j] = acc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int64_t eo = P.eoff[e];
    if (P.upper_only) {                     // the Newton loop reads entries i <= j only (the element's columns are sorted)
        for (int t = lane; t < ct * (ct + 1) / 2; t += 64) {
            int j = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
            while ((j + 1) * (j + 2) / 2 <= t) ++j;
            while (j * (j + 1) / 2 > t) --j;
            const int i = t - j * (j + 1) / 2;
            const int a = sl[i];
            double acc = 0.0;
            for (int rr = 0; rr < p; ++rr) acc += Pl[rr + p * i] * Tl[(a * p + rr) + nrow * j];
            const int64_t o = eo + i + ct * j;
            P.slab[P.spos ? P.spos[o] : o] = acc;
        }
        return;
    }
    for (int t = lane; t < ct * ct; t += 64) {
        int j = (int)(((float)t + 0.5f) * inv_ct);
        if (j * ct > t) --j;
        if ((j + 1) * ct <= t) ++j;
        const int i = t - j * ct;
        const int a = sl[i];
        double acc = 0.0;
        for (int rr = 0; rr < p; ++rr) acc += Pl[rr + p * i] * Tl[(a * p + rr) + nrow * j];
        P.slab[P.spos ? P.spos[eo + t] : eo + t] = acc;                       // entry i + ct * j of the element's block
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// Projection on the matrix cores (round 4).  The loop kernels above spend their time decoding flat indices and on two LDS
// reads per multiply-add; the arithmetic itself is two small dense products per element and state pair (a, b),
//     U = Hel_ab * P_b   (p x c_b)      and      B_ab = P_a' U   (c_a x c_b, K = p),
// i.e. 16 x 16 tiles of v_mfma_f64_16x16x4 with K = p padded to a multiple of 4.  The element's columns are laid out with
// every state's range padded to a multiple of 16, so a tile belongs to one state; `cmap` takes a padded column back to the
// element's compact index, -1 for padding.  One workgroup per element, its four waves share the tile pairs I <= J; U never
// touches LDS: register r of the first product's result, D[i = fk + 4 r][j = fr], IS the second product's B operand of
// k-step r (B[k = 4 r + fk][j = fr]).  LDS holds P and the element block only (13 KB at 96 padded columns: eight
// workgroups per compute unit; a first version that staged T = Hel P kept three, and the launch is latency-bound:
// processing several elements per workgroup in sequence was slower still).
// Operand convention of the instruction as used throughout this library (mf_numeric.hip): lane (fr = lane & 15,
// fk = lane >> 4) supplies A[i = fr][k = fk] and B[k = fk][j = fr]; afterwards register r holds D[i = fk + 4 r][j = fr].
typedef double pp_double4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int pp_round_up(int v, int q) { return (v + q - 1) / q * q; }

struct PanelMfmaLayout {          // LDS layout in doubles (host and device agree through this one function)
    int ppad, KP, NR, HC, oP, oH, oC, total;
};
__host__ __device__ inline PanelMfmaLayout panel_mfma_layout(int p, int nu, int ctpad) {
    PanelMfmaLayout L;
    L.ppad = pp_round_up(p, 4);
    L.KP = L.ppad + 1;                               // leading dimension of P (k fastest)
    L.NR = nu * p + 1;                               // leading dimension of the symmetric element block (row fastest)
    L.HC = nu * L.ppad;                              // its columns: state b, k padded (zeros)
    L.oP = 0;
    L.oH = L.oP + L.KP * ctpad;
    L.oC = L.oH + L.NR * L.HC;
    L.total = L.oC + (ctpad + 1) / 2 + 8;            // cmap: ctpad int32
    return L;
}

__global__ __launch_bounds__(256) void panel_project_mfma_kernel(const PanelParams P, int32_t ctpad_max) {
    extern __shared__ double sh[];
    static_assert(MGBHIP_MAX_NU == 4, "the state offsets below are written out for four states");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t e = blockIdx.x;
    const int p = P.p, nu = P.nu, pp = p * p;
    const int nblk = nu * (nu + 1) / 2;
    const PanelMfmaLayout Y = panel_mfma_layout(p, nu, ctpad_max);
    double* Pl = sh + Y.oP;
    double* Hf = sh + Y.oH;
    int32_t* cmap = reinterpret_cast<int32_t*>(sh + Y.oC);
    // compact (c) and padded (q) start of every state's column range, as scalars (an indexed array would live in scratch)
    const int32_t* ec = P.ecol_ptr + e * nu;
    const int32_t cbase = ec[0];
    const int w0 = ec[1] - cbase, w1 = nu > 1 ? ec[2] - ec[1] : 0, w2 = nu > 2 ? ec[3] - ec[2] : 0, w3 = nu > 3 ? ec[4] - ec[3] : 0;
    const int c1 = w0, c2 = c1 + w1, c3 = c2 + w2, ct = c3 + w3;
    const int q1 = pp_round_up(w0, 16), q2 = q1 + pp_round_up(w1, 16), q3 = q2 + pp_round_up(w2, 16), ctpad = q3 + pp_round_up(w3, 16);
    const int nJt = ctpad / 16;                      // ctpad <= ctpad_max by construction of the launch
    auto state_of_padded = [&](int jp) { return (jp >= q1 && nu > 1) + (jp >= q2 && nu > 2) + (jp >= q3 && nu > 3); };
    auto qoff = [&](int a) { return a == 0 ? 0 : a == 1 ? q1 : a == 2 ? q2 : q3; };
    auto coff = [&](int a) { return a == 0 ? 0 : a == 1 ? c1 : a == 2 ? c2 : c3; };
    auto wid = [&](int a) { return a == 0 ? w0 : a == 1 ? w1 : a == 2 ? w2 : w3; };
    // ---- stage: P in gather form (zeros in the padding), the symmetric element block (zero padding columns), cmap -----
    const double* pan = P.panels + (int64_t)p * cbase;
    for (int t = tid; t < Y.KP * ctpad; t += 256) {
        const int jp = t / Y.KP, k = t - jp * Y.KP;
        const int a = state_of_padded(jp);
        const int ia = jp - qoff(a);
        const bool real = k < p && ia < wid(a);
        Pl[t] = real ? pan[k + p * (coff(a) + ia)] : 0.0;
        if (k == 0) cmap[jp] = ia < wid(a) ? coff(a) + ia : -1;
    }
    for (int t = tid; t < Y.NR * Y.HC; t += 256) Hf[t] = 0.0;
    __syncthreads();
    for (int t = tid; t < nblk * pp; t += 256) {
        const int blk = t / pp, q = t - blk * pp;
        const int ss = q / p, rr = q - ss * p;       // Hel_ab[rr + p ss], a <= b
        int a = 0, rem = blk;
        while (rem >= nu - a) { rem -= nu - a; ++a; }
        const int b = a + rem;
        const double v = P.hel[((int64_t)blk * P.N + e) * (int64_t)pp + q];
        Hf[(a * p + rr) + Y.NR * (b * Y.ppad + ss)] = v;
        if (a != b) Hf[(b * p + ss) + Y.NR * (a * Y.ppad + rr)] = v;
    }
    __syncthreads();
    const int fr = lane & 15, fk = lane >> 4;
    const int ksteps = Y.ppad / 4;                   // <= 16 (p <= 64)
    const int64_t eo = P.eoff[e];
    // ---- tile pairs I <= J: U = Hel_ab P_J (p x 16, in the accumulators), B = P_I' U --------------------------------
    const int npair = nJt * (nJt + 1) / 2;
    for (int tile = wave; tile < npair; tile += 4) {
        int J = 0, rem = tile;
        while (rem > J) { rem -= J + 1; ++J; }
        const int I = rem;                           // I <= J
        const int a = state_of_padded(16 * I), b = state_of_padded(16 * J);
        pp_double4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int rt = 0; rt < ksteps; rt += 4) {     // 16 rows of U at a time: rows 4 rt .. 4 rt + 15 of the p (padded) rows
            pp_double4 u = {0.0, 0.0, 0.0, 0.0};
            const int urow = 4 * rt + fr;            // A operand row of U's tile
            for (int kk = 0; kk < ksteps; ++kk)
                u = __builtin_amdgcn_mfma_f64_16x16x4f64(urow < p ? Hf[(a * p + urow) + Y.NR * (b * Y.ppad + 4 * kk + fk)] : 0.0,
                                                        Pl[(4 * kk + fk) + Y.KP * (16 * J + fr)], u, 0, 0, 0);
            // u[r] = U[4 rt + fk + 4 r][j = fr]: the B operand of k-step rt + r
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (rt + r < ksteps)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Pl[(4 * (rt + r) + fk) + Y.KP * (16 * I + fr)], u[r], acc, 0, 0, 0);
        }
        const int cj = cmap[16 * J + fr];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = cmap[16 * I + fk + 4 * r];
            if (ci < 0 || cj < 0) continue;
            if (ci <= cj) {
                const int64_t o = eo + ci + (int64_t)ct * cj;
                P.slab[P.spos ? P.spos[o] : o] = acc[r];
            }
            if (!P.upper_only && (I != J ? true : ci > cj)) {      // the other triangle: mirror of an off-diagonal tile, or
                const int64_t o = I != J ? eo + cj + (int64_t)ct * ci : eo + ci + (int64_t)ct * cj;   // the lower half of a diagonal one
                P.slab[P.spos ? P.spos[o] : o] = acc[r];
            }
        }
    }
}

__global__ __launch_bounds__(256) void invert_lists_kernel(const int32_t* __restrict__ cidx, int64_t total, int32_t* __restrict__ spos) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < total) spos[cidx[t]] = (int32_t)t;
}

}  // namespace

void launch_panel_accumulate(const PanelParams& P, const int32_t* ecols, int32_t m, int32_t nstream, int32_t nsplit,
                             int32_t chunk, int32_t ctmax, double* partial, double* H, hipStream_t st) {
    if (m == 0) return;
    const size_t lds = ((size_t)chunk + panel_stage_doubles(P.p, P.nu, ctmax)) * sizeof(double);
    MGB_REQUIRE(lds <= PANEL_ACC_LDS_MAX, "coarse-level accumulator + panels exceed the LDS budget");
    MGB_REQUIRE(panel_accumulate_fits(P.p, P.nu, ctmax), "coarse-level panels exceed the register staging of the accumulation kernel");
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute((const void*)panel_accumulate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)PANEL_ACC_LDS_MAX);
        (void)hipGetLastError();
    });
    hipLaunchKernelGGL(panel_accumulate_kernel, dim3((unsigned)nstream, (unsigned)nsplit), dim3(256), lds, st, P, ecols, m,
                       ctmax, chunk, partial);
    hipLaunchKernelGGL(accumulate_reduce_kernel, dim3((unsigned)(((int64_t)m * m + 255) / 256)), dim3(256), 0, st, m,
                       nstream, partial, H);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_panel_project_staged(const PanelParams& P, int32_t ctmax, hipStream_t st) {
    if (P.N == 0) return;
    const size_t lds = panel_accumulate_lds(P.p, P.nu, ctmax);
    MGB_REQUIRE(lds <= PANEL_ACC_LDS_MAX, "coarse-level panels too wide for the staged projection kernel");
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute((const void*)panel_project_staged_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)PANEL_ACC_LDS_MAX);
        (void)hipGetLastError();
    });
    hipLaunchKernelGGL(panel_project_staged_kernel, dim3((unsigned)((P.N + 3) / 4)), dim3(256), lds, st, P, ctmax);
    MGB_HIP_CHECK(hipGetLastError());
}

bool launch_panel_project_mfma(const PanelParams& P, hipStream_t st) {
    if (P.N == 0) return true;
    if (P.nu > MGBHIP_MAX_NU || P.p > 64) return false;
    const int ctpad = P.nu * pp_round_up(P.cmax, 16);            // every state's range padded to a tile
    const PanelMfmaLayout Y = panel_mfma_layout(P.p, P.nu, ctpad);
    const size_t lds = (size_t)Y.total * sizeof(double);
    static const bool off = env_on("MGBHIP_NO_MFMA_PROJECT");
    // narrow supports (2-D hierarchies: a dozen columns per element) are faster through the staged loop kernel, four elements
    // per workgroup (L = 9: 120 us per launch); wide ones (3-D) are not
    if (off || lds > 64 * 1024 || ctpad < 48) return false;
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute((const void*)panel_project_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        (void)hipGetLastError();
    });
    hipLaunchKernelGGL(panel_project_mfma_kernel, dim3((unsigned)P.N), dim3(256), lds, st, P, ctpad);
    MGB_HIP_CHECK(hipGetLastError());
    return true;
}

void launch_invert_lists(const int32_t* cidx, int64_t total, int32_t* spos, hipStream_t st) {
    if (total <= 0) return;
    hipLaunchKernelGGL(invert_lists_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cidx, total, spos);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_panel_project(const PanelParams& P, hipStream_t st) {
    if (P.N == 0) return;
    const size_t lds = (size_t)4 * P.p * P.cmax * sizeof(double);
    // 64-node elements with full-width panels (fem3d k = 3 on a geometric ladder) need 128 KB: opt in once
    static const bool big_lds = hipFuncSetAttribute((const void*)panel_project_kernel,
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024) == hipSuccess;
    if (!big_lds) (void)hipGetLastError();
    MGB_REQUIRE(lds <= (big_lds ? 144 : 64) * 1024, "coarse-level panels too wide for the projection kernel");
    hipLaunchKernelGGL(panel_project_kernel, dim3((unsigned)((P.N + 3) / 4)), dim3(256), lds, st, P);
    MGB_HIP_CHECK(hipGetLastError());
}

}  // namespace mgbhip
