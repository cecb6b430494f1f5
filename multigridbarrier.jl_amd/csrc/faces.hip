// faces.hip -- the facets of a mesh (mgbhip_faces_*): which (element, local face) pairs are the two sides of one face
// and which lie on the boundary, and on them the integrals of u and of the flux a(grad u) . n over the boundary and of
// the squared jumps of u and of the normal flux over the interior faces.
//
// Topology.  One lane per incidence i = element * F + local face forms a key from the sorted global ids of the face's
// corner nodes (two ids in 2-D, the three smallest of four in 3-D).  The keys go through the one stable pair sort of
// device_prims.hpp -- in one pass while the key fits a 64-bit word, else in two stable passes, lowest id first -- and a
// run of equal keys is one face: one incidence is a boundary face, two are the L (lower incidence) and R sides of an
// interior face, more is an error.  The run heads scatter flags back to incidence order, two integer scans number the
// boundary faces in ascending incidence and the interior faces in ascending L incidence, and an emit pass writes the
// arrays.  No atomics and no floating point: the numbering is fixed by the mesh alone.
//
// Face quantities.  The host hands over, per local face, the rule's points and the basis at them (phi, dphi), the
// reference tangents and the reference outward normal, so nothing here knows an element family.  One lane takes one
// (face, point) pair; at point q of local face f of an element with nodes x_i and values z_i
//   J = sum_i x_i (grad_xi phi_i)^T,  C = cof J (J^-T = C / det J),  grad u = C (sum_i (z_i - z_0) grad_xi phi_i) / det J,
//   n = C n_ref / |C n_ref|,  ds = wf_q |J t| (2-D) or wf_q |J t1 x J t2| (3-D),  a = |grad u|^(p-2) grad u (0 at grad u = 0).
// Every sum over the nodes is a chain of fused multiply-adds in node order; the file is compiled like quadrature.hip,
// with the compiler's default contraction (fast: a product feeding a sum may be fused, which only removes roundings).
// An interior face evaluates each side through its own element map, the R side at point perm[orientation][q].
//
// Summation order.  No atomics.  The Qf terms of a face are added by a halving tree over its Qf lanes (the lines of
// quadrature.hip's), which depends on Qf alone; totals are the column reduction of quad_device.hpp over the faces (or the
// elements): the very kernel quadrature.hip runs.  The indicator gathers an element's interior faces through
// element_faces in local face order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "device_prims.hpp"
#include "faces.hpp"
#include "quad_device.hpp"

namespace mgbhip {

namespace {

// ---- topology -------------------------------------------------------------------------------------------------------

// khi / klo of incidence i from the sorted corner ids; shift = bits per id.  One word: khi holds every id (klo unused).
template <int NC>
__global__ void __launch_bounds__(BLOCK) face_key_kernel(int64_t M, int F, int p, const int32_t* __restrict__ t,
                                                         const int32_t* __restrict__ corners, unsigned shift, int two_words,
                                                         uint64_t* __restrict__ khi, uint32_t* __restrict__ klo,
                                                         int32_t* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int64_t e = i / F;
    const int f = (int)(i - e * F);
    uint64_t id[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) id[c] = (uint64_t)(uint32_t)t[e * p + corners[f * NC + c]];
    auto cswap = [](uint64_t& a, uint64_t& b) {
        const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
        a = lo;
        b = hi;
    };
    if constexpr (NC == 2) {
        cswap(id[0], id[1]);
        khi[i] = (id[0] << shift) | id[1];
    } else {
        cswap(id[0], id[1]); cswap(id[2], id[3]); cswap(id[0], id[2]); cswap(id[1], id[3]); cswap(id[1], id[2]);
        if (two_words) {
            khi[i] = (id[0] << shift) | id[1];
            klo[i] = (uint32_t)id[2];
        } else {
            khi[i] = (id[0] << (2 * shift)) | (id[1] << shift) | id[2];
        }
    }
    val[i] = (int32_t)i;
}

__global__ void __launch_bounds__(BLOCK) face_gather_kernel(int64_t M, const uint64_t* __restrict__ khi,
                                                            const int32_t* __restrict__ val, uint64_t* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < M) out[j] = khi[val[j]];
}

// sv: the incidences in key order (stable: ascending within a run).  The head of a run writes, for every incidence of the
// run, is_b (a boundary face), is_i (the L side of an interior face), partner (the other side, or -1) and over (the length of
// a run of more than two, at its head): every entry is written exactly once.
__global__ void __launch_bounds__(BLOCK) face_run_kernel(int64_t M, const int32_t* __restrict__ sv, const uint64_t* __restrict__ khi,
                                                         const uint32_t* __restrict__ klo, int two_words,
                                                         int32_t* __restrict__ is_b, int32_t* __restrict__ is_i,
                                                         int32_t* __restrict__ partner, int32_t* __restrict__ over) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const int32_t v = sv[j];
    auto same = [&](int32_t a, int32_t b) { return khi[a] == khi[b] && (!two_words || klo[a] == klo[b]); };
    if (j > 0 && same(sv[j - 1], v)) return;
    int64_t c = 1;
    while (j + c < M && same(v, sv[j + c])) ++c;
    for (int64_t m = 0; m < c; ++m) {
        const int32_t w = sv[j + m];
        is_b[w] = c == 1 ? 1 : 0;
        is_i[w] = (c == 2 && m == 0) ? 1 : 0;
        partner[w] = c == 2 ? sv[j + 1 - m] : -1;
        over[w] = (c > 2 && m == 0) ? (int32_t)c : 0;
    }
}

// The arrays in their final numbering.  The orientation code of an interior face: i0, i1 = where L's first two face
// corners sit among R's face corners; 2-D: i0; 3-D: 2 i0 + (0 if L's first face axis runs along R's first, 1 along R's
// second); -1 if they are not there or not neighbours (the host refuses the mesh).
template <int NC>
__global__ void __launch_bounds__(BLOCK) face_emit_kernel(int64_t M, int F, int p, const int32_t* __restrict__ t,
                                                          const int32_t* __restrict__ corners, const int32_t* __restrict__ is_b,
                                                          const int32_t* __restrict__ is_i, const int32_t* __restrict__ partner,
                                                          const int32_t* __restrict__ off_b, const int32_t* __restrict__ off_i,
                                                          int32_t* __restrict__ boundary, int32_t* __restrict__ interior,
                                                          int32_t* __restrict__ orientation, int32_t* __restrict__ element_faces) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int64_t e = i / F;
    const int f = (int)(i - e * F);
    if (is_b[i]) {
        const int32_t b = off_b[i];
        boundary[2 * (int64_t)b] = (int32_t)e;
        boundary[2 * (int64_t)b + 1] = f;
        element_faces[i] = -1 - b;
    } else if (is_i[i]) {
        const int64_t idx = off_i[i];
        const int64_t r = partner[i];
        const int64_t er = r / F;
        const int fr = (int)(r - er * F);
        interior[4 * idx] = (int32_t)e;
        interior[4 * idx + 1] = f;
        interior[4 * idx + 2] = (int32_t)er;
        interior[4 * idx + 3] = fr;
        element_faces[i] = (int32_t)idx;
        element_faces[r] = (int32_t)idx;
        const int32_t c0 = t[e * p + corners[f * NC]], c1 = t[e * p + corners[f * NC + 1]];
        int i0 = -1, i1 = -1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int32_t id = t[er * p + corners[fr * NC + c]];
            if (id == c0) i0 = c;
            if (id == c1) i1 = c;
        }
        int code = -1;
        if (i0 >= 0 && i1 >= 0) {
            if constexpr (NC == 2) code = (i0 != i1) ? i0 : -1;
            else code = (i0 ^ i1) == 1 ? 2 * i0 : (i0 ^ i1) == 2 ? 2 * i0 + 1 : -1;
        }
        orientation[idx] = code;
    }
}

// ---- geometry of a face point -------------------------------------------------------------------------------------

template <int D>
struct FaceGeo {
    double C[D][D];          // the cofactors of J = dx / dxi: J^-T = C / det J
    double det, rdet;        // det J and its reciprocal
    double nv[D];            // C n_ref: a positive multiple of the outward normal
    double rnn;              // 1 / |C n_ref|
    double ds;               // wf_q |J t| (2-D), wf_q |J t1 x J t2| (3-D)
};

// Point q of the local face whose tables are tabf [p][1 + D][Qf] and whose tangents and normal are fg, on the element
// with nodes xe [p][D]; with X also the point itself.
template <int D, bool X>
__device__ __forceinline__ void face_geo(const double* xe, const double* tabf, const double* __restrict__ fg, int p, int Qf,
                                         int q, double wq, FaceGeo<D>& geo, double* xq) {
    double J[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        if (X) xq[a] = 0.0;
#pragma unroll
        for (int b = 0; b < D; ++b) J[a][b] = 0.0;
    }
    for (int i = 0; i < p; ++i) {
        const double* t = tabf + (size_t)i * (1 + D) * Qf + q;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const double xa = xe[i * D + a];
            if (X) xq[a] = __builtin_fma(t[0], xa, xq[a]);
#pragma unroll
            for (int b = 0; b < D; ++b) J[a][b] = __builtin_fma(t[(size_t)(1 + b) * Qf], xa, J[a][b]);
        }
    }
    double s2;
    if constexpr (D == 2) {
        geo.C[0][0] = J[1][1];
        geo.C[0][1] = -J[1][0];
        geo.C[1][0] = -J[0][1];
        geo.C[1][1] = J[0][0];
        geo.det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        const double t0 = J[0][0] * fg[0] + J[0][1] * fg[1], t1 = J[1][0] * fg[0] + J[1][1] * fg[1];
        s2 = t0 * t0 + t1 * t1;
    } else {
        geo.C[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        geo.C[0][1] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        geo.C[0][2] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        geo.C[1][0] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
        geo.C[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
        geo.C[1][2] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
        geo.C[2][0] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
        geo.C[2][1] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
        geo.C[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        geo.det = J[0][0] * geo.C[0][0] + J[0][1] * geo.C[0][1] + J[0][2] * geo.C[0][2];
        double u[3], v[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            u[a] = J[a][0] * fg[0] + J[a][1] * fg[1] + J[a][2] * fg[2];
            v[a] = J[a][0] * fg[3] + J[a][1] * fg[4] + J[a][2] * fg[5];
        }
        const double c0 = u[1] * v[2] - u[2] * v[1], c1 = u[2] * v[0] - u[0] * v[2], c2 = u[0] * v[1] - u[1] * v[0];
        s2 = c0 * c0 + c1 * c1 + c2 * c2;
    }
    geo.ds = wq * sqrt(s2);
    geo.rdet = 1.0 / geo.det;
    const double* nr = fg + (D - 1) * D;
    double n2 = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < D; ++b) s = __builtin_fma(geo.C[a][b], nr[b], s);
        geo.nv[a] = s;
        n2 = __builtin_fma(s, s, n2);
    }
    geo.rnn = 1.0 / sqrt(n2);
}

// u (FACE_VALUE) or a(grad u) . n (FACE_FLUX) at the point, for the column whose nodal values are zc[i * QUAD_CHUNK]
template <int D, int KIND>
__device__ __forceinline__ double face_eval(const FaceGeo<D>& geo, const double* zc, const double* tabf, int p, int Qf, int q,
                                            int pmode, double pexp) {
    double u = 0.0, gx[D];
#pragma unroll
    for (int b = 0; b < D; ++b) gx[b] = 0.0;
    // The gradient is that of u - z_0 (the dphi_i sum to zero): a constant z has the gradient 0.0 exactly, whatever the
    // rounding of the tables, and the sum's rounding error is that of the differences, not of the values.
    const double z0 = zc[0];
    for (int i = 0; i < p; ++i) {
        const double* t = tabf + (size_t)i * (1 + D) * Qf + q;
        const double zi = zc[i * QUAD_CHUNK];
        if constexpr (KIND == FACE_VALUE) u = __builtin_fma(t[0], zi, u);
        else {
            const double dz = zi - z0;
#pragma unroll
            for (int b = 0; b < D; ++b) gx[b] = __builtin_fma(t[(size_t)(1 + b) * Qf], dz, gx[b]);
        }
    }
    if constexpr (KIND == FACE_VALUE) return u;
    double s2 = 0.0, gn = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < D; ++b) s = __builtin_fma(geo.C[a][b], gx[b], s);
        const double ga = s * geo.rdet;
        s2 = __builtin_fma(ga, ga, s2);
        gn = __builtin_fma(ga, geo.nv[a], gn);
    }
    gn *= geo.rnn;
    if (s2 == 0.0) return 0.0;                     // a(0) = 0 for every p >= 1
    return pmode == 2 ? gn : pmode == 1 ? gn / sqrt(s2) : pow(s2, 0.5 * (pexp - 2.0)) * gn;
}

// ---- the face kernel ------------------------------------------------------------------------------------------------

struct FaceParams {
    const double* x;           // (p N) x d
    const double* wf;          // Qf
    const double* tab;         // [F][p][1 + d][Qf]
    const double* fgeo;        // [F][(d-1) d + d]
    const int32_t* perm;       // [ncode][Qf]
    const int32_t* faces;      // nf x 2 [element, face] (boundary) or nf x 4 [eL, fL, eR, fR] (interior)
    const int32_t* orient;     // nf (interior)
    const double* z;           // (p N) x ncol
    const double* weight;      // nf x Qf or null (boundary)
    double* out;               // nf x ncol
    int64_t nf;
    int32_t p, Qf, F, ncol, G;
    int32_t pmode;             // 1: p = 1, 2: p = 2 (neither calls pow), 0: any other exponent
    double pexp;
};

template <int D, int SIDES, int KIND, bool TAB_LDS>
__global__ __launch_bounds__(QUAD_THREADS) void face_kernel(const FaceParams P) {
    extern __shared__ __attribute__((aligned(16))) double face_lds[];
    const int tid = threadIdx.x, p = P.p, Qf = P.Qf, G = P.G, ncol = P.ncol;
    constexpr int SW = 2 * SIDES, FG = (D - 1) * D + D;
    double* xs = face_lds;
    double* zs = xs + face_lds_xs(G, SIDES, p, D);
    double* red = zs + face_lds_zs(G, SIDES, p);
    const double* tab = P.tab;
    if constexpr (TAB_LDS) {
        double* tl = red + quad_lds_red();
        const int n = P.F * (1 + D) * Qf * p;
        for (int i = tid; i < n; i += QUAD_THREADS) tl[i] = P.tab[i];
        tab = tl;                                   // first read after the barrier behind the z chunk
    }
    const int g = tid / Qf, q = tid - g * Qf;
    int tree = 1;
    while (tree < Qf) tree <<= 1;
    const int per = p * D;
    const size_t tabf_len = (size_t)p * (1 + D) * Qf;
    const int64_t groups = (P.nf + G - 1) / G;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t f0 = grp * G;
        const int nfl = (int)((P.nf - f0) < (int64_t)G ? (P.nf - f0) : (int64_t)G);
        const int sides = nfl * SIDES;
        __syncthreads();
        for (int i = tid; i < sides * per; i += QUAD_THREADS) {
            const int gs = i / per, r = i - gs * per;
            const int64_t e = P.faces[(f0 + gs / SIDES) * SW + 2 * (gs % SIDES)];
            xs[i] = P.x[e * per + r];
        }
        const bool active = g < nfl;
        int fL = 0, fR = 0, qR = 0;
        if (active) {
            const int32_t* fi = P.faces + (f0 + g) * SW;
            fL = fi[1];
            if constexpr (SIDES == 2) {
                fR = fi[3];
                qR = P.perm[P.orient[f0 + g] * Qf + q];
            }
        }
        FaceGeo<D> geoL, geoR;
        for (int c0 = 0; c0 < ncol; c0 += QUAD_CHUNK) {
            const int nc = (ncol - c0) < QUAD_CHUNK ? (ncol - c0) : QUAD_CHUNK;
            for (int i = tid; i < sides * p * nc; i += QUAD_THREADS) {
                const int row = i / nc, c = i - row * nc;
                const int gs = row / p, node = row - gs * p;
                const int64_t e = P.faces[(f0 + gs / SIDES) * SW + 2 * (gs % SIDES)];
                zs[row * QUAD_CHUNK + c] = P.z[(e * p + node) * ncol + c0 + c];
            }
            __syncthreads();
            if (active) {
                const double* tabL = tab + fL * tabf_len;
                const double* tabR = tab + fR * tabf_len;
                if (c0 == 0) {
                    face_geo<D, false>(xs + (g * SIDES) * per, tabL, P.fgeo + fL * FG, p, Qf, q, P.wf[q], geoL, nullptr);
                    if constexpr (SIDES == 2)
                        face_geo<D, false>(xs + (g * SIDES + 1) * per, tabR, P.fgeo + fR * FG, p, Qf, qR, P.wf[qR], geoR, nullptr);
                }
                double w = geoL.ds;
                if constexpr (SIDES == 1)
                    if (P.weight) w *= P.weight[(f0 + g) * Qf + q];
                for (int c = 0; c < nc; ++c) {
                    const double vL = face_eval<D, KIND>(geoL, zs + (g * SIDES) * p * QUAD_CHUNK + c, tabL, p, Qf, q, P.pmode, P.pexp);
                    double term;
                    if constexpr (SIDES == 1) {
                        term = w * vL;
                    } else {
                        const double vR = face_eval<D, KIND>(geoR, zs + (g * SIDES + 1) * p * QUAD_CHUNK + c, tabR, p, Qf, qR, P.pmode, P.pexp);
                        const double j = KIND == FACE_VALUE ? vL - vR : vL + vR;
                        term = w * (j * j);
                    }
                    red[c * QUAD_THREADS + tid] = term;
                }
            }
            for (int off = tree >> 1; off > 0; off >>= 1) {         // the halving tree: quad_kernel has these lines with a max branch
                __syncthreads();
                if (active && q < off && q + off < Qf) {
                    for (int c = 0; c < nc; ++c) {
                        double* r = red + c * QUAD_THREADS + tid;
                        *r = r[0] + r[off];
                    }
                }
            }
            __syncthreads();
            quad_write_items(P.out, red, tid, f0, nfl, Qf, ncol, c0, nc);
        }
    }
}

// points (nf x Qf x d), normals (nf x Qf x d) and measures (nf x Qf) of the faces whose [element, face] pairs start every
// row of `faces` (stride sw); any may be null
template <int D>
__global__ __launch_bounds__(QUAD_THREADS) void face_geometry_kernel(const double* __restrict__ x, const double* __restrict__ wf,
                                                                     const double* __restrict__ tab, const double* __restrict__ fgeo,
                                                                     const int32_t* __restrict__ faces, int sw, int64_t nf, int p, int Qf,
                                                                     double* __restrict__ points, double* __restrict__ normals,
                                                                     double* __restrict__ measures) {
    const int64_t idx = (int64_t)blockIdx.x * QUAD_THREADS + threadIdx.x;
    if (idx >= nf * Qf) return;
    const int64_t fc = idx / Qf;
    const int q = (int)(idx - fc * Qf);
    const int64_t e = faces[fc * sw];
    const int f = faces[fc * sw + 1];
    constexpr int FG = (D - 1) * D + D;
    FaceGeo<D> geo;
    double xq[D];
    face_geo<D, true>(x + e * p * D, tab + (size_t)f * p * (1 + D) * Qf, fgeo + f * FG, p, Qf, q, wf[q], geo, xq);
#pragma unroll
    for (int a = 0; a < D; ++a) {
        if (points) points[idx * D + a] = xq[a];
        if (normals) normals[idx * D + a] = geo.nv[a] * geo.rnn;
    }
    if (measures) measures[idx] = geo.ds;
}

// bad[i] = 1 where det J is non-positive or non-finite at a point of incidence i = element * F + face
template <int D>
__global__ __launch_bounds__(BLOCK) void face_det_kernel(const double* __restrict__ x, const double* __restrict__ wf,
                                                         const double* __restrict__ tab, const double* __restrict__ fgeo, int64_t M,
                                                         int F, int p, int Qf, int32_t* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int64_t e = i / F;
    const int f = (int)(i - e * F);
    constexpr int FG = (D - 1) * D + D;
    int32_t b = 0;
    for (int q = 0; q < Qf; ++q) {
        FaceGeo<D> geo;
        face_geo<D, false>(x + e * p * D, tab + (size_t)f * p * (1 + D) * Qf, fgeo + f * FG, p, Qf, q, wf[q], geo, nullptr);
        if (!(geo.det > 0.0) || geo.det > 1.79e308) b = 1;
    }
    bad[i] = b;
}

// hF[f] = |F|^(1/(d-1)), |F| the sum of the face's Qf measures in point order
__global__ __launch_bounds__(BLOCK) void face_size_kernel(const double* __restrict__ measures, int64_t nf, int Qf, int d,
                                                          double* __restrict__ hF) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    double s = 0.0;
    for (int q = 0; q < Qf; ++q) s += measures[f * Qf + q];
    hF[f] = d == 2 ? s : sqrt(s);
}

// eta2[e][c] = sum over the interior faces of element e, in local face order, of (hF / 2) * jump[face][c]; the product is
// rounded before it is added (no contraction), so the gather can be repeated anywhere bit for bit
__global__ __launch_bounds__(BLOCK) void face_indicator_kernel(const int32_t* __restrict__ element_faces, const double* __restrict__ hF,
                                                               const double* __restrict__ jump, int64_t N, int F, int ncol,
                                                               double* __restrict__ eta2) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * ncol) return;
    const int64_t e = i / ncol;
    const int c = (int)(i - e * ncol);
    double s = 0.0;
    for (int f = 0; f < F; ++f) {
        const int32_t idx = element_faces[e * F + f];
        if (idx >= 0) {
            const double term = (0.5 * hF[idx]) * jump[(int64_t)idx * ncol + c];
            s = s + term;
        }
    }
    eta2[i] = s;
}

// ---- launchers ------------------------------------------------------------------------------------------------------

template <int D, int SIDES>
void launch_face_kind(int kind, const FaceParams& P, const QuadPlan& plan, hipStream_t st) {
    if (kind == FACE_VALUE) {
        if (plan.tables_lds) quad_launch<face_kernel<D, SIDES, FACE_VALUE, true>>("faces", P, plan, st);
        else quad_launch<face_kernel<D, SIDES, FACE_VALUE, false>>("faces", P, plan, st);
    } else {
        if (plan.tables_lds) quad_launch<face_kernel<D, SIDES, FACE_FLUX, true>>("faces", P, plan, st);
        else quad_launch<face_kernel<D, SIDES, FACE_FLUX, false>>("faces", P, plan, st);
    }
}

// the face kernel over the boundary (sides = 1) or the interior faces (sides = 2) into Fc.face (nf x ncol); z is on the device
void run_faces(Faces& Fc, int sides, int32_t kind, double pexp, int32_t ncol, const double* weight, hipStream_t st) {
    const int64_t nf = sides == 1 ? Fc.B : Fc.I;
    if (nf == 0) return;
    const QuadPlan plan = face_decide(Fc.d, Fc.p, Fc.Qf, Fc.F, sides, nf);
    Fc.face.ensure((size_t)nf * ncol);
    FaceParams P{};
    P.x = Fc.x.p; P.wf = Fc.wf.p; P.tab = Fc.tab.p; P.fgeo = Fc.fgeo.p; P.perm = Fc.perm.p;
    P.faces = sides == 1 ? Fc.boundary.p : Fc.interior.p;
    P.orient = Fc.orientation.p;
    P.z = Fc.z.p; P.weight = weight; P.out = Fc.face.p;
    P.nf = nf; P.p = Fc.p; P.Qf = Fc.Qf; P.F = Fc.F; P.ncol = ncol; P.G = plan.G;
    P.pmode = quad_pmode(pexp);
    P.pexp = pexp;
    if (Fc.d == 2) {
        if (sides == 1) launch_face_kind<2, 1>(kind, P, plan, st);
        else launch_face_kind<2, 2>(kind, P, plan, st);
    } else {
        if (sides == 1) launch_face_kind<3, 1>(kind, P, plan, st);
        else launch_face_kind<3, 2>(kind, P, plan, st);
    }
}

void launch_geometry(const Faces& Fc, const int32_t* faces, int sw, int64_t nf, double* points, double* normals, double* measures,
                     hipStream_t st) {
    if (nf == 0) return;
    const unsigned grid = (unsigned)((nf * Fc.Qf + QUAD_THREADS - 1) / QUAD_THREADS);
    if (Fc.d == 2)
        hipLaunchKernelGGL((face_geometry_kernel<2>), dim3(grid), dim3(QUAD_THREADS), 0, st, Fc.x.p, Fc.wf.p, Fc.tab.p, Fc.fgeo.p, faces, sw,
                           nf, Fc.p, Fc.Qf, points, normals, measures);
    else
        hipLaunchKernelGGL((face_geometry_kernel<3>), dim3(grid), dim3(QUAD_THREADS), 0, st, Fc.x.p, Fc.wf.p, Fc.tab.p, Fc.fgeo.p, faces, sw,
                           nf, Fc.p, Fc.Qf, points, normals, measures);
    MGB_HIP_CHECK(hipGetLastError());
}

template <int NC>
void build_topology(Faces& Fc, unsigned bits, hipStream_t st) {
    const int64_t M = Fc.N * Fc.F;
    const int F = Fc.F, p = Fc.p;
    const int ids = NC == 2 ? 2 : 3;
    const bool two = ids * bits > 64;
    DevBuf<uint64_t> khi, kg, ks;
    DevBuf<uint32_t> klo, klo_s;
    DevBuf<int32_t> val, val_t, sv, is_b, is_i, partner, over, off_b, off_i, off_o;
    DevBuf<char> tmp;
    khi.alloc((size_t)M); ks.alloc((size_t)M); val.alloc((size_t)M); sv.alloc((size_t)M);
    if (two) { klo.alloc((size_t)M); klo_s.alloc((size_t)M); kg.alloc((size_t)M); val_t.alloc((size_t)M); }
    hipLaunchKernelGGL((face_key_kernel<NC>), dim3(grid_1d(M)), dim3(BLOCK), 0, st, M, F, p, Fc.t.p, Fc.corners.p, bits, two ? 1 : 0,
                       khi.p, klo.p, val.p);
    MGB_HIP_CHECK(hipGetLastError());
    if (two) {
        sort_pairs(klo.p, klo_s.p, val.p, val_t.p, M, bits, tmp, st);
        hipLaunchKernelGGL(face_gather_kernel, dim3(grid_1d(M)), dim3(BLOCK), 0, st, M, khi.p, val_t.p, kg.p);
        MGB_HIP_CHECK(hipGetLastError());
        sort_pairs(kg.p, ks.p, val_t.p, sv.p, M, 2 * bits, tmp, st);
    } else {
        sort_pairs(khi.p, ks.p, val.p, sv.p, M, ids * bits, tmp, st);
    }
    is_b.alloc((size_t)M); is_i.alloc((size_t)M); partner.alloc((size_t)M); over.alloc((size_t)M);
    off_b.alloc((size_t)M); off_i.alloc((size_t)M); off_o.alloc((size_t)M);
    hipLaunchKernelGGL(face_run_kernel, dim3(grid_1d(M)), dim3(BLOCK), 0, st, M, sv.p, khi.p, klo.p, two ? 1 : 0, is_b.p, is_i.p,
                       partner.p, over.p);
    MGB_HIP_CHECK(hipGetLastError());
    exclusive_scan(is_b.p, off_b.p, M, tmp, st);
    exclusive_scan(is_i.p, off_i.p, M, tmp, st);
    exclusive_scan(over.p, off_o.p, M, tmp, st);
    if (scan_total(over.p, off_o.p, M, st) > 0) {
        std::vector<int32_t> h((size_t)M);
        over.download(h.data(), (size_t)M, st);
        MGB_HIP_CHECK(hipStreamSynchronize(st));
        int32_t most = 0;
        for (int32_t c : h) most = c > most ? c : most;
        throw InvalidArgument("faces: a face is shared by " + std::to_string(most) + " elements (at most 2 can share one)");
    }
    Fc.B = scan_total(is_b.p, off_b.p, M, st);
    Fc.I = scan_total(is_i.p, off_i.p, M, st);
    Fc.boundary.alloc((size_t)Fc.B * 2 + 2);
    Fc.interior.alloc((size_t)Fc.I * 4 + 4);
    Fc.orientation.alloc((size_t)Fc.I + 1);
    Fc.element_faces.alloc((size_t)M);
    hipLaunchKernelGGL((face_emit_kernel<NC>), dim3(grid_1d(M)), dim3(BLOCK), 0, st, M, F, p, Fc.t.p, Fc.corners.p, is_b.p, is_i.p,
                       partner.p, off_b.p, off_i.p, Fc.boundary.p, Fc.interior.p, Fc.orientation.p, Fc.element_faces.p);
    MGB_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> orient((size_t)Fc.I);
    Fc.orientation.download(orient.data(), (size_t)Fc.I, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));          // the temporaries above are locals
    for (int32_t c : orient)
        if (c < 0 || c >= Fc.ncode)
            throw InvalidArgument("faces: two elements share the corner ids of a face without sharing the face (the mesh is not conforming)");
}

}  // namespace

void faces_build(Faces& Fc, const FacesIn& in, hipStream_t st) {
    const int d = in.d, p = in.p, F = in.F, Qf = in.Qf;
    Fc.d = d; Fc.p = p; Fc.F = F; Fc.Qf = Qf; Fc.ncode = in.ncode; Fc.N = in.N;
    const int NC = 1 << (d - 1), FG = (d - 1) * d + d;
    std::vector<double> tab((size_t)F * p * (1 + d) * Qf), fgeo((size_t)F * FG);
    for (int f = 0; f < F; ++f) {
        const size_t at = (size_t)f * Qf * p;
        quad_repack_tables(d, p, Qf, in.phi + at, in.dphi + at * d, tab.data() + at * (1 + d));
        for (int j = 0; j < (d - 1) * d; ++j) fgeo[(size_t)f * FG + j] = in.tangents[(size_t)f * (d - 1) * d + j];
        for (int a = 0; a < d; ++a) fgeo[(size_t)f * FG + (d - 1) * d + a] = in.normals[(size_t)f * d + a];
    }
    int32_t top = 0;
    for (int64_t i = 0; i < (int64_t)p * in.N; ++i) top = in.t[i] > top ? in.t[i] : top;
    Fc.x.upload(in.x, (size_t)p * in.N * d, st);
    Fc.t.upload(in.t, (size_t)p * in.N, st);
    Fc.wf.upload(in.wf, (size_t)Qf, st);
    Fc.tab.upload(tab, st);
    Fc.fgeo.upload(fgeo, st);
    Fc.corners.upload(in.corners, (size_t)F * NC, st);
    Fc.perm.upload(in.perm, (size_t)in.ncode * Qf, st);
    Fc.ev.mark(3, st);
    if (d == 2) build_topology<2>(Fc, key_bits((uint64_t)top), st);
    else build_topology<4>(Fc, key_bits((uint64_t)top), st);
    Fc.ev.mark(4, st);
    // det J at every face point of every element
    const int64_t M = in.N * F;
    DevBuf<int32_t> bad;
    bad.alloc((size_t)M);
    if (d == 2)
        hipLaunchKernelGGL((face_det_kernel<2>), dim3(grid_1d(M)), dim3(BLOCK), 0, st, Fc.x.p, Fc.wf.p, Fc.tab.p, Fc.fgeo.p, M, F, p, Qf, bad.p);
    else
        hipLaunchKernelGGL((face_det_kernel<3>), dim3(grid_1d(M)), dim3(BLOCK), 0, st, Fc.x.p, Fc.wf.p, Fc.tab.p, Fc.fgeo.p, M, F, p, Qf, bad.p);
    MGB_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> hb((size_t)M);
    bad.download(hb.data(), (size_t)M, st);
    // the sizes of the interior faces
    Fc.hF.alloc((size_t)Fc.I + 1);
    if (Fc.I > 0) {
        Fc.geo.ensure((size_t)Fc.I * Qf);
        launch_geometry(Fc, Fc.interior.p, 4, Fc.I, nullptr, nullptr, Fc.geo.p, st);
        hipLaunchKernelGGL(face_size_kernel, dim3(grid_1d(Fc.I)), dim3(BLOCK), 0, st, Fc.geo.p, Fc.I, Qf, d, Fc.hF.p);
        MGB_HIP_CHECK(hipGetLastError());
    }
    MGB_HIP_CHECK(hipStreamSynchronize(st));       // tab, fgeo, bad are locals
    for (int64_t i = 0; i < M; ++i)
        if (hb[(size_t)i])
            throw InvalidArgument("faces: det J is not positive and finite on a face of element " + std::to_string(i / F) +
                                  " (local face " + std::to_string(i % F) + ")");
}

void faces_topology(const Faces& Fc, int32_t* boundary, int32_t* interior, int32_t* orientation, int32_t* element_faces, hipStream_t st) {
    if (boundary) Fc.boundary.download(boundary, (size_t)Fc.B * 2, st);
    if (interior) Fc.interior.download(interior, (size_t)Fc.I * 4, st);
    if (orientation) Fc.orientation.download(orientation, (size_t)Fc.I, st);
    if (element_faces) Fc.element_faces.download(element_faces, (size_t)Fc.N * Fc.F, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void faces_geometry(Faces& Fc, int32_t which, double* points, double* normals, double* measures, hipStream_t st) {
    const int64_t nf = which == 0 ? Fc.B : Fc.I;
    const int64_t n = nf * Fc.Qf;
    if (n == 0) return;
    Fc.geo.ensure((size_t)n * (2 * Fc.d + 1));
    double* dp = points ? Fc.geo.p : nullptr;
    double* dn = normals ? Fc.geo.p + n * Fc.d : nullptr;
    double* dm = measures ? Fc.geo.p + 2 * n * Fc.d : nullptr;
    launch_geometry(Fc, which == 0 ? Fc.boundary.p : Fc.interior.p, which == 0 ? 2 : 4, nf, dp, dn, dm, st);
    if (points) MGB_HIP_CHECK(hipMemcpyAsync(points, dp, (size_t)n * Fc.d * sizeof(double), hipMemcpyDeviceToHost, st));
    if (normals) MGB_HIP_CHECK(hipMemcpyAsync(normals, dn, (size_t)n * Fc.d * sizeof(double), hipMemcpyDeviceToHost, st));
    if (measures) MGB_HIP_CHECK(hipMemcpyAsync(measures, dm, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void faces_sizes(const Faces& Fc, double* hF, hipStream_t st) {
    Fc.hF.download(hF, (size_t)Fc.I, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
}

void faces_integrate(Faces& Fc, int32_t kind, double pexp, int32_t ncol, const double* z, const double* weight,
                     double* per_face, double* totals, hipStream_t st) {
    Fc.z.upload(z, (size_t)Fc.p * Fc.N * ncol, st);
    if (weight) Fc.weight.upload(weight, (size_t)Fc.B * Fc.Qf, st);
    Fc.totals.ensure((size_t)ncol);
    Fc.ev.begin(st);
    run_faces(Fc, 1, kind, pexp, ncol, weight ? Fc.weight.p : nullptr, st);
    Fc.ev.mark(1, st);
    quad_reduce_columns(Fc.face.p, Fc.B, ncol, false, Fc.totals.p, st);
    Fc.ev.mark(2, st);
    Fc.totals.download(totals, (size_t)ncol, st);
    if (per_face) Fc.face.download(per_face, (size_t)Fc.B * ncol, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    Fc.ev.timed = true;
}

void faces_jumps(Faces& Fc, int32_t kind, double pexp, int32_t ncol, const double* z, double* out, hipStream_t st) {
    Fc.z.upload(z, (size_t)Fc.p * Fc.N * ncol, st);
    Fc.ev.begin(st);
    run_faces(Fc, 2, kind, pexp, ncol, nullptr, st);
    Fc.ev.mark(1, st);
    Fc.ev.mark(2, st);
    Fc.face.download(out, (size_t)Fc.I * ncol, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    Fc.ev.timed = true;
}

void faces_indicator(Faces& Fc, double pexp, int32_t ncol, const double* z, double* eta2, double* totals, hipStream_t st) {
    Fc.z.upload(z, (size_t)Fc.p * Fc.N * ncol, st);
    Fc.elem.ensure((size_t)Fc.N * ncol);
    Fc.totals.ensure((size_t)ncol);
    Fc.face.ensure(1);
    Fc.ev.begin(st);
    run_faces(Fc, 2, FACE_FLUX, pexp, ncol, nullptr, st);
    Fc.ev.mark(1, st);
    hipLaunchKernelGGL(face_indicator_kernel, dim3(grid_1d(Fc.N * ncol)), dim3(BLOCK), 0, st, Fc.element_faces.p, Fc.hF.p, Fc.face.p,
                       Fc.N, Fc.F, (int)ncol, Fc.elem.p);
    MGB_HIP_CHECK(hipGetLastError());
    quad_reduce_columns(Fc.elem.p, Fc.N, ncol, false, Fc.totals.p, st);
    Fc.ev.mark(2, st);
    Fc.elem.download(eta2, (size_t)Fc.N * ncol, st);
    Fc.totals.download(totals, (size_t)ncol, st);
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    Fc.ev.timed = true;
}

void faces_times(const Faces& Fc, double* ms) {
    for (int i = 0; i < 2; ++i) ms[i] = Fc.ev.timed ? Fc.ev.ms(i) : 0.0;
    ms[2] = Fc.ev.ms(3);
}

}  // namespace mgbhip
