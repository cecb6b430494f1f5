// elem_layout.hpp -- evaluation modes, lane grouping and LDS layout of the element kernels.  Plain C++ (no HIP): the
// kernels, their launchers, the staging decision of problem.cpp and the host test all read the layout from here.
#pragma once
#include <cstddef>
#include <type_traits>

namespace mgbhip {

enum ElemMode { MODE_F0 = 0, MODE_F1 = 1, MODE_F2 = 2, MODE_NODE_F = 3, MODE_NODE_SLACK = 4,
                MODE_F01 = 5 };   // MODE_F01: value and gradient of one line-search trial in ONE pass over the operators

// Runtime mode -> f(std::integral_constant<int, MODE_*>): the one place a kernel template's MODE instantiations are
// listed, for launching and for attribute calls alike.  F01 = false leaves MODE_F01 out (the dense node kernels have
// none).  Returns false on a mode outside the list.
template <bool F01 = true, class F>
bool dispatch_mode(int mode, F&& f) {
    switch (mode) {
        case MODE_F0: f(std::integral_constant<int, MODE_F0>{}); return true;
        case MODE_F1: f(std::integral_constant<int, MODE_F1>{}); return true;
        case MODE_F2: f(std::integral_constant<int, MODE_F2>{}); return true;
        case MODE_NODE_F: f(std::integral_constant<int, MODE_NODE_F>{}); return true;
        case MODE_NODE_SLACK: f(std::integral_constant<int, MODE_NODE_SLACK>{}); return true;
        case MODE_F01:
            if constexpr (F01) { f(std::integral_constant<int, MODE_F01>{}); return true; }
            return false;
        default: return false;
    }
}

constexpr int elem_group(int p) {                        // lanes per element (power of two >= p, at least 2)
    int g = 1;
    while (g < p) g <<= 1;
    return g < 2 ? 2 : g;
}

// wide path: threads per workgroup of the element Hessian kernel (the other modes run 256, like the narrow kernels, so
// that f0's workgroup partials keep their count elem_grid(p, N))
constexpr int WIDE_F2_THREADS = 128;
constexpr int elem_threads(bool wide, int mode) { return (wide && mode == MODE_F2) ? WIDE_F2_THREADS : 256; }

// Dynamic LDS of an element workgroup, three regions of doubles in this order (EPB * G = threads):
//   zl  [EPB][nu][G]        broken-basis values of the workgroup's elements        elem_lds_z
//   opL [nstage][EPB][pp]   staged operator blocks                                 elem_lds_ops
//   YL  [EPB][rows][G]      node weights: nD rows (MODE_F1 / MODE_F01), nD(nD+1)/2 (MODE_F2), none otherwise
// The kernels place opL and YL with the first two (threads * nu is formed in the caller's integer type: int 256 in the
// narrow kernels, size_t blockDim.x in the wide one); the launchers size the allocation with elem_lds_bytes.
template <class T>
__attribute__((always_inline)) constexpr size_t elem_lds_z(T threads, int nu) { return threads * nu; }
__attribute__((always_inline)) constexpr size_t elem_lds_ops(int nstage, int epb, int pp) { return (size_t)nstage * epb * pp; }
constexpr size_t elem_lds_y(int threads, int nD, int mode) {
    return (mode == MODE_F1 || mode == MODE_F01) ? (size_t)threads * nD : (mode == MODE_F2) ? (size_t)threads * (nD * (nD + 1) / 2) : 0;
}
constexpr size_t elem_lds_bytes(int threads, int p, int nu, int nD, int nstage, int mode) {
    const size_t d = elem_lds_z(threads, nu) + elem_lds_ops(nstage, threads / elem_group(p), p * p) + elem_lds_y(threads, nD, mode);
    return (d < 256 ? 256 : d) * sizeof(double);      // floor: the workgroup reduction reuses the front of the allocation
}

// Launch cap of the element kernels, and the staging rule of a problem's operators: nstage operators are staged through
// LDS while the operator tiles of a workgroup stay under 64 KB and the whole f2 working set under 150 KB.
constexpr size_t ELEM_LDS_MAX = 160 * 1024;
constexpr bool elem_stage_fits(int p, int nu, int nD, int nstage, bool wide) {
    const size_t tiles = elem_lds_ops(nstage, 256 / elem_group(p), p * p) * sizeof(double);     // at 256 threads on both paths
    return tiles <= 64 * 1024 && elem_lds_bytes(elem_threads(wide, MODE_F2), p, nu, nD, nstage, MODE_F2) <= 150 * 1024;
}

// ---- which kernel a launch runs ----------------------------------------------------------------------------------------
// The one dispatch decision of the element family: launch_elem, launch_elem_f2_condense and the generic launchers run what
// elem_decide returns, and mgbhip_elem_plan reports it read-only.
enum ElemKind { ELEM_DENSE = 0, ELEM_WIDE = 1, ELEM_FAST_DEFAULT = 2, ELEM_FAST_RUNTIME = 3, ELEM_CONDENSE = 4, ELEM_GENERIC = 5 };

// (NY, P) of the compile-time specialisations elem_f2_fast / elem_f01_fast, in the order they are tried: the
// discretisations of the BASELINE configs (fem2d_P2 with bubble, fem1d, fem3d Q1, fem2d_P2 without bubble) and their
// phase-I images.  Each exists for the default D-table signature (SigDefault<NY>) and for a runtime one.
constexpr int ELEM_FAST_COUNT = 8;
constexpr int ELEM_FAST_TABLE[ELEM_FAST_COUNT][2] = {{4, 7}, {3, 2}, {5, 8}, {4, 6}, {7, 7}, {6, 2}, {8, 8}, {7, 6}};
constexpr int elem_fast_index(int NY, int P) {
    for (int i = 0; i < ELEM_FAST_COUNT; ++i)
        if (ELEM_FAST_TABLE[i][0] == NY && ELEM_FAST_TABLE[i][1] == P) return i;
    return -1;
}
// the condensing f2 (elem_f2_fast<4, 7, SigDefault<4>, true>): fem2d_P2 with bubble, both operators staged
constexpr int ELEM_CONDENSE_NY = 4, ELEM_CONDENSE_P = 7, ELEM_CONDENSE_NU = 2, ELEM_CONDENSE_NSTAGE = 2;

struct ElemPlan {
    int kind;            // ElemKind
    int NY, P;           // the instantiation: (NY, P) of a fast kernel, (nD, 0) of elem_kernel<NY>, (0, 0) wide and dense
    int threads, G, EPB; // workgroup size, lanes per element, elements per workgroup (0 on the dense path)
    long long grid;      // workgroups (0 on the dense path: dense.hip sizes its own launches)
    size_t lds;          // dynamic LDS bytes
};

// all_staged: no D row reads its operator from HBM (D_stage == -2).  default_sig: the D table and ymask are SigDefault<nD>'s.
// condensing: the caller asks for the leaf-condensing f2; where it does not apply the plain decision for `mode` is returned.
constexpr ElemPlan elem_decide(int p, int nu, int nD, int nstage, bool wide, bool dense, bool all_staged, bool default_sig,
                               int mode, bool condensing, long long N) {
    if (dense) return ElemPlan{ELEM_DENSE, 0, 0, 0, 0, 0, 0, 0};
    const int threads = elem_threads(wide, mode);
    const int G = elem_group(p);
    const int EPB = threads / G;
    const long long grid = (N + EPB - 1) / EPB;
    const size_t lds = elem_lds_bytes(threads, p, nu, nD, nstage, mode);
    if (wide) return ElemPlan{ELEM_WIDE, 0, 0, threads, G, EPB, grid, lds};
    if (condensing && mode == MODE_F2 && nD == ELEM_CONDENSE_NY && p == ELEM_CONDENSE_P && nu == ELEM_CONDENSE_NU &&
        nstage == ELEM_CONDENSE_NSTAGE && default_sig && all_staged)
        return ElemPlan{ELEM_CONDENSE, nD, p, threads, G, EPB, grid, lds};
    if ((mode == MODE_F2 || mode == MODE_F01) && elem_fast_index(nD, p) >= 0 && all_staged && lds <= ELEM_LDS_MAX)
        return ElemPlan{default_sig ? ELEM_FAST_DEFAULT : ELEM_FAST_RUNTIME, nD, p, threads, G, EPB, grid, lds};
    return ElemPlan{ELEM_GENERIC, nD, 0, threads, G, EPB, grid, lds};
}

}  // namespace mgbhip
