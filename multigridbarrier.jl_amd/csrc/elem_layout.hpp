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

}  // namespace mgbhip
