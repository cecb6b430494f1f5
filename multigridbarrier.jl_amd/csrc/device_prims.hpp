// device_prims.hpp -- what the post-processing translation units share below their own kernels, one definition each: the
// launch shape, the two rocPRIM calls they are all built from (an exclusive scan and a stable radix sort of pairs) with
// the temporary-storage handshake around them, the read-back of a scan's total and the kernel that turns sorted keys into
// segment starts.  No other file names rocPRIM.
//
// Only integers go through these scans: a scan adds in an order that depends on its launch shape, which is exact for
// integers and is not for floating-point values (see polyline.hip).
//
// Everything here has internal linkage (the library is built without relocatable device code, so every translation unit
// carries its own copy of the kernels it launches).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"

namespace mgbhip {

namespace {

constexpr int BLOCK = 256;

inline unsigned grid_1d(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// the end bit of a radix sort whose keys are all below n (at least 1)
inline unsigned key_bits(uint64_t n) {
    unsigned bits = 1;
    while (bits < 64 && (n >> bits) != 0) ++bits;
    return bits;
}

// out[i] = in[0] + .. + in[i-1], out[0] = 0; tmp grows to what the scan asks for and is kept.  Queued on st.
template <class T>
void exclusive_scan(const T* in, T* out, int64_t n, DevBuf<char>& tmp, hipStream_t st) {
    size_t bytes = 0;
    MGB_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, (T)0, (size_t)n, rocprim::plus<T>(), st));
    tmp.ensure(bytes + 16);
    MGB_HIP_CHECK(rocprim::exclusive_scan((void*)tmp.p, bytes, in, out, (T)0, (size_t)n, rocprim::plus<T>(), st));
}

// (k_out, v_out) = (k_in, v_in) sorted stably by bits [0, end_bit) of the key; tmp as above.  Queued on st.
template <class Key, class Value>
void sort_pairs(const Key* k_in, Key* k_out, const Value* v_in, Value* v_out, int64_t n, unsigned end_bit,
                DevBuf<char>& tmp, hipStream_t st) {
    size_t bytes = 0;
    MGB_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0u, end_bit, st));
    tmp.ensure(bytes + 16);
    MGB_HIP_CHECK(rocprim::radix_sort_pairs((void*)tmp.p, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0u, end_bit, st));
}

// the sum of count[0 .. n), n > 0, from its exclusive scan off: off[n-1] + count[n-1].  Waits for st.
template <class T>
T scan_total(const T* count, const T* off, int64_t n, hipStream_t st) {
    T last_off = 0, last_count = 0;
    MGB_HIP_CHECK(hipMemcpyAsync(&last_off, off + (n - 1), sizeof(T), hipMemcpyDeviceToHost, st));
    MGB_HIP_CHECK(hipMemcpyAsync(&last_count, count + (n - 1), sizeof(T), hipMemcpyDeviceToHost, st));
    MGB_HIP_CHECK(hipStreamSynchronize(st));
    return last_off + last_count;
}

// start[c] = first position of the M sorted keys that holds a key >= c, for c in [0, K] (start[K] = M); the keys lie in
// [0, K).  One lane per position and one past the end; every entry of start is written exactly once.
template <class Key>
__global__ void __launch_bounds__(BLOCK) segment_starts(int64_t M, int64_t K, const Key* __restrict__ keys,
                                                        int32_t* __restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > M) return;
    const int64_t a = i == 0 ? -1 : (int64_t)keys[i - 1];
    const int64_t b = i == M ? K : (int64_t)keys[i];
    for (int64_t c = a + 1; c <= b; ++c) start[c] = (int32_t)i;
}

}  // namespace

}  // namespace mgbhip
