// vector_kernels.hpp -- CSR matvecs and vector kernels (included by kernels.hip, after reduce_kernels.hpp).
#pragma once
#include "reduce_kernels.hpp"

namespace mgbhip {

namespace {

// ---- sparse matvecs ------------------------------------------------------------------------------

template <bool ADD>
__global__ __launch_bounds__(256) void csr_matvec_row_kernel(int64_t rows, const int32_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ col,
                                                             const double* __restrict__ val,
                                                             const double* __restrict__ x, double* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    double s = 0.0;
    for (int32_t q = ptr[i]; q < ptr[i + 1]; ++q) s += val[q] * x[col[q]];
    y[i] = ADD ? y[i] + s : s;
}

template <bool ADD>
__global__ __launch_bounds__(256) void csr_matvec_wave_kernel(int64_t rows, const int32_t* __restrict__ ptr,
                                                              const int32_t* __restrict__ col,
                                                              const double* __restrict__ val,
                                                              const double* __restrict__ x, double* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    DSum a;
    for (int32_t q = ptr[i] + lane; q < ptr[i + 1]; q += 64) a.add(val[q] * x[col[q]]);
    dsum_wave_reduce(a);
    if (lane == 0) y[i] = ADD ? y[i] + a.value() : a.value();
}

// Very long rows (restriction onto a handful of coarse unknowns: every row of R' spans a large
// part of the mesh): a workgroup per (row, 4096-entry chunk), partial sums to scratch, then a
// fixed-order sum over the chunks -- deterministic, and the whole GPU works on a 3-row matvec.
constexpr int CHUNK = 4096;
__global__ __launch_bounds__(256) void csr_matvec_chunk_kernel(const int32_t* __restrict__ ptr,
                                                               const int32_t* __restrict__ col,
                                                               const double* __restrict__ val,
                                                               const double* __restrict__ x,
                                                               double* __restrict__ partial, int nchunk) {
    __shared__ double red[256];
    const int row = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
    const int32_t q0 = ptr[row] + ch * CHUNK;
    const int32_t q1 = min(ptr[row + 1], q0 + CHUNK);
    __shared__ double redc[256];
    DSum a;
    for (int32_t q = q0 + tid; q < q1; q += 256) a.add(val[q] * x[col[q]]);
    red[tid] = a.s;
    redc[tid] = a.c;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            DSum b;
            b.s = red[tid]; b.c = redc[tid];
            b.merge(red[tid + off], redc[tid + off]);
            red[tid] = b.s; redc[tid] = b.c;
        }
        __syncthreads();
    }
    if (tid == 0) {            // (sum, carried error) of the chunk
        partial[2 * ((int64_t)row * nchunk + ch)] = red[0];
        partial[2 * ((int64_t)row * nchunk + ch) + 1] = redc[0];
    }
}

// one wave per row: the lanes stride over the chunk sums (a row of the coarsest level has 224 of them at L = 9; one thread
// walking them serially took 19 us for a 2-row matvec), fixed shuffle tree
__global__ __launch_bounds__(256) void csr_matvec_chunk_sum_kernel(int64_t rows, const double* __restrict__ partial,
                                                                   int nchunk, double* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    DSum a;
    for (int c = lane; c < nchunk; c += 64) a.merge(partial[2 * (i * nchunk + c)], partial[2 * (i * nchunk + c) + 1]);
    dsum_wave_reduce(a);
    if (lane == 0) y[i] = a.value();
}

// zfull = z0 + R*s  (src/convex.jl:156): one thread per broken row, so the element kernels
// read their local values with independent coalesced loads instead of a dependent
// rowptr -> col/val -> s chain per tile.
__global__ __launch_bounds__(256) void prolong_kernel(int64_t rows, const int32_t* __restrict__ ptr,
                                                      const int32_t* __restrict__ col,
                                                      const double* __restrict__ val,
                                                      const double* __restrict__ s, const double* __restrict__ z0,
                                                      double* __restrict__ zfull) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    double v = z0[i];
    for (int32_t q = ptr[i]; q < ptr[i + 1]; ++q) v += val[q] * s[col[q]];
    zfull[i] = v;
}

__global__ __launch_bounds__(256) void step_kernel(const double* __restrict__ x, const double* __restrict__ nn,
                                                   double s, double* __restrict__ xn, int64_t len,
                                                   int32_t* __restrict__ moved, int32_t stamp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool m = false;
    if (i < len) {
        const double xi = x[i];
        const double v = __builtin_fma(-s, nn[i], xi);       // one rounding (what the contraction of xi - s * nn[i] gave): z_at forms the same value on the fly
        xn[i] = v;
        m = (v != xi);
    }
    // one store per workgroup at most, and only when something moved (atomics on one word
    // from every wave serialise at the memory side)
    __shared__ int any_moved;
    if (threadIdx.x == 0) any_moved = 0;
    __syncthreads();
    if (m) any_moved = 1;
    __syncthreads();
    // the flag carries the caller's stamp of THIS step (a fresh value per launch): nobody has to clear it beforehand
    if (threadIdx.x == 0 && any_moved) *moved = stamp;
}

__global__ __launch_bounds__(256) void scale_copy_kernel(const double* __restrict__ src, double alpha,
                                                         double* __restrict__ dst, int64_t len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < len) dst[i] = alpha * src[i];
}

// border column of the bordered Newton system: tail[0 .. m) = -g, tail[m] = -1 (one launch).  x_one (optional): the entry
// x[m] = 1 the backward sweep of this system starts from, when the border front has no launch of its own
__global__ __launch_bounds__(256) void border_tail_kernel(const double* __restrict__ g, double* __restrict__ tail, int64_t m,
                                                          double* __restrict__ x_one) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) tail[i] = -1.0 * g[i];
    else if (i == m) {
        tail[i] = -1.0;
        if (x_one) *x_one = 1.0;
    }
}

__global__ __launch_bounds__(256) void axpy_kernel(double alpha, const double* __restrict__ x,
                                                   double* __restrict__ y, int64_t len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < len) y[i] += alpha * x[i];
}

__global__ __launch_bounds__(256) void fill_kernel(double value, double* __restrict__ y, int64_t len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < len) y[i] = value;
}

}  // namespace

__global__ __launch_bounds__(256) void index_gather_kernel(const double* __restrict__ v, const int32_t* __restrict__ idx,
                                                           int64_t cnt, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cnt) out[i] = v[idx[i]];
}
__global__ __launch_bounds__(256) void index_scatter_kernel(const double* __restrict__ in, const int32_t* __restrict__ idx,
                                                            int64_t cnt, double* __restrict__ v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cnt) v[idx[i]] = in[i];
}
void launch_index_gather(const double* v, const int32_t* idx, int64_t cnt, double* out, hipStream_t st) {
    if (cnt == 0) return;
    hipLaunchKernelGGL(index_gather_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, v, idx, cnt, out);
    MGB_HIP_CHECK(hipGetLastError());
}
void launch_index_scatter(const double* in, const int32_t* idx, int64_t cnt, double* v, hipStream_t st) {
    if (cnt == 0) return;
    hipLaunchKernelGGL(index_scatter_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, in, idx, cnt, v);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_csr_matvec(int64_t rows, const int32_t* ptr, const int32_t* col, const double* val,
                       const double* x, double* y, bool add, bool long_rows, hipStream_t st) {
    if (rows == 0) return;
    if (long_rows) {
        const dim3 grid((unsigned)((rows + 3) / 4));
        if (add) hipLaunchKernelGGL(csr_matvec_wave_kernel<true>, grid, dim3(256), 0, st, rows, ptr, col, val, x, y);
        else hipLaunchKernelGGL(csr_matvec_wave_kernel<false>, grid, dim3(256), 0, st, rows, ptr, col, val, x, y);
    } else {
        const dim3 grid((unsigned)((rows + 255) / 256));
        if (add) hipLaunchKernelGGL(csr_matvec_row_kernel<true>, grid, dim3(256), 0, st, rows, ptr, col, val, x, y);
        else hipLaunchKernelGGL(csr_matvec_row_kernel<false>, grid, dim3(256), 0, st, rows, ptr, col, val, x, y);
    }
    MGB_HIP_CHECK(hipGetLastError());
}

int csr_chunks(int64_t max_row_len) { return (int)((max_row_len + CHUNK - 1) / CHUNK); }

void launch_csr_matvec_chunked(int64_t rows, const int32_t* ptr, const int32_t* col, const double* val,
                               const double* x, double* y, double* scratch, int nchunk, hipStream_t st) {
    if (rows == 0) return;
    hipLaunchKernelGGL(csr_matvec_chunk_kernel, dim3((unsigned)nchunk, (unsigned)rows), dim3(256), 0, st, ptr, col, val, x,
                       scratch, nchunk);
    hipLaunchKernelGGL(csr_matvec_chunk_sum_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rows, scratch,
                       nchunk, y);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_prolong(int64_t rows, const int32_t* ptr, const int32_t* col, const double* val, const double* s,
                    const double* z0, double* zfull, hipStream_t st) {
    if (rows == 0) return;
    hipLaunchKernelGGL(prolong_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, rows, ptr, col, val, s,
                       z0, zfull);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_step(const double* x, const double* n, double s, double* xn, int64_t len, int32_t* moved, int32_t stamp,
                 hipStream_t st) {
    if (len == 0) return;
    hipLaunchKernelGGL(step_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, x, n, s, xn, len, moved, stamp);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_scale_copy(const double* src, double alpha, double* dst, int64_t len, hipStream_t st) {
    if (len == 0) return;
    hipLaunchKernelGGL(scale_copy_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, src, alpha, dst, len);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_border_tail(const double* g, double* tail, int64_t m, hipStream_t st, double* x_one) {
    hipLaunchKernelGGL(border_tail_kernel, dim3((unsigned)((m + 1 + 255) / 256)), dim3(256), 0, st, g, tail, m, x_one);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_axpy(double alpha, const double* x, double* y, int64_t len, hipStream_t st) {
    if (len == 0) return;
    hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, alpha, x, y, len);
    MGB_HIP_CHECK(hipGetLastError());
}

void launch_fill(double value, double* y, int64_t len, hipStream_t st) {
    if (len == 0) return;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, value, y, len);
    MGB_HIP_CHECK(hipGetLastError());
}

}  // namespace mgbhip
