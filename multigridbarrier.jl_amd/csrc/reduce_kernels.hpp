// reduce_kernels.hpp -- compensated sums, reductions and the finishing launches (included by kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "dsum.hpp"        // DSum, dsum_wave_reduce
#include "kernels.hpp"

namespace mgbhip {

namespace {

// ---- reductions ------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void reduce_partials_kernel(const double* __restrict__ partials, int64_t count,
                                                              double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < count; i += 256) s += partials[i];
    red[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) out[0] = red[0];
}

// MODE 0: sum a*b ; MODE 1: sum a*a and count of non-finite a
template <int MODE>
__global__ __launch_bounds__(256) void block_reduce_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                           int64_t n, double* __restrict__ partials,
                                                           const double* __restrict__ mask) {
    __shared__ double red[256];
    __shared__ double red2[256];
    const int tid = threadIdx.x;
    double s = 0.0, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = a[i];
        const double w = mask ? mask[i] : 1.0;       // domain decomposition: 1 on the entries this rank owns, else 0
        if (MODE == 0) s += mask ? w * (v * b[i]) : v * b[i];
        else {
            s += mask ? w * (v * v) : v * v;
            bad += isfinite(v) ? 0.0 : 1.0;
        }
    }
    red[tid] = s;
    red2[tid] = bad;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) { red[tid] += red[tid + off]; red2[tid] += red2[tid + off]; }
        __syncthreads();
    }
    if (tid == 0) {
        partials[blockIdx.x] = red[0];
        if (MODE == 1) partials[gridDim.x + blockIdx.x] = red2[0];
    }
}

// Line-search trial, everything behind the element kernel in ONE launch: the restriction g = R' ret (row gather, as
// csr_matvec_row_kernel), the partial sums of |g|^2 and its non-finite count (the same grid-stride order and LDS tree as
// block_reduce_kernel<1>: identical partials), and the step kernel's work -- xn = x - s n with its own fused multiply-add and
// the "moved" stamp.  Three launches fewer per trial than restrict + block_reduce + step.
__global__ __launch_bounds__(256) void restrict_trial_kernel(int64_t rows, const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                             const double* __restrict__ val, const double* __restrict__ ret,
                                                             double* __restrict__ g, double* __restrict__ partials,
                                                             const double* __restrict__ x, const double* __restrict__ nn, double s,
                                                             double* __restrict__ xn, int32_t* __restrict__ moved, int32_t stamp) {
    __shared__ double red[256];
    __shared__ double red2[256];
    __shared__ int any_moved;
    const int tid = threadIdx.x;
    if (tid == 0) any_moved = 0;
    __syncthreads();
    double ss = 0.0, bad = 0.0;
    bool m = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < rows; i += (int64_t)gridDim.x * 256) {
        double acc = 0.0;
        for (int32_t q = ptr[i]; q < ptr[i + 1]; ++q) acc += val[q] * ret[col[q]];
        g[i] = acc;
        ss += acc * acc;
        bad += isfinite(acc) ? 0.0 : 1.0;
        if (xn) {
            const double xi = x[i];
            const double v = __builtin_fma(-s, nn[i], xi);
            xn[i] = v;
            m = m || (v != xi);
        }
    }
    red[tid] = ss;
    red2[tid] = bad;
    if (m) any_moved = 1;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) { red[tid] += red[tid + off]; red2[tid] += red2[tid + off]; }
        __syncthreads();
    }
    if (tid == 0) {
        partials[blockIdx.x] = red[0];
        partials[gridDim.x + blockIdx.x] = red2[0];
        if (any_moved) *moved = stamp;
    }
}

// Newton direction statistics in one pass: sum v*v, count of non-finite v, and g.v (the same per-block partial sums
// and trees as block_reduce_kernel<1> and <0>: identical values, two launches fewer per Newton iteration)
__global__ __launch_bounds__(256) void dir_stats_kernel(const double* __restrict__ v, const double* __restrict__ g, int64_t n,
                                                        double* __restrict__ partials, const double* __restrict__ mask) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    double s = 0.0, bad = 0.0, d = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = v[i];
        const double w = mask ? mask[i] : 1.0;
        s += mask ? w * (x * x) : x * x;
        bad += isfinite(x) ? 0.0 : 1.0;
        d += mask ? w * (g[i] * x) : g[i] * x;
    }
    red[0][tid] = s; red[1][tid] = bad; red[2][tid] = d;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] += red[0][tid + off];
            red[1][tid] += red[1][tid + off];
            red[2][tid] += red[2][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        partials[blockIdx.x] = red[0][0];
        partials[gridDim.x + blockIdx.x] = red[1][0];
        partials[2 * gridDim.x + blockIdx.x] = red[2][0];
    }
}

// The finishing launch (FinishParams: readback.hpp).  Its jobs do not depend on each other, and almost none of the kernel's time is bandwidth: it is one
// dependent memory latency per rolled `s += src[i]` and ten barriers per job.  So: the partials of ALL jobs are requested
// before the first addition (U loads per job in flight, larger counts in chunks of 256 U), and the jobs' LDS trees run side
// by side, one barrier per level.  Per job every thread still forms s = 0.0; s += src[tid]; s += src[tid + 256]; ... in
// ascending order and the tree pairs as before (off = 128 .. 1, red[tid] += red[tid + off]): the sums are bit for bit
// those of finish_serial_kernel (MGBHIP_FINISH_SERIAL=1 launches that one).
constexpr int FINISH_LOADS_IN_FLIGHT = 8;       // 8 and 16 measure the same at L = 9 (6.8 / 6.9 us per launch): the smaller kernel
template <int U>
__global__ __launch_bounds__(256) void finish_kernel(const FinishParams P) {
    __shared__ double red[4][256];
    __shared__ double res[RB_SLOTS];
    const int tid = threadIdx.x;
    if (tid < P.nints) {
        res[P.ints_out + tid] = (double)P.ints[tid];
        if (P.reset) P.ints[tid] = 0;
    }
    int64_t cnt[4], cmax = 0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        cnt[o] = o < P.njobs ? P.job[o].count : 0;      // a job that is not there loads nothing and sums to 0.0
        cmax = cnt[o] > cmax ? cnt[o] : cmax;
    }
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t base = 0; base < cmax; base += 256 * U) {
        double v[4][U];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const double* __restrict__ src = P.job[o].src;
            // (one uniform test per job and chunk.  Past the end a lane re-reads the job's last partial and drops it below:
            // no load sits behind a branch of its own -- a uniform test per row of 256 measured 1.1 us slower per launch)
            if (base < cnt[o]) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t i = base + u * 256 + tid;
                    v[o][u] = src[i < cnt[o] ? i : cnt[o] - 1];
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) v[o][u] = 0.0;
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + u * 256 + tid;
                if (i < cnt[o]) s[o] += v[o][u];
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) red[o][tid] = s[o];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int o = 0; o < 4; ++o) red[o][tid] += red[o][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (o < P.njobs) res[P.job[o].out] = red[o][0];
    }
    __syncthreads();
    // results -> device scalar block (every slot this launch produced) and -> host
    if (tid < RB_SLOTS) {
        bool mine = false;
        for (int o = 0; o < P.njobs; ++o) mine = mine || (P.job[o].out == tid);
        if (tid >= P.ints_out && tid < P.ints_out + P.nints) mine = true;
        if (mine) P.out[tid] = res[tid];
        if (P.host && tid >= P.host_lo && tid < P.host_lo + P.host_n) P.host[tid] = mine ? res[tid] : P.out[tid];
    }
    if (P.host && P.seq != 0.0) {
        __threadfence_system();                      // this thread's result stores are visible to the host ...
        __syncthreads();                             // ... for every writing thread, before the stamp
        if (tid == 0) {
            __hip_atomic_store(P.host + RB_STAMP, P.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// The jobs one after another (MGBHIP_FINISH_SERIAL=1): the kernel finish_kernel<U> is held to, bit for bit.
__global__ __launch_bounds__(256) void finish_serial_kernel(const FinishParams P) {
    __shared__ double red[256];
    __shared__ double res[RB_SLOTS];
    const int tid = threadIdx.x;
    if (tid < P.nints) {
        res[P.ints_out + tid] = (double)P.ints[tid];
        if (P.reset) P.ints[tid] = 0;
    }
    for (int o = 0; o < P.njobs; ++o) {
        const double* __restrict__ src = P.job[o].src;
        const int64_t cnt = P.job[o].count;
        double s = 0.0;
        for (int64_t i = tid; i < cnt; i += 256) s += src[i];
        red[tid] = s;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) red[tid] += red[tid + off];
            __syncthreads();
        }
        if (tid == 0) res[P.job[o].out] = red[0];
        __syncthreads();
    }
    __syncthreads();
    // results -> device scalar block (every slot this launch produced) and -> host
    if (tid < RB_SLOTS) {
        bool mine = false;
        for (int o = 0; o < P.njobs; ++o) mine = mine || (P.job[o].out == tid);
        if (tid >= P.ints_out && tid < P.ints_out + P.nints) mine = true;
        if (mine) P.out[tid] = res[tid];
        if (P.host && tid >= P.host_lo && tid < P.host_lo + P.host_n) P.host[tid] = mine ? res[tid] : P.out[tid];
    }
    if (P.host && P.seq != 0.0) {
        __threadfence_system();                      // this thread's result stores are visible to the host ...
        __syncthreads();                             // ... for every writing thread, before the stamp
        if (tid == 0) {
            __hip_atomic_store(P.host + RB_STAMP, P.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace

void launch_reduce_partials(const double* partials, int64_t count, double* out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, st, partials, count, out);
    MGB_HIP_CHECK(hipGetLastError());
}

static int reduce_blocks(int64_t n);      // workgroups of a vector reduction: kernels.hip (the gate tests read its cap from there)

int64_t reduce_scratch_doubles(int64_t n) { return 3 * (int64_t)reduce_blocks(n); }

static void launch_finish(const FinishParams& F, hipStream_t st) {
    static const bool serial = env_on("MGBHIP_FINISH_SERIAL");
    if (serial) hipLaunchKernelGGL(finish_serial_kernel, dim3(1), dim3(256), 0, st, F);
    else hipLaunchKernelGGL(finish_kernel<FINISH_LOADS_IN_FLIGHT>, dim3(1), dim3(256), 0, st, F);
    MGB_HIP_CHECK(hipGetLastError());
}

// stats: block[slot] = sum v^2, block[slot + 1] = count of non-finite v
void launch_vec_stats(const double* v, int64_t n, double* scratch, double* block, int32_t slot, hipStream_t st, const double* mask) {
    const int nb = reduce_blocks(n);
    hipLaunchKernelGGL(block_reduce_kernel<1>, dim3(nb), dim3(256), 0, st, v, (const double*)nullptr, n, scratch, mask);
    launch_finish(finish_plain(scratch, nb, 2, block, slot), st);
}

void launch_dot(const double* a, const double* b, int64_t n, double* scratch, double* block, int32_t slot, hipStream_t st,
                const double* mask) {
    const int nb = reduce_blocks(n);
    hipLaunchKernelGGL(block_reduce_kernel<0>, dim3(nb), dim3(256), 0, st, a, b, n, scratch, mask);
    launch_finish(finish_plain(scratch, nb, 1, block, slot), st);
}

// n <= RB_SLOTS scalars of the device block to the pinned host block (through its device pointer) with the sequence stamp behind
// them: what a hipMemcpyAsync + hipStreamSynchronize pair did with a runtime copy kernel (11 us) and the runtime's wait.
__global__ void publish_kernel(const double* __restrict__ src, int n, double* __restrict__ host, double* __restrict__ stamp, double seq) {
    const int tid = threadIdx.x;
    if (tid < n) host[tid] = src[tid];
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(stamp, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

void launch_publish(const double* src, int n, double* host_block, int host_lo, double seq, hipStream_t st) {
    // host_block: device pointer of the pinned block
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, st, src, n, host_block + host_lo, host_block + RB_STAMP, seq);
    MGB_HIP_CHECK(hipGetLastError());
}

// The two read-backs of a Newton iteration (slots: readback.hpp, finish_direction_params / finish_trial_params)
void launch_dir_finish(const double* v, const double* g, int64_t n, double* scratch, double* scal, int32_t* status2, double* host,
                       hipStream_t st, const double* mask, double seq) {
    const int nb = reduce_blocks(n);
    hipLaunchKernelGGL(dir_stats_kernel, dim3(nb), dim3(256), 0, st, v, g, n, scratch, mask);
    launch_finish(finish_direction_params(scratch, nb, scal, status2, host, seq), st);
}

void launch_trial_finish(const double* g, int64_t n, double* scratch, const double* f0_partials, int64_t f0_count, double* scal,
                         int32_t* moved, double* host, hipStream_t st, const double* mask, double seq, bool partials_ready) {
    const int nb = reduce_blocks(n);
    if (!partials_ready) hipLaunchKernelGGL(block_reduce_kernel<1>, dim3(nb), dim3(256), 0, st, g, (const double*)nullptr, n, scratch, mask);
    launch_finish(finish_trial_params(f0_partials, f0_count, scratch, nb, scal, moved, host, seq), st);
}

void launch_restrict_trial(int64_t rows, const int32_t* ptr, const int32_t* col, const double* val, const double* ret, double* g,
                            double* scratch, const double* x, const double* nn, double s, double* xn, int32_t* moved, int32_t stamp,
                            hipStream_t st) {
    if (rows == 0) return;
    const int nb = reduce_blocks(rows);                      // the partial-sum layout launch_trial_finish reads
    hipLaunchKernelGGL(restrict_trial_kernel, dim3(nb), dim3(256), 0, st, rows, ptr, col, val, ret, g, scratch, x, nn, s, xn, moved, stamp);
    MGB_HIP_CHECK(hipGetLastError());
}

}  // namespace mgbhip
