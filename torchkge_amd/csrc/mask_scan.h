// Exclusive prefix count of a byte mask, the scheme the corruption kernels share (corrupt.hip, triplet.hip, relation_corrupt.hip): every
// position of a batch learns how many non-zero mask bytes lie before it, which is its index into the draw arrays.
//
//   mask_count_kernel    one int32 count per block of MS_CB positions
//   mask_scan_kernel     exclusive scan of the block counts in place (one block)
//   mask_thread_prefix   inside the consumer kernel: block base + wave scan = #ones before the thread's first element
//
// The consumer is launched with MS_CT threads over ceil(n / MS_CB) blocks and thread t of block b owns positions
// b * MS_CB + t * MS_CE + [0, MS_CE).  Workspace: mask_scan_ws_elems(n) int32.
#pragma once
#include "kge_common.h"

namespace {

constexpr int MS_CT = 256;              // threads per block
constexpr int MS_CE = 4;                // elements per thread
constexpr int MS_CB = MS_CT * MS_CE;    // elements per block

__global__ __launch_bounds__(MS_CT) void mask_count_kernel(const uint8_t *__restrict__ mask, int64_t n,
                                                           int32_t *block_counts)
{
    __shared__ int sh[MS_CT / 64];
    const int64_t base = (int64_t)blockIdx.x * MS_CB;
    int c = 0;
#pragma unroll
    for (int e = 0; e < MS_CE; ++e) {
        const int64_t j = base + threadIdx.x * MS_CE + e;
        if (j < n) c += mask[j] != 0;
    }
    c = wave_sum_i(c);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < MS_CT / 64; ++i) t += sh[i];
        block_counts[blockIdx.x] = t;
    }
}

// exclusive scan of block_counts in place (single block, serial carry over chunks)
__global__ __launch_bounds__(MS_CT) void mask_scan_kernel(int32_t *block_counts, int64_t nb)
{
    __shared__ int sh[MS_CT];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += MS_CT) {
        const int64_t j = base + threadIdx.x;
        const int v = j < nb ? block_counts[j] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < MS_CT; o <<= 1) { // Hillis-Steele inclusive scan
            int add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        const int incl = sh[threadIdx.x];
        if (j < nb) block_counts[j] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == MS_CT - 1) carry += incl;
        __syncthreads();
    }
}

// m[e] = (mask of the thread's e-th position != 0), 0 past n; returns the number of non-zero mask bytes before the
// thread's first position.  Every thread of the block must call (one __syncthreads inside).
__device__ __forceinline__ int mask_thread_prefix(const uint8_t *__restrict__ mask, int64_t n,
                                                  const int32_t *__restrict__ block_base, int (&m)[MS_CE])
{
    __shared__ int sh[MS_CT / 64];
    const int64_t base = (int64_t)blockIdx.x * MS_CB;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int c = 0;
#pragma unroll
    for (int e = 0; e < MS_CE; ++e) {
        const int64_t j = base + threadIdx.x * MS_CE + e;
        m[e] = (j < n) ? (mask[j] != 0) : 0;
        c += m[e];
    }
    // exclusive scan of per-thread counts: within wave, then across waves
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) sh[w] = incl;
    __syncthreads();
    int wbase = 0;
    for (int i = 0; i < w; ++i) wbase += sh[i];
    return block_base[blockIdx.x] + wbase + incl - c;
}

inline int64_t mask_scan_blocks(int64_t n) { return (n + MS_CB - 1) / MS_CB; }
inline int64_t mask_scan_ws_elems(int64_t n) { return mask_scan_blocks(n) + 1; }

// the two launches that leave every block's base in ws[0 .. blocks); n > 0
inline int mask_scan_launch(const uint8_t *mask, int64_t n, int32_t *ws, hipStream_t s)
{
    const int64_t nb = mask_scan_blocks(n);
    hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)nb), dim3(MS_CT), 0, s, mask, n, ws);
    KGE_CHECK_LAUNCH();
    hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(MS_CT), 0, s, ws, nb);
    KGE_CHECK_LAUNCH();
    return 0;
}

} // namespace
