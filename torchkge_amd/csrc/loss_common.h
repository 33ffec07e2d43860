// What the training criteria share: the quad accessors, softplus / sigma, and the fixed fp64 summation tree documented
// in include/kge_hip_train.h ("The sum") -- ONE definition behind kge_pair_loss (pair_loss.hip) and kge_group_loss
// (group_loss.hip).  The tree over n fp32 terms, indexed 0 .. n - 1:
//   stage 1   G = st_grid(n) blocks of ST_THREADS threads; thread t of block b owns the terms
//             (k * G + b) * ST_CHUNK + 4 t + {0, 1, 2, 3}, k = 0, 1, ...: st_thread_sum() hands every such quad to the
//             caller's functor, which produces the four terms (and whatever else belongs to them: gradients, row
//             outputs); terms from n on count 0.  st_block_sum(): butterfly, then LDS across the four wavefronts.
//   stage 2   G > 1: st_final_kernel, one block over the G partials of the workspace.
// Every addition is in fp64 and its order is a function of n alone.
#ifndef KGE_LOSS_COMMON_H
#define KGE_LOSS_COMMON_H

#include "kge_common.h"
#include "../../include/kge_hip_train.h"

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_CHUNK = KGE_PAIR_LOSS_CHUNK;   // terms per block and turn
constexpr int ST_MAX_BLOCKS = 1024;
static_assert(ST_CHUNK == 4 * ST_THREADS, "a thread owns one quad per turn");

inline int st_grid(int64_t n)
{
    const int64_t g = (n + ST_CHUNK - 1) / ST_CHUNK;
    return (int)(g < ST_MAX_BLOCKS ? g : ST_MAX_BLOCKS);
}

// the turns of one thread in ascending order: term4(j, t) fills the terms of the quad at j (entries from n on are
// ignored); the four are widened and added as (t0 + t1) + (t2 + t3)
template <class Term4>
__device__ __forceinline__ double st_thread_sum(int64_t n, Term4 term4)
{
    double acc = 0.0;
    const int64_t step = (int64_t)gridDim.x * ST_CHUNK;
    for (int64_t j = (int64_t)blockIdx.x * ST_CHUNK + 4 * threadIdx.x; j < n; j += step) {
        float t[4];
        term4(j, t);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = j + e < n ? t[e] : 0.f;
        acc += ((double)t[0] + (double)t[1]) + ((double)t[2] + (double)t[3]);
    }
    return acc;
}

// the 256 fp64 values of a block, in the fixed order of the header; the result is valid in thread 0
__device__ __forceinline__ double st_block_sum(double v, double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ void st_write_loss(float *loss, float *acc_io, double s)
{
    const float l = (float)s;
    *loss = l;
    if (acc_io) *acc_io = *acc_io + l;
}

// stage 1's last step: G = 1 writes *loss itself, otherwise the block's partial goes to the workspace
__device__ __forceinline__ void st_finish_block(double acc, double *sh, double *part, float *loss, float *acc_io)
{
    const double s = st_block_sum(acc, sh);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) st_write_loss(loss, acc_io, s);
        else part[blockIdx.x] = s;
    }
}

__device__ __forceinline__ void load_quad(const float *__restrict__ x, int64_t j, int64_t n, bool vec, float (&v)[4])
{
    if (vec && j + 4 <= n) {
        const float4 q = *reinterpret_cast<const float4 *>(x + j);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = j + e < n ? x[j + e] : 0.f;
    }
}

__device__ __forceinline__ void store_quad(float *__restrict__ x, int64_t j, int64_t n, bool vec, const float (&v)[4])
{
    if (vec && j + 4 <= n) {
        *reinterpret_cast<float4 *>(x + j) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j + e < n) x[j + e] = v[e];
    }
}

// softplus(x) and sigma(x) from one e = exp(-|x|) in (0, 1]: no overflow, no inf / inf
__device__ __forceinline__ void softplus_sigma(float x, float &sp, float &sg)
{
    const float e = expf(-fabsf(x));
    sp = fmaxf(x, 0.f) + log1pf(e);
    const float den = 1.f + e;
    sg = (x >= 0.f ? 1.f : e) / den;
}

__global__ __launch_bounds__(ST_THREADS) void st_final_kernel(const double *part, int G, float *loss, float *acc_io)
{
    __shared__ double sh[ST_THREADS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < G; i += ST_THREADS) acc += part[i];
    const double s = st_block_sum(acc, sh);
    if (threadIdx.x == 0) st_write_loss(loss, acc_io, s);
}

} // namespace
#endif /* KGE_LOSS_COMMON_H */
