// Ordering of small-integer ids for the backward's sorted gradient reduction (gfx950).
//
// score_triples_bwd writes one gradient row per (triple, operand) and kge_segment_sum_rows adds the rows of equal
// target id with one atomic row-add per run -- which needs the positions of [k0 | k1] ordered by id.  The ids are
// entity / relation indices (< 2^key_bits), so a device radix sort over key_bits bits of (id, position) pairs does it in
// two or three passes: rocPRIM's radix_sort_pairs on 32-bit keys and a counting iterator for the positions.
// (kge_key_hist / kge_key_scatter at the end of this file are the counting-sort alternative: their wave-aggregated atomics
// walk up to 64 distinct ids per wavefront one after the other, 113 us per id stream at B = 32768 against ~25 here.)
#include "kge_common.h"
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace {

__global__ void key_pack_kernel(const int64_t *__restrict__ k0, int64_t n0, const int64_t *__restrict__ k1, int64_t n1,
                                unsigned *__restrict__ keys)
{
    const int64_t n = n0 + n1;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x)
        keys[j] = (unsigned)(j < n0 ? k0[j] : k1[j - n0]);
}

__global__ void perm_widen_kernel(const unsigned *__restrict__ pos, int64_t n, int64_t *__restrict__ perm)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x)
        perm[j] = (int64_t)pos[j];
}

// counting sort of small-integer keys (entity / relation ids): histogram, (host: cumsum), scatter.
// Atomics are aggregated per wavefront: one atomic per DISTINCT key among a wavefront's 64 keys.  Real
// graphs are heavy-tailed (a hub entity / relation owns 10% of a batch) and same-address atomics
// serialise at ~12 ns each past the L2s: 100 us per launch at B = 32768 on a Zipf batch before this.
__device__ __forceinline__ int64_t readlane64(int64_t v, int src)
{
    const unsigned lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffll), src);
    const unsigned hi = __builtin_amdgcn_readlane((int)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__global__ void key_hist_kernel(const int64_t *__restrict__ k0, int64_t n0, const int64_t *__restrict__ k1, int64_t n1,
                                int32_t *hist)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = n0 + n1, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t jb = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; jb < n; jb += stride) {   // wave-uniform trip count
        const int64_t j = jb + lane;
        const bool act = j < n;
        const int64_t key = act ? (j < n0 ? k0[j] : k1[j - n0]) : -1;
        unsigned long long todo = __ballot(act);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int64_t kl = readlane64(key, lead);
            const unsigned long long same = __ballot(act && key == kl);
            if (lane == lead) atomicAdd(&hist[kl], (int)__popcll(same));
            todo &= ~same;
        }
    }
}
__global__ void key_scatter_kernel(const int64_t *__restrict__ k0, int64_t n0, const int64_t *__restrict__ k1,
                                   int64_t n1, const int64_t *__restrict__ offsets, int32_t *cursor, int64_t *perm)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = n0 + n1, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t jb = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; jb < n; jb += stride) {
        const int64_t j = jb + lane;
        const bool act = j < n;
        const int64_t key = act ? (j < n0 ? k0[j] : k1[j - n0]) : -1;
        unsigned long long todo = __ballot(act);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int64_t kl = readlane64(key, lead);
            const unsigned long long same = __ballot(act && key == kl);
            int base = 0;
            if (lane == lead) base = atomicAdd(&cursor[kl], (int)__popcll(same));
            base = __builtin_amdgcn_readlane(base, lead);
            if (act && key == kl) perm[offsets[kl] + base + (int)__popcll(same & ((1ull << lane) - 1ull))] = j;
            todo &= ~same;
        }
    }
}

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

size_t sort_temp_bytes(int64_t n, int key_bits)
{
    size_t bytes = 0;
    unsigned *nul = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, nul, nul, rocprim::counting_iterator<unsigned>(0), nul, (size_t)n, 0u,
                                    (unsigned)key_bits);
    return bytes;
}

} // namespace

/* bytes of workspace kge_key_sort needs for n ids of key_bits bits */
extern "C" int64_t kge_key_sort_ws_bytes(int64_t n, int key_bits)
{
    if (n <= 0 || key_bits <= 0 || key_bits > 32 || n > 0x7fffffffll) return 0;
    return (int64_t)(3 * align256((size_t)n * 4) + align256(sort_temp_bytes(n, key_bits)));
}

/* perm[j] = position (into [k0 | k1]) of the j-th id in ascending id order (stable); ids must be < 2^key_bits */
extern "C" int kge_key_sort(const int64_t *k0, int64_t n0, const int64_t *k1, int64_t n1, int key_bits, int64_t *perm,
                            void *ws, int64_t ws_bytes, kge_stream_t stream)
{
    if (n0 < 0 || n1 < 0 || !perm || (n0 > 0 && !k0) || (n1 > 0 && !k1) || key_bits <= 0 || key_bits > 32) return KGE_EINVAL;
    const int64_t n = n0 + n1;
    if (n == 0) return 0;
    if (n > 0x7fffffffll || !ws || ws_bytes < kge_key_sort_ws_bytes(n, key_bits)) return KGE_EINVAL;
    hipStream_t s = kge_s(stream);
    char *w = reinterpret_cast<char *>(ws);
    const size_t a = align256((size_t)n * 4);
    unsigned *keys_in = reinterpret_cast<unsigned *>(w), *keys_out = reinterpret_cast<unsigned *>(w + a),
             *pos_out = reinterpret_cast<unsigned *>(w + 2 * a);
    void *temp = w + 3 * a;
    size_t temp_bytes = (size_t)ws_bytes - 3 * a;
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(key_pack_kernel, dim3(grid), dim3(256), 0, s, k0, n0, k1, n1, keys_in);
    KGE_CHECK_LAUNCH();
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, rocprim::counting_iterator<unsigned>(0),
                                             pos_out, (size_t)n, 0u, (unsigned)key_bits, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(perm_widen_kernel, dim3(grid), dim3(256), 0, s, pos_out, n, perm);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_key_hist(const int64_t *k0, int64_t n0, const int64_t *k1, int64_t n1, int32_t *hist,
                            kge_stream_t stream)
{
    if (n0 < 0 || n1 < 0 || !hist || (n0 > 0 && !k0) || (n1 > 0 && !k1)) return KGE_EINVAL;
    if (n0 + n1 == 0) return 0;
    const int64_t n = n0 + n1;
    hipLaunchKernelGGL(key_hist_kernel, dim3((int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0,
                       kge_s(stream), k0, n0, k1, n1, hist);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_key_scatter(const int64_t *k0, int64_t n0, const int64_t *k1, int64_t n1, const int64_t *offsets,
                               int32_t *cursor, int64_t *perm, kge_stream_t stream)
{
    if (n0 < 0 || n1 < 0 || !offsets || !cursor || !perm || (n0 > 0 && !k0) || (n1 > 0 && !k1)) return KGE_EINVAL;
    if (n0 + n1 == 0) return 0;
    const int64_t n = n0 + n1;
    hipLaunchKernelGGL(key_scatter_kernel, dim3((int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0,
                       kge_s(stream), k0, n0, k1, n1, offsets, cursor, perm);
    KGE_CHECK_LAUNCH();
    return 0;
}
