// kge_segment_sum_rows (include/kge_hip.h): the segmented row sum behind every model's backward -- per-triple gradient
// rows added by target row, with one atomic row-add per run of equal keys.  Its counterpart without a float atomic and
// with a fixed summation order is kge_segment_sum_ordered (segment_sum_ordered.hip); the two share the chunk size, the
// grid and the argument check (segment_levels.h), not the chunk walk.
#include "kge_common.h"
#include "segment_levels.h"

namespace {

// Reduction of per-triple gradient rows by target row, in SORTED key order: a wavefront walks 32
// consecutive sorted entries, sums runs of equal keys in registers and flushes each run with one
// atomic row-add -- a handful of atomics per chunk instead of one per (triple, dimension), and the
// heavily shared relation rows (n_rel << B) stop serialising on the same addresses.
template <int NE>
__global__ __launch_bounds__(256) void segment_sum_kernel(const float *__restrict__ rows, int64_t ld, int d,
                                                          const int64_t *__restrict__ k0, int64_t n0,
                                                          const int64_t *__restrict__ k1, int64_t n1,
                                                          const int64_t *__restrict__ perm,
                                                          float *__restrict__ out, int64_t out_ld)
{
    constexpr int CH = KGE_DET_CH, UN = 4;
    const int64_t M = n0 + n1;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t j0 = wave * CH; j0 < M; j0 += nwaves * CH) {
        const int n = (int)min((int64_t)CH, M - j0);
        // the chunk's (row, key) pairs: one coalesced load, then broadcast by shuffle
        const int64_t jl = j0 + min(lane, n - 1);
        const int64_t my_row = perm[jl], my_key = my_row < n0 ? k0[my_row] : k1[my_row - n0];
        float acc[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] = 0.f;
        int64_t cur = __shfl(my_key, 0, 64);
        for (int j = 0; j < n; j += UN) {
            float v[UN][NE];
            int64_t kk[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {      // UN independent row loads in flight
                const int ju = min(j + u, n - 1);
                kk[u] = __shfl(my_key, ju, 64);
                const float *row = rows + __shfl(my_row, ju, 64) * ld;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int k = lane + 64 * e;
                    v[u][e] = (k < d && j + u < n) ? row[k] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                if (j + u < n && kk[u] != cur) {    // wave-uniform
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int k = lane + 64 * e;
                        if (k < d && acc[e] != 0.f) atomicAdd(out + cur * out_ld + k, acc[e]);
                        acc[e] = 0.f;
                    }
                    cur = kk[u];
                }
#pragma unroll
                for (int e = 0; e < NE; ++e) acc[e] += v[u][e];
            }
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int k = lane + 64 * e;
            if (k < d && acc[e] != 0.f) atomicAdd(out + cur * out_ld + k, acc[e]);
        }
    }
}

} // namespace

extern "C" int kge_segment_sum_rows(const float *rows, int64_t ld, int d, const int64_t *k0, int64_t n0,
                                    const int64_t *k1, int64_t n1, const int64_t *perm, float *out, int64_t out_ld,
                                    kge_stream_t stream)
{
    const int todo = kge_seg_check_args(rows, ld, d, k0, n0, k1, n1, perm, out, out_ld);
    if (todo <= 0) return todo < 0 ? KGE_EINVAL : 0;
    const int grid = kge_seg_grid(n0 + n1);
    hipStream_t s = kge_s(stream);
    if (d <= 256) hipLaunchKernelGGL(segment_sum_kernel<4>, dim3(grid), dim3(256), 0, s, rows, ld, d, k0, n0, k1, n1, perm, out, out_ld);
    else if (d <= 512) hipLaunchKernelGGL(segment_sum_kernel<8>, dim3(grid), dim3(256), 0, s, rows, ld, d, k0, n0, k1, n1, perm, out, out_ld);
    else hipLaunchKernelGGL(segment_sum_kernel<16>, dim3(grid), dim3(256), 0, s, rows, ld, d, k0, n0, k1, n1, perm, out, out_ld);
    KGE_CHECK_LAUNCH();
    return 0;
}
