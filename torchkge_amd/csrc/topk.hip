// K6: top-k selection on a materialised score matrix or one tile of it (gfx950): kge_topk, kge_topk_chunk.
//   the (b, N) sort + slice of EntityInference.evaluate  inference.py:216-250, as per-tile top-k + merge
#include "kge_common.h"

namespace {

// top-k of each row in the strict order (score descending, index ascending):
// pass j finds the largest element that is strictly after the (j-1)-th pick, so
// nothing is marked or copied; k passes over a row that stays in L2.  NaNs are
// never selected (as with `>`-based comparison); exhausted rows yield (-inf, -1).
__global__ __launch_bounds__(RB) void topk_kernel(const float *__restrict__ scores, int64_t ld, int64_t B,
                                                  int64_t N, int k, int64_t *out_idx, float *out_val)
{
    __shared__ float sv[RB / 64];
    __shared__ int64_t si[RB / 64];
    for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
        const float *row = scores + i * ld;
        float last_v = INFINITY;
        int64_t last_i = -1;
        for (int j = 0; j < k; ++j) {
            float bv = -INFINITY;
            int64_t bi = -1;
            for (int64_t c = threadIdx.x; c < N; c += blockDim.x) {
                const float v = row[c];
                const bool after = (v < last_v) || (v == last_v && c > last_i);   // not picked yet
                const bool better = (v > bv) || (v == bv && (bi < 0 || c < bi));
                if (after && better && v == v) { bv = v; bi = c; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int64_t oi = __shfl_xor(bi, o, 64);
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            __syncthreads();
            if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
            __syncthreads();
            bv = sv[0]; bi = si[0];
            for (int w = 1; w < RB / 64; ++w)
                if (si[w] >= 0 && (bi < 0 || sv[w] > bv || (sv[w] == bv && si[w] < bi))) { bv = sv[w]; bi = si[w]; }
            if (threadIdx.x == 0) { out_idx[i * k + j] = bi; out_val[i * k + j] = bi >= 0 ? bv : -INFINITY; }
            if (bi < 0) { last_v = -INFINITY; last_i = N; } else { last_v = bv; last_i = bi; }
        }
    }
}

// Top-k of a row CHUNK: the columns are candidates [c_base, c_base + C) of a larger candidate set (one tile of the
// entity table, or one entity shard), processed tile by tile so that only (B, C) scores ever exist.  Optionally the
// known targets of the row's filter segment that fall into the chunk are masked first (filter_scores with
// true_idx = None, utils/modeling.py:83-84 as used by inference.py:146, :241) -- in place, the tile is scratch.
// Output slot `col_off` of a (B, ldo) buffer: the tile's k best as (score, GLOBAL id), order (score descending, id
// ascending).  The same kernel MERGES partial lists: `ids_in` then names the candidates of the columns (entries
// with id < 0 are padding and never selected); partial lists laid out chunk after chunk keep the id-ascending tie
// order because every chunk's list is itself in that order and chunks are ascending id ranges.
__global__ __launch_bounds__(RB) void topk_chunk_kernel(float *__restrict__ scores, int64_t ld, int64_t B, int64_t C,
                                                        int64_t c_base, int k, const int64_t *__restrict__ seg_lo,
                                                        const int64_t *__restrict__ seg_hi,
                                                        const int32_t *__restrict__ targets,
                                                        const int64_t *__restrict__ ids_in, int64_t ld_ids,
                                                        int64_t *out_idx, float *out_val, int64_t ldo, int64_t col_off)
{
    __shared__ float sv[RB / 64];
    __shared__ int64_t si[RB / 64];
    for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
        float *row = scores + i * ld;
        if (targets) {
            for (int64_t j = seg_lo[i] + threadIdx.x; j < seg_hi[i]; j += blockDim.x) {
                const int64_t t = (int64_t)targets[j] - c_base;
                if (t >= 0 && t < C) row[t] = -INFINITY;
            }
            __syncthreads();
        }
        const int64_t *ids = ids_in ? ids_in + i * ld_ids : nullptr;
        float last_v = INFINITY;
        int64_t last_i = -1;
        for (int j = 0; j < k; ++j) {
            float bv = -INFINITY;
            int64_t bi = -1;
            for (int64_t c = threadIdx.x; c < C; c += blockDim.x) {
                const float v = row[c];
                const bool after = (v < last_v) || (v == last_v && c > last_i);   // not picked yet
                const bool better = (v > bv) || (v == bv && (bi < 0 || c < bi));
                const bool real = ids ? ids[c] >= 0 : true;
                if (after && better && v == v && real) { bv = v; bi = c; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int64_t oi = __shfl_xor(bi, o, 64);
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            __syncthreads();
            if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
            __syncthreads();
            bv = sv[0]; bi = si[0];
            for (int w = 1; w < RB / 64; ++w)
                if (si[w] >= 0 && (bi < 0 || sv[w] > bv || (sv[w] == bv && si[w] < bi))) { bv = sv[w]; bi = si[w]; }
            if (threadIdx.x == 0) {
                out_idx[i * ldo + col_off + j] = bi < 0 ? -1 : (ids ? ids[bi] : bi + c_base);
                out_val[i * ldo + col_off + j] = bi >= 0 ? bv : -INFINITY;
            }
            if (bi < 0) { last_v = -INFINITY; last_i = C; } else { last_v = bv; last_i = bi; }
        }
        __syncthreads();
    }
}

// The same selection in ONE pass over the tile for k <= KMAX (r04): a wavefront per row, every lane keeps the KMAX best
// of its columns (lane, lane + 64, ...) as a sorted register list -- a compare-exchange chain per visited element whose
// list it enters --, then the 64 lists are merged by k rounds of a wave arg-max over the list heads (the winner's list
// shifts up).  Order (score descending, id ascending), NaN never selected, -inf entries fill up in id order, padding
// ids (< 0, merge mode) skipped: output identical to topk_chunk_kernel's, which re-read the whole tile k times.
template <int KMAX>
__global__ __launch_bounds__(RB) void topk_chunk_reg_kernel(float *__restrict__ scores, int64_t ld, int64_t B, int64_t C,
                                                            int64_t c_base, int k, const int64_t *__restrict__ seg_lo,
                                                            const int64_t *__restrict__ seg_hi,
                                                            const int32_t *__restrict__ targets,
                                                            const int64_t *__restrict__ ids_in, int64_t ld_ids,
                                                            int64_t *out_idx, float *out_val, int64_t ldo, int64_t col_off)
{
    constexpr int EMPTY = 0x7fffffff;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t i0 = (int64_t)blockIdx.x * (RB / 64); i0 < B; i0 += (int64_t)gridDim.x * (RB / 64)) {
        const int64_t i = i0 + wv;
        const bool active = i < B;
        float *row = scores + (active ? i : 0) * ld;
        if (targets) {
            if (active)
                for (int64_t j = seg_lo[i] + lane; j < seg_hi[i]; j += 64) {
                    const int64_t t = (int64_t)targets[j] - c_base;
                    if (t >= 0 && t < C) row[t] = -INFINITY;
                }
            __syncthreads();
        }
        if (!active) continue;      // (no block-wide barrier below this point)
        const int64_t *ids = ids_in ? ids_in + i * ld_ids : nullptr;
        float lv[KMAX];
        int li[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) { lv[j] = -INFINITY; li[j] = EMPTY; }
        // Wave-wide pruning threshold: after 16 / 64 / 256 full iterations the k-th best entry of the 64 lists is selected
        // (on copies).  Every later element has a LARGER id than all entries seen so far (iteration t covers ids
        // [64 t, 64 t + 63]), so one whose score does not exceed that k-th score already has k entries ahead of it in
        // the (score descending, id ascending) order and can never be selected: after the first thousand columns only
        // ~k ln(C / 1024) elements per ROW still run the insertion chain, and the scan is bandwidth bound.
        float tau = 0.f;
        bool tau_on = false;
        auto refresh_tau = [&]() __attribute__((always_inline)) {    // (every lane active)
            float cv[KMAX];
            int ci[KMAX];
#pragma unroll
            for (int j = 0; j < KMAX; ++j) { cv[j] = lv[j]; ci[j] = li[j]; }
            float bv = -INFINITY;
            int bi = EMPTY;
            for (int j = 0; j < k; ++j) {
                bv = cv[0];
                bi = ci[0];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ov = __shfl_xor(bv, o, 64);
                    const int oi = __shfl_xor(bi, o, 64);
                    if (oi != EMPTY && (bi == EMPTY || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
                }
                if (bi != EMPTY && ci[0] == bi) {
#pragma unroll
                    for (int q = 0; q + 1 < KMAX; ++q) { cv[q] = cv[q + 1]; ci[q] = ci[q + 1]; }
                    cv[KMAX - 1] = -INFINITY;
                    ci[KMAX - 1] = EMPTY;
                }
            }
            tau_on = bi != EMPTY;       // k real entries exist: their k-th score prunes
            tau = bv;
        };
        auto visit = [&](float v, int64_t c, bool real) __attribute__((always_inline)) {
            // enters the list iff it beats the list's last entry (strictly, or at equal score by the smaller column)
            if (real && (!tau_on || v > tau) && (v > lv[KMAX - 1] || (v == lv[KMAX - 1] && (int)c < li[KMAX - 1]))) {
                float cv = v;
                int ci = (int)c;
#pragma unroll
                for (int j = 0; j < KMAX; ++j) {
                    const bool gt = cv > lv[j] || (cv == lv[j] && ci < li[j]);
                    const float tv = gt ? lv[j] : cv;
                    const int ti = gt ? li[j] : ci;
                    lv[j] = gt ? cv : lv[j];
                    li[j] = gt ? ci : li[j];
                    cv = tv;
                    ci = ti;
                }
            }
        };
        // full steps of UN iterations (every lane active): the UN loads are issued together, then visited in id order
        constexpr int UN = 8;
        int64_t t = 0;                                  // iteration = 64 consecutive columns
        const int64_t t_full = C / (64 * UN) * UN;      // iterations covered by full steps
        for (; t < t_full; t += UN) {
            if (t == 16 || t == 64 || t == 256) refresh_tau();
            float v[UN];
            bool real[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int64_t c = (t + u) * 64 + lane;
                v[u] = row[c];
                real[u] = ids ? ids[c] >= 0 : true;
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) visit(v[u], (t + u) * 64 + lane, real[u]);
        }
        for (int64_t c = t * 64 + lane; c < C; c += 64) visit(row[c], c, ids ? ids[c] >= 0 : true);
        for (int j = 0; j < k; ++j) {
            float bv = lv[0];
            int bi = li[0];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (oi != EMPTY && (bi == EMPTY || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            if (lane == 0) {
                out_idx[i * ldo + col_off + j] = bi == EMPTY ? -1 : (ids ? ids[bi] : (int64_t)bi + c_base);
                out_val[i * ldo + col_off + j] = bi != EMPTY ? bv : -INFINITY;
            }
            if (bi != EMPTY && li[0] == bi) {     // this lane's head was taken: its list moves up
#pragma unroll
                for (int q = 0; q + 1 < KMAX; ++q) { lv[q] = lv[q + 1]; li[q] = li[q + 1]; }
                lv[KMAX - 1] = -INFINITY;
                li[KMAX - 1] = EMPTY;
            }
        }
    }
}

} // namespace

extern "C" int kge_topk_chunk(float *scores, int64_t ld, int64_t B, int64_t C, int64_t c_base, int k,
                              const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *targets,
                              const int64_t *ids_in, int64_t ld_ids, int64_t *out_idx, float *out_val, int64_t ldo,
                              int64_t col_off, kge_stream_t stream)
{
    if (B < 0 || C <= 0 || ld < C || k <= 0 || col_off < 0 || ldo < col_off + k) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!scores || !out_idx || !out_val) return KGE_EINVAL;
    if (targets && (!seg_lo || !seg_hi)) return KGE_EINVAL;
    if (ids_in && ld_ids < C) return KGE_EINVAL;
    // k <= 32 (and columns that fit an int): the single-pass register selection; larger k: k passes over the tile
    static const int reg_topk = kge_env_int("KGE_TOPK_REG", 1);
    if (reg_topk && k <= 32 && C < 0x7fffffff) {
        const dim3 grid(grid1d(B, RB / 64)), block(RB);
        if (k <= 8)
            hipLaunchKernelGGL(topk_chunk_reg_kernel<8>, grid, block, 0, kge_s(stream), scores, ld, B, C, c_base, k, seg_lo, seg_hi,
                               targets, ids_in, ld_ids, out_idx, out_val, ldo, col_off);
        else if (k <= 16)
            hipLaunchKernelGGL(topk_chunk_reg_kernel<16>, grid, block, 0, kge_s(stream), scores, ld, B, C, c_base, k, seg_lo, seg_hi,
                               targets, ids_in, ld_ids, out_idx, out_val, ldo, col_off);
        else
            hipLaunchKernelGGL(topk_chunk_reg_kernel<32>, grid, block, 0, kge_s(stream), scores, ld, B, C, c_base, k, seg_lo, seg_hi,
                               targets, ids_in, ld_ids, out_idx, out_val, ldo, col_off);
        KGE_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(topk_chunk_kernel, dim3(grid1d(B, 1)), dim3(RB), 0, kge_s(stream), scores, ld, B, C, c_base, k,
                       seg_lo, seg_hi, targets, ids_in, ld_ids, out_idx, out_val, ldo, col_off);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_topk(const float *scores, int64_t ld, int64_t B, int64_t N, int k, int64_t *out_idx,
                        float *out_val, kge_stream_t stream)
{
    if (B < 0 || N <= 0 || ld < N || k <= 0) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!scores || !out_idx || !out_val) return KGE_EINVAL;
    hipLaunchKernelGGL(topk_kernel, dim3(grid1d(B, 1)), dim3(RB), 0, kge_s(stream), scores, ld, B, N, k, out_idx, out_val);
    KGE_CHECK_LAUNCH();
    return 0;
}
