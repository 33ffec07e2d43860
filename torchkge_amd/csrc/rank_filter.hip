// K4: rank / filter kernels (integer results, bit-exact to the reference) and
// the entry points that dispatch the all-candidates scorers (gfx950).
//   get_rank                      utils/operations.py:37-61
//   get_true_targets/filter_scores utils/modeling.py:53-102
//   the rank/filter half of LinkPredictionEvaluator.evaluate  evaluation.py:290-300
// HBM-bound streaming over the (B,N) matrix when it is materialised; the fused
// path (pair scores + count_ge + filter_sub + finalize) never materialises it.
#include "kge_common.h"

int kge_lp_gemm_run(const kge_lp_desc *d, float *out, int64_t ldo, const float *s_true,
                    int32_t *raw_count, hipStream_t s);
int kge_lp_direct_count_cols(const kge_lp_desc *d, const float *s_true, int32_t *raw_count, const int64_t *rep,
                             const int32_t *col_q, int64_t n_single_p, const int32_t *members, int64_t n_multi_p,
                             hipStream_t s);
int kge_lp_direct_run(const kge_lp_desc *d, float *out, int64_t ldo, const float *s_true,
                      int32_t *raw_count, hipStream_t s);

namespace {

__device__ __forceinline__ int count_row(const float *__restrict__ row, int64_t N, float tv, bool low)
{
    int c = 0;
    const int64_t head = ((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) >> 2; // floats to 16B
    const int64_t nh = head < N ? head : N;
    for (int64_t j = threadIdx.x; j < nh; j += blockDim.x) c += low ? (row[j] <= tv) : (row[j] >= tv);
    const int64_t n4 = (N - nh) >> 2;
    const float4 *r4 = reinterpret_cast<const float4 *>(row + nh);
    for (int64_t j = threadIdx.x; j < n4; j += blockDim.x) {
        const float4 v = r4[j];
        if (low) c += (v.x <= tv) + (v.y <= tv) + (v.z <= tv) + (v.w <= tv);
        else c += (v.x >= tv) + (v.y >= tv) + (v.z >= tv) + (v.w >= tv);
    }
    for (int64_t j = nh + (n4 << 2) + threadIdx.x; j < N; j += blockDim.x)
        c += low ? (row[j] <= tv) : (row[j] >= tv);
    return c;
}

__global__ __launch_bounds__(RB) void get_rank_kernel(const float *__restrict__ scores, int64_t ld,
                                                      const int64_t *__restrict__ true_idx, int64_t B,
                                                      int64_t N, int low, int64_t *rank)
{
    __shared__ int sh[RB / 64];
    for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
        const float *row = scores + i * ld;
        const float tv = row[true_idx[i]];
        const int c = block_sum_i(count_row(row, N, tv, low != 0), sh);
        if (threadIdx.x == 0) rank[i] = c;
    }
}

__global__ __launch_bounds__(RB) void filtered_rank_kernel(const float *__restrict__ scores, int64_t ld,
                                                           const int64_t *__restrict__ true_idx,
                                                           const int64_t *__restrict__ seg_lo,
                                                           const int64_t *__restrict__ seg_hi,
                                                           const int32_t *__restrict__ targets, int64_t B,
                                                           int64_t N, int64_t *rank, int64_t *filt)
{
    __shared__ int sh[RB / 64];
    for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
        const float *row = scores + i * ld;
        const int64_t ti = true_idx[i];
        const float tv = row[ti];
        const int raw = block_sum_i(count_row(row, N, tv, false), sh);
        int sub = 0, found = 0;
        const int neg_inf_counts = (-INFINITY >= tv) ? 1 : 0;
        for (int64_t j = seg_lo[i] + threadIdx.x; j < seg_hi[i]; j += blockDim.x) {
            const int64_t c = targets[j];
            if (c == ti) { found = 1; continue; }
            if (c >= 0 && c < N) sub += ((row[c] >= tv) ? 1 : 0) - neg_inf_counts;
        }
        sub = block_sum_i(sub, sh);
        found = block_sum_i(found, sh);
        if (threadIdx.x == 0) {
            rank[i] = raw;
            filt[i] = found ? raw - sub : raw;
        }
    }
}

// Ranks of `rows` queries whose score rows arrive as P RANK-MAJOR tiles (the receive buffer of the score all-to-all of
// the entity-sharded path, kge_hip_coll.h): tile p = (m, per) holds the scores of global candidates [p*per, (p+1)*per),
// row i of every tile belongs to query q_first + i.  Same arithmetic as filtered_rank_kernel on the (B, N) matrix the
// tiles would concatenate to -- no re-layout, every tile row read as one contiguous segment.  Results go straight to
// the (4, ld) result matrix of kge_rank_finalize_both (query q < B: tail side of fact q, else head side of fact q - B).
__global__ __launch_bounds__(RB) void filtered_rank_tiles_kernel(const float *__restrict__ tiles, int64_t m, int64_t per,
                                                                 int P, int64_t N, const int64_t *__restrict__ true_idx,
                                                                 const int64_t *__restrict__ seg_lo,
                                                                 const int64_t *__restrict__ seg_hi,
                                                                 const int32_t *__restrict__ targets, int64_t rows,
                                                                 int64_t q_first, int64_t B, int64_t *out, int64_t ld,
                                                                 int64_t off, const int64_t *__restrict__ pos,
                                                                 const float *__restrict__ own, int own_rank)
{
    __shared__ int sh[RB / 64];
    // tile p: the receive buffer's block p -- or, for the caller's own rank, the block it scored itself, read where the
    // scorer wrote it (`own`): the own block never needs to be copied
    auto tile = [&](int64_t p) -> const float * { return (own && p == own_rank) ? own : tiles + p * m * per; };
    for (int64_t i = blockIdx.x; i < rows; i += gridDim.x) {
        const int64_t ti = true_idx[i];
        const int64_t tp = ti / per;
        const float tv = tile(tp)[i * per + (ti - tp * per)];
        int c = 0;
        for (int p = 0; p < P; ++p) {
            const int64_t w = N - (int64_t)p * per;      // candidates this tile really holds (the last one may be short)
            if (w <= 0) break;
            c += count_row(tile(p) + i * per, w < per ? w : per, tv, false);
        }
        const int raw = block_sum_i(c, sh);
        int sub = 0, found = 0;
        const int neg_inf_counts = (-INFINITY >= tv) ? 1 : 0;
        for (int64_t j = seg_lo[i] + threadIdx.x; j < seg_hi[i]; j += blockDim.x) {
            const int64_t cc = targets[j];
            if (cc == ti) { found = 1; continue; }
            if (cc >= 0 && cc < N) {
                const int64_t cp = cc / per;
                sub += ((tile(cp)[i * per + (cc - cp * per)] >= tv) ? 1 : 0) - neg_inf_counts;
            }
        }
        sub = block_sum_i(sub, sh);
        found = block_sum_i(found, sh);
        if (threadIdx.x == 0) {
            const int64_t q = q_first + i;
            const bool tail = q < B;
            const int64_t j = off + (tail ? q : q - B);
            const int64_t f = pos ? pos[j] : j;
            out[(tail ? 1 : 0) * ld + f] = raw;
            out[(tail ? 3 : 2) * ld + f] = found ? raw - sub : raw;
        }
    }
}

__global__ __launch_bounds__(RB) void filter_scores_kernel(float *scores, int64_t ld,
                                                           const int64_t *__restrict__ true_idx,
                                                           const int64_t *__restrict__ seg_lo,
                                                           const int64_t *__restrict__ seg_hi,
                                                           const int32_t *__restrict__ targets, int64_t B,
                                                           int64_t N)
{
    __shared__ int sh[RB / 64];
    for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
        const int64_t lo = seg_lo[i], hi = seg_hi[i];
        // true_idx == NULL (get_true_targets(..., true_idx=None), modeling.py:83-84): mask every known target
        const int64_t ti = true_idx ? true_idx[i] : -1;
        if (true_idx) {
            int found = 0;
            for (int64_t j = lo + threadIdx.x; j < hi; j += blockDim.x) found |= (targets[j] == ti);
            found = block_sum_i(found, sh);
            if (!found) continue; // KeyError / set.remove KeyError: row untouched (modeling.py:87-88)
        }
        float *row = scores + i * ld;
        for (int64_t j = lo + threadIdx.x; j < hi; j += blockDim.x) {
            const int64_t c = targets[j];
            if (c != ti && c >= 0 && c < N) row[c] = -INFINITY;
        }
    }
}

__global__ void filter_lookup_kernel(const int64_t *__restrict__ keys, int64_t n_keys,
                                     const int64_t *__restrict__ offsets, const int64_t *__restrict__ key1,
                                     const int64_t *__restrict__ key2, int64_t n_key2, int64_t B,
                                     int64_t *seg_lo, int64_t *seg_hi)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t key = key1[i] * n_key2 + key2[i];
        int64_t lo = 0, hi = n_keys;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < n_keys && keys[lo] == key) { seg_lo[i] = offsets[lo]; seg_hi[i] = offsets[lo + 1]; }
        else { seg_lo[i] = 0; seg_hi[i] = 0; }
    }
}

__global__ void filter_lookup_both_kernel(const int64_t *__restrict__ keys_t, int64_t n_t,
                                          const int64_t *__restrict__ offs_t, const int64_t *__restrict__ keys_h,
                                          int64_t n_h, const int64_t *__restrict__ offs_h, int64_t base_h,
                                          const int64_t *__restrict__ h, const int64_t *__restrict__ t,
                                          const int64_t *__restrict__ r, int64_t n_key2, int64_t B,
                                          int64_t *seg_lo, int64_t *seg_hi, int64_t *true_idx)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * B; i += (int64_t)gridDim.x * blockDim.x) {
        const bool tail = i < B;
        const int64_t f = tail ? i : i - B;
        const int64_t *keys = tail ? keys_t : keys_h, *offs = tail ? offs_t : offs_h;
        const int64_t n_keys = tail ? n_t : n_h, base = tail ? 0 : base_h;
        const int64_t key = (tail ? h[f] : t[f]) * n_key2 + r[f];
        int64_t lo = 0, hi = n_keys;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < n_keys && keys[lo] == key) { seg_lo[i] = offs[lo] + base; seg_hi[i] = offs[lo + 1] + base; }
        else { seg_lo[i] = 0; seg_hi[i] = 0; }
        true_idx[i] = tail ? t[f] : h[f];
    }
}

__global__ void rank_finalize_kernel(const int32_t *__restrict__ raw, const int32_t *__restrict__ sub,
                                     const int32_t *__restrict__ found, int64_t B, int64_t *rank, int64_t *filt)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = raw[i];
        rank[i] = r;
        filt[i] = found[i] ? r - sub[i] : r;
    }
}

// 2B-query batches (tail-side queries first): ranks straight into the evaluator's (4, n) result rows
// [head raw, tail raw, head filtered, tail filtered] at column off + fact
__global__ void rank_finalize_both_kernel(const int32_t *__restrict__ raw, const int32_t *__restrict__ sub,
                                          const int32_t *__restrict__ found, int64_t B, int64_t *out, int64_t ld,
                                          int64_t off, const int64_t *__restrict__ pos,
                                          float *__restrict__ guard, float *flags, int zero_guard,
                                          int64_t *const *out_indirect)
{
    // (r06) out_indirect: the result matrix of THIS launch is *out_indirect -- a device-visible pointer the host stores there
    // before the launch (a hipGraph replays the launch with the pointer of the day): pinned host memory, so that the ranks
    // need no copy of their own; the flags then sit behind the four rows, as in the evaluator's packed buffer
    if (out_indirect) {
        out = *out_indirect;
        if (flags) flags = reinterpret_cast<float *>(out + 4 * ld);
    }
    // the evaluation's two guard decisions ride the last finalize (instead of an add + a copy node of their own):
    // flags[0] = max ||q||^2 + max ||e||^2 (norm-expansion guard), flags[1] = overflow of the uncertain-pair list
    if (flags && blockIdx.x == 0 && threadIdx.x == 0) {
        flags[0] = guard[0] + guard[1];
        flags[1] = guard[2];
        flags[2] = guard[6];        // pairs the split prefilter re-scored in this evaluation (kge_lp_split_recheck list_stat)
        // ... and the guard vector is left ZEROED for the next evaluation (nobody reads it after this point): the next
        // evaluate() starts without a fill node of its own
        if (zero_guard) {
#pragma unroll
            for (int j = 0; j < 8; ++j) guard[j] = 0.f;
        }
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * B; i += (int64_t)gridDim.x * blockDim.x) {
        const bool tail = i < B;
        const int64_t j = off + (tail ? i : i - B);
        const int64_t f = pos ? pos[j] : j;        // facts processed in another order (e.g. sorted by relation)
        const int64_t r = raw[i];
        out[(tail ? 1 : 0) * ld + f] = r;
        out[(tail ? 3 : 2) * ld + f] = found[i] ? r - sub[i] : r;
    }
}

// generic per-query candidate matrices: one wavefront per (query, candidate)
__global__ __launch_bounds__(256) void lp_batched_kernel(int mode, const float *__restrict__ q, int64_t ldq,
                                                         const float *__restrict__ cand, int64_t stride_b,
                                                         int64_t stride_n, int64_t B, int64_t N, int K,
                                                         float *out, int64_t ldo)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t total = B * N;
    for (int64_t pidx = wave; pidx < total; pidx += (int64_t)gridDim.x * 4) {
        const int64_t i = pidx / N, c = pidx - i * N;
        const float *qq = q + i * ldq;
        const float *cc = cand + i * stride_b + c * stride_n;
        float acc = 0.f;
        if (mode == KGE_LP_CMOD) {      // lanes over the complex coordinates of the interleaved rows (K even)
            for (int k = 2 * lane; k < K; k += 128) acc = acc + lp_cmod_pair(qq[k] - cc[k], qq[k + 1] - cc[k + 1]);
        } else
        for (int k = lane; k < K; k += 64) {
            if (mode == KGE_LP_DOT) acc = fmaf(qq[k], cc[k], acc);
            else {
                const float diff = qq[k] - cc[k];
                switch (mode) {
                case KGE_LP_L1_DIRECT: acc = acc + fabsf(diff); break;
                case KGE_LP_TORUS_L1: acc = acc + lp_direct_term<KGE_LP_TORUS_L1>(diff); break;
                case KGE_LP_TORUS_L2: acc = acc + lp_direct_term<KGE_LP_TORUS_L2>(diff); break;
                case KGE_LP_TORUS_EL2: acc = acc + lp_direct_term<KGE_LP_TORUS_EL2>(diff); break;
                default: acc = fmaf(diff, diff, acc);
                }
            }
        }
        acc = wave_sum(acc);
        float s = acc;
        switch (mode) {
        case KGE_LP_DOT: break;
        case KGE_LP_TORUS_L1: s = lp_direct_finish<KGE_LP_TORUS_L1>(acc); break;
        case KGE_LP_TORUS_L2: s = lp_direct_finish<KGE_LP_TORUS_L2>(acc); break;
        case KGE_LP_TORUS_EL2: s = lp_direct_finish<KGE_LP_TORUS_EL2>(acc); break;
        default: s = -acc;
        }
        if (lane == 0) out[i * ldo + c] = s;
    }
}

} // namespace

extern "C" int kge_get_rank(const float *scores, int64_t ld, const int64_t *true_idx, int64_t B, int64_t N,
                            int low_values, int64_t *rank, kge_stream_t stream)
{
    if (B < 0 || N <= 0 || ld < N) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!scores || !true_idx || !rank) return KGE_EINVAL;
    hipLaunchKernelGGL(get_rank_kernel, dim3(grid1d(B, 1)), dim3(RB), 0, kge_s(stream), scores, ld, true_idx, B, N,
                       low_values, rank);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_filter_lookup(const int64_t *keys, int64_t n_keys, const int64_t *offsets,
                                 const int64_t *key1, const int64_t *key2, int64_t n_key2, int64_t B,
                                 int64_t *seg_lo, int64_t *seg_hi, kge_stream_t stream)
{
    if (B < 0 || n_keys < 0 || n_key2 <= 0) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!key1 || !key2 || !seg_lo || !seg_hi || (n_keys > 0 && (!keys || !offsets))) return KGE_EINVAL;
    hipLaunchKernelGGL(filter_lookup_kernel, dim3(grid1d(B, 256)), dim3(256), 0, kge_s(stream), keys, n_keys,
                       offsets, key1, key2, n_key2, B, seg_lo, seg_hi);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_filter_lookup_both(const int64_t *keys_t, int64_t n_keys_t, const int64_t *offsets_t,
                                      const int64_t *keys_h, int64_t n_keys_h, const int64_t *offsets_h,
                                      int64_t targets_base_h, const int64_t *h, const int64_t *t, const int64_t *r,
                                      int64_t n_key2, int64_t B, int64_t *seg_lo, int64_t *seg_hi,
                                      int64_t *true_idx, kge_stream_t stream)
{
    if (B < 0 || n_keys_t < 0 || n_keys_h < 0 || n_key2 <= 0 || targets_base_h < 0) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!h || !t || !r || !seg_lo || !seg_hi || !true_idx || (n_keys_t > 0 && (!keys_t || !offsets_t)) ||
        (n_keys_h > 0 && (!keys_h || !offsets_h)))
        return KGE_EINVAL;
    hipLaunchKernelGGL(filter_lookup_both_kernel, dim3(grid1d(2 * B, 256)), dim3(256), 0, kge_s(stream), keys_t,
                       n_keys_t, offsets_t, keys_h, n_keys_h, offsets_h, targets_base_h, h, t, r, n_key2, B, seg_lo,
                       seg_hi, true_idx);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_filter_scores(float *scores, int64_t ld, const int64_t *true_idx, const int64_t *seg_lo,
                                 const int64_t *seg_hi, const int32_t *targets, int64_t B, int64_t N,
                                 kge_stream_t stream)
{
    if (B < 0 || N <= 0 || ld < N) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!scores || !seg_lo || !seg_hi) return KGE_EINVAL; // true_idx may be NULL: filter all known targets
    hipLaunchKernelGGL(filter_scores_kernel, dim3(grid1d(B, 1)), dim3(RB), 0, kge_s(stream), scores, ld, true_idx,
                       seg_lo, seg_hi, targets, B, N);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_filtered_rank_from_scores(const float *scores, int64_t ld, const int64_t *true_idx,
                                             const int64_t *seg_lo, const int64_t *seg_hi,
                                             const int32_t *targets, int64_t B, int64_t N, int64_t *rank,
                                             int64_t *filt_rank, kge_stream_t stream)
{
    if (B < 0 || N <= 0 || ld < N) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!scores || !true_idx || !seg_lo || !seg_hi || !rank || !filt_rank) return KGE_EINVAL;
    hipLaunchKernelGGL(filtered_rank_kernel, dim3(grid1d(B, 1)), dim3(RB), 0, kge_s(stream), scores, ld, true_idx,
                       seg_lo, seg_hi, targets, B, N, rank, filt_rank);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_filtered_rank_from_tiles(const float *tiles, int64_t m, int64_t per, int world, int64_t N,
                                            const int64_t *true_idx, const int64_t *seg_lo, const int64_t *seg_hi,
                                            const int32_t *targets, int64_t rows, int64_t q_first, int64_t B,
                                            int64_t *out, int64_t ld, int64_t off, const int64_t *pos,
                                            const float *own, int own_rank, kge_stream_t stream)
{
    if (rows < 0 || rows > m || per <= 0 || world < 1 || N <= 0 || N > (int64_t)world * per) return KGE_EINVAL;
    if (own && (own_rank < 0 || own_rank >= world)) return KGE_EINVAL;
    if (B < 0 || off < 0 || ld < off + B || q_first < 0 || q_first + rows > 2 * B) return KGE_EINVAL;
    if (rows == 0) return 0;
    if ((!tiles && !(own && world == 1)) || !true_idx || !seg_lo || !seg_hi || !out) return KGE_EINVAL;
    hipLaunchKernelGGL(filtered_rank_tiles_kernel, dim3(grid1d(rows, 1)), dim3(RB), 0, kge_s(stream), tiles, m, per,
                       world, N, true_idx, seg_lo, seg_hi, targets, rows, q_first, B, out, ld, off, pos, own, own_rank);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_lp_scores(const kge_lp_desc *d, float *out, int64_t ldo, kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (d->B == 0 || d->N == 0) return 0;
    if (!out || ldo < d->N) return KGE_EINVAL;
    if (KGE_LP_IS_MFMA(d->mode)) return kge_lp_gemm_run(d, out, ldo, nullptr, nullptr, kge_s(stream));
    return kge_lp_direct_run(d, out, ldo, nullptr, nullptr, kge_s(stream));
}

extern "C" int kge_lp_count_ge(const kge_lp_desc *d, const float *s_true, int32_t *raw_count, kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (d->B == 0 || d->N == 0) return 0;
    if (!s_true || !raw_count) return KGE_EINVAL;
    if (KGE_LP_IS_MFMA(d->mode)) return kge_lp_gemm_run(d, nullptr, 0, s_true, raw_count, kge_s(stream));
    return kge_lp_direct_run(d, nullptr, 0, s_true, raw_count, kge_s(stream));
}

extern "C" int kge_lp_count_ge_cols(const kge_lp_desc *d, const float *s_true, int32_t *raw_count, const int64_t *rep,
                                    const int32_t *col_q, int64_t n_single_p, const int32_t *members, int64_t n_multi_p,
                                    kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (d->B == 0 || d->N == 0) return 0;
    return kge_lp_direct_count_cols(d, s_true, raw_count, rep, col_q, n_single_p, members, n_multi_p, kge_s(stream));
}

extern "C" int kge_rank_finalize(const int32_t *raw, const int32_t *sub, const int32_t *found, int64_t B,
                                 int64_t *rank, int64_t *filt_rank, kge_stream_t stream)
{
    if (B < 0) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!raw || !sub || !found || !rank || !filt_rank) return KGE_EINVAL;
    hipLaunchKernelGGL(rank_finalize_kernel, dim3(grid1d(B, 256)), dim3(256), 0, kge_s(stream), raw, sub, found, B,
                       rank, filt_rank);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_rank_finalize_both(const int32_t *raw, const int32_t *sub, const int32_t *found, int64_t B,
                                      int64_t *out, int64_t ld, int64_t off, const int64_t *pos, float *guard,
                                      float *flags, int zero_guard, int64_t *const *out_indirect, kge_stream_t stream)
{
    if (B < 0 || off < 0 || ld < off + B) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!raw || !sub || !found || (!out && !out_indirect) || (flags && !guard)) return KGE_EINVAL;
    hipLaunchKernelGGL(rank_finalize_both_kernel, dim3(grid1d(2 * B, 256)), dim3(256), 0, kge_s(stream), raw, sub,
                       found, B, out, ld, off, pos, guard, flags, (flags && zero_guard) ? 1 : 0, out_indirect);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_lp_scores_batched(int mode, const float *q, int64_t ldq, const float *cand,
                                     int64_t stride_b, int64_t stride_n, int64_t B, int64_t N, int K,
                                     float *out, int64_t ldo, kge_stream_t stream)
{
    if (mode != KGE_LP_DOT && mode != KGE_LP_L1_DIRECT && mode != KGE_LP_L2_DIRECT && mode != KGE_LP_TORUS_L1 &&
        mode != KGE_LP_TORUS_L2 && mode != KGE_LP_TORUS_EL2 && mode != KGE_LP_CMOD)
        return KGE_EINVAL;
    if (mode == KGE_LP_CMOD && (K & 1)) return KGE_EINVAL;
    if (B < 0 || N < 0 || K <= 0 || ldo < N) return KGE_EINVAL;
    if (B == 0 || N == 0) return 0;
    if (!q || !cand || !out) return KGE_EINVAL;
    hipLaunchKernelGGL(lp_batched_kernel, dim3(grid1d(B * N, 4)), dim3(256), 0, kge_s(stream), mode, q, ldq, cand,
                       stride_b, stride_n, B, N, K, out, ldo);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_abi_version(void) { return 33; }

__global__ __launch_bounds__(256) void copy_i64_indirect_kernel(const int64_t *__restrict__ src, int64_t n, int64_t *const *dst_ind)
{
    int64_t *dst = *dst_ind;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
}

/* dst[0 .. n) = src[0 .. n) with dst = *dst_indirect read on the device when the launch runs (see kge_rank_finalize_both's
 * out_indirect): the packed result of an evaluation whose finalize launches had to scatter (facts processed in another
 * order) leaves for pinned host memory as ONE coalesced pass at the end of the captured graph instead of a copy of its own. */
extern "C" int kge_copy_i64_indirect(const int64_t *src, int64_t n, int64_t *const *dst_indirect, kge_stream_t stream)
{
    if (n < 0 || (n > 0 && (!src || !dst_indirect))) return KGE_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(copy_i64_indirect_kernel, dim3(grid1d(n, 256)), dim3(256), 0, kge_s(stream), src, n, dst_indirect);
    KGE_CHECK_LAUNCH();
    return 0;
}

/* *dev = the device-visible address of pinned (hipHostMalloc / hipHostRegister) host memory -- what a kernel may be handed as
 * kge_rank_finalize_both's *out_indirect.  KGE_EINVAL when the memory is not mapped into the device's address space. */
extern "C" int kge_host_device_pointer(void *host, void **dev)
{
    if (!host || !dev) return KGE_EINVAL;
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess || !d) { (void)hipGetLastError(); return KGE_EINVAL; }
    *dev = d;
    return 0;
}
extern "C" const char *kge_build_arch(void) { return "gfx950"; }
