// Exact scores of LISTED (query, candidate) pairs and the filter correction built on them (gfx950): kge_lp_pair_scores,
// kge_lp_filter_sub and its grouped / planned forms.  Every score is the bits of lp_pair_score (kge_common.h); which
// flavour of it a descriptor runs is decided in lp_pair_exact.h.
//   get_true_targets/filter_scores utils/modeling.py:53-102, the filter half of evaluation.py:290-300
#include "lp_pair_exact.h"

namespace {

// one lane per pair, 64 pairs per wavefront round (one wavefront per block; staged variants: rows staged cooperatively)
template <class V>
__global__ __launch_bounds__(64, 2) void pair_scores_kernel(const kge_lp_desc d, const int64_t *__restrict__ qi,
                                                         const int64_t *__restrict__ ci, int64_t P, float *out)
{
    KGE_PAIR_LDS(V);
    const int lane = threadIdx.x;
    const int64_t ngroups = (P + 63) >> 6;
    for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int64_t p = grp * 64 + lane;
        int64_t i = 0, c = -1;
        if (p < P) { i = qi ? qi[p] : p; c = ci[p] - d.c_base; }
        const bool ok = p < P && c >= 0 && c < d.N;
        const float sc = V::score(d, ok, i, c, qs, es);
        if (p < P) out[p] = ok ? sc : 0.f;
    }
}

// 8 lanes per query (8 queries per wavefront); the lanes of a group stride over
// the query's filter segment and score each listed candidate with the same
// arithmetic as the tile kernels.  Most segments hold a handful of entities.
__global__ __launch_bounds__(256) void filter_sub_kernel(const kge_lp_desc d, const float *__restrict__ s_true,
                                                         const int64_t *__restrict__ true_idx,
                                                         const int64_t *__restrict__ seg_lo,
                                                         const int64_t *__restrict__ seg_hi,
                                                         const int32_t *__restrict__ targets,
                                                         int32_t *sub_out, int32_t *found_out)
{
    constexpr int LPQ = 8;
    const int sub_lane = threadIdx.x & (LPQ - 1);
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPQ;
    const int64_t ngroups = (int64_t)gridDim.x * 256 / LPQ;
    const int64_t rounds = (d.B + ngroups - 1) / ngroups;   // uniform trip count: shuffles need all lanes
    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t i = group + rd * ngroups;
        int sub = 0, found = 0;
        if (i < d.B) {
            const float tv = s_true[i];
            const int64_t ti = true_idx[i];
            const int neg_inf_counts = (-INFINITY >= tv) ? 1 : 0;
            for (int64_t j = seg_lo[i] + sub_lane; j < seg_hi[i]; j += LPQ) {
                const int64_t cg = targets[j];
                const int64_t c = cg - d.c_base;
                if (c < 0 || c >= d.N) continue;
                if (cg == ti) { found = 1; continue; }
                sub += ((lp_pair_score(d, i, c) >= tv) ? 1 : 0) - neg_inf_counts;
            }
        }
#pragma unroll
        for (int o = LPQ / 2; o > 0; o >>= 1) {
            sub += __shfl_xor(sub, o, 64);
            found += __shfl_xor(found, o, 64);
        }
        if (i < d.B && sub_lane == 0) { sub_out[i] = sub; found_out[i] = found ? 1 : 0; }
    }
}

// MFMA modes: the same 8-lanes-per-query walk, but every round's 64 (query, candidate)
// pairs are scored through the cooperative row staging (one wavefront per block)
template <class V>
__global__ __launch_bounds__(64, 2) void filter_sub_staged_kernel(const kge_lp_desc d, const float *__restrict__ s_true,
                                                               const int64_t *__restrict__ true_idx,
                                                               const int64_t *__restrict__ seg_lo,
                                                               const int64_t *__restrict__ seg_hi,
                                                               const int32_t *__restrict__ targets,
                                                               int32_t *sub_out, int32_t *found_out)
{
    constexpr int LPQ = 8;
    KGE_PAIR_LDS(V);
    const int lane = threadIdx.x, sub_lane = lane & (LPQ - 1);
    const int64_t nq = (d.B + 7) >> 3;                 // groups of 8 queries
    for (int64_t qg = blockIdx.x; qg < nq; qg += gridDim.x) {
        const int64_t i = qg * 8 + (lane >> 3);
        const bool live = i < d.B;
        int sub = 0, found = 0;
        const float tv = live ? s_true[i] : 0.f;
        const int64_t ti = live ? true_idx[i] : -1;
        const int64_t lo = live ? seg_lo[i] : 0, hi = live ? seg_hi[i] : 0;
        const int neg_inf_counts = (-INFINITY >= tv) ? 1 : 0;
        int len = (int)(hi - lo);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_xor(len, o, 64));
        for (int j0 = 0; j0 < len; j0 += LPQ) {        // wave-uniform trip count
            const int64_t j = lo + j0 + sub_lane;
            bool score = false;
            int64_t c = 0;
            if (j < hi) {
                const int64_t cg = targets[j];
                c = cg - d.c_base;
                if (c >= 0 && c < d.N) {
                    if (cg == ti) found = 1;
                    else score = true;
                }
            }
            if (__ballot(score) == 0ull) continue;      // this round lists only true entities / other shards' candidates
            const float sc = V::score(d, score, i, c, qs, es);
            if (score) sub += ((sc >= tv) ? 1 : 0) - neg_inf_counts;
        }
#pragma unroll
        for (int o = LPQ / 2; o > 0; o >>= 1) {
            sub += __shfl_xor(sub, o, 64);
            found += __shfl_xor(found, o, 64);
        }
        if (live && sub_lane == 0) { sub_out[i] = sub; found_out[i] = found ? 1 : 0; }
    }
}

// ---- filter correction, grouped and flattened (kge_lp_filter_sub_grouped) ----------------------
// Real link-prediction test splits are heavy-tailed: many queries share a key -- (h, r) on the tail
// side, (t, r) on the head side -- and a hub key's filter list holds thousands of entities (FB15k-237:
// gender / nationality / profession).  A key fixes BOTH the filter list and the query row, so the
// exact scores of a list are the same for every query of that key.  Instead of walking each query's
// list (8 lanes per query, the wavefront looping to its longest list: the r01 kernel), the lists the
// batch touches are scored ONCE per key into fs[] (indexed like targets[]), all (key, target) pairs
// flattened over the whole grid, and every query then only COMPARES its true score with its list's
// scores.  Work is bounded by the size of the target array, whatever the skew.
//   claim[T]  : smallest query index whose segment starts at that target position (0xffffffff: none)
//   woff[B+1] : exclusive prefix sum of the claimed segments' lengths (the flattened work list)
// (only the entries the batch touches are reset: O(B), not O(n_targets), and no memset node in a captured graph)
__global__ void fsub_reset_kernel(const int64_t *__restrict__ seg_lo, const int64_t *__restrict__ seg_hi, int64_t B,
                                  unsigned *claim)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x)
        if (seg_hi[i] > seg_lo[i]) claim[seg_lo[i]] = 0xffffffffu;
}
__global__ void fsub_claim_kernel(const int64_t *__restrict__ seg_lo, const int64_t *__restrict__ seg_hi, int64_t B,
                                  unsigned *claim)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x)
        if (seg_hi[i] > seg_lo[i]) atomicMin(&claim[seg_lo[i]], (unsigned)i);
}

// exclusive prefix sum of the claimed segments' lengths, reduce-then-scan over blocks of FS_SCAN_T queries:
//   fsub_len_kernel   len[i] (0 for queries that are not their segment's leader) + one sum per block
//   fsub_bscan_kernel exclusive scan of the block sums (one block; any number of block sums)
//   fsub_off_kernel   woff[i] = block base + exclusive scan inside the block;  woff[B] = total
constexpr int FS_SCAN_T = 1024;
__device__ __forceinline__ int64_t fsub_shfl_up64(int64_t v, int o)
{
    const unsigned vlo = __shfl_up((unsigned)(v & 0xffffffffll), o, 64);
    const unsigned vhi = __shfl_up((unsigned)((uint64_t)v >> 32), o, 64);
    return (int64_t)(((uint64_t)vhi << 32) | vlo);
}
// inclusive scan of one value per thread over a block of FS_SCAN_T threads; returns (inclusive, block total)
__device__ __forceinline__ int64_t fsub_block_scan(int64_t v, int64_t *wsum, int64_t &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t u = fsub_shfl_up64(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int64_t before = 0, tot = 0;
    for (int w = 0; w < FS_SCAN_T / 64; ++w) {
        const int64_t x = wsum[w];
        if (w < wv) before += x;
        tot += x;
    }
    total = tot;
    return before + inc;
}
__global__ __launch_bounds__(FS_SCAN_T) void fsub_len_kernel(const int64_t *__restrict__ seg_lo,
                                                             const int64_t *__restrict__ seg_hi, int64_t B,
                                                             const unsigned *__restrict__ claim, int64_t *woff,
                                                             int64_t *bsum)
{
    __shared__ int64_t wsum[FS_SCAN_T / 64];
    const int64_t i = (int64_t)blockIdx.x * FS_SCAN_T + threadIdx.x;
    int64_t l = 0;
    if (i < B) {
        const int64_t lo = seg_lo[i], hi = seg_hi[i];
        if (hi > lo && claim[lo] == (unsigned)i) l = hi - lo;
        woff[i] = l;     // (turned into the offset by fsub_off_kernel)
    }
    int64_t total;
    fsub_block_scan(l, wsum, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
__global__ __launch_bounds__(FS_SCAN_T) void fsub_bscan_kernel(int64_t *bsum, int64_t nb, int64_t *woff_total)
{
    __shared__ int64_t wsum[FS_SCAN_T / 64];
    int64_t carry = 0;
    for (int64_t base = 0; base < nb; base += FS_SCAN_T) {
        const int64_t b = base + threadIdx.x;
        const int64_t v = b < nb ? bsum[b] : 0;
        int64_t total;
        const int64_t inc = fsub_block_scan(v, wsum, total);
        if (b < nb) bsum[b] = carry + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *woff_total = carry;
}
__global__ __launch_bounds__(FS_SCAN_T) void fsub_off_kernel(int64_t B, int64_t *woff, const int64_t *__restrict__ bsum)
{
    __shared__ int64_t wsum[FS_SCAN_T / 64];
    const int64_t i = (int64_t)blockIdx.x * FS_SCAN_T + threadIdx.x;
    const int64_t l = i < B ? woff[i] : 0;
    int64_t total;
    const int64_t inc = fsub_block_scan(l, wsum, total);
    if (i < B) woff[i] = bsum[blockIdx.x] + inc - l;
}

// scores of the flattened (claimed key, target) pairs: one lane per pair, 64 pairs per wavefront round
template <class V>
__global__ __launch_bounds__(64, 2) void fsub_score_kernel(const kge_lp_desc d, const int64_t *__restrict__ seg_lo,
                                                        const int32_t *__restrict__ targets,
                                                        const int64_t *__restrict__ woff, float *fs)
{
    KGE_PAIR_LDS(V);
    const int lane = threadIdx.x;
    const int64_t W = woff[d.B];
    for (int64_t w0 = (int64_t)blockIdx.x * 64; w0 < W; w0 += (int64_t)gridDim.x * 64) {
        const int64_t w = w0 + lane;
        const bool valid = w < W;
        int64_t lo = 0, hi = d.B; // first index with woff[idx] > w, minus one (zero-length entries are skipped)
        if (valid) {
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (woff[mid + 1] <= w) lo = mid + 1; else hi = mid;
            }
        }
        const int64_t i = lo;
        int64_t j = 0, c = -1;
        if (valid) {
            j = seg_lo[i] + (w - woff[i]);
            c = (int64_t)targets[j] - d.c_base;
        }
        const bool ok = valid && c >= 0 && c < d.N;
        const float sc = V::score(d, ok, i, c, qs, es);
        if (ok) fs[j] = sc;
    }
}

// Comparison of every query's true score with the scores of its list.  Lists of up to FS_SHORT entries: one
// wavefront per query, 8 independent loads per lane in flight (a hub list walked 64 entries per dependent
// round was ~1 us per round).  Longer lists (hub keys: thousands of entities, shared by hundreds of queries):
// `long_q` names those queries and one 256-thread BLOCK takes each; without it the wavefront loops.
constexpr int FS_SHORT = 512;
__device__ __forceinline__ void fsub_cmp(const kge_lp_desc &d, const int32_t *__restrict__ targets,
                                         const float *__restrict__ fs, int64_t j, int64_t hi, int64_t ti, float tv,
                                         int neg_inf_counts, int &sub, int &found)
{
    if (j >= hi) return;
    const int64_t cg = targets[j];
    const int64_t c = cg - d.c_base;
    if (c < 0 || c >= d.N) return;
    if (cg == ti) { found = 1; return; }
    sub += ((fs[j] >= tv) ? 1 : 0) - neg_inf_counts;
}
// the two compare kernels of the filter correction: short lists (a wavefront per query) and hub lists (a block per
// query); bodies as device functions so that ONE launch can run both side by side (fsub_count_both_kernel)
__device__ __forceinline__ void fsub_count_short(const kge_lp_desc &d, const float *__restrict__ s_true,
                                                 const int64_t *__restrict__ true_idx, const int64_t *__restrict__ seg_lo,
                                                 const int64_t *__restrict__ seg_hi, const int32_t *__restrict__ targets,
                                                 const float *__restrict__ fs, int skip_long, int32_t *sub_out,
                                                 int32_t *found_out, int bid, int nblk)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)bid * 4 + (threadIdx.x >> 6), nwaves = (int64_t)nblk * 4;
    for (int64_t i = wave; i < d.B; i += nwaves) {
        const int64_t lo = seg_lo[i], hi = seg_hi[i];
        if (skip_long && hi - lo > FS_SHORT) continue;      // the hub-list body writes this query
        int sub = 0, found = 0;
        if (hi > lo) {
            const float tv = s_true[i];
            const int64_t ti = true_idx[i];
            const int neg_inf_counts = (-INFINITY >= tv) ? 1 : 0;
            for (int64_t j0 = lo; j0 < hi; j0 += FS_SHORT) {
#pragma unroll
                for (int u = 0; u < FS_SHORT / 64; ++u)
                    fsub_cmp(d, targets, fs, j0 + u * 64 + lane, hi, ti, tv, neg_inf_counts, sub, found);
            }
            sub = wave_sum_i(sub);
            found = wave_sum_i(found);
        }
        if (lane == 0) { sub_out[i] = sub; found_out[i] = found ? 1 : 0; }
    }
}
__device__ __forceinline__ void fsub_count_long(const kge_lp_desc &d, const float *__restrict__ s_true,
                                                const int64_t *__restrict__ true_idx, const int64_t *__restrict__ seg_lo,
                                                const int64_t *__restrict__ seg_hi, const int32_t *__restrict__ targets,
                                                const float *__restrict__ fs, const int64_t *__restrict__ long_q,
                                                int64_t n_long, int32_t *sub_out, int32_t *found_out, int bid, int nblk,
                                                int *sh)
{
    for (int64_t q = bid; q < n_long; q += nblk) {
        const int64_t i = long_q[q];
        const int64_t lo = seg_lo[i], hi = seg_hi[i];
        const float tv = s_true[i];
        const int64_t ti = true_idx[i];
        const int neg_inf_counts = (-INFINITY >= tv) ? 1 : 0;
        int sub = 0, found = 0;
        for (int64_t j0 = lo; j0 < hi; j0 += 1024) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                fsub_cmp(d, targets, fs, j0 + u * 256 + threadIdx.x, hi, ti, tv, neg_inf_counts, sub, found);
        }
        sub = block_sum_i(sub, sh);
        found = block_sum_i(found, sh);
        if (threadIdx.x == 0) { sub_out[i] = sub; found_out[i] = found ? 1 : 0; }
    }
}
__global__ __launch_bounds__(256) void fsub_count_kernel(const kge_lp_desc d, const float *__restrict__ s_true,
                                                         const int64_t *__restrict__ true_idx,
                                                         const int64_t *__restrict__ seg_lo,
                                                         const int64_t *__restrict__ seg_hi,
                                                         const int32_t *__restrict__ targets,
                                                         const float *__restrict__ fs, int skip_long,
                                                         int32_t *sub_out, int32_t *found_out)
{
    fsub_count_short(d, s_true, true_idx, seg_lo, seg_hi, targets, fs, skip_long, sub_out, found_out, blockIdx.x, gridDim.x);
}
// ONE launch for both: the first gridDim.x - short_blocks blocks run the hub-list body, the rest the short-list body (they write disjoint
// queries) -- the two kernels were 17 + 17 us back to back, each far from filling the GPU
__global__ __launch_bounds__(256) void fsub_count_both_kernel(const kge_lp_desc d, const float *__restrict__ s_true,
                                                              const int64_t *__restrict__ true_idx,
                                                              const int64_t *__restrict__ seg_lo,
                                                              const int64_t *__restrict__ seg_hi,
                                                              const int32_t *__restrict__ targets,
                                                              const float *__restrict__ fs,
                                                              const int64_t *__restrict__ long_q, int64_t n_long,
                                                              int short_blocks, int32_t *sub_out, int32_t *found_out)
{
    __shared__ int sh[4];
    const int long_blocks = (int)gridDim.x - short_blocks;     // the hub-list blocks come FIRST: they are the long ones
    if ((int)blockIdx.x < long_blocks)
        fsub_count_long(d, s_true, true_idx, seg_lo, seg_hi, targets, fs, long_q, n_long, sub_out, found_out,
                        (int)blockIdx.x, long_blocks, sh);
    else
        fsub_count_short(d, s_true, true_idx, seg_lo, seg_hi, targets, fs, 1, sub_out, found_out,
                         (int)blockIdx.x - long_blocks, short_blocks);
}

} // namespace

extern "C" int kge_lp_pair_scores(const kge_lp_desc *d, const int64_t *qi, const int64_t *ci, int64_t P,
                                  float *out, kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (P < 0) return KGE_EINVAL;
    if (P == 0) return 0;
    if (!ci || !out) return KGE_EINVAL;
    return lp_pair_dispatch<PAIR_DEFAULT>(*d, [&](auto v) {
        hipLaunchKernelGGL(pair_scores_kernel<decltype(v)>, dim3(lp_pair_grid(P)), dim3(64), 0, kge_s(stream), *d, qi, ci, P, out);
        KGE_CHECK_LAUNCH();
        return 0;
    });
}

extern "C" int kge_lp_filter_sub(const kge_lp_desc *d, const float *s_true, const int64_t *true_idx,
                                 const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *targets,
                                 int32_t *sub, int32_t *found, kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (d->B == 0) return 0;
    if (!s_true || !true_idx || !seg_lo || !seg_hi || !sub || !found) return KGE_EINVAL;
    return lp_pair_dispatch<PAIR_MFMA_ELSE_SCALAR>(*d, [&](auto v) {
        using V = decltype(v);
        if constexpr (V::staged)        // 8 lanes per query: a wavefront per 8 queries
            hipLaunchKernelGGL(filter_sub_staged_kernel<V>, dim3(lp_pair_grid(d->B * 8)), dim3(64), 0, kge_s(stream), *d, s_true,
                               true_idx, seg_lo, seg_hi, targets, sub, found);
        else
            hipLaunchKernelGGL(filter_sub_kernel, dim3(grid1d(d->B, 32)), dim3(256), 0, kge_s(stream), *d, s_true, true_idx,
                               seg_lo, seg_hi, targets, sub, found);
        KGE_CHECK_LAUNCH();
        return 0;
    });
}

static inline int64_t fsub_align(int64_t x) { return (x + 255) & ~(int64_t)255; }
static inline int64_t fsub_nblocks(int64_t B) { return (B + FS_SCAN_T - 1) / FS_SCAN_T; }

extern "C" int64_t kge_lp_filter_sub_ws_bytes(int64_t B, int64_t n_targets)
{
    if (B < 0 || n_targets < 0) return 0;
    return fsub_align(n_targets * 4) * 2 + fsub_align((B + 1) * 8) + fsub_align((fsub_nblocks(B) + 1) * 8);
}

// scoring of the flattened work list + the per-query comparison (shared by the two entry points below)
static int fsub_score_and_count(const kge_lp_desc *d, const float *s_true, const int64_t *true_idx,
                                const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *targets, int64_t n_pairs_max,
                                const int64_t *woff, const int64_t *long_q, int64_t n_long, float *fs, int32_t *sub,
                                int32_t *found, hipStream_t st)
{
    if (n_pairs_max > 0 && d->N > 0) {      // n_pairs_max: upper bound of the flattened work (the exact total is read on the device)
        lp_pair_dispatch<PAIR_DEFAULT>(*d, [&](auto v) {
            hipLaunchKernelGGL(fsub_score_kernel<decltype(v)>, dim3(lp_pair_grid(n_pairs_max)), dim3(64), 0, st, *d, seg_lo, targets,
                               woff, fs);
            return 0;
        });
    }
    if (long_q && n_long > 0) {
        const int sb = grid1d(d->B, 4), lb = (int)(n_long < 256 * 16 ? n_long : 256 * 16);
        hipLaunchKernelGGL(fsub_count_both_kernel, dim3(sb + lb), dim3(256), 0, st, *d, s_true, true_idx, seg_lo, seg_hi,
                           targets, fs, long_q, n_long, sb, sub, found);
    } else {
        hipLaunchKernelGGL(fsub_count_kernel, dim3(grid1d(d->B, 4)), dim3(256), 0, st, *d, s_true, true_idx, seg_lo, seg_hi,
                           targets, fs, long_q ? 1 : 0, sub, found);
    }
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_lp_filter_sub_grouped(const kge_lp_desc *d, const float *s_true, const int64_t *true_idx,
                                         const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *targets,
                                         int64_t n_targets, int32_t *sub, int32_t *found, void *ws, int64_t ws_bytes,
                                         kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (d->B == 0) return 0;
    if (!s_true || !true_idx || !seg_lo || !seg_hi || !sub || !found || n_targets < 0) return KGE_EINVAL;
    if (n_targets > 0 && (!targets || !ws || ws_bytes < kge_lp_filter_sub_ws_bytes(d->B, n_targets))) return KGE_EINVAL;
    if (d->B > INT32_MAX || d->N > INT32_MAX) return KGE_EINVAL;
    hipStream_t st = kge_s(stream);
    char *w8 = static_cast<char *>(ws);
    unsigned *claim = reinterpret_cast<unsigned *>(w8);
    float *fs = reinterpret_cast<float *>(w8 + fsub_align(n_targets * 4));
    int64_t *woff = reinterpret_cast<int64_t *>(w8 + 2 * fsub_align(n_targets * 4));
    int64_t *bsum = reinterpret_cast<int64_t *>(w8 + 2 * fsub_align(n_targets * 4) + fsub_align((d->B + 1) * 8));
    if (n_targets > 0 && d->N > 0) {
        const int nb = (int)fsub_nblocks(d->B);
        hipLaunchKernelGGL(fsub_reset_kernel, dim3(grid1d(d->B, 256)), dim3(256), 0, st, seg_lo, seg_hi, d->B, claim);
        hipLaunchKernelGGL(fsub_claim_kernel, dim3(grid1d(d->B, 256)), dim3(256), 0, st, seg_lo, seg_hi, d->B, claim);
        hipLaunchKernelGGL(fsub_len_kernel, dim3(nb), dim3(FS_SCAN_T), 0, st, seg_lo, seg_hi, d->B, claim, woff, bsum);
        hipLaunchKernelGGL(fsub_bscan_kernel, dim3(1), dim3(FS_SCAN_T), 0, st, bsum, (int64_t)nb, woff + d->B);
        hipLaunchKernelGGL(fsub_off_kernel, dim3(nb), dim3(FS_SCAN_T), 0, st, d->B, woff, bsum);
    }
    return fsub_score_and_count(d, s_true, true_idx, seg_lo, seg_hi, targets, n_targets, woff, nullptr, 0, fs, sub, found, st);
}

extern "C" int kge_lp_filter_sub_planned(const kge_lp_desc *d, const float *s_true, const int64_t *true_idx,
                                         const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *targets,
                                         int64_t n_targets, const int64_t *woff, int64_t n_pairs,
                                         const int64_t *long_q, int64_t n_long, float *fs, int32_t *sub, int32_t *found,
                                         kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (d->B == 0) return 0;
    if (!s_true || !true_idx || !seg_lo || !seg_hi || !sub || !found || !woff || n_targets < 0 || n_pairs < 0 || n_long < 0)
        return KGE_EINVAL;
    if (n_targets > 0 && (!targets || !fs)) return KGE_EINVAL;
    if (n_long > 0 && !long_q) return KGE_EINVAL;
    if (d->B > INT32_MAX || d->N > INT32_MAX) return KGE_EINVAL;
    return fsub_score_and_count(d, s_true, true_idx, seg_lo, seg_hi, targets, n_pairs, woff, long_q, n_long, fs, sub, found,
                                kge_s(stream));
}
