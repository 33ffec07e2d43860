// Filtered negative sampling, gfx950 (include/kge_hip_filtered.h): the replacement of a fact's head or tail drawn exactly
// over the entities that are neither a known answer of the fact's key nor the replaced entity, and the known-fact
// diagnostic.
//
//   filtered_corrupt_kernel    one thread per position p = k * B + i: the list of the replaced side, a membership search
//                              of the replaced entity x, the draw reduced modulo the number c of free entities, the rank
//                              of x skipped when x is not in the list, and the v-th entity of the list's complement by
//                              one search over the non-decreasing L[j] - j
//   triples_known_kernel       one thread per triple: a key search, then a search of the key's segment
//
// A thread per position, not a wavefront per fact: neighbouring lanes read neighbouring facts, bounds, masks and draws
// and write neighbouring outputs, every lane works whatever n_neg is (a wavefront per fact idles 64 - n_neg lanes below
// 64 negatives), and the searches of the lanes of a wavefront diverge per draw in either geometry.  The four bounds of a
// fact are re-read by its n_neg positions from L2.  Integer work only: no float operation, no atomic, ordinary vector
// stores.
#include "kge_common.h"
#include "../../include/kge_hip_filtered.h"

namespace {

constexpr int FC_THREADS = 256;

// the number of entries of the ascending L[0 .. m) below x
__device__ __forceinline__ int64_t fc_rank(const int32_t *__restrict__ L, int64_t m, int64_t x)
{
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)L[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the number of entries with L[j] - j <= v (L ascending and distinct: L[j] - j is non-decreasing)
__device__ __forceinline__ int64_t fc_skipped(const int32_t *__restrict__ L, int64_t m, int64_t v)
{
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)L[mid] - mid <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(FC_THREADS) void filtered_corrupt_kernel(
    const int64_t *__restrict__ h, const int64_t *__restrict__ t, int64_t B, int64_t n, const uint8_t *__restrict__ mask,
    const int64_t *__restrict__ draws, const int64_t *__restrict__ tail_lo, const int64_t *__restrict__ tail_hi,
    const int32_t *__restrict__ tail_targets, const int64_t *__restrict__ head_lo, const int64_t *__restrict__ head_hi,
    const int32_t *__restrict__ head_targets, int64_t n_ent, int64_t *__restrict__ neg_h, int64_t *__restrict__ neg_t,
    uint8_t *__restrict__ exhausted)
{
    for (int64_t p = (int64_t)blockIdx.x * FC_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * FC_THREADS) {
        const int64_t i = p % B;
        const bool head = mask[p] != 0;
        const int64_t hi_ = h[i], ti_ = t[i];
        const int64_t x = head ? hi_ : ti_;
        const int64_t s_lo = head ? head_lo[i] : tail_lo[i], s_hi = head ? head_hi[i] : tail_hi[i];
        const int32_t *L = (head ? head_targets : tail_targets) + s_lo;
        const int64_t m = s_hi > s_lo ? s_hi - s_lo : 0;
        const int64_t below = fc_rank(L, m, x);                 // #{l in L : l < x}
        const bool in = below < m && (int64_t)L[below] == x;
        const int64_t c = n_ent - m - (in ? 0 : 1);
        int64_t e = x;
        if (c > 0) {
            int64_t v = (int64_t)((uint64_t)draws[p] % (uint64_t)c);
            if (!in) v += (v >= x - below);
            e = v + fc_skipped(L, m, v);
        }
        neg_h[p] = head ? e : hi_;
        neg_t[p] = head ? ti_ : e;
        if (exhausted) exhausted[p] = c > 0 ? 0 : 1;
    }
}

__global__ __launch_bounds__(FC_THREADS) void triples_known_kernel(
    const int64_t *__restrict__ keys, int64_t n_keys, const int64_t *__restrict__ offsets,
    const int32_t *__restrict__ targets, int64_t key_span, const int64_t *__restrict__ key1,
    const int64_t *__restrict__ key2, const int64_t *__restrict__ value, int64_t n, uint8_t *__restrict__ out)
{
    for (int64_t p = (int64_t)blockIdx.x * FC_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * FC_THREADS) {
        // (unsigned arithmetic: an id outside the index's range wraps instead of overflowing, and is then simply absent)
        const int64_t key = (int64_t)((uint64_t)key1[p] * (uint64_t)key_span + (uint64_t)key2[p]);
        int64_t lo = 0, hi = n_keys;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        uint8_t found = 0;
        if (lo < n_keys && keys[lo] == key) {
            const int64_t s_lo = offsets[lo], s_hi = offsets[lo + 1];
            const int64_t m = s_hi > s_lo ? s_hi - s_lo : 0, x = value[p];
            const int64_t at = fc_rank(targets + s_lo, m, x);
            found = at < m && (int64_t)targets[s_lo + at] == x;
        }
        out[p] = found;
    }
}

} // namespace

extern "C" int kge_filtered_corrupt(const int64_t *h, const int64_t *t, int64_t B, int64_t n_neg, const uint8_t *mask,
                                    const int64_t *draws, const int64_t *tail_lo, const int64_t *tail_hi,
                                    const int32_t *tail_targets, const int64_t *head_lo, const int64_t *head_hi,
                                    const int32_t *head_targets, int64_t n_ent, int64_t *neg_h, int64_t *neg_t,
                                    uint8_t *exhausted, kge_stream_t stream)
{
    if (B < 0 || n_ent < 1 || n_ent > INT32_MAX) return KGE_EINVAL;
    if (B == 0) return 0;
    if (n_neg < 1 || n_neg > INT32_MAX / B) return KGE_EINVAL;      // B * n_neg < 2^31
    if (!h || !t || !mask || !draws || !tail_lo || !tail_hi || !tail_targets || !head_lo || !head_hi || !head_targets ||
        !neg_h || !neg_t)
        return KGE_EINVAL;
    const int64_t n = B * n_neg;
    hipLaunchKernelGGL(filtered_corrupt_kernel, dim3(grid1d(n, FC_THREADS)), dim3(FC_THREADS), 0, kge_s(stream), h, t, B, n,
                       mask, draws, tail_lo, tail_hi, tail_targets, head_lo, head_hi, head_targets, n_ent, neg_h, neg_t,
                       exhausted);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_triples_known(const int64_t *keys, int64_t n_keys, const int64_t *offsets, const int32_t *targets,
                                 int64_t key_span, const int64_t *key1, const int64_t *key2, const int64_t *value,
                                 int64_t n, uint8_t *out, kge_stream_t stream)
{
    if (n < 0 || n > INT32_MAX || n_keys < 0 || key_span < 1) return KGE_EINVAL;
    if (n == 0) return 0;
    if (!key1 || !key2 || !value || !out || (n_keys > 0 && (!keys || !offsets || !targets))) return KGE_EINVAL;
    hipLaunchKernelGGL(triples_known_kernel, dim3(grid1d(n, FC_THREADS)), dim3(FC_THREADS), 0, kge_s(stream), keys, n_keys,
                       offsets, targets, key_span, key1, key2, value, n, out);
    KGE_CHECK_LAUNCH();
    return 0;
}
