// The integer half of BernoulliRelationNegativeSampler.corrupt_batch (sampling.py:526-553), gfx950
// (include/kge_hip_relation.h):
//
//   neg_rels [mask_ent == 0]                 = draws_r      (consumed in position order)
//   neg_heads[mask_ent == 1 & mask_head == 1] = draws_h     (mask_head is compact: one byte per entity position)
//   neg_tails[mask_ent == 1 & mask_head == 0] = draws_t
//
// Two DEPENDENT prefix counts (mask_scan.h for both): p = #entity positions before j indexes mask_head, and only then
// is the byte known whose prefix count q indexes draws_h.  So:
//
//   count + scan of mask_ent                     block bases A
//   relation_derive_kernel                       d[j] = mask_ent[j] && mask_head[p_j]   (a byte mask in the workspace)
//   count + scan of d                            block bases B
//   relation_scatter_kernel                      p from A, q from B, the three outputs
//
// Five small HBM-latency-bound launches besides the scatter; no atomic, no device->host read (the reference needs two).
#include "mask_scan.h"
#include "../../include/kge_hip_relation.h"

namespace {

__global__ __launch_bounds__(MS_CT) void relation_derive_kernel(const uint8_t *__restrict__ mask_ent,
                                                                const uint8_t *__restrict__ mask_head, int64_t n,
                                                                const int32_t *__restrict__ base_ent, uint8_t *derived)
{
    const int64_t base = (int64_t)blockIdx.x * MS_CB;
    int m[MS_CE];
    int p = mask_thread_prefix(mask_ent, n, base_ent, m);     // #entity positions before this thread's first position
#pragma unroll
    for (int e = 0; e < MS_CE; ++e) {
        const int64_t j = base + threadIdx.x * MS_CE + e;
        if (j < n) {
            derived[j] = (m[e] && mask_head) ? (mask_head[p] != 0) : 0;
            p += m[e];
        }
    }
}

__global__ __launch_bounds__(MS_CT) void relation_scatter_kernel(
    const int64_t *__restrict__ heads, const int64_t *__restrict__ tails, const int64_t *__restrict__ rels,
    const uint8_t *__restrict__ mask_ent, const uint8_t *__restrict__ derived, const int64_t *__restrict__ draws_r,
    const int64_t *__restrict__ draws_h, const int64_t *__restrict__ draws_t, int64_t B, int64_t n,
    const int32_t *__restrict__ base_ent, const int32_t *__restrict__ base_head, int64_t *neg_heads, int64_t *neg_tails,
    int64_t *neg_rels)
{
    const int64_t base = (int64_t)blockIdx.x * MS_CB;
    int me[MS_CE], mh[MS_CE];
    int p = mask_thread_prefix(mask_ent, n, base_ent, me);    // #entity positions before this thread's first position
    __syncthreads();                                          // (the two calls share one LDS array)
    int q = mask_thread_prefix(derived, n, base_head, mh);    // #head positions before it
#pragma unroll
    for (int e = 0; e < MS_CE; ++e) {
        const int64_t j = base + threadIdx.x * MS_CE + e;
        if (j < n) {
            const int64_t b = j % B;
            int64_t h = heads[b], t = tails[b], r = rels[b];
            if (!me[e]) { if (draws_r) r = draws_r[j - p]; }
            else if (mh[e]) { if (draws_h) h = draws_h[q]; }
            else { if (draws_t) t = draws_t[p - q]; }
            neg_heads[j] = h;
            neg_tails[j] = t;
            neg_rels[j] = r;
            p += me[e];
            q += mh[e];
        }
    }
}

// workspace: [bases of mask_ent | bases of the derived mask | the derived mask, n bytes]
inline int64_t rc_derived_off(int64_t n) { return 2 * mask_scan_ws_elems(n); }

} // namespace

extern "C" int64_t kge_relation_corrupt_ws_elems(int64_t n) { return n > 0 ? rc_derived_off(n) + (n + 3) / 4 : 0; }

extern "C" int kge_relation_corrupt(const int64_t *heads, const int64_t *tails, const int64_t *rels, const uint8_t *mask_ent,
                                    const uint8_t *mask_head, const int64_t *draws_r, const int64_t *draws_h,
                                    const int64_t *draws_t, int64_t B, int64_t n_neg, int64_t *neg_heads, int64_t *neg_tails,
                                    int64_t *neg_rels, int32_t *ws, kge_stream_t stream)
{
    if (B < 0 || n_neg < 1) return KGE_EINVAL;
    if (B == 0) return 0;
    if (n_neg > INT32_MAX / B) return KGE_EINVAL;       // the prefix counts are int32
    const int64_t n = B * n_neg;
    if (!heads || !tails || !rels || !mask_ent || !neg_heads || !neg_tails || !neg_rels || !ws) return KGE_EINVAL;
    // mask_head / draws_* may legitimately be empty (all-zero / all-one masks): dereferenced only where their branch is taken
    hipStream_t s = kge_s(stream);
    int32_t *base_ent = ws, *base_head = ws + mask_scan_ws_elems(n);
    uint8_t *derived = reinterpret_cast<uint8_t *>(ws + rc_derived_off(n));
    const dim3 grid((unsigned)mask_scan_blocks(n));
    int rc = mask_scan_launch(mask_ent, n, base_ent, s);
    if (rc) return rc;
    hipLaunchKernelGGL(relation_derive_kernel, grid, dim3(MS_CT), 0, s, mask_ent, mask_head, n, base_ent, derived);
    KGE_CHECK_LAUNCH();
    rc = mask_scan_launch(derived, n, base_head, s);
    if (rc) return rc;
    hipLaunchKernelGGL(relation_scatter_kernel, grid, dim3(MS_CT), 0, s, heads, tails, rels, mask_ent, derived, draws_r,
                       draws_h, draws_t, B, n, base_ent, base_head, neg_heads, neg_tails, neg_rels);
    KGE_CHECK_LAUNCH();
    return 0;
}
