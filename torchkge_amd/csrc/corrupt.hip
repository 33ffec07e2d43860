// K5: the integer half of BernoulliNegativeSampler.corrupt_batch /
// UniformNegativeSampler.corrupt_batch (sampling.py:313-325, :206-221), gfx950.
//
//   neg_heads = heads.repeat(n_neg); neg_tails = tails.repeat(n_neg)
//   neg_heads[mask == 1] = draws_h      (k   values, consumed in position order)
//   neg_tails[mask == 0] = draws_t      (n-k values, consumed in position order)
//
// as a pure function of (heads, tails, mask, draws_h, draws_t): an exclusive
// prefix sum of the mask gives every position its index into the draw arrays.
// Three small HBM-bound launches (block counts, scan of counts, scatter); no
// device->host sync (the reference needs one for mask.sum().item()).
#include "mask_scan.h"

namespace {

__global__ __launch_bounds__(MS_CT) void corrupt_scatter_kernel(const int64_t *__restrict__ heads,
                                                                const int64_t *__restrict__ tails,
                                                                const uint8_t *__restrict__ mask,
                                                                const int64_t *__restrict__ draws_h,
                                                                const int64_t *__restrict__ draws_t, int64_t B,
                                                                int64_t n, const int32_t *__restrict__ block_base,
                                                                int64_t *neg_heads, int64_t *neg_tails)
{
    const int64_t base = (int64_t)blockIdx.x * MS_CB;
    int m[MS_CE];
    int ph = mask_thread_prefix(mask, n, block_base, m); // #ones before this thread's first element
#pragma unroll
    for (int e = 0; e < MS_CE; ++e) {
        const int64_t j = base + threadIdx.x * MS_CE + e;
        if (j < n) {
            const int64_t b = j % B;
            if (m[e]) { neg_heads[j] = draws_h[ph]; neg_tails[j] = tails[b]; }
            else      { neg_heads[j] = heads[b];    neg_tails[j] = draws_t[j - ph]; }
            ph += m[e];
        }
    }
}

} // namespace

extern "C" int64_t kge_corrupt_ws_elems(int64_t n) { return mask_scan_ws_elems(n); }

extern "C" int kge_corrupt_scatter(const int64_t *heads, const int64_t *tails, const uint8_t *mask,
                                   const int64_t *draws_h, const int64_t *draws_t, int64_t B, int64_t n_neg,
                                   int64_t *neg_heads, int64_t *neg_tails, int32_t *ws, kge_stream_t stream)
{
    if (B < 0 || n_neg < 1) return KGE_EINVAL;
    const int64_t n = B * n_neg;
    if (n == 0) return 0;
    if (!heads || !tails || !mask || !neg_heads || !neg_tails || !ws) return KGE_EINVAL;
    // draws_h / draws_t may legitimately be empty (all-zero / all-one mask)
    hipStream_t s = kge_s(stream);
    const int rc = mask_scan_launch(mask, n, ws, s);
    if (rc) return rc;
    hipLaunchKernelGGL(corrupt_scatter_kernel, dim3((unsigned)mask_scan_blocks(n)), dim3(MS_CT), 0, s, heads, tails, mask,
                       draws_h, draws_t, B, n, ws, neg_heads, neg_tails);
    KGE_CHECK_LAUNCH();
    return 0;
}
