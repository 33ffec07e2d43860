// Triplet classification (include/kge_hip_triplet.h), gfx950: the integer half of
// PositionalNegativeSampler.corrupt_batch (sampling.py:428-504) and the two reductions of
// TripletClassificationEvaluator (evaluation.py:513-580).
//
//   kge_positional_corrupt   mask prefix count (mask_scan.h) + one gather / scatter kernel
//   kge_relation_max         per-relation maximum through an order-preserving integer code: LDS table per
//                            workgroup, then integer atomic max -- no float atomics, schedule-independent bits
//   kge_threshold_count      the two strict compares against thr[rels[j]], one integer atomic add per workgroup
//
// All three are HBM-latency bound at evaluation sizes (1e4 .. 1e5 elements); none holds a floating-point sum.
#include "mask_scan.h"
#include "../../include/kge_hip_triplet.h"

namespace {

// ---- positional corruption ------------------------------------------------------------------------------------
// index of the draw inside a segment of n > 0 entities: the reference's (n.float() * rand).floor().long(), clamped
__device__ __forceinline__ int64_t pos_choice(int64_t n, float u)
{
    const float x = floorf((float)n * u);       // one fp32 multiply (-ffp-contract=off), n converted round-to-nearest
    if (!(x > 0.0f)) return 0;                  // 0, negative, NaN
    if (x >= 9.0e18f) return n - 1;             // (+inf, or past int64: keeps the float -> int conversion in range)
    const int64_t c = (int64_t)x;
    return c < n ? c : n - 1;
}

__device__ __forceinline__ int64_t pos_replace(const int64_t *__restrict__ offsets, const int32_t *__restrict__ values,
                                               int64_t n_rel, int64_t r, float u, const int64_t *__restrict__ fb,
                                               int64_t p, int64_t keep)
{
    int64_t lo = 0, n = 0;
    if (r >= 0 && r < n_rel) { lo = offsets[r]; n = offsets[r + 1] - lo; }
    if (n > 0) return (int64_t)values[lo + pos_choice(n, u)];
    return fb ? fb[p] : keep;
}

__global__ __launch_bounds__(MS_CT) void positional_scatter_kernel(
    const int64_t *__restrict__ heads, const int64_t *__restrict__ tails, const int64_t *__restrict__ rels,
    const uint8_t *__restrict__ mask, const float *__restrict__ u_h, const float *__restrict__ u_t,
    const int64_t *__restrict__ fb_h, const int64_t *__restrict__ fb_t, const int64_t *__restrict__ offsets_h,
    const int32_t *__restrict__ values_h, const int64_t *__restrict__ offsets_t, const int32_t *__restrict__ values_t,
    int64_t n_rel, int64_t B, const int32_t *__restrict__ block_base, int64_t *neg_heads, int64_t *neg_tails)
{
    const int64_t base = (int64_t)blockIdx.x * MS_CB;
    int m[MS_CE];
    int64_t ph = mask_thread_prefix(mask, B, block_base, m);    // #ones before this thread's first position
#pragma unroll
    for (int e = 0; e < MS_CE; ++e) {
        const int64_t j = base + threadIdx.x * MS_CE + e;
        if (j < B) {
            const int64_t h = heads[j], t = tails[j], r = rels[j];
            if (m[e]) {
                neg_heads[j] = pos_replace(offsets_h, values_h, n_rel, r, u_h[ph], fb_h, ph, h);
                neg_tails[j] = t;
            } else {
                const int64_t pt = j - ph;
                neg_heads[j] = h;
                neg_tails[j] = pos_replace(offsets_t, values_t, n_rel, r, u_t[pt], fb_t, pt, t);
            }
            ph += m[e];
        }
    }
}

// ---- per-relation maximum -------------------------------------------------------------------------------------
// Order-preserving code of an fp32: a < b  <=>  code(a) < code(b) as unsigned, every NaN -> the largest code, so the
// integer maximum propagates a NaN as torch.max does.  Code 0 would be the bits of a negative NaN, which never gets
// one: 0 is "no score seen", below the code of -inf (0x007fffff).
constexpr unsigned RM_NAN = 0xffffffffu;
__device__ __forceinline__ unsigned rm_code(float x)
{
    if (x != x) return RM_NAN;
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float rm_value(unsigned k)
{
    if (k == RM_NAN) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

constexpr int RM_CT = 256;          // threads per block
constexpr int RM_LDS = 4096;        // relations whose per-block maxima fit the LDS table (16 KiB)
constexpr int RM_MAX_BLOCKS = 256;  // grid-stride blocks (each flushes up to n_rel maxima)

// tab[0 .. n_rel): per-relation maximum code, tab[n_rel]: the overall one; zeroed before the launch
template <bool LDS>
__global__ __launch_bounds__(RM_CT) void relation_max_kernel(const float *__restrict__ scores,
                                                             const int64_t *__restrict__ rels, int64_t n, int64_t n_rel,
                                                             unsigned *tab)
{
    __shared__ unsigned sh[LDS ? RM_LDS : 1];
    __shared__ unsigned shg[RM_CT / 64];
    if (LDS) {
        for (int i = threadIdx.x; i < n_rel; i += RM_CT) sh[i] = 0u;
        __syncthreads();
    }
    unsigned g = 0u;
    for (int64_t j = (int64_t)blockIdx.x * RM_CT + threadIdx.x; j < n; j += (int64_t)gridDim.x * RM_CT) {
        const unsigned k = rm_code(scores[j]);
        const int64_t r = rels[j];
        g = k > g ? k : g;
        if (r >= 0 && r < n_rel) {
            if (LDS) atomicMax(&sh[r], k);
            else kge_atomic_max_u32(tab + r, k);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned v = (unsigned)__shfl_xor((int)g, o, 64);
        g = v > g ? v : g;
    }
    if ((threadIdx.x & 63) == 0) shg[threadIdx.x >> 6] = g;
    __syncthreads();
    if (LDS) {
        for (int i = threadIdx.x; i < n_rel; i += RM_CT) {
            const unsigned k = sh[i];
            if (k) kge_atomic_max_u32(tab + i, k);
        }
    }
    if (threadIdx.x == 0) {
        for (int i = 1; i < RM_CT / 64; ++i) g = shg[i] > g ? shg[i] : g;
        if (g) kge_atomic_max_u32(tab + n_rel, g);
    }
}

__global__ __launch_bounds__(RM_CT) void relation_max_finish_kernel(const unsigned *__restrict__ tab, int64_t n_rel,
                                                                    float *__restrict__ thr)
{
    const int64_t r = (int64_t)blockIdx.x * RM_CT + threadIdx.x;
    if (r < n_rel) {
        const unsigned k = tab[r];
        thr[r] = rm_value(k ? k : tab[n_rel]);      // a relation without a score: the overall maximum
    }
}

// ---- threshold count --------------------------------------------------------------------------------------------
constexpr int TC_CT = 256;
constexpr int TC_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(TC_CT) void threshold_count_kernel(const float *__restrict__ pos,
                                                                const float *__restrict__ neg,
                                                                const int64_t *__restrict__ rels,
                                                                const float *__restrict__ thr, int64_t n, int64_t n_rel,
                                                                unsigned long long *counts)
{
    __shared__ long long sh[2][TC_CT / 64];
    long long cp = 0, cn = 0;
    for (int64_t j = (int64_t)blockIdx.x * TC_CT + threadIdx.x; j < n; j += (int64_t)gridDim.x * TC_CT) {
        const int64_t r = rels[j];
        if (r >= 0 && r < n_rel) {
            const float t = thr[r];
            cp += pos[j] > t;
            cn += neg[j] < t;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cp += __shfl_xor(cp, o, 64);
        cn += __shfl_xor(cn, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = cp; sh[1][threadIdx.x >> 6] = cn; }
    __syncthreads();
    if (threadIdx.x < 2) {
        long long t = 0;
        for (int i = 0; i < TC_CT / 64; ++i) t += sh[threadIdx.x][i];
        if (t) atomicAdd(counts + threadIdx.x, (unsigned long long)t);
    }
}

} // namespace

extern "C" int64_t kge_positional_ws_elems(int64_t B) { return B > 0 ? mask_scan_ws_elems(B) : 0; }

extern "C" int kge_positional_corrupt(const int64_t *heads, const int64_t *tails, const int64_t *rels, const uint8_t *mask,
                                      const float *u_h, const float *u_t, const int64_t *fb_h, const int64_t *fb_t,
                                      const int64_t *offsets_h, const int32_t *values_h, const int64_t *offsets_t,
                                      const int32_t *values_t, int64_t n_rel, int64_t B, int64_t *neg_heads,
                                      int64_t *neg_tails, int32_t *ws, kge_stream_t stream)
{
    if (B < 0 || n_rel <= 0) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!heads || !tails || !rels || !mask || !u_h || !u_t || !offsets_h || !offsets_t || !neg_heads || !neg_tails || !ws)
        return KGE_EINVAL;
    // values_h / values_t are dereferenced only inside a non-empty segment; fb_h / fb_t only for an empty one
    hipStream_t s = kge_s(stream);
    const int rc = mask_scan_launch(mask, B, ws, s);
    if (rc) return rc;
    hipLaunchKernelGGL(positional_scatter_kernel, dim3((unsigned)mask_scan_blocks(B)), dim3(MS_CT), 0, s, heads, tails, rels,
                       mask, u_h, u_t, fb_h, fb_t, offsets_h, values_h, offsets_t, values_t, n_rel, B, ws, neg_heads,
                       neg_tails);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t kge_relation_max_ws_elems(int64_t n_rel) { return n_rel > 0 ? n_rel + 1 : 0; }

extern "C" int kge_relation_max(const float *scores, const int64_t *rels, int64_t n, int64_t n_rel, float *thr, int32_t *ws,
                                kge_stream_t stream)
{
    if (n < 0 || n_rel <= 0) return KGE_EINVAL;
    if (n == 0) return 0;
    if (!scores || !rels || !thr || !ws) return KGE_EINVAL;
    hipStream_t s = kge_s(stream);
    unsigned *tab = reinterpret_cast<unsigned *>(ws);
    hipError_t e = hipMemsetAsync(tab, 0, (size_t)(n_rel + 1) * sizeof(unsigned), s);
    if (e != hipSuccess) return (int)e;
    int64_t nb = (n + RM_CT - 1) / RM_CT;
    if (nb > RM_MAX_BLOCKS) nb = RM_MAX_BLOCKS;
    if (n_rel <= RM_LDS)
        hipLaunchKernelGGL(relation_max_kernel<true>, dim3((unsigned)nb), dim3(RM_CT), 0, s, scores, rels, n, n_rel, tab);
    else
        hipLaunchKernelGGL(relation_max_kernel<false>, dim3((unsigned)nb), dim3(RM_CT), 0, s, scores, rels, n, n_rel, tab);
    KGE_CHECK_LAUNCH();
    hipLaunchKernelGGL(relation_max_finish_kernel, dim3((unsigned)((n_rel + RM_CT - 1) / RM_CT)), dim3(RM_CT), 0, s, tab,
                       n_rel, thr);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_threshold_count(const float *pos, const float *neg, const int64_t *rels, const float *thr, int64_t n,
                                   int64_t n_rel, int64_t *counts, kge_stream_t stream)
{
    if (n < 0 || n_rel <= 0) return KGE_EINVAL;
    if (n == 0) return 0;
    if (!pos || !neg || !rels || !thr || !counts) return KGE_EINVAL;
    hipStream_t s = kge_s(stream);
    hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    int64_t nb = (n + TC_CT - 1) / TC_CT;
    if (nb > TC_MAX_BLOCKS) nb = TC_MAX_BLOCKS;
    hipLaunchKernelGGL(threshold_count_kernel, dim3((unsigned)nb), dim3(TC_CT), 0, s, pos, neg, rels, thr, n, n_rel,
                       reinterpret_cast<unsigned long long *>(counts));
    KGE_CHECK_LAUNCH();
    return 0;
}
