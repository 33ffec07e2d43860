// Exact recheck of the f16-split prefilter (lp_split_mfma.hip has the error analysis): the pairs the count sweep listed
// as uncertain are re-scored by the exact scalar chain, from one global list or region by region.
#include "lp_split_common.h"
#include "lp_pair_exact.h"

namespace {

// (the listed pairs of one global list: lp_pair_exact.h: lp_list_recheck_kernel, instantiated by kge_lp_split_recheck below)

// ---- exact re-scoring REGION BY REGION (r05) -------------------------------------------------------------------------
// The free-running sweep can leave its uncertain pairs in regions of the list, one per (query panel, 32-query sub-tile)
// (kge_split_args.region_count).  A block takes a region: the sub-tile's 32 query rows go to LDS ONCE (fp32, row stride an
// odd number of 16-byte pieces: conflict-free b128 reads at per-lane rows), then every pair costs the candidate row
// alone -- staged cooperatively like lp_staged_segment's -- instead of both rows: the recheck is bound by the L2's row
// bandwidth (8.8 TB/s of 1.6 KB per pair at cfg2), so half the bytes is most of half the time.  Same chains (lp_chain_dot
// on 32-column chunks, segment after segment), same epilogue: same bits as lp_pair_score.  Rows must be float4-readable
// (kge_lp_vec4).
__device__ __forceinline__ float recheck_e_segment(const float *__restrict__ T, int64_t ldt, int K, int ci,
                                                   const float *__restrict__ qrow, float *es, float acc)
{
    const int lane = threadIdx.x & 63;
    // (ONE 32-column chunk in flight per wavefront, as lp_staged_segment: with two -- 175 VGPRs -- the kernel took 83 us
    // instead of 68, profiles/r05/region_recheck_ab.txt)
    int k0 = 0;
    if (K >= KGE_PS_KC) {
        float4 e0, e1, e2, e3, e4, e5, e6, e7;
#define KGE_RR_FETCH(IT, KK)                                                                                  \
    {                                                                                                         \
        const int idx_ = lane + 64 * IT, rr_ = idx_ >> 3, pc_ = idx_ & 7;                                     \
        const int rc_ = __shfl(ci, rr_, 64);                                                                  \
        e##IT = *reinterpret_cast<const float4 *>(T + (int64_t)rc_ * ldt + (KK) + pc_ * 4);                   \
    }
#define KGE_RR_STORE(IT)                                                                                      \
    {                                                                                                         \
        const int idx_ = lane + 64 * IT, rr_ = idx_ >> 3, pc_ = idx_ & 7;                                     \
        *reinterpret_cast<float4 *>(es + rr_ * KGE_PS_LD + pc_ * 4) = e##IT;                                  \
    }
#define KGE_RR_ALL(M, ...) M(0, ##__VA_ARGS__) M(1, ##__VA_ARGS__) M(2, ##__VA_ARGS__) M(3, ##__VA_ARGS__) \
                           M(4, ##__VA_ARGS__) M(5, ##__VA_ARGS__) M(6, ##__VA_ARGS__) M(7, ##__VA_ARGS__)
        KGE_RR_ALL(KGE_RR_FETCH, 0)
        for (; k0 + KGE_PS_KC <= K; k0 += KGE_PS_KC) {
            KGE_RR_ALL(KGE_RR_STORE)
            if (k0 + 2 * KGE_PS_KC <= K) { KGE_RR_ALL(KGE_RR_FETCH, k0 + KGE_PS_KC) }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            acc = lp_chain_dot(qrow + k0, es + lane * KGE_PS_LD, KGE_PS_KC, acc);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
#undef KGE_RR_ALL
#undef KGE_RR_STORE
#undef KGE_RR_FETCH
    }
    for (; k0 < K; k0 += KGE_PS_KC) {      // the last, partial chunk (K % 4 == 0)
        const int kc = min(KGE_PS_KC, K - k0);
        const int pieces = kc >> 2;
        for (int idx = lane; idx < 64 * pieces; idx += 64) {
            const int rr = idx / pieces, pc = idx - rr * pieces;
            const int rc = __shfl(ci, rr, 64);
            *reinterpret_cast<float4 *>(es + rr * KGE_PS_LD + pc * 4) =
                *reinterpret_cast<const float4 *>(T + (int64_t)rc * ldt + k0 + pc * 4);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        acc = lp_chain_dot(qrow + k0, es + lane * KGE_PS_LD, kc, acc);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    return acc;
}

// Rows longer than one LDS segment (r06; K > 256 or so -- DistMult / ComplEx d = 400: the recheck was 20 % of cfg4's step, all
// of it row fetches): the region's query rows pass through LDS in SEGMENTS of seg_cols logical columns of [A0 | A1] while the
// chains of up to RR_G pair groups per wave (a batch of NWV * 64 * RR_G pairs: a whole region, typically) rest in registers
// between segments -- the sequential chain is cut, not reordered: same bits.  One segment (K <= seg_cols) is r05's form.
constexpr int RR_G = 4;

template <int NWV>
__global__ __launch_bounds__(64 * NWV) void split_recheck_regions_kernel(const kge_lp_desc d, const float *__restrict__ s_true,
                                                                        const int32_t *__restrict__ list, int32_t region_cap,
                                                                        const int32_t *__restrict__ region_count, int n_regions,
                                                                        int ldq, int seg_cols, int32_t *raw_count, float *list_stat,
                                                                        int32_t *list_count)
{
    extern __shared__ __attribute__((aligned(16))) float rr_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float *qrows = rr_smem;
    float *es = rr_smem + RR_ROWS * ldq + wv * 64 * KGE_PS_LD;
    const int K = d.K0 + d.K1;
    int n_block = 0;
    // logical columns [c0, c1) of the region's 32 query rows -> LDS (row stride ldq)
    auto stage = [&](int64_t q0, int c0, int c1) {
        const int np = (c1 - c0) >> 2;
        for (int idx = tid; idx < RR_ROWS * np; idx += 64 * NWV) {
            const int rr = idx / np, pc = idx - rr * np;
            const int64_t q = min(q0 + rr, d.B - 1);
            const int col = c0 + pc * 4;        // (K0 % 4 == 0: a piece lies in one segment of the operand)
            const float4 v = col < d.K0 ? *reinterpret_cast<const float4 *>(d.A0 + q * d.lda0 + col)
                                        : *reinterpret_cast<const float4 *>(d.A1 + q * d.lda1 + (col - d.K0));
            *reinterpret_cast<float4 *>(qrows + rr * ldq + pc * 4) = v;
        }
    };
    // the chain of one pair over the staged columns [c0, c1): operand segment 0, then 1
    auto chain = [&](float acc, int ci, const float *qrow, int c0, int c1) -> float {
        if (c0 < d.K0) acc = recheck_e_segment(d.T0 + c0, d.ldt0, min(c1, d.K0) - c0, ci, qrow, es, acc);
        if (c1 > d.K0 && d.K1 > 0) {
            const int s0 = max(c0, d.K0);
            acc = recheck_e_segment(d.T1 + (s0 - d.K0), d.ldt1, c1 - s0, ci, qrow + (s0 - c0), es, acc);
        }
        return acc;
    };
    for (int reg = blockIdx.x; reg < n_regions; reg += gridDim.x) {
        const int n = (int)min((unsigned)region_count[reg], (unsigned)region_cap);   // (past the capacity: overflow flagged by the sweep)
        if (n == 0) continue;                   // (block-uniform)
        n_block += n;
        const int64_t q0 = (int64_t)(reg / 3) * RR_PANEL + (reg % 3) * RR_ROWS;
        const int2 *ent = reinterpret_cast<const int2 *>(list) + (int64_t)reg * region_cap;
        if (K <= seg_cols) {
            __syncthreads();                    // the previous region's readers are done
            stage(q0, 0, K);
            __syncthreads();
            for (int c0 = wv * 64; c0 < n; c0 += NWV * 64) {
                const int pi = c0 + lane;
                const bool valid = pi < n;
                const int2 e = ent[valid ? pi : c0];       // idle lanes shadow the group's first pair
                const int qi = e.x, ci = e.y;
                const float acc = chain(0.0f, ci, qrows + (int)(qi - q0) * ldq, 0, K);
                const float sc = lp_epilogue_any(d, acc, qi, ci);
                if (valid && !(sc >= s_true[qi])) atomicSub(&raw_count[qi], 1);
            }
            continue;
        }
        for (int b0 = 0; b0 < n; b0 += NWV * 64 * RR_G) {       // (block-uniform trip counts: barriers inside)
            float acc[RR_G];
            int qi[RR_G], ci[RR_G];
#pragma unroll
            for (int g = 0; g < RR_G; ++g) {
                const int c0 = b0 + (g * NWV + wv) * 64;
                const int pi = c0 + lane;
                const int2 e = ent[min(pi < n ? pi : c0, n - 1)];   // idle lanes shadow the group's first pair (idle groups: the last pair)
                qi[g] = e.x; ci[g] = e.y; acc[g] = 0.0f;
            }
            for (int c0 = 0; c0 < K; c0 += seg_cols) {
                const int c1 = min(K, c0 + seg_cols);
                __syncthreads();                // the previous segment's / region's readers are done
                stage(q0, c0, c1);
                __syncthreads();
#pragma unroll
                for (int g = 0; g < RR_G; ++g)
                    if (b0 + (g * NWV + wv) * 64 < n)       // (wave-uniform)
                        acc[g] = chain(acc[g], ci[g], qrows + (int)(qi[g] - q0) * ldq, c0, c1);
            }
#pragma unroll
            for (int g = 0; g < RR_G; ++g) {
                const int pi = b0 + (g * NWV + wv) * 64 + lane;
                if (pi < n) {
                    const float sc = lp_epilogue_any(d, acc[g], qi[g], ci[g]);
                    if (!(sc >= s_true[qi[g]])) atomicSub(&raw_count[qi[g]], 1);
                }
            }
        }
    }
    if (tid == 0 && n_block > 0) {              // pairs re-scored per evaluation (level policy) / the list's length
        if (list_stat) atomicAdd(list_stat, (float)n_block);
        if (list_count) atomicAdd(list_count, n_block);
    }
}

} // namespace

extern "C" int kge_lp_split_recheck(const kge_lp_desc *d, const float *s_true, const int32_t *list, int32_t cap,
                                    const int32_t *list_count, int32_t *raw_count, float *list_stat, kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (d->B == 0 || d->N == 0) return 0;
    if (!s_true || !list || cap <= 0 || !list_count || !raw_count) return KGE_EINVAL;
    if (!KGE_LP_IS_MFMA(d->mode)) return KGE_EINVAL;
    const int grid = split_num_cus() * kge_env_int("KGE_SPLIT_RECHECK_WAVES", 160 * 1024 / (2 * 64 * KGE_PS_LD * 4));
    return lp_pair_dispatch<PAIR_STAGED>(*d, [&](auto v) {
        using V = decltype(v);
        if constexpr (V::chain != PAIR_DOT) return KGE_EINVAL;      // (not reached: the MFMA modes run the dot chain)
        else {
            hipLaunchKernelGGL(lp_list_recheck_kernel<V>, dim3(grid), dim3(64), 0, kge_s(stream), *d, s_true, list, cap,
                               list_count, raw_count, list_stat);
            KGE_CHECK_LAUNCH();
            return 0;
        }
    });
}

/* regions of the list of n queries' sweep: 3 per panel of 96 queries (kge_split_args.region_count) */
extern "C" int kge_lp_split_regions(int64_t B)
{
    return (int)(kge_lp_split_rows_padded(B, 1) / RR_PANEL) * 3;
}

// LDS segment of the region recheck: logical columns of the query rows resident at a time (a multiple of 32, the chunk of the
// candidate-row staging), from the byte budget of the 32 rows (KGE_REGION_MAX_BYTES, default 36 KiB: at K = 200 the region's
// 26 KB of query rows leave six wavefronts per CU; measured r05 -- profiles/r05/region_recheck_ab.txt -- a WHOLE 52 KB row
// block at K = 400 left four and was slower than no regions; r06 passes longer rows through in segments instead)
static int region_seg_cols(int K)
{
    const int max_ld = kge_env_int("KGE_REGION_MAX_BYTES", 36 * 1024) / (RR_ROWS * 4);
    const int ld_full = K + (((K >> 2) & 1) ? 0 : 4);
    if (ld_full <= max_ld) return K;
    // longer rows: SMALLER segments than the budget of a whole row block -- more wavefronts per CU is what the kernel lives on
    // (cfg4, DistMult d = 400, same box: no regions 2.107 ms per evaluate, 36 KiB segments 2.083, 20 KiB 2.031, 12 KiB 2.036;
    // profiles/r06/region_segments_ab.txt)
    const int seg_ld = min(max_ld, kge_env_int("KGE_REGION_SEG_BYTES", 20 * 1024) / (RR_ROWS * 4));
    int seg = ((seg_ld - 4) / 32) * 32;
    return seg < 32 ? 32 : seg;
}

/* 1 if kge_lp_split_count / kge_lp_split_recheck_regions take a list cut into regions for this problem */
extern "C" int kge_lp_split_regions_supported(const kge_lp_desc *d)
{
    if (kge_lp_desc_check(d) || !KGE_LP_IS_MFMA(d->mode) || !kge_lp_vec4(*d)) return 0;
    const int K = d->K0 + d->K1;
    // (rows of the free-running kernel's range: the chunked-panel kernel of longer rows keeps one global list; segments of the
    // operand must not cut a 16-byte piece: K0 % 4 == 0 is part of kge_lp_vec4)
    if ((K + 2 + 15) / 16 > 32) return 0;
    if (region_seg_cols(K) < K && kge_env_int("KGE_REGION_SEGMENTS", 1) == 0) return 0;
    return 1;
}

extern "C" int kge_lp_split_recheck_regions(const kge_lp_desc *d, const float *s_true, const int32_t *list, int32_t cap,
                                            const int32_t *region_count, int32_t *raw_count, float *list_stat,
                                            int32_t *list_count, kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (d->B == 0 || d->N == 0) return 0;
    if (!s_true || !list || cap <= 0 || !region_count || !raw_count) return KGE_EINVAL;
    if (!kge_lp_split_regions_supported(d)) return KGE_EINVAL;
    const int n_regions = kge_lp_split_regions(d->B);
    const int32_t region_cap = cap / n_regions;
    if (region_cap <= 0) return KGE_EINVAL;
    const int K = d->K0 + d->K1;
    const int seg = region_seg_cols(K);
    const int ldq = seg + (((seg >> 2) & 1) ? 0 : 4);   // floats: a multiple of 4, an odd number of 16-byte pieces
    const int nwv = kge_env_int("KGE_RECHECK_REGION_WAVES", 2);
    const int smem = (RR_ROWS * ldq + (nwv == 4 ? 4 : 2) * 64 * KGE_PS_LD) * 4;
    const int want = split_num_cus() * 6;
    const int grid = n_regions < want ? n_regions : want;
    static int attr2[16], attr4[16];     // per device
    if (nwv == 4) {
        auto k = split_recheck_regions_kernel<4>;
        if (int e = kge_ensure_dyn_smem(reinterpret_cast<const void *>(k), smem, attr4)) return e;
        hipLaunchKernelGGL(k, dim3(grid), dim3(256), smem, kge_s(stream), *d, s_true, list, region_cap, region_count, n_regions,
                           ldq, seg, raw_count, list_stat, list_count);
    } else {
        auto k = split_recheck_regions_kernel<2>;
        if (int e = kge_ensure_dyn_smem(reinterpret_cast<const void *>(k), smem, attr2)) return e;
        hipLaunchKernelGGL(k, dim3(grid), dim3(128), smem, kge_s(stream), *d, s_true, list, region_cap, region_count, n_regions,
                           ldq, seg, raw_count, list_stat, list_count);
    }
    KGE_CHECK_LAUNCH();
    return 0;
}
