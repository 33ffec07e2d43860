// The exact scorer of LISTED (query, candidate) pairs (gfx950): the staged forms of kge_common.h's lp_pair_score and the
// one place that knows which of them a descriptor runs.  Used by the pair / filter-correction kernels (lp_pairs.hip) and
// the two list rechecks (lp_split_recheck.hip, lp_l1_sad.hip).
#pragma once
#include "kge_common.h"

// ---- wave-cooperative exact pair scores (MFMA modes) ------------------------------
// One lane per (query, candidate) pair runs the scalar chain of lp_pair_score -- one
// accumulator in a fixed order, it cannot be split across lanes -- but the two
// rows of each of the wavefront's 64 pairs are fetched COOPERATIVELY, 32 k at a
// time, as 128-byte row segments (8 lanes x float4 per row, all of a chunk's
// loads in flight together) and handed to their lane through LDS (row stride 36
// floats: conflict-free b128 stores and loads).  A lane-per-row gather touches 64
// different cache lines per load instruction and is ~5x slower.
// Every lane of the wavefront must call; `qs`/`es` are this wavefront's own
// 64 x KGE_PS_LD floats of LDS.  Bit-identical to lp_pair_score.
#ifndef KGE_PS_KC_V
#define KGE_PS_KC_V 32      /* 8 float4 pieces per row: the piece -> (row, column) split is shifts, and hipcc keeps */
#define KGE_PS_LD_V 36      /* the pipelined loop at 88 VGPRs (40 / 44 hoisted 80 address registers and spilled)   */
#endif
constexpr int KGE_PS_KC = KGE_PS_KC_V, KGE_PS_LD = KGE_PS_LD_V;

static inline bool kge_lp_vec4(const kge_lp_desc &d)
{
    bool v = (d.K0 % 4 == 0) && (d.lda0 % 4 == 0) && (d.ldt0 % 4 == 0) && kge_aligned16(d.A0) && kge_aligned16(d.T0);
    if (d.K1 > 0)
        v = v && (d.K1 % 4 == 0) && (d.lda1 % 4 == 0) && (d.ldt1 % 4 == 0) && kge_aligned16(d.A1) && kge_aligned16(d.T1);
    return v;
}

// the chain a pair runs: the scalar walk of lp_pair_score (any mode, any layout), or one of the staged chains
enum PairChain { PAIR_SCALAR, PAIR_DOT, PAIR_L1, PAIR_L2, PAIR_TL1, PAIR_TL2, PAIR_TEL2, PAIR_CMOD };
// the kge_lp_desc mode whose per-element term / finish (lp_direct_term, lp_direct_finish) a staged direct chain uses
constexpr int pair_chain_mode(PairChain ch)
{
    return ch == PAIR_TL1 ? (int)KGE_LP_TORUS_L1 : ch == PAIR_TL2 ? (int)KGE_LP_TORUS_L2
         : ch == PAIR_TEL2 ? (int)KGE_LP_TORUS_EL2 : ch == PAIR_CMOD ? (int)KGE_LP_CMOD
         : ch == PAIR_L2 ? (int)KGE_LP_L2_DIRECT : (int)KGE_LP_L1_DIRECT;
}

// the direct modes' chains (lp_pair_score without the rank-1 term), one accumulator: L2 one fmaf per k in
// ascending order; L1, the torus modes and the complex modulus one add per aligned 4-group of k (lp_direct_group: the
// group's terms as (m0+m1)+(m2+m3), or the moduli of its two pairs).  `a` / `t` must be readable (zero-filled) up to the
// next multiple of 4 -- the staged chunks below are.
template <PairChain CH>
__device__ __forceinline__ float lp_chain_direct(const float *__restrict__ a, const float *__restrict__ t, int K, float acc)
{
    if (CH != PAIR_L2) {
        constexpr int OP = pair_chain_mode(CH);
        for (int k = 0; k < K; k += 4) {
            const float4 av = *reinterpret_cast<const float4 *>(a + k), tv = *reinterpret_cast<const float4 *>(t + k);
            acc = acc + lp_direct_group<OP>(av.x - tv.x, av.y - tv.y, av.z - tv.z, av.w - tv.w);
        }
    } else {
        for (int k = 0; k < K; ++k) {
            const float diff = a[k] - t[k];
            acc = fmaf(diff, diff, acc);
        }
    }
    return acc;
}

// CH: PAIR_DOT = the MFMA modes' dot chain (lp_chain_dot), else that direct chain
template <bool VEC4, PairChain CH = PAIR_DOT>
__device__ __forceinline__ float lp_staged_segment(const float *__restrict__ A, int64_t lda,
                                                   const float *__restrict__ T, int64_t ldt, int K, int qi, int ci,
                                                   float *qs, float *es, float acc)
{
    const int lane = threadIdx.x & 63;
    // Full chunks (16-byte aligned rows): software-pipelined -- the NEXT chunk's 16 row loads are issued before
    // the current chunk's sequential chain runs, so the chain (32 dependent FMAs fed from LDS) hides under the
    // loads' latency instead of following it: a pair costs one load latency plus the chains, not one per chunk.
    // The 16 in-flight float4 are NAMED scalars (macro-expanded): as arrays carried around the chunk loop hipcc
    // left them in scratch memory (272 B of private segment, 3.5x slower than no pipelining at all).
    static_assert(KGE_PS_KC == 32, "the fetch / store macros below are written out for 8 float4 pieces per row");
    int k0 = 0;
    if (VEC4 && K >= KGE_PS_KC) {
        float4 q0, q1, q2, q3, q4, q5, q6, q7, e0, e1, e2, e3, e4, e5, e6, e7;
#define KGE_PS_FETCH(IT, KK)                                                                                  \
    {                                                                                                         \
        const int idx_ = lane + 64 * IT, rr_ = idx_ >> 3, pc_ = idx_ & 7;                                     \
        const int rq_ = __shfl(qi, rr_, 64), rc_ = __shfl(ci, rr_, 64);                                      \
        q##IT = *reinterpret_cast<const float4 *>(A + (int64_t)rq_ * lda + (KK) + pc_ * 4);                   \
        e##IT = *reinterpret_cast<const float4 *>(T + (int64_t)rc_ * ldt + (KK) + pc_ * 4);                   \
    }
#define KGE_PS_STORE(IT)                                                                                      \
    {                                                                                                         \
        const int idx_ = lane + 64 * IT, rr_ = idx_ >> 3, pc_ = idx_ & 7;                                     \
        *reinterpret_cast<float4 *>(qs + rr_ * KGE_PS_LD + pc_ * 4) = q##IT;                                  \
        *reinterpret_cast<float4 *>(es + rr_ * KGE_PS_LD + pc_ * 4) = e##IT;                                  \
    }
#define KGE_PS_ALL(M, ...) M(0, ##__VA_ARGS__) M(1, ##__VA_ARGS__) M(2, ##__VA_ARGS__) M(3, ##__VA_ARGS__) \
                           M(4, ##__VA_ARGS__) M(5, ##__VA_ARGS__) M(6, ##__VA_ARGS__) M(7, ##__VA_ARGS__)
        KGE_PS_ALL(KGE_PS_FETCH, 0)
        for (; k0 + KGE_PS_KC <= K; k0 += KGE_PS_KC) {
            KGE_PS_ALL(KGE_PS_STORE)
            if (k0 + 2 * KGE_PS_KC <= K) { KGE_PS_ALL(KGE_PS_FETCH, k0 + KGE_PS_KC) }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // same wave: LDS executes in order
            if (CH == PAIR_DOT) acc = lp_chain_dot(qs + lane * KGE_PS_LD, es + lane * KGE_PS_LD, KGE_PS_KC, acc);
            else acc = lp_chain_direct<CH>(qs + lane * KGE_PS_LD, es + lane * KGE_PS_LD, KGE_PS_KC, acc);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
#undef KGE_PS_ALL
#undef KGE_PS_STORE
#undef KGE_PS_FETCH
    }
    for (; k0 < K; k0 += KGE_PS_KC) {      // the last, partial chunk (and everything when rows are not 16-byte aligned)
        const int kc = min(KGE_PS_KC, K - k0);
        {
            const int pieces = (kc + 3) >> 2;
            for (int idx = lane; idx < 64 * pieces; idx += 64) { // uniform trip count
                const int rr = idx / pieces, pc = idx - rr * pieces;
                const int rq = __shfl(qi, rr, 64), rc = __shfl(ci, rr, 64);
                const float *qp = A + (int64_t)rq * lda + k0 + pc * 4;
                const float *ep = T + (int64_t)rc * ldt + k0 + pc * 4;
                const int left = kc - pc * 4;
                float4 qv, ev;
                qv.x = qp[0]; ev.x = ep[0];
                qv.y = left > 1 ? qp[1] : 0.f; ev.y = left > 1 ? ep[1] : 0.f;
                qv.z = left > 2 ? qp[2] : 0.f; ev.z = left > 2 ? ep[2] : 0.f;
                qv.w = left > 3 ? qp[3] : 0.f; ev.w = left > 3 ? ep[3] : 0.f;
                *reinterpret_cast<float4 *>(qs + rr * KGE_PS_LD + pc * 4) = qv;
                *reinterpret_cast<float4 *>(es + rr * KGE_PS_LD + pc * 4) = ev;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (CH == PAIR_DOT) acc = lp_chain_dot(qs + lane * KGE_PS_LD, es + lane * KGE_PS_LD, kc, acc);
        else acc = lp_chain_direct<CH>(qs + lane * KGE_PS_LD, es + lane * KGE_PS_LD, kc, acc);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    return acc;
}

// plain direct or torus modes (no rank-1 term) by chain, bit-identical to lp_pair_score
template <bool VEC4, PairChain CH>
__device__ __forceinline__ float lp_pair_score_staged_ch(const kge_lp_desc &d, int qi, int ci, float *qs, float *es)
{
    static_assert(CH != PAIR_SCALAR && CH != PAIR_DOT, "a direct chain");
    return lp_direct_finish<pair_chain_mode(CH)>(lp_staged_segment<VEC4, CH>(d.A0, d.lda0, d.T0, d.ldt0, d.K0, qi, ci, qs, es, 0.0f));
}

// MFMA modes only (KGE_LP_IS_MFMA); (qi, ci) must be valid rows on every lane
template <bool VEC4>
__device__ __forceinline__ float lp_pair_score_staged(const kge_lp_desc &d, int qi, int ci, float *qs, float *es)
{
    float acc = lp_staged_segment<VEC4>(d.A0, d.lda0, d.T0, d.ldt0, d.K0, qi, ci, qs, es, 0.0f);
    if (d.K1 > 0) acc = lp_staged_segment<VEC4>(d.A1, d.lda1, d.T1, d.ldt1, d.K1, qi, ci, qs, es, acc);
    return lp_epilogue_any(d, acc, qi, ci);
}

// ---- one variant type, one selector ------------------------------------------------------------------------------------
// A kernel that scores listed pairs is a template over ONE of these: the chain and whether rows are float4-readable.
template <PairChain CHAIN, bool VEC4>
struct PairVariant {
    static constexpr PairChain chain = CHAIN;
    static constexpr bool staged = CHAIN != PAIR_SCALAR;
    static constexpr int lds_floats = staged ? 64 * KGE_PS_LD : 1;      // each of qs / es (scalar: never referenced)
    // The bits of lp_pair_score(d, i, c) on `ok` lanes, anything on the others (idle lanes stage row 0 of both operands).
    // Staged variants: every lane of the wavefront must call.
    __device__ __forceinline__ static float score(const kge_lp_desc &d, bool ok, int64_t i, int64_t c, float *qs, float *es)
    {
        if constexpr (!staged) return ok ? lp_pair_score(d, i, c) : 0.f;
        else if constexpr (CHAIN == PAIR_DOT) return lp_pair_score_staged<VEC4>(d, ok ? (int)i : 0, ok ? (int)c : 0, qs, es);
        else return lp_pair_score_staged_ch<VEC4, CHAIN>(d, ok ? (int)i : 0, ok ? (int)c : 0, qs, es);
    }
};
// the staging rows `qs` / `es` of a one-wavefront block.  (TWO LDS objects: as members of one struct hipcc addresses es off
// qs and allocates 9 - 17 fewer VGPRs in the float4 variants -- not the kernels that were measured)
#define KGE_PAIR_LDS(V)                                                   \
    __shared__ __attribute__((aligned(16))) float qs[V::lds_floats];      \
    __shared__ __attribute__((aligned(16))) float es[V::lds_floats]

// What an entry point wants from the selector -- the rows of the table it reproduces, not an extension point:
//   PAIR_DEFAULT            MFMA modes: staged dot; plain direct / torus / CMOD with float4 rows and no rank-1 term: the staged
//                           chain of the mode; everything else, and B or N outside (0, INT32_MAX]: scalar
//   PAIR_MFMA_ELSE_SCALAR   MFMA modes: staged dot (same B, N condition); everything else scalar
//   PAIR_STAGED             staged or KGE_EINVAL: MFMA modes the dot chain, plain L1 / L2 without rank-1 term their chain,
//                           with or without float4 rows (the caller has checked B, N > 0; list entries are int32)
enum PairPolicy { PAIR_DEFAULT, PAIR_MFMA_ELSE_SCALAR, PAIR_STAGED };

// calls f(PairVariant<...>{}) exactly once and returns its result (or KGE_EINVAL: PAIR_STAGED on a mode it cannot stage)
template <PairPolicy POL, class F>
int lp_pair_dispatch(const kge_lp_desc &d, F &&f)
{
    const bool mfma = KGE_LP_IS_MFMA(d.mode), vec4 = kge_lp_vec4(d);
    const bool fits = d.B > 0 && d.N > 0 && d.B <= INT32_MAX && d.N <= INT32_MAX;   // the staged scorers take int rows
    if (mfma && (fits || POL == PAIR_STAGED)) return vec4 ? f(PairVariant<PAIR_DOT, true>{}) : f(PairVariant<PAIR_DOT, false>{});
    if constexpr (POL == PAIR_STAGED) {
        if (d.Wq) return KGE_EINVAL;
        if (d.mode == KGE_LP_L1_DIRECT) return vec4 ? f(PairVariant<PAIR_L1, true>{}) : f(PairVariant<PAIR_L1, false>{});
        if (d.mode == KGE_LP_L2_DIRECT) return vec4 ? f(PairVariant<PAIR_L2, true>{}) : f(PairVariant<PAIR_L2, false>{});
        return KGE_EINVAL;
    } else {
        if constexpr (POL == PAIR_DEFAULT) {
            if (!mfma && !d.Wq && vec4 && fits) {
                switch (d.mode) {   // (the torus modes and the complex modulus: the same staging, their terms)
                case KGE_LP_L1_DIRECT: return f(PairVariant<PAIR_L1, true>{});
                case KGE_LP_TORUS_L1: return f(PairVariant<PAIR_TL1, true>{});
                case KGE_LP_TORUS_L2: return f(PairVariant<PAIR_TL2, true>{});
                case KGE_LP_TORUS_EL2: return f(PairVariant<PAIR_TEL2, true>{});
                case KGE_LP_CMOD: return f(PairVariant<PAIR_CMOD, true>{});
                default: return f(PairVariant<PAIR_L2, true>{});
                }
            }
        }
        return f(PairVariant<PAIR_SCALAR, false>{});
    }
}

// grid of the one-wavefront kernels (pairs here, rows in lp_prep.hip): a block per 64 items up to `cap` blocks, past it
// the blocks loop
static inline int lp_pair_grid(int64_t pairs)
{
    const int64_t groups = (pairs + 63) / 64, cap = 256 * 14;
    return (int)(groups < cap ? groups : cap);
}

namespace {    // (internal linkage: every translation unit's instantiations are built with that file's own flags)

// Exact re-scoring of a prefilter's list of uncertain pairs (list[2 p] = query, list[2 p + 1] = local candidate): one lane
// per pair, rows staged cooperatively; 1 comes off raw_count[query] for every pair whose exact score is below s_true.
template <class V>
__global__ __launch_bounds__(64, 2) void lp_list_recheck_kernel(const kge_lp_desc d, const float *__restrict__ s_true,
                                                              const int32_t *__restrict__ list, int32_t cap,
                                                              const int32_t *__restrict__ list_count, int32_t *raw_count,
                                                              float *list_stat)
{
    KGE_PAIR_LDS(V);
    const int lane = threadIdx.x;
    const int n = (int)min((unsigned)*list_count, (unsigned)cap);   // (a count past the capacity means overflow: the caller redoes the count)
    if (list_stat && blockIdx.x == 0 && lane == 0) atomicAdd(list_stat, (float)n);   // pairs re-scored per evaluation (level policy)
    const int ngroups = (n + 63) >> 6;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int pi = grp * 64 + lane;
        const bool valid = pi < n;
        const int pj = valid ? pi : grp * 64;       // idle lanes shadow the group's first pair
        const int qi = list[2 * pj], ci = list[2 * pj + 1];
        const float sc = V::score(d, true, qi, ci, qs, es);
        if (valid && !(sc >= s_true[qi])) atomicSub(&raw_count[qi], 1);
    }
}

} // namespace
