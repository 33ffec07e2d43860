// Shared device helpers for libkge_hip.so (gfx950 only).
// Compiled with -ffp-contract=off: every fused multiply-add in this library is
// an explicit fmaf(), so the fp32 arithmetic is exactly what the source says
// (and what oracle/kge_oracle.c restates on the CPU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/kge_hip.h"
#include "../../include/kge_hip_rotate.h"

#define KGE_WAVE 64

#define KGE_CHECK_LAUNCH()                          \
    do {                                            \
        hipError_t e__ = hipGetLastError();         \
        if (e__ != hipSuccess) return (int)e__;     \
    } while (0)

static inline hipStream_t kge_s(kge_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// KGE_RESCAL / KGE_HOLE behind kge_score_triples / kge_score_triples_bwd (bilinear_xform.hip)
int kge_bilinear_score_fwd(int kind, const float *t0, const float *t1, int d_ent, int d_rel, const int64_t *h,
                           const int64_t *t, const int64_t *r, int64_t B, float *out, hipStream_t s);
int kge_bilinear_score_bwd(int kind, const float *t0, const float *t1, int d_ent, int d_rel, const int64_t *h,
                           const int64_t *t, const int64_t *r, int64_t B, const float *go, float *g0, float *g1,
                           float *rows, int64_t rows_ld, hipStream_t s);

// KGE_TRANSR behind kge_score_triples / kge_score_triples_bwd (transr_xform.hip)
int kge_transr_score_fwd(const float *E, const float *R, const float *M, int d_ent, int d_rel, const int64_t *h,
                         const int64_t *t, const int64_t *r, int64_t B, float *out, hipStream_t s);
int kge_transr_score_bwd(const float *E, const float *R, const float *M, int d_ent, int d_rel, const int64_t *h,
                         const int64_t *t, const int64_t *r, int64_t B, const float *go, float *rows, int64_t rows_ld,
                         hipStream_t s);

// KGE_ROTATE behind kge_score_triples / kge_score_triples_bwd (rotate.hip; gradient rows only)
int kge_rotate_score_fwd(const float *E, const float *P, int d_ent, int d_rel, const int64_t *h, const int64_t *t,
                         const int64_t *r, int64_t B, float *out, hipStream_t s);
int kge_rotate_score_bwd(const float *E, const float *P, int d_ent, int d_rel, const int64_t *h, const int64_t *t,
                         const int64_t *r, int64_t B, const float *go, float *rows, int64_t rows_ld, hipStream_t s);

// gM[rho] = sum over the triples of relation rho, in the order of perm, of U_i V_i^T (d_r x d_e): the reduction behind
// kge_transr_rel_grad and, with d_r = d_e, kge_rescal_rel_grad, which validate their own arguments (transr_xform.hip)
int kge_rel_outer_grad(const float *U, int64_t ldu, const float *V, int64_t ldv, int d_r, int d_e, const int64_t *r,
                       const int64_t *perm, int64_t B, int64_t n_rel, float *gM, int64_t ldg, hipStream_t s);

static inline bool kge_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Running maximum in a device scalar (non-negative floats compared as bit patterns).  Same-address atomics
// serialise at ~12 ns each on this part (they are resolved past the per-XCD L2s), so a wave first LOOKS:
// the scalar only grows, a stale (smaller) reading merely costs the atomic it would have saved.
__device__ __forceinline__ void kge_atomic_max_u32(unsigned *addr, unsigned v)
{
    if (v > __builtin_nontemporal_load(addr)) atomicMax(addr, v);
}

// Maximum over the wavefront of BIT PATTERNS (non-negative floats sort like their bits, a NaN above +inf: it survives)
__device__ __forceinline__ unsigned wave_max_u32(unsigned m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    return m;
}
// ... over a block of 4 wavefronts, on every thread; sh[4] is the caller's (one barrier; reuse needs another in between)
__device__ __forceinline__ unsigned block_max_u32(unsigned m, unsigned *sh)
{
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    return max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int RB = 256; // threads per row-block

__device__ __forceinline__ int block_sum_i(int v, int *sh)
{
    v = wave_sum_i(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    int t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    return t;
}

static inline int grid1d(int64_t n, int per_block)
{
    int64_t b = (n + per_block - 1) / per_block;
    const int64_t cap = 256 * 16;
    return (int)(b < cap ? (b > 0 ? b : 1) : cap);
}

// ---- the scoring contract of kge_lp_desc (see include/kge_hip.h) ----------
__device__ __forceinline__ float lp_chain_dot(const float *__restrict__ a, const float *__restrict__ t,
                                              int K, float acc)
{
    // the MFMA kernel's accumulation order: 8-blocks ascending, and inside an
    // 8-block k = 0,4,1,5,2,6,3,7 (lane-half h of the wave supplies k = 4h + j
    // to MFMA j, and v_mfma_f32_32x32x2_f32 adds half 0's product first)
    int kb = 0;
    for (; kb + 8 <= K; kb += 8) { // full 8-blocks: 16 independent loads, then the dependent chain
        float av[8], tv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { av[j] = a[kb + j]; tv[j] = t[kb + j]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc = fmaf(av[j], tv[j], acc);
            acc = fmaf(av[4 + j], tv[4 + j], acc);
        }
    }
    if (kb < K) { // partial last block
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k0 = kb + j, k1 = kb + 4 + j;
            if (k0 < K) acc = fmaf(a[k0], t[k0], acc);
            if (k1 < K) acc = fmaf(a[k1], t[k1], acc);
        }
    }
    return acc;
}

__device__ __forceinline__ float lp_epilogue(int mode, float dot, float qn, float en)
{
    if (mode == KGE_LP_L2_EXPAND) {
        float d2 = fmaf(-2.0f, dot, qn + en);
        return -fmaxf(d2, 0.0f);
    }
    return dot;
}

// epilogue of the projection modes (include/kge_hip.h): `v0` = fmaf(-2, dot, qn + en)
__device__ __forceinline__ float lp_epilogue_proj(int mode, float v0, float x, float y, float p, float z)
{
    float v;
    if (mode == KGE_LP_L2_PROJH) v = fmaf(x, fmaf(x, z, p), v0);
    else v = fmaf(y, fmaf(y, z, fmaf(2.0f, x, p)), v0);
    return -fmaxf(v, 0.0f);
}
__device__ __forceinline__ float lp_epilogue_any(const kge_lp_desc &d, float dot, int64_t i, int64_t c)
{
    if (d.mode == KGE_LP_DOT) return dot;
    const float v0 = fmaf(-2.0f, dot, d.qn[i] + d.en[c]);
    if (d.mode == KGE_LP_L2_EXPAND) return -fmaxf(v0, 0.0f);
    const float x = d.scal[d.r_idx[i] * d.scal_ld + c];
    const float y = d.mode == KGE_LP_L2_PROJD ? d.yc[c] : 0.f;
    return lp_epilogue_proj(d.mode, v0, x, y, d.Wq[i * d.ldw], d.Wq[i * d.ldw + 1]);
}

// ---- per-element terms of the group-of-four direct chains: L1, the torus modes and -- per PAIR of elements -- the complex
// modulus (include/kge_hip.h) ------------------------------------------------------------------------------------------
// x = q - t; every term is 0 at x = 0 (zero-filled padding k counts as nothing).  The compiler must not contract x * x
// into the following subtraction (-ffp-contract=off): 1 - v rounds the ROUNDED square, as torch's `1 - (a - b) ** 2`.
constexpr float KGE_TWO_PI_F = 6.2831855f;      // fp32(2 pi): the reference's `2 * pi * tmp` on an fp32 tensor
template <int MODE>
__device__ __forceinline__ float lp_direct_term(float x)
{
    static_assert(MODE != KGE_LP_CMOD, "the complex modulus is a term of a pair: lp_cmod_pair");
    if (MODE == KGE_LP_TORUS_L1) {
        const float a = fabsf(x);
        return fminf(a, 1.0f - a);
    } else if (MODE == KGE_LP_TORUS_L2) {
        const float v = x * x;
        return fminf(v, 1.0f - v);
    } else if (MODE == KGE_LP_TORUS_EL2) {
        const float u = fminf(x, 1.0f - x);
        return 1.0f - cosf(KGE_TWO_PI_F * u);
    }
    return fabsf(x);    // KGE_LP_L1_DIRECT
}
// KGE_LP_CMOD: the modulus of one complex coordinate, x = (re, im) of q - t stored interleaved.  sqrtf is the correctly
// rounded fp32 square root (hipcc's default); 0 at x = (0, 0), so an absent pair counts as nothing.
__device__ __forceinline__ float lp_cmod_pair(float xr, float xi) { return sqrtf(fmaf(xi, xi, xr * xr)); }
// what an aligned group of four k adds to the accumulator: the terms as a tree, or the two moduli of its two pairs
template <int MODE>
__device__ __forceinline__ float lp_direct_group(float x0, float x1, float x2, float x3)
{
    if constexpr (MODE == KGE_LP_CMOD) return lp_cmod_pair(x0, x1) + lp_cmod_pair(x2, x3);
    else return (lp_direct_term<MODE>(x0) + lp_direct_term<MODE>(x1)) + (lp_direct_term<MODE>(x2) + lp_direct_term<MODE>(x3));
}
// score from the accumulated terms (power-of-two scalings: exact, the same bits as scaling every term)
template <int MODE>
__device__ __forceinline__ float lp_direct_finish(float acc)
{
    if (MODE == KGE_LP_TORUS_L1) return -(2.0f * acc);
    if (MODE == KGE_LP_TORUS_L2) return -(4.0f * acc);
    if (MODE == KGE_LP_TORUS_EL2) return -(0.5f * acc);
    return -acc;
}
// one accumulator, one add per aligned group of four k, the group's terms summed as (m0 + m1) + (m2 + m3), absent k = 0
template <int MODE>
__device__ __forceinline__ float lp_group_chain(const float *q, const float *t, int K)
{
    float acc = 0.0f;
    for (int k = 0; k < K; k += 4) {
        float x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = k + e < K ? q[k + e] - t[k + e] : 0.0f;
        acc = acc + lp_direct_group<MODE>(x[0], x[1], x[2], x[3]);
    }
    return acc;
}

// score of query i against LOCAL candidate c, any mode (scalar reference path
// used by the pair / filter kernels; bit-identical to the tile kernels).
__device__ __forceinline__ float lp_pair_score(const kge_lp_desc &d, int64_t i, int64_t c)
{
    if (KGE_LP_IS_MFMA(d.mode)) {
        float acc = lp_chain_dot(d.A0 + i * d.lda0, d.T0 + c * d.ldt0, d.K0, 0.0f);
        if (d.K1 > 0) acc = lp_chain_dot(d.A1 + i * d.lda1, d.T1 + c * d.ldt1, d.K1, acc);
        return lp_epilogue_any(d, acc, i, c);
    }
    const float *q = d.A0 + i * d.lda0;
    const float *t = d.T0 + c * d.ldt0;
    switch (d.mode) {   // the torus modes and the complex modulus: no rank-1 term (kge_lp_desc_check)
    case KGE_LP_TORUS_L1: return lp_direct_finish<KGE_LP_TORUS_L1>(lp_group_chain<KGE_LP_TORUS_L1>(q, t, d.K0));
    case KGE_LP_TORUS_L2: return lp_direct_finish<KGE_LP_TORUS_L2>(lp_group_chain<KGE_LP_TORUS_L2>(q, t, d.K0));
    case KGE_LP_TORUS_EL2: return lp_direct_finish<KGE_LP_TORUS_EL2>(lp_group_chain<KGE_LP_TORUS_EL2>(q, t, d.K0));
    case KGE_LP_CMOD: return lp_direct_finish<KGE_LP_CMOD>(lp_group_chain<KGE_LP_CMOD>(q, t, d.K0));
    default: break;
    }
    float acc = 0.0f;
    const bool l1 = d.mode == KGE_LP_L1_DIRECT;
    const float a = d.Wq ? d.scal[c * d.scal_ld + (d.scal_ld > 1 ? d.r_idx[i] : 0)] : 0.0f;
    const float *w = d.Wq ? d.Wq + i * d.ldw : nullptr;
    if (l1) {   // one add per aligned 4-group of k, the group as (|d0|+|d1|)+(|d2|+|d3|), absent k = 0
        for (int k = 0; k < d.K0; k += 4) {
            float m[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float diff = 0.0f;
                if (k + e < d.K0) {
                    diff = q[k + e] - t[k + e];
                    if (w) diff = fmaf(a, w[k + e], diff);
                }
                m[e] = fabsf(diff);
            }
            acc = acc + ((m[0] + m[1]) + (m[2] + m[3]));
        }
    } else {
        for (int k = 0; k < d.K0; ++k) {
            float diff = q[k] - t[k];
            if (w) diff = fmaf(a, w[k], diff);
            acc = fmaf(diff, diff, acc);
        }
    }
    return -acc;
}

// tuning knob for experiments (env KGE_LP_TARGET_BLOCKS), default `dflt`
static inline int kge_env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

static inline int kge_lp_desc_check(const kge_lp_desc *d)
{
    if (!d) return KGE_EINVAL;
    if (d->mode < KGE_LP_DOT || d->mode > KGE_LP_CMOD) return KGE_EINVAL;
    if (d->B < 0 || d->N < 0 || d->K0 <= 0 || d->K1 < 0) return KGE_EINVAL;
    if (d->mode == KGE_LP_CMOD && (d->K0 & 1)) return KGE_EINVAL;       // rows of interleaved (re, im) pairs
    if (d->B == 0 || d->N == 0) return 0; // empty problem: nothing is dereferenced
    if (!d->A0 || !d->T0) return KGE_EINVAL;
    if (d->K1 > 0 && (!d->A1 || !d->T1)) return KGE_EINVAL;
    if (d->K1 > 0 && d->mode != KGE_LP_DOT) return KGE_EINVAL;
    if (d->mode == KGE_LP_L2_EXPAND && (!d->qn || !d->en)) return KGE_EINVAL;
    if (d->mode >= KGE_LP_TORUS_L1) return d->Wq ? KGE_EINVAL : 0;     // plain per-element chains, no rank-1 term
    if (d->mode == KGE_LP_L2_PROJH || d->mode == KGE_LP_L2_PROJD) {
        if (!d->qn || !d->en || !d->Wq || d->ldw < 2 || !d->scal || d->scal_ld < d->N || !d->r_idx) return KGE_EINVAL;
        if (d->mode == KGE_LP_L2_PROJD && !d->yc) return KGE_EINVAL;
        return 0;
    }
    if (d->Wq && (!d->scal || d->scal_ld < 1 || (d->scal_ld > 1 && !d->r_idx))) return KGE_EINVAL;
    if (d->Wq && d->mode < KGE_LP_L1_DIRECT) return KGE_EINVAL;
    return 0;
}

// ---- free-running one-product count kernel (lp_hi_stream.hip), launched by kge_lp_split_count ----------------------
struct kge_hi_stream_params {
    const char *Ef;             // candidates: FRAGMENT-MAJOR hi table [rows_p / 32][units_p][64 lanes][16 B] (kge_lp_hi_rows, frag = 1)
    const char *Qh;             // queries: planar hi operand [q_rows][q_row_bytes]
    int64_t q_row_bytes;
    int units, units_p;         // k16 units holding data / units per 32-row group of Ef
    int64_t rows_p;             // candidate rows of Ef (a multiple of 64)
    int64_t q_rows;             // rows of Qh (a multiple of 96)
    int64_t B;                  // queries (thr / raw_count are indexed by query)
    const float2 *thr;
    const float4 *thr4;         // projection modes: (a_lo, a_hi, p_i, z_i)
    const float *X;             // projection modes: X (n_rel, ldx)
    int64_t ldx;
    const int64_t *r_idx;
    const float *yc;
    int32_t *raw_count;
    int32_t *list;
    int32_t cap;
    int32_t *list_count;
    float *overflow;
    const int32_t *col_q;       // optional: column -> query id (< 0: padding)
    const int32_t *members;     // grouped launch (r06): [q_rows][sets] query ids (< 0: unused) -- Qh row = one column of up to `sets` queries
    int32_t *region_count;      // optional [q_panels * 3], zeroed: the list is cut into REGIONS of region_cap entries, one per
    int32_t region_cap;         // (panel, 32-query sub-tile); entries land in their query's region, list_count is not touched
    const int64_t *true_idx;    // optional: GLOBAL id of the entity whose exact score is the query's threshold s_true ...
    int64_t c_base;             // ... local candidate c is global entity c_base + c
    // filled by kge_hi_stream_launch
    int q_panels, c_tiles, qg;  // qg: panels interleaved under one candidate sweep (a power of two dividing the blocks per XCD)
    int64_t n_items;
    int panel_bytes;
};
int kge_hi_stream_max_units(void);
int kge_hi_stream_launch(kge_hi_stream_params p, int pm, int num_cus, hipStream_t s);
// ... and its chunked-panel form for rows too long for a resident panel (lp_hi_chunk.hip; PM = 0, one global list)
int kge_hi_chunk_supported(int units);
int kge_hi_chunk_launch(kge_hi_stream_params p, int num_cus, hipStream_t s);

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: remember what was set per device
// (`cache`: 16 zero-initialised ints owned by the launch site), not once per process.
static inline int kge_ensure_dyn_smem(const void *func, int smem, int *cache)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
    if (dev >= 0 && __atomic_load_n(&cache[dev], __ATOMIC_RELAXED) >= smem) return 0;
    hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0) __atomic_store_n(&cache[dev], smem, __ATOMIC_RELAXED);   // (racing first calls both set the attribute: idempotent)
    return 0;
}
