// Private to the four translation units of the certified f16-split prefilter -- lp_split_mfma.hip (error analysis,
// thresholds, count sweep), lp_split_operands.hip (operand preparation), lp_split_query.hip (fused query side),
// lp_split_recheck.hip (exact recheck): the tile geometry, THE definition of each error band (of the operands the bands
// certify: lp_operand_cells.h) and the fold of per-block maxima into the device scalars the bands read --
// the threshold kernel and the fused query pipelines call the same functions, so their thresholds agree bit for bit
// (tests/test_gpu_parity.py::test_pipeline_thresholds_equal_the_threshold_kernel_bit_for_bit).
#pragma once
#include "lp_operand_cells.h"
#ifndef KGE_BUILD_NO_SLP
#error "build with -fno-slp-vectorize -DKGE_BUILD_NO_SLP=1 (torchkge_amd/csrc/build.py): SLP-packed v_pk_fma_f32 with a lane-crossing op_sel misreads beside co-executing MFMAs (profiles/r06/slp_bisect.txt)"
#endif

namespace {

constexpr int TQ = 192, TC = 256;               // 256 accumulator registers leave hipcc no slack: 4 x 3 tiles
constexpr int GSETS = 4;                        // grouped columns: queries that share one query row (threshold sets per column)
constexpr int RR_ROWS = 32, RR_PANEL = 96;      // queries per region / per panel of the free-running sweep (lp_hi_stream.hip)

// Per-block maxima left as plain stores by a producer kernel (bmax[2][n]; no same-address atomics, no zero-fill) -> the
// two device scalars, folded into what those already hold (the guard vector is zeroed per evaluation, other shards may
// add): EVERY block of a 256-thread consumer reduces them on its way in and gets (max0, max1), block 0 stores the
// scalars.  s1 may be NULL: 0.  Values >= 0: ordered like their bits.  (A thread that reads a scalar after block 0 stored
// it folds the same maximum in again.)
__device__ __forceinline__ float2 split_fold_block_max2(const float *bmax, int n, float *s0, float *s1)
{
    __shared__ unsigned fold2[8];
    unsigned m0 = 0u, m1 = 0u;
    for (int j = threadIdx.x; j < n; j += 256) {
        m0 = max(m0, __float_as_uint(bmax[j]));
        m1 = max(m1, __float_as_uint(bmax[n + j]));
    }
    m0 = wave_max_u32(m0);
    m1 = wave_max_u32(m1);
    if ((threadIdx.x & 63) == 0) { fold2[threadIdx.x >> 6] = m0; fold2[4 + (threadIdx.x >> 6)] = m1; }
    __syncthreads();
    m0 = max(max(fold2[0], fold2[1]), max(fold2[2], fold2[3]));
    m1 = max(max(fold2[4], fold2[5]), max(fold2[6], fold2[7]));
    const float v0 = __uint_as_float(max(m0, __float_as_uint(*s0)));
    const float v1 = s1 ? __uint_as_float(max(m1, __float_as_uint(*s1))) : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *s0 = v0;
        if (s1) *s1 = v1;
    }
    return make_float2(v0, v1);
}
// ... of one array bmax[n] into one scalar
__device__ __forceinline__ float split_fold_block_max(const float *bmax, int n, float *s)
{
    __shared__ unsigned fold1[4];
    unsigned m = 0u;
    for (int j = threadIdx.x; j < n; j += 256) m = max(m, __float_as_uint(bmax[j]));
    const float v = __uint_as_float(max(block_max_u32(m, fold1), __float_as_uint(*s)));
    if (blockIdx.x == 0 && threadIdx.x == 0) *s = v;
    return v;
}

// One step of the per-query magnitude sum: prefix += cell sum;  amag += sqrt(prefix * e2pref[u])
__device__ __forceinline__ void split_amag_step(float &prefix, float &amag, float ss, float e2u)
{
    prefix = prefix + ss;
    amag = amag + sqrtf(prefix * e2u);
}

// ---- the error bands: ONE definition each, called by split_thr_kernel and by the fused query pipelines -----------------
// The count kernel reads "v >= a_lo" off the sign of v - a_lo, which is wrong only for v = -0, a_lo = +0:
// a zero threshold is moved down to the next normal number (widening the band is always safe).
__device__ __forceinline__ float split_nonzero_lo(float lo) { return lo == 0.f ? -1.17549435e-38f : lo; }

// amag: the sum over the k16 units of the bound on the accumulator's magnitude in that unit (split_amag_step,
// times 1.003 for the cross terms and f16 roundings), or < 0 when the prefix norms are not at hand: every unit is
// then charged with the full ||q|| ||e||.
__device__ __forceinline__ float split_acc_err(float amag, float aug_mag, float mag, int units, float c_acc,
                                               float adds_per_unit = 48.0f)
{
    const float two24 = 5.9604645e-8f;
    const float sum_mag = amag >= 0.f ? amag * 1.003f + aug_mag : (float)units * mag;
    return c_acc * adds_per_unit * two24 * sum_mag;  // 48 (one-product level: 16) additions per unit, each within c_acc * 2^-24 of the magnitude
}
// Rounding error of the exact fp32 chain the counts are defined by: one fmaf rounding per element, each within
// 2^-24 of the partial sum it produces (running error bound) -- 16 per unit against the same prefix magnitudes,
// or gamma_K * ||q|| ||e|| without them.
__device__ __forceinline__ float split_chain_err(float amag, float mag, int K)
{
    const float two24 = 5.9604645e-8f;
    return amag >= 0.f ? 16.16f * two24 * amag * 1.003f : 1.01f * (float)K * two24 * mag;
}

// ONE-PRODUCT level (LV = 1 of the count kernel): acc = sum_k qh*eh (+ the two-term augmentation column), i.e. the
// split residual is no longer 3 * 2^-22 of the magnitude but the operands' own f16 rounding residuals,
//     q.e - qh.eh = dq.e + qh.de,    |.| <= ||dq|| ||e|| + ||qh|| ||de||,   ||qh|| <= ||q|| + ||dq||,
// with dq = q - hi(q) MEASURED per query (dq2 = ||dq||^2, exact differences summed in fp32) and de2m >= max_c ||de_c||^2:
// ~4.7e-4 of ||q|| max||e|| at K = 200 (a third of the candidates' values round up, a third down ...), 8 x the band of the
// three-product sweep -- which buys one MFMA per k16 unit instead of three and half the operand bytes.  The augmentation
// column -||e||^2/2 rides as TWO columns (hi, lo: residual 2^-22); the accumulation term has 16 additions per unit.
__device__ __forceinline__ float split_hi_resid(float qnrm, float enrm, float em_aug, float dq2, float de2m)
{
    const float two22 = 2.3841858e-7f;
    const float dqn = sqrtf(dq2) * 1.0001f, den = sqrtf(de2m) * 1.0001f;
    return (dqn * enrm + (qnrm + dqn) * den) * 1.0005f + 1.01f * two22 * em_aug;
}

// Band of the L2 expansion, unscaled: (mid, hw) -- count c iff v_c <= u = -st, v = ||q||^2 + ||e||^2 - 2 q.e, i.e. iff
// q.e - ||e_c||^2/2 >= mid = (||q||^2 - u)/2, known to within hw.  level 0: three products, amag as split_acc_err's;
// level 1: one product, the residuals dq2, de2m.  The projection modes add their own term to hw (split_thr_kernel).
__device__ __forceinline__ float2 split_band_l2(int level, float q, float st, float em, int K, int units, float c_acc,
                                                float eps_scale, float amag, float dq2, float de2m)
{
    const float two22 = 2.3841858e-7f;
    const float eps_rel = 3.01f * two22;             // split residual
    const float enrm = sqrtf(em) * 1.000001f, qnrm = sqrtf(q) * 1.000001f;
    const float u = -st;
    const float mag = qnrm * enrm + 0.5f * em;       // >= sum of |products|
    const float eps_dot = level == 1
        ? split_acc_err(-1.0f, 0.5f * em, mag, units, c_acc, 16.0f) + split_chain_err(-1.0f, mag, K) +
          split_hi_resid(qnrm, enrm, 0.5f * em, dq2, de2m) + 2.5e-7f * (qnrm + enrm) + 4e-9f
        : split_acc_err(amag, 0.5f * em, mag, units, c_acc) + split_chain_err(amag, mag, K) + eps_rel * mag +
          2.5e-7f * (qnrm + enrm) + 4e-9f;
    const float eps_v = (2.0f * eps_dot + 4.0f * two22 * (q + em + fabsf(u))) * eps_scale;
    const float mid = 0.5f * (q - u);
    const float hw = 0.5f * eps_v + two22 * (fabsf(q) + fabsf(u));
    return make_float2(mid, hw);
}

// (a_lo, a_hi) = mid -+ hw of a band (mid, hw), scaled like the accumulators of the L2 operands
__device__ __forceinline__ float2 split_thr_pack_l2(float2 band)
{
    const float out_scale = (float)(1 << SPLIT_SCALE_LOG2) * (float)(1 << SPLIT_SCALE_LOG2);
    return make_float2(split_nonzero_lo((band.x - band.y) * out_scale), (band.x + band.y) * out_scale);
}

__device__ __forceinline__ float2 split_thr_l2(float q, float st, float em, int K, int units, float c_acc, float eps_scale,
                                               float amag)
{
    return split_thr_pack_l2(split_band_l2(0, q, st, em, K, units, c_acc, eps_scale, amag, 0.f, 0.f));
}

__device__ __forceinline__ float2 split_thr_l2_hi(float q, float st, float em, int K, int units, float c_acc, float eps_scale,
                                                  float dq2, float de2m)
{
    return split_thr_pack_l2(split_band_l2(1, q, st, em, K, units, c_acc, eps_scale, -1.0f, dq2, de2m));
}

// thresholds of one DOT query on the one-product level, operand scales s_q (its own) and s_e
__device__ __forceinline__ float2 split_thr_dot_hi(float q, float st, float em, int K, int units, float c_acc, float eps_scale,
                                                   float dq2, float de2m, float qm, float s_q, float s_e)
{
    const float two22 = 2.3841858e-7f;
    const float enrm = sqrtf(em) * 1.000001f, qnrm = sqrtf(q) * 1.000001f;
    const float out_scale = s_q * s_e;
    const float sqk = sqrtf((float)K);
    const float eps_abs = 1.4901161e-8f * sqk * (sqrtf(qm) * enrm + sqrtf(em) * qnrm) + 1e-30f;
    const float eps_dot = (split_acc_err(-1.0f, 0.f, qnrm * enrm, units, c_acc, 16.0f) + split_chain_err(-1.0f, qnrm * enrm, K) +
                           split_hi_resid(qnrm, enrm, 0.f, dq2, de2m) + eps_abs) * eps_scale;
    const float hw = eps_dot + two22 * fabsf(st);
    return make_float2(split_nonzero_lo((st - hw) * out_scale), (st + hw) * out_scale);
}

int split_num_cus()
{
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            n = prop.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

} // namespace
