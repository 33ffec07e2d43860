// Certified f16-split prefilter for the fused rank count (gfx950).
//
// The rank of a test fact only needs  #{c : s[i,c] >= s_true[i]}  (get_rank,
// utils/operations.py:37-61), not the scores.  For TransE-L2 through the norm
// expansion  s = -max(||q||^2 + ||e||^2 - 2 q.e, 0)  the comparison
// s[i,c] >= s_true[i] is  q.e - ||e_c||^2/2 >= (||q_i||^2 + s_true_i)/2 ;
// for DistMult / ComplEx (KGE_LP_DOT, K = K0 + K1 columns) it is  q.e >= s_true_i.
// This file evaluates the left side APPROXIMATELY on the f16 matrix cores
// (16x the fp32 MFMA rate) with a rigorous error bound eps_i:
//
//   x  = hi + lo + rho,  hi = f16(x), lo = f16(x - hi), |rho| <= 2^-22 |x|
//   q.e ~ sum_k  qh*eh + qh*el + ql*eh          (3 v_mfma_f32_32x32x16_f16, fp32 accumulate)
//
// and classifies every (query, candidate) pair against two per-query thresholds:
//   acc >= a_hi : certainly counted          acc < a_lo : certainly not counted
//   a_lo <= acc < a_hi : UNCERTAIN -> appended to a list and re-scored by the
//   exact scalar chain (lp_pair_exact.h: lp_pair_score_staged, bit-identical to the
//   fp32 MFMA tile kernel and to oracle/kge_oracle.c).
// raw_count[i] first receives #{acc >= a_lo}; kge_lp_split_recheck then takes 1
// off for every listed pair whose exact score is below s_true.  The resulting
// counts are therefore EXACTLY those of kge_lp_count_ge -- integer work stays
// bit-exact -- while ~99.9% of the pairs never touch the fp32 pipe.
//
// Error bound used for the thresholds (split_thr_kernel), per unit of
// P >= sum_k |q_k e_k| (+ |augmentation term|), P = ||q|| * max||e|| (+ max||e||^2 / 2):
//   split residual   3 * 2^-22            (ql*el dropped, rho_q*e, q*rho_e)
//   accumulation     c_acc * n_terms * 2^-24  (n_terms = 3 * 16 * units products; c_acc = 2 covers any fp32
//                                          adder, rounding or truncating, in any order; 1.25 when the
//                                          device passed kge_mfma_f16_selftest, measured 9/8)
//   exact chain      K * 2^-24            (the scalar fmaf chain it is compared with)
// plus absolute
// terms for f16 subnormal lo parts (flushed or not) and for the roundings of
// the threshold arithmetic itself.  tools/probe/mfma_probe.hip measures what the
// MFMA really does (two passes of acc + 8 products, addends truncated 24 bits
// below the largest, one RNE rounding; subnormals kept): <= 9 * 2^-24 per pass,
// inside the assumption.  tests/test_gpu_parity.py checks the counts against the
// exact kernel, also with the band shrunk 16x.
//
// Data layout: a split operand is [rows_p][units_p] cells of 64 bytes,
//   cell = [hi k0..7][hi k8..15][lo k0..7][lo k8..15]   (f16, k within the 16-unit)
// rows_p = rows rounded up to the tile (256 candidates / 192 queries; zero rows),
// units_p = k16 units rounded up to 2; one extra column carries the augmentation
// (L2: 1 for queries, -||e||^2/2 for candidates; DOT: a per-query guard value
// against 0); padding candidates hold -65504 there and can never count.  L2
// operands are scaled by 2^12 (|x| <= 4 is implied by the evaluator's norm guard,
// L2_EXPAND_LIMIT), DOT operands by a power of two derived on the device from
// the squared-norm maxima (split_scale).
//
// Kernel: block tile 256 candidates (MFMA rows) x 192 queries (MFMA columns =
// lanes), 8 waves of 64 x 96 (2x3 tiles of 32x32: 96 accumulator VGPRs, two waves
// per SIMD -- accumulators stay in architectural VGPRs, which the VALU epilogue
// can compare directly; AGPR accumulators would cost a v_accvgpr_read each).
// K is staged 32 at a time into double-buffered LDS by LDS-DMA
// (global_load_lds_dwordx4, pieces issued between the MFMA groups) with an XOR
// swizzle (16-byte chunk c of row r sits at chunk c ^ ((r>>1)&7)): the fragment
// ds_read_b128 are bank-conflict free without padding.  Queries on the lane axis
// make thresholds and counters per-lane constants, so the epilogue is two
// compares and an add-with-carry per element.
//
// This file: the thresholds (split_thr_kernel) and the count sweep.  The other stages: lp_split_operands.hip (operand
// preparation), lp_split_query.hip (fused query side), lp_split_recheck.hip (exact recheck); lp_split_common.h holds
// the tile geometry and the one definition of each error band.
#include "lp_split_common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int NT = 3;                           // 32x32 query tiles per wave (2 wave columns)
constexpr int E_STAGE_BYTES = TC * 128;         // candidate operand, one stage (2 k16 units)
constexpr int Q_STAGE_BYTES = TQ * 128;
constexpr int STAGE_BYTES = E_STAGE_BYTES + Q_STAGE_BYTES;
constexpr int UNC_CAP = 2048;                   // uncertain pairs buffered per tile
// + per-panel (thr4, X row) of the projection modes, or the (a_lo, a_hi) sets + counters of a grouped panel
constexpr int SMEM_BYTES = 2 * STAGE_BYTES + 16 + UNC_CAP * 4 + TQ * 20 + TQ * GSETS * 12 + 16;

struct SplitParams {
    const char *Es, *Qs;  // split operands
    int row_bytes;        // units_p * 64
    int units;            // k16 units holding data (MFMA work)
    int stages;           // units_p / 2
    int64_t B, N;
    const float2 *thr;    // (a_lo, a_hi) per padded query, scaled like the accumulators
    const float4 *thr4;   // projection modes: (a_lo, a_hi, p_i, z_i) per padded query
    const float *X;       // projection modes: X (n_rel, ldx), ldx % 4 == 0, readable up to the padded tile edge
    int64_t ldx;
    const int64_t *r_idx; // row of X per query
    const float *yc;      // PROJD: y_c per (padded) candidate
    int32_t *raw_count;
    int32_t *list;        // cap x (query, candidate)
    int32_t cap;
    int32_t *list_count;  // device scalar
    float *overflow;      // set to 1 when a buffer or the list overflowed
    // Columns instead of queries (queries that share a key share the query ROW: its accumulators are computed once).
    // col_q: column -> query id (< 0: padding column) for a launch whose columns carry ONE query each (NULL: column
    // == query); members: [column][GSETS] query ids (< 0: unused set) for the grouped launch (template GS > 0).
    const int32_t *col_q, *members;
    int q_panels, c_tiles;
    int qg;               // query panels interleaved under one sweep of the candidate tiles (work order)
    int64_t n_items;
    int dbg;              // env KGE_SPLIT_DBG (timing probes, wrong results): 1 no global loads, 4 no epilogue,
                          // 16 no LDS fragment reads, 32 no barriers, 128 every block streams tile (0,0),
                          // 1024 hi*hi product only (one-product first level), 2048 half of the LDS-DMA pieces,
                          // 4096 (LV = 1) cycle stamps of the stage phases into the head of the pair list
                          // (a planar hi table would move half the bytes)
};

// Self-test of the accumulation model behind c_acc = 1.25 (tools/probe/mfma_probe.hip is the long
// version): v_mfma_f32_32x32x16_f16 computes each output as two passes  acc <- acc + sum of 8 products,
// the 9 addends of a pass aligned to the largest exponent and truncated (toward zero) 24 bits below
// it, the sum exact, one round-to-nearest-even at the end; f16 subnormal inputs are kept.  Hence at
// most 9 * 2^-24 * |running magnitude| of error per 8 products.  The vectors below tell this model
// apart from sequential fp32 adds, from wider / narrower alignment and from other roundings.
__global__ void mfma_selftest_kernel(const float *__restrict__ ab, const float *__restrict__ c, float *out, int n)
{
    const int lane = threadIdx.x, half = lane >> 5;
    for (int t = 0; t < n; ++t) {
        f16x8 fa, fb;
        for (int j = 0; j < 8; ++j) {
            fa[j] = (_Float16)ab[t * 32 + half * 8 + j];
            fb[j] = (_Float16)ab[t * 32 + 16 + half * 8 + j];
        }
        f32x16 acc;
        for (int r = 0; r < 16; ++r) acc[r] = c[t];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc, 0, 0, 0);
        if (lane == 0) out[t] = acc[0];
    }
}

struct SplitThrParams {
    int mode;                       // KGE_LP_L2_EXPAND or KGE_LP_DOT
    const float *qn0, *qn1;         // per-query squared norms (segment 1 optional)
    const float *s_true;
    const float *qmax0, *qmax1;     // device scalars (DOT: scale of the query operand)
    const float *emax0, *emax1;     // device scalars: max ||e||^2 per segment
    int64_t B, Bp;
    int K, units;
    float eps_scale;
    float2 *thr;
    int32_t *list_count;
    float *overflow;
    const float *pz;                // projection modes: (p_i, z_i) pairs, stride ldw
    int64_t ldw;
    const float *xabsmax, *yabsmax; // device scalars >= max |X|, max |y_c|
    float4 *thr4;
    float c_acc;                    // accumulation-error coefficient per product (2: any adder; 1.25: measured model)
    int K0;                         // columns of the first K-segment (K - K0 of the second)
    const float *q_cell_ss;         // optional [units_p][ss_ld] cell sums of the queries (kge_lp_split_rows) ...
    const int64_t *ss_index;        // ... read at column ss_index[i] instead of i (query columns); ss_ld = their row stride
    int64_t ss_ld;
    const float *e2pref;            // ... and prefix squared-norm maxima of the candidates (kge_lp_split_prefix_max)
    int units_p;
    int level;                      // 1: thresholds of the one-product sweep (q_dn2, de2max; L2_EXPAND and DOT modes)
    const float *q_dn2;             // ||q_i - hi(q_i)||^2, read at q_dn2_index[i] when given (query columns)
    const int64_t *q_dn2_index;
    const float *de2max;            // device scalar >= max_c ||e_c - hi(e_c)||^2
    const float *tp_bmax;           // optional [2][tp_blocks]: block maxima left by kge_lp_table_prep_l2 (emax0, de2max): folded
    int tp_blocks;                  // into the two scalars by every block on its way in, stored by block 0
    float *emax_out, *de2max_out;
    int32_t *zero_i32;              // optional: zero_n int32 zeroed by this launch (the region counters of the sweep's list)
    int zero_n;
    int q_scale_per_query;          // DOT, level 1: the query operand of row i is scaled by split_scale(||q_i||^2), its own norm
                                    // (kge_lp_dot_query_pipeline), not by the batch maximum's; qn0 then holds the total
};

__global__ void split_thr_kernel(const SplitThrParams p)
{
    const float two24_c = 5.9604645e-8f;
    const float two22 = 2.3841858e-7f;
    float em, de2m = 0.f;
    if (p.tp_bmax) {        // (as query_pipeline_kernel: the table preparation's per-block maxima -> the two scalars)
        __shared__ unsigned red[8];
        unsigned m0 = 0u, m1 = 0u;
        for (int j = threadIdx.x; j < p.tp_blocks; j += blockDim.x) {
            m0 = max(m0, __float_as_uint(p.tp_bmax[j]));
            m1 = max(m1, __float_as_uint(p.tp_bmax[p.tp_blocks + j]));
        }
        for (int off = 32; off > 0; off >>= 1) {
            m0 = max(m0, (unsigned)__shfl_xor((int)m0, off, 64));
            m1 = max(m1, (unsigned)__shfl_xor((int)m1, off, 64));
        }
        const int wv_ = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { red[wv_] = m0; red[4 + wv_] = m1; }
        __syncthreads();
        m0 = max(max(red[0], red[1]), max(red[2], red[3]));
        m1 = max(max(red[4], red[5]), max(red[6], red[7]));
        em = __uint_as_float(max(m0, __float_as_uint(*p.emax0)));
        de2m = __uint_as_float(max(m1, p.de2max ? __float_as_uint(*p.de2max) : 0u));
        __syncthreads();
        if (blockIdx.x == 0 && threadIdx.x == 0) { *p.emax_out = em; if (p.de2max_out) *p.de2max_out = de2m; }
    } else {
        em = *p.emax0 + (p.emax1 ? *p.emax1 : 0.f);
        if (p.level == 1) de2m = *p.de2max;
    }
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < p.zero_n; j += gridDim.x * blockDim.x) p.zero_i32[j] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *p.list_count = 0;
        // non-finite norms (diverged embeddings): f16 operands would hold inf / NaN and the
        // comparisons would silently fail -- hand the count back to the exact fp32 path
        const float qm = p.qmax0 ? *p.qmax0 + (p.qmax1 ? *p.qmax1 : 0.f) : 0.f;
        if (!(em < INFINITY) || !(qm < INFINITY)) *p.overflow = 1.0f;
    }
    // accumulation: 48*units fp32 additions, c_acc = 2 (adders that truncate instead of rounding, any order)
    // or 1.25 when kge_mfma_f16_selftest confirmed the measured behaviour (<= 9/8 per product, see below);
    // exact chain: K fmaf roundings (gamma_K <= 1.01 K u); split residual 3 * 2^-22 * (1 + 2^-10)
    const float eps_rel = 3.01f * two22;             // split residual
    const float enrm = sqrtf(em) * 1.000001f;
    const bool have_pref = p.q_cell_ss && p.e2pref;
    // two K-segments whose first is not a multiple of 8 long: the exact chain's 8-blocks of the second segment
    // straddle the k16 cells, a partial sum may reach one cell ahead of its own -- one more full magnitude
    // covers the 16 roundings per unit that are then charged to the earlier (smaller) prefix
    const float straddle = (have_pref && p.K0 % 8 != 0 && p.K0 < p.K) ? 16.16f * two24_c : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.Bp; i += (int64_t)gridDim.x * blockDim.x) {
        if (i >= p.B) {
            if (p.mode >= KGE_LP_L2_PROJH) p.thr4[i] = make_float4(INFINITY, INFINITY, 0.f, 0.f);
            else p.thr[i] = make_float2(INFINITY, INFINITY);
            continue;
        }
        const float q = p.qn0[i] + (p.qn1 ? p.qn1[i] : 0.f);
        const float qnrm = sqrtf(q) * 1.000001f;
        float amag = -1.0f;
        if (have_pref) {
            float prefix = 0.f;
            amag = 0.f;
            for (int u = 0; u < p.units; ++u) split_amag_step(prefix, amag, p.q_cell_ss[(int64_t)u * p.ss_ld + (p.ss_index ? p.ss_index[i] : i)], p.e2pref[u]);
        }
        const float dq2 = p.level == 1 ? p.q_dn2[p.q_dn2_index ? p.q_dn2_index[i] : i] : 0.f;
        if (p.mode == KGE_LP_L2_EXPAND && p.level == 1) {
            p.thr[i] = split_thr_l2_hi(q, p.s_true[i], em, p.K, p.units, p.c_acc, p.eps_scale, dq2, de2m);
        } else if (p.mode == KGE_LP_L2_EXPAND) {
            p.thr[i] = split_thr_l2(q, p.s_true[i], em, p.K, p.units, p.c_acc, p.eps_scale, amag);
        } else if (p.mode >= KGE_LP_L2_PROJH) {
            const float2 b = split_band_l2(p.level, q, p.s_true[i], em, p.K, p.units, p.c_acc, p.eps_scale, amag, dq2, de2m);
            // + the projection term corr = x (x z + p)  resp.  y (y z + 2 g + p): it is computed exactly in fp32
            // by both paths but enters in a different association -> a few ulps of its largest possible size
            const float pi = p.pz[i * p.ldw], zi = p.pz[i * p.ldw + 1];
            // |X[r_i, c]| = |w_i . e_c| <= ||w_i|| max||e||  (Cauchy-Schwarz; ||w_i||^2 = z_i + 2 for TransH, z_i for TransD) when
            // no measured maximum is given: the term below is 2^-22 of cmax, a looser bound costs nothing
            const float wn2 = p.mode == KGE_LP_L2_PROJH ? zi + 2.0f : zi;
            const float xm = p.xabsmax ? *p.xabsmax : sqrtf(fmaxf(wn2, 0.f) * em) * 1.000001f;
            const float ym = p.mode == KGE_LP_L2_PROJD ? *p.yabsmax : 0.f;
            const float cmax = p.mode == KGE_LP_L2_PROJH ? xm * (xm * fabsf(zi) + fabsf(pi))
                                                         : ym * (ym * fabsf(zi) + 2.0f * xm + fabsf(pi));
            const float2 t = split_thr_pack_l2(make_float2(b.x, b.y + (8.0f * two22 * cmax * p.eps_scale + two22 * cmax)));
            p.thr4[i] = make_float4(t.x, t.y, pi, zi);
        } else if (p.level == 1) {
            // count c iff dot_c >= s_true; both operands carry their own power-of-two scale
            const float qm = p.q_scale_per_query ? q : *p.qmax0 + (p.qmax1 ? *p.qmax1 : 0.f);
            p.thr[i] = split_thr_dot_hi(q, p.s_true[i], em, p.K, p.units, p.c_acc, p.eps_scale, dq2, de2m, qm, split_scale(qm),
                                        split_scale(em));
        } else {
            // ... on three products: the one copy of this band (prefix magnitudes, the straddle term; per-query scales
            // exist on the one-product level only, kge_lp_split_count checks)
            const float qm = *p.qmax0 + (p.qmax1 ? *p.qmax1 : 0.f);
            const float out_scale = split_scale(qm) * split_scale(em);
            const float st = p.s_true[i];
            const float sqk = sqrtf((float)p.K);
            const float eps_abs = 1.4901161e-8f * sqk * (sqrtf(qm) * enrm + sqrtf(em) * qnrm) + 1e-30f;
            const float eps_dot = (split_acc_err(amag, 0.f, qnrm * enrm, p.units, p.c_acc) +
                                   split_chain_err(amag, qnrm * enrm, p.K) + straddle * qnrm * enrm +
                                   eps_rel * qnrm * enrm + eps_abs) * p.eps_scale;
            const float hw = eps_dot + two22 * fabsf(st);
            p.thr[i] = make_float2(split_nonzero_lo((st - hw) * out_scale), (st + hw) * out_scale);
        }
    }
}

// ---- the count kernel --------------------------------------------------------
// GS > 0: GROUPED columns -- every column (one split query row) carries up to GS queries that share the row but
// have their own true entity, hence their own thresholds: the MFMA sweep runs once per column, the epilogue once
// per (column, set); thresholds and counters of the panel's sets live in LDS.
// LV = 1: the ONE-PRODUCT level.  Operands are PLANAR hi tables (kge_lp_hi_rows: 32 bytes per k16 unit), a 128-byte stage
// row holds FOUR units, and a stage is four MFMA groups qh*eh instead of 2 x 3 -- a third of the matrix work and half
// the operand bytes per (pair, unit); same tile, same LDS-DMA staging and swizzle, same epilogue against thresholds
// that carry the operands' measured f16 residuals (split_thr_l2_hi).  p.units / p.stages then count hi units / 4-unit stages.
template <int NWAVES, bool DBG, int PM, int GS = 0, int LV = 0>   // PM: 0 plain thresholds, 1 TransH projection term, 2 TransD
__global__ __launch_bounds__(64 * NWAVES, 1) void lp_split_count_kernel(const SplitParams p)
{
    static_assert(GS == 0 || GS == GSETS, "grouped columns carry GSETS threshold sets");
    const int dbg = DBG ? p.dbg : 0;                                // probes compile away in the product kernel
    constexpr int NTHREADS = 64 * NWAVES;
    constexpr int MT = TC / 32 / (NWAVES / 2);                      // 32x32 candidate tiles per wave
    constexpr int EJ = TC * 8 / NTHREADS, QJ = TQ * 8 / NTHREADS;   // staged 16-byte chunks per thread
    constexpr int SROWS = NTHREADS / 8;                             // rows covered by one staging pass
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *unc_cnt = reinterpret_cast<int *>(smem + 2 * STAGE_BYTES);
    unsigned *unc_list = reinterpret_cast<unsigned *>(smem + 2 * STAGE_BYTES + 16);
    float4 *pthr = reinterpret_cast<float4 *>(smem + 2 * STAGE_BYTES + 16 + UNC_CAP * 4);   // PM: per query of the panel
    int *prow = reinterpret_cast<int *>(pthr + TQ);
    float2 *gthr = reinterpret_cast<float2 *>(prow + TQ);                  // GS: [set][TQ] thresholds ...
    int *gcnt = reinterpret_cast<int *>(gthr + (GS ? GS : 1) * TQ);         // ... [set][TQ] counters ...
    int *gsets = gcnt + (GS ? GS : 1) * TQ;                                 // ... and the number of sets in use
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: the LDS-DMA targets become SALU arithmetic)
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;   // waves: (NWAVES/2) x 2

    // Work order.  The (query panel, candidate tile) items are listed with QG (= p.qg: 4 or 16) query panels
    // interleaved under a sweep of the candidate tiles:  (g*4+0, ct) (g*4+1, ct) .. (g*4+3, ct)
    // (g*4+0, ct+1) ...;  XCD x (the blocks with bid % 8 == x, one per CU) owns an eighth of the
    // list and its blocks take the positions  start + loc, start + loc + nbx, ...  So at any moment
    // the ~32 CUs that share an L2 work on 4 query panels x 8 candidate tiles: every split row
    // that enters the L2 is used by 8 (queries) or 4 (candidates) CUs before it is evicted, and a
    // block stays on one query panel for a whole sweep (its rank counters live in registers).
    const int QG = p.qg;
    const int nb = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, loc = bid >> 3;
    const int nbx = (nb - xcd + 7) >> 3;                                   // blocks on this XCD
    const int nx = nb < 8 ? nb : 8;                                        // XCD slots in use
    const int64_t x_begin = p.n_items * xcd / nx, x_end = p.n_items * (xcd + 1) / nx;
    const int64_t item_begin = x_begin + loc;
    const int nitems = item_begin < x_end ? (int)((x_end - item_begin + nbx - 1) / nbx) : 0;
    if (nitems <= 0) return;
    const int per_group = QG * p.c_tiles, n_groups = (p.q_panels + QG - 1) / QG;
    auto item_qp_ct = [&](int i, int &qp, int &ct) __attribute__((always_inline)) {   // i-th item of this block
        const int idx = (int)item_begin + i * nbx;
        const int grp = min(idx / per_group, n_groups - 1);
        const int r = idx - grp * per_group, gsz = min(QG, p.q_panels - grp * QG);
        ct = r / gsz;
        qp = grp * QG + (r - ct * gsz);
    };
    const int S = p.stages, G = nitems * S;
    if (tid == 0) { *unc_cnt = 0; if (GS) *gsets = 0; }
    if (GS) __syncthreads();

    // staging: 8 lanes cover one 128-byte row segment of a stage
    const int srow = tid >> 3, scs = tid & 7;
    const int sch = scs ^ ((srow >> 1) & 7);        // global chunk that lands in LDS chunk slot scs
    const int64_t rstep = (int64_t)SROWS * p.row_bytes;
    static_assert(EJ == 4 && QJ == 3, "the stage body below places 4 + 3 LDS-DMA pieces per wave");
    int pf_it = 0, pf_s = 0;
    const char *pfE = nullptr, *pfQ = nullptr;
    auto pf_new_item = [&]() __attribute__((always_inline)) {
        int qp, ct;
        item_qp_ct(pf_it, qp, ct);
        if (dbg & 128) qp = ct = 0;     // every block streams tile (0,0): cache-ceiling probe
        const int64_t q0 = (int64_t)qp * TQ, c0 = (int64_t)ct * TC;
        pfE = p.Es + (c0 + srow) * p.row_bytes + sch * 16;
        pfQ = p.Qs + (q0 + srow) * p.row_bytes + sch * 16;
    };
    // global -> LDS directly (LDS-DMA, 1 KiB per wave-instruction: the 64 lanes' 16-byte pieces land
    // at consecutive LDS addresses, which is exactly this wave's 8 rows x 128 bytes of the stage)
    auto dma = [&](const char *g, char *l) __attribute__((always_inline)) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                         (__attribute__((address_space(3))) void *)l, 16, 0, 0);
    };

    // fragment addressing: row r of a tile, chunk (u*4 + piece*2 + half) ^ ((r>>1)&7)
    const int sw = (l31 >> 1) & 7;
    const int a_row = (wr * (MT * 32) + l31) * 128;
    const int b_row = E_STAGE_BYTES + (wc * 96 + l31) * 128;
    // byte addresses inside a stage of this lane's fragments: [k16 unit][hi / lo]
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
    unsigned a_off[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) a_off[u][pc] = lds0 + a_row + ((u * 4 + pc * 2 + half) ^ sw) * 16;
    unsigned h_off[4];      // LV = 1: the hi fragment of unit j of a stage is chunk 2 j + half
#pragma unroll
    for (int j = 0; j < 4; ++j) h_off[j] = lds0 + a_row + ((j * 2 + half) ^ sw) * 16;
    // the query fragments sit a wave-uniform distance behind the candidate fragments (scalar register)
    const unsigned b_delta = __builtin_amdgcn_readfirstlane(b_row - a_row);

    f32x16 acc[MT][NT];
    int cnt[NT] = {0, 0, 0};
    float alo[NT] = {0.f, 0.f, 0.f}, ahi[NT] = {0.f, 0.f, 0.f};
    auto load_panel = [&](int64_t q0) __attribute__((always_inline)) {
        if (GS) {   // thresholds of every (column, set) of the panel + zeroed counters; sets in use (block-wide max)
            int used = 0;
            for (int idx = tid; idx < TQ * GS; idx += NTHREADS) {
                const int c = idx / GS, gs = idx - c * GS;
                const int q = p.members[(q0 + c) * GS + gs];
                float2 t = make_float2(INFINITY, INFINITY);
                if (q >= 0) {
                    if (PM) { const float4 t4 = p.thr4[q]; t = make_float2(t4.x, t4.y); }
                    else t = p.thr[q];
                }
                gthr[gs * TQ + c] = t;
                gcnt[gs * TQ + c] = 0;
                if (q >= 0) used = max(used, gs + 1);
                if (PM && gs == 0) {    // the queries of a column share the key, hence relation and projection scalars
                    pthr[c] = q >= 0 ? p.thr4[q] : make_float4(INFINITY, INFINITY, 0.f, 0.f);
                    prow[c] = (int)p.r_idx[max(q, 0)];
                }
            }
            if (used > 0) atomicMax(gsets, used);
            return;
        }
        if (PM) {   // thresholds + projection scalars + X row of the panel's queries live in LDS
            if (tid < TQ) {
                const int64_t q = p.col_q ? (int64_t)p.col_q[q0 + tid] : q0 + tid;
                pthr[tid] = q >= 0 ? p.thr4[q] : make_float4(INFINITY, INFINITY, 0.f, 0.f);
                prow[tid] = (int)p.r_idx[min(max(q, (int64_t)0), p.B - 1)];
            }
            return;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int64_t col = q0 + wc * 96 + nt * 32 + l31;
            const int64_t q = p.col_q ? (int64_t)p.col_q[col] : col;
            const float2 t = q >= 0 ? p.thr[q] : make_float2(INFINITY, INFINITY);
            alo[nt] = t.x;
            ahi[nt] = t.y;
        }
    };
    auto flush_counts = [&](int64_t q0) __attribute__((always_inline)) {
        if (GS) {   // (same idx -> thread mapping as load_panel: a thread flushes and re-zeroes its own entries)
            for (int idx = tid; idx < TQ * GS; idx += NTHREADS) {
                const int c = idx / GS, gs = idx - c * GS;
                const int q = p.members[(q0 + c) * GS + gs];
                const int v = gcnt[gs * TQ + c];
                if (q >= 0 && v != 0) atomicAdd(&p.raw_count[q], v);
            }
            __syncthreads();
            if (tid == 0) *gsets = 0;
            __syncthreads();
            return;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int v = cnt[nt] + __shfl_xor(cnt[nt], 32, 64);
            const int64_t col = q0 + wc * 96 + nt * 32 + l31;
            const int64_t q = p.col_q ? (int64_t)p.col_q[col] : col;
            if (half == 0 && v != 0 && q >= 0 && q < p.B) atomicAdd(&p.raw_count[q], v);
            cnt[nt] = 0;
        }
    };

    int64_t cur_q0;
    {
        int qp, ct;
        item_qp_ct(0, qp, ct);
        cur_q0 = (int64_t)qp * TQ;
    }
    load_panel(cur_q0);
    pf_new_item();
    {   // stage 0 of the first tile
        char *nE = smem + wid * 1024, *nQ = nE + E_STAGE_BYTES;
#pragma unroll
        for (int j = 0; j < EJ; ++j) dma(pfE + j * rstep, nE + j * SROWS * 128);
#pragma unroll
        for (int j = 0; j < QJ; ++j) dma(pfQ + j * rstep, nQ + j * SROWS * 128);
        if (++pf_s == S) {
            pf_s = 0;
            if (++pf_it < nitems) pf_new_item();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();

    // Fragment loads are inline asm with hand-placed waits: hipcc tracks the LDS-DMA instructions as
    // FLAT accesses, after which every lgkmcnt wait it inserts is a full drain -- it then waits for the
    // fragment loads it has just issued (before MFMAs that do not use them) instead of letting them
    // fly under the next MFMA group.  KGE_SWAIT ties the registers to the wait, so no use can move above it.
    static_assert(MT == 2 && NT == 3, "KGE_SLOAD / KGE_SWAIT are written out for 2 x 3 tiles per wave");
#define KGE_DSR(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:" #OFF : "=v"(DST) : "v"(ADDR) : "memory")
#define KGE_SLOAD(AH, AL, BH, BL, BASE, U)                                                          \
    {                                                                                               \
        const unsigned ah_ = (BASE) + a_off[U][0], al_ = (BASE) + a_off[U][1];                      \
        const unsigned bh_ = ah_ + b_delta, bl_ = al_ + b_delta;                                    \
        KGE_DSR(AH[0], ah_, 0); KGE_DSR(BH[0], bh_, 0); KGE_DSR(AH[1], ah_, 4096);                  \
        KGE_DSR(BH[1], bh_, 4096); KGE_DSR(BH[2], bh_, 8192);                                       \
        KGE_DSR(BL[0], bl_, 0); KGE_DSR(BL[1], bl_, 4096); KGE_DSR(BL[2], bl_, 8192);               \
        KGE_DSR(AL[0], al_, 0); KGE_DSR(AL[1], al_, 4096);                                          \
        /* the address registers stay live past the last load: no destination may be allocated on them */ \
        asm volatile("" :: "v"(ah_), "v"(al_), "v"(bh_), "v"(bl_));                                 \
    }
#define KGE_SWAIT(AH, AL, BH, BL)                                                                   \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(AH[0]), "+v"(AH[1]), "+v"(AL[0]), "+v"(AL[1]),      \
                 "+v"(BH[0]), "+v"(BH[1]), "+v"(BH[2]), "+v"(BL[0]), "+v"(BL[1]), "+v"(BL[2]) :: "memory");
#define KGE_HLOAD(AH, BH, BASE, J) /* LV = 1: the hi fragments of unit J of the stage at BASE */     \
    {                                                                                               \
        const unsigned ah_ = (BASE) + h_off[J];                                                     \
        const unsigned bh_ = ah_ + b_delta;                                                         \
        KGE_DSR(AH[0], ah_, 0); KGE_DSR(BH[0], bh_, 0); KGE_DSR(AH[1], ah_, 4096);                  \
        KGE_DSR(BH[1], bh_, 4096); KGE_DSR(BH[2], bh_, 8192);                                       \
        asm volatile("" :: "v"(ah_), "v"(bh_));                                                     \
    }
#define KGE_HWAIT(AH, BH)                                                                           \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(AH[0]), "+v"(AH[1]), "+v"(BH[0]), "+v"(BH[1]), "+v"(BH[2]) :: "memory");
#define KGE_SMMA_P(A, B, C) /* one of the three split products over the wave's MT x NT tiles, given C */ \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                               \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                           \
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[mt], B[nt], C, 0, 0, 0);
#define KGE_SMMA_PA(A, B)                                                                           \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                               \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                           \
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[mt], B[nt], acc[mt][nt], 0, 0, 0);

    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
    f16x8 zero8;
#pragma unroll
    for (int r = 0; r < 8; ++r) zero8[r] = (_Float16)0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = zero16;

    f16x8 ah0[MT], al0[MT], bh0[NT], bl0[NT], ah1[MT], al1[MT], bh1[NT], bl1[NT];
    if (LV == 1) { KGE_HLOAD(ah0, bh0, 0u, 0) } else { KGE_SLOAD(ah0, al0, bh0, bl0, 0u, 0) }
    int it = 0, s = 0;
    // probe 4096 (DBG kernel, LV = 1): cycle stamps of the phases of the first KGE_TL_STAGES stages of block 0, waves 0 and 4
    // (partners on one SIMD), written to the head of the pair list (combine with 64: no list flush) -- tools/split_timeline.py
    constexpr int KGE_TL_STAGES = 48;
    unsigned long long tsv[16];
#define KGE_TS(I) if (DBG && tl) tsv[I] = __builtin_readcyclecounter();
    for (int g = 0; g < G; ++g) {
        const bool tl = DBG && LV == 1 && (dbg & 4096) && bid == 0 && (wid == 0 || wid == 4) && g < KGE_TL_STAGES;
        const int buf = g & 1;
        const bool more = g + 1 < G;
        const unsigned sb = buf * STAGE_BYTES, sb_next = (buf ^ 1) * STAGE_BYTES;
        const int nunits = min(2, p.units - 2 * s);
        const bool two = nunits == 2;              // the last stage of a tile may hold a single k16 unit
        // In the product kernel the LDS-DMA pieces are issued unconditionally (after the block's last
        // stage they re-fetch valid rows into the buffer nobody reads): a branch around them makes
        // hipcc drain lgkmcnt to 0 at the join, i.e. wait for the fragment loads it just issued.
        const bool pf = DBG ? (more && !(dbg & 1)) : true;
        // LDS-DMA of the next stage into the other buffer, one piece at a time between the MFMA
        // groups: an LDS-DMA instruction holds the issuing wave for 60+ cycles, which hides behind
        // matrix work only if the pieces are spread over the stage (and the other wave of the SIMD
        // is in its MFMAs)
        char *nE = smem + (buf ^ 1) * STAGE_BYTES + wid * 1024, *nQ = nE + E_STAGE_BYTES;
        const char *gE = pfE + pf_s * 128, *gQ = pfQ + pf_s * 128;

        // (grouped columns: on a tile's last stage the next stage's first fragments are fetched AFTER the multi-pass
        // epilogue -- their registers are what its temporaries need; the LDS buffer stays valid through the next stage)
        const bool defer_frag = GS != 0 && s == S - 1;
        if constexpr (LV == 1) {
            // ONE product per k16 unit, four units per stage: [u0] dma E0 E1 | frag u1 [u1] dma E2 E3 | frag u2 [u2] dma Q |
            // frag u3 -- barrier -- frag u0 of the next stage [u3].  Every fragment overwrite has an LDS wait (or an MFMA
            // group) between it and the MFMAs that last read those registers.
            const int nu = min(4, p.units - 4 * s);
            const bool frag = !DBG || !(dbg & 16);      // (probe: no fragment loads after the first)
            const char *gE1 = gE + rstep;
            KGE_TS(0)
            KGE_HWAIT(ah0, bh0)
            KGE_TS(1)
            if (s == 0) { KGE_SMMA_P(ah0, bh0, zero16) } else { KGE_SMMA_PA(ah0, bh0) }
            __builtin_amdgcn_sched_barrier(0);
            KGE_TS(2)
            if (pf) { dma(gE, nE); dma(gE1, nE + SROWS * 128); }
            __builtin_amdgcn_sched_barrier(0);
            KGE_TS(3)
            if (frag) { KGE_HLOAD(ah1, bh1, sb, 1) }
            asm volatile("" :: "v"(gE), "v"(gE1));
            __builtin_amdgcn_sched_barrier(0);
            KGE_TS(4)
            KGE_HWAIT(ah1, bh1)
            KGE_TS(5)
            if (nu > 1) { KGE_SMMA_PA(ah1, bh1) }
            __builtin_amdgcn_sched_barrier(0);
            KGE_TS(6)
            if (pf) { dma(gE + 2 * rstep, nE + 2 * SROWS * 128); dma(gE + 3 * rstep, nE + 3 * SROWS * 128); }
            __builtin_amdgcn_sched_barrier(0);
            KGE_TS(7)
            if (frag) { KGE_HLOAD(ah0, bh0, sb, 2) }
            __builtin_amdgcn_sched_barrier(0);
            KGE_HWAIT(ah0, bh0)
            KGE_TS(8)
            if (nu > 2) { KGE_SMMA_PA(ah0, bh0) }
            __builtin_amdgcn_sched_barrier(0);
            KGE_TS(9)
            if (pf) { dma(gQ, nQ); dma(gQ + rstep, nQ + SROWS * 128); dma(gQ + 2 * rstep, nQ + 2 * SROWS * 128); }
            if (more && pf) {
                if (++pf_s == S) {
                    pf_s = 0;
                    if (++pf_it < nitems) pf_new_item();
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            KGE_TS(10)
            if (frag) { KGE_HLOAD(ah1, bh1, sb, 3) }
            __builtin_amdgcn_sched_barrier(0);
            KGE_HWAIT(ah1, bh1)
            KGE_TS(11)
            if (!DBG || !(dbg & 512)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's pieces of the next stage landed in LDS
            KGE_TS(12)
            if (!DBG || !(dbg & 32)) __syncthreads();
            KGE_TS(13)
            if (more && !defer_frag && frag) { KGE_HLOAD(ah0, bh0, sb_next, 0) }
            __builtin_amdgcn_sched_barrier(0);
            if (nu > 3) { KGE_SMMA_PA(ah1, bh1) }
            __builtin_amdgcn_sched_barrier(0);
            KGE_TS(14)
        } else {
            // (this stage's first k16 fragments were fetched behind the previous stage's barrier, below)
            KGE_SWAIT(ah0, al0, bh0, bl0)
            if (s == 0) { KGE_SMMA_P(ah0, bh0, zero16) } else { KGE_SMMA_PA(ah0, bh0) }
            __builtin_amdgcn_sched_barrier(0);
            const char *gE1 = gE + rstep;
            if (pf) { dma(gE, nE); dma(gE1, nE + SROWS * 128); }
            __builtin_amdgcn_sched_barrier(0);
            if (!(dbg & 16) || g == 0) { KGE_SLOAD(ah1, al1, bh1, bl1, sb, 1) }
            // (hipcc would drain lgkmcnt before a fragment load whose destination reuses the address
            // registers of an LDS-DMA still in flight: keep those registers occupied until here)
            asm volatile("" :: "v"(gE), "v"(gE1));
            __builtin_amdgcn_sched_barrier(0);
            const bool hi1 = DBG && (dbg & 1024), halfdma = DBG && (dbg & 2048);
            if (!hi1) { KGE_SMMA_PA(ah0, bl0) }
            __builtin_amdgcn_sched_barrier(0);
            if (pf && !halfdma) { dma(gE + 2 * rstep, nE + 2 * SROWS * 128); dma(gE + 3 * rstep, nE + 3 * SROWS * 128); }
            __builtin_amdgcn_sched_barrier(0);
            if (!hi1) { KGE_SMMA_PA(al0, bh0) }
            __builtin_amdgcn_sched_barrier(0);
            if (pf) { dma(gQ, nQ); if (!halfdma) { dma(gQ + rstep, nQ + SROWS * 128); dma(gQ + 2 * rstep, nQ + 2 * SROWS * 128); } }
            if (more && pf) {
                if (++pf_s == S) {
                    pf_s = 0;
                    if (++pf_it < nitems) pf_new_item();
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            KGE_SWAIT(ah1, al1, bh1, bl1)
            if (two) { KGE_SMMA_PA(ah1, bh1) }
            __builtin_amdgcn_sched_barrier(0);
            // The stage's last two MFMA groups run BEHIND the barrier, next to the fetch of the next
            // stage's first fragments: right after a barrier all 8 waves read LDS at once (80 KB), and
            // without matrix work in flight the MFMA pipe would idle for that long.
            if (!(dbg & 512)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the next stage landed in LDS
            if (dbg & 512) __builtin_amdgcn_s_barrier();   // probe: barrier without waiting for the DMA pieces
            else if (!(dbg & 32)) __syncthreads();
            if (more && !(dbg & 16) && !defer_frag) { KGE_SLOAD(ah0, al0, bh0, bl0, sb_next, 0) }
            __builtin_amdgcn_sched_barrier(0);
            if (two && !hi1) { KGE_SMMA_PA(ah1, bl1) }
            __builtin_amdgcn_sched_barrier(0);
            if (two && !hi1) { KGE_SMMA_PA(al1, bh1) }
            __builtin_amdgcn_sched_barrier(0);

        }

        const bool tile_done = s == S - 1;
        if (tile_done && !(dbg & 4)) {
            int qp_cur, ct;
            item_qp_ct(it, qp_cur, ct);
            const int64_t c0 = (int64_t)ct * TC;
            // opaque to the optimiser: otherwise the ~100 list-entry constants below are
            // hoisted out of the tile loop and held in registers across the MFMA stream
            int cl_base = wr * (MT * 32) + 4 * half, ql_base = wc * 96 + l31;
            asm volatile("" : "+v"(cl_base), "+v"(ql_base));
            if (GS) {
                // Grouped columns: the accumulators of a column are compared with the thresholds of each of its
                // queries in turn (block-uniform number of sets; the accumulators stay intact, w lives in temporaries).
                const int nsets = *gsets;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int ql = ql_base + nt * 32;
                    if (PM) {   // acc <- acc - 2^23 * corr once per element: the corrected value serves every set
                        const float4 t4 = pthr[ql];
                        const float p_n = t4.z, z_n = t4.w;
                        const float *xrow = p.X + (int64_t)prow[ql] * p.ldx + c0 + wr * (MT * 32) + 4 * half;
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            float4 x4[4], y4[4];
#pragma unroll
                            for (int g4 = 0; g4 < 4; ++g4) {
                                x4[g4] = *reinterpret_cast<const float4 *>(xrow + mt * 32 + 8 * g4);
                                if (PM == 2)
                                    y4[g4] = *reinterpret_cast<const float4 *>(p.yc + c0 + wr * (MT * 32) + 4 * half + mt * 32 + 8 * g4);
                            }
#pragma unroll
                            for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    const float xe = e == 0 ? x4[g4].x : (e == 1 ? x4[g4].y : (e == 2 ? x4[g4].z : x4[g4].w));
                                    float corr;
                                    if (PM == 1) {
                                        corr = xe * fmaf(xe, z_n, p_n);
                                    } else {
                                        const float ye = e == 0 ? y4[g4].x : (e == 1 ? y4[g4].y : (e == 2 ? y4[g4].z : y4[g4].w));
                                        corr = ye * fmaf(ye, z_n, fmaf(2.0f, xe, p_n));
                                    }
                                    acc[mt][nt][g4 * 4 + e] = fmaf(corr, -8388608.0f, acc[mt][nt][g4 * 4 + e]);
                                }
                        }
                    }
                    for (int gs = 0; gs < nsets; ++gs) {
                        const float2 th = gthr[gs * TQ + ql];
                        const f32x2 nlo2 = {-th.x, -th.x};
                        const float hwf = th.y - th.x;
                        const unsigned hwb = hwf >= 0.f ? __float_as_uint(hwf) : 0u;
                        unsigned smask = 0u;
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                            for (int g4 = 0; g4 < 4; ++g4) {
                                const f32x2 w01 = (f32x2){acc[mt][nt][g4 * 4 + 0], acc[mt][nt][g4 * 4 + 1]} + nlo2;
                                const f32x2 w23 = (f32x2){acc[mt][nt][g4 * 4 + 2], acc[mt][nt][g4 * 4 + 3]} + nlo2;
                                const unsigned b0 = __float_as_uint(w01.x), b1 = __float_as_uint(w01.y);
                                const unsigned b2 = __float_as_uint(w23.x), b3 = __float_as_uint(w23.y);
                                smask = __builtin_amdgcn_alignbit(smask, b0, 31);
                                smask = __builtin_amdgcn_alignbit(smask, b1, 31);
                                smask = __builtin_amdgcn_alignbit(smask, b2, 31);
                                smask = __builtin_amdgcn_alignbit(smask, b3, 31);
                                const unsigned mq = min(min(min(b0, b1), b2), b3);
                                if (__ballot(mq <= hwb)) {
#define KGE_GLIST(BITS, E)                                                                              \
    if ((BITS) <= hwb) {                                                                                \
        const int idx = atomicAdd(unc_cnt, 1);                                                          \
        if (idx < UNC_CAP)                                                                              \
            unc_list[idx] = ((unsigned)(cl_base + mt * 32 + (E) + 8 * g4) << 10) | ((unsigned)gs << 8) | (unsigned)ql; \
    }
                                    KGE_GLIST(b0, 0) KGE_GLIST(b1, 1) KGE_GLIST(b2, 2) KGE_GLIST(b3, 3)
#undef KGE_GLIST
                                }
                                __builtin_amdgcn_sched_barrier(0);   // one quad at a time: its temporaries die here
                            }
                        }
                        // the two lane halves hold the two row halves of the same column
                        int v = 32 - __popc(smask);
                        v += __shfl_xor(v, 32, 64);
                        if (half == 0 && v != 0) atomicAdd(&gcnt[gs * TQ + ql], v);
                    }
                }
            }
#pragma unroll
            for (int nt = 0; nt < (GS ? 0 : NT); ++nt) {
                float lo_n = alo[nt], hi_n = ahi[nt], p_n = 0.f, z_n = 0.f;
                const float *xrow = nullptr;
                if (PM) {
                    const int ql = wc * 96 + nt * 32 + l31;
                    const float4 t4 = pthr[ql];
                    lo_n = t4.x; hi_n = t4.y; p_n = t4.z; z_n = t4.w;
                    xrow = p.X + (int64_t)prow[ql] * p.ldx + c0 + wr * (MT * 32) + 4 * half;
                }
                asm volatile("" : "+v"(lo_n), "+v"(hi_n));   // (keeps the derived constants out of the MFMA loop's registers)
                const f32x2 nlo2 = {-lo_n, -lo_n};
                // band width as bits; padding queries carry a_lo = a_hi = +inf (inf - inf = NaN, of either sign):
                // width 0 there, so that none of their pairs can be listed
                const float hwf = hi_n - lo_n;
                const unsigned hwb = hwf >= 0.f ? __float_as_uint(hwf) : 0u;
                unsigned smask = 0u;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    float4 x4[4], y4[4];
                    if (PM) {   // the 4 quads' gathers X[r_i, c..c+3] (and y_c) issued together
#pragma unroll
                        for (int g4 = 0; g4 < 4; ++g4) {
                            x4[g4] = *reinterpret_cast<const float4 *>(xrow + mt * 32 + 8 * g4);
                            if (PM == 2)
                                y4[g4] = *reinterpret_cast<const float4 *>(p.yc + c0 + wr * (MT * 32) + 4 * half + mt * 32 + 8 * g4);
                        }
                    }
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {   // 4 accumulator registers = rows 8*g4 + 4*half + {0..3}
                        float vq[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            vq[e] = acc[mt][nt][g4 * 4 + e];
                            if (PM) {   // acc - 2^23 * corr: the comparison of v = qn + en - 2 dot + corr against u
                                const float xe = e == 0 ? x4[g4].x : (e == 1 ? x4[g4].y : (e == 2 ? x4[g4].z : x4[g4].w));
                                float corr;
                                if (PM == 1) {
                                    corr = xe * fmaf(xe, z_n, p_n);
                                } else {
                                    const float ye = e == 0 ? y4[g4].x : (e == 1 ? y4[g4].y : (e == 2 ? y4[g4].z : y4[g4].w));
                                    corr = ye * fmaf(ye, z_n, fmaf(2.0f, xe, p_n));
                                }
                                vq[e] = fmaf(corr, -8388608.0f, vq[e]);
                            }
                        }
                        // 2.25 VALU per element instead of 3 VALU + 2 SALU (compare / add-with-carry /
                        // compare / mask logic): w = v - a_lo as packed f32 adds; the SIGN bits of the 32
                        // w's of this lane's query are shifted into one register (v >= a_lo  <=>  sign clear:
                        // a float subtraction never gets the sign wrong, and a_lo is never +-0) and counted
                        // with one popcount per 32 elements; a pair is uncertain (a_lo <= v < a_hi) only if
                        // 0 <= w <= fl(a_hi - a_lo) -- rounding is monotonic -- i.e. iff the bits of w,
                        // read as unsigned, are <= those of the band width: one unsigned min3 + min per quad.
                        const f32x2 w01 = (f32x2){vq[0], vq[1]} + nlo2, w23 = (f32x2){vq[2], vq[3]} + nlo2;
                        const unsigned b0 = __float_as_uint(w01.x), b1 = __float_as_uint(w01.y);
                        const unsigned b2 = __float_as_uint(w23.x), b3 = __float_as_uint(w23.y);
                        smask = __builtin_amdgcn_alignbit(smask, b0, 31);
                        smask = __builtin_amdgcn_alignbit(smask, b1, 31);
                        smask = __builtin_amdgcn_alignbit(smask, b2, 31);
                        smask = __builtin_amdgcn_alignbit(smask, b3, 31);
                        const unsigned mq = min(min(min(b0, b1), b2), b3);
                        const unsigned long long any = __ballot(mq <= hwb);
                        // (w replaces v in the accumulator registers -- they are dead after the epilogue, the next
                        // tile starts from C = 0 -- so the epilogue needs no registers of its own)
                        acc[mt][nt][g4 * 4 + 0] = w01.x; acc[mt][nt][g4 * 4 + 1] = w01.y;
                        acc[mt][nt][g4 * 4 + 2] = w23.x; acc[mt][nt][g4 * 4 + 3] = w23.y;
                        if (any) { // some lane holds an uncertain pair among these 4 rows: list them
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                // 0 <= w <= fl(a_hi - a_lo): every pair of the band, and only counted pairs
                                if (__float_as_uint(acc[mt][nt][g4 * 4 + e]) <= hwb) {
                                    const int cl = cl_base + mt * 32 + e + 8 * g4;
                                    const int idx = atomicAdd(unc_cnt, 1);
                                    if (idx < UNC_CAP)
                                        unc_list[idx] = ((unsigned)cl << 8) | (unsigned)(ql_base + nt * 32);
                                }
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);   // one quad at a time: its temporaries die here
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                cnt[nt] += 32 - __popc(smask);      // the 32 elements (2 tiles x 16) of this lane's query
            }
            __syncthreads();
            if (wid == 0 && !(dbg & 64)) { // hand this tile's uncertain pairs to the global list
                const int n = *unc_cnt;
                const int nc = min(n, UNC_CAP);
                if (n > 0) {
                    int base = 0;
                    // (a degenerate all-tied model can push the counter past 2^31: positions are compared as
                    // unsigned, so nothing is ever written outside the list, and the sticky overflow flag makes
                    // the caller redo the count on the exact kernel)
                    if (lane == 0) base = atomicAdd(p.list_count, nc);
                    base = __shfl(base, 0, 64);
                    if (n > UNC_CAP && lane == 0) *p.overflow = 1.0f;
                    for (int i = lane; i < nc; i += 64) {
                        const unsigned e = unc_list[i];
                        const int pos = base + i;
                        if ((unsigned)pos < (unsigned)p.cap) {
                            // (grouped: [cl:8][set:2][column:8]; columns with one query: [cl][column:8], via col_q if given)
                            int32_t qid;
                            if (GS) qid = p.members[(cur_q0 + (e & 255u)) * GS + ((e >> 8) & 3u)];
                            else qid = p.col_q ? p.col_q[cur_q0 + (e & 255u)] : (int32_t)(cur_q0 + (e & 255u));
                            // (one 8-byte store per pair: consecutive lanes fill consecutive entries)
                            reinterpret_cast<int2 *>(p.list)[pos] = make_int2(qid, (int32_t)(c0 + (e >> (GS ? 10 : 8))));
                        } else {
                            *p.overflow = 1.0f;
                        }
                    }
                    if (lane == 0) *unc_cnt = 0;
                }
            }
            if (GS && more && !(dbg & 16)) {
                if (LV == 1) { KGE_HLOAD(ah0, bh0, sb_next, 0) } else { KGE_SLOAD(ah0, al0, bh0, bl0, sb_next, 0) }
            }
            if (more) { // query panel change (block-uniform): flush counters, load the next thresholds
                int qp_next, ct_next;
                item_qp_ct(it + 1, qp_next, ct_next);
                const int64_t next_q0 = (int64_t)qp_next * TQ;
                if (next_q0 != cur_q0) {
                    flush_counts(cur_q0);
                    cur_q0 = next_q0;
                    load_panel(cur_q0);
                }
            }
        }
        if (DBG && tl) {
            tsv[15] = __builtin_readcyclecounter();     // (behind the epilogue of a tile's last stage)
            if (lane == 0) {
                unsigned long long *o = reinterpret_cast<unsigned long long *>(p.list) + ((wid >> 2) * KGE_TL_STAGES + g) * 16;
#pragma unroll
                for (int i = 0; i < 16; ++i) o[i] = tsv[i];
            }
        }
        if (++s == S) { s = 0; ++it; }
    }
#undef KGE_TS
#undef KGE_SMMA_PA
#undef KGE_SMMA_P
#undef KGE_HLOAD
#undef KGE_HWAIT
#undef KGE_SLOAD
#undef KGE_SWAIT
#undef KGE_DSR
    flush_counts(cur_q0);
}

template <int NWAVES, bool DBG, int PM, int GS = 0, int LV = 0>
int launch_split(const SplitParams &p, int grid, hipStream_t s)
{
    auto k = lp_split_count_kernel<NWAVES, DBG, PM, GS, LV>;
    static int attr_dev[16];    // per instantiation, per device
    if (int e = kge_ensure_dyn_smem(reinterpret_cast<const void *>(k), SMEM_BYTES, attr_dev)) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(64 * NWAVES), SMEM_BYTES, s, p);
    KGE_CHECK_LAUNCH();
    return 0;
}

// The 14 instantiations: level x threshold form (pm: 0 plain, 1 TransH, 2 TransD) x plain / grouped columns (gs: 0 or
// GSETS), and the probe kernel (dbg) of the plain per-query sweep at both levels.
int launch_split_for(int pm, int gs, bool lv1, bool dbg, const SplitParams &p, int grid, hipStream_t s)
{
    if (dbg && pm == 0 && gs == 0) return lv1 ? launch_split<8, true, 0, 0, 1>(p, grid, s) : launch_split<8, true, 0, 0, 0>(p, grid, s);
    switch (pm + (gs ? 3 : 0) + (lv1 ? 6 : 0)) {
    case 0: return launch_split<8, false, 0, 0, 0>(p, grid, s);
    case 1: return launch_split<8, false, 1, 0, 0>(p, grid, s);
    case 2: return launch_split<8, false, 2, 0, 0>(p, grid, s);
    case 3: return launch_split<8, false, 0, GSETS, 0>(p, grid, s);
    case 4: return launch_split<8, false, 1, GSETS, 0>(p, grid, s);
    case 5: return launch_split<8, false, 2, GSETS, 0>(p, grid, s);
    case 6: return launch_split<8, false, 0, 0, 1>(p, grid, s);
    case 7: return launch_split<8, false, 1, 0, 1>(p, grid, s);
    case 8: return launch_split<8, false, 2, 0, 1>(p, grid, s);
    case 9: return launch_split<8, false, 0, GSETS, 1>(p, grid, s);
    case 10: return launch_split<8, false, 1, GSETS, 1>(p, grid, s);
    case 11: return launch_split<8, false, 2, GSETS, 1>(p, grid, s);
    }
    return KGE_EINVAL;
}

} // namespace

extern "C" int kge_lp_split_count(const kge_lp_desc *d, const kge_split_args *a, const float *s_true,
                                  int32_t *raw_count, kge_stream_t stream)
{
    int rc = kge_lp_desc_check(d);
    if (rc) return rc;
    if (!KGE_LP_IS_MFMA(d->mode)) return KGE_EINVAL;
    const bool proj = d->mode >= KGE_LP_L2_PROJH;
    if (d->B == 0 || d->N == 0) return 0;
    if (proj && (!a || (d->mode == KGE_LP_L2_PROJD && !a->yabsmax) || d->scal_ld % 4 != 0 ||
                 !kge_aligned16(d->scal)))
        return KGE_EINVAL;
    if (!a || !a->Qs || !a->Es || !s_true || !a->emax0 || !a->thr || !raw_count || !a->list || a->cap <= 0 ||
        !a->list_count || !a->overflow)
        return KGE_EINVAL;
    const bool pq = a->q_scale_per_query != 0;     // (DOT, one-product level: per-query operand scales, qn0 = the total norm)
    if (pq && (d->mode != KGE_LP_DOT || a->level != 1 || !a->qn0)) return KGE_EINVAL;
    if (d->mode == KGE_LP_DOT && !pq && (!a->qn0 || !a->qmax0 || (d->K1 > 0 && (!a->qn1 || !a->qmax1 || !a->emax1))))
        return KGE_EINVAL;
    if (d->mode == KGE_LP_DOT && d->K1 > 0 && !a->emax1) return KGE_EINVAL;
    if (d->B > INT32_MAX || d->N > INT32_MAX) return KGE_EINVAL;
    if (a->level != 0 && a->level != 1) return KGE_EINVAL;
    const bool lv1 = a->level == 1;     // one-product level: planar hi operands, plain thresholds
    if (lv1 && !a->thr_ready && (!a->q_dn2 || !a->de2max)) return KGE_EINVAL;
    hipStream_t s = kge_s(stream);
    const int K = d->K0 + d->K1;
    const int units_p = lv1 ? kge_lp_hi_units(K) : kge_lp_split_units(K, 1);
    const int units = lv1 ? (K + 2 + 15) / 16 : (K + 1 + 15) / 16;
    const int64_t Bp = kge_lp_split_rows_padded(d->B, 1);
    SplitThrParams t;
    t.mode = d->mode;
    t.qn0 = d->mode != KGE_LP_DOT ? d->qn : a->qn0;
    t.qn1 = (d->mode == KGE_LP_DOT && d->K1 > 0 && !pq) ? a->qn1 : nullptr;
    t.s_true = s_true;
    t.qmax0 = a->qmax0; t.qmax1 = (d->K1 > 0 && !pq) ? a->qmax1 : nullptr;
    t.q_scale_per_query = pq ? 1 : 0;
    // (thresholds recomputed = another sweep on these operands: the list's region counters start from zero like *list_count)
    t.zero_i32 = a->region_count; t.zero_n = a->region_count ? kge_lp_split_regions(d->B) : 0;
    t.emax0 = a->emax0; t.emax1 = (d->mode == KGE_LP_DOT && d->K1 > 0) ? a->emax1 : nullptr;
    t.B = d->B; t.Bp = Bp; t.K = K; t.units = units;
    t.eps_scale = a->eps_scale;
    t.thr = reinterpret_cast<float2 *>(a->thr);
    t.thr4 = reinterpret_cast<float4 *>(a->thr);
    t.pz = d->Wq; t.ldw = d->ldw;
    t.xabsmax = a->xabsmax; t.yabsmax = a->yabsmax;
    t.c_acc = a->accum_model == 1 ? 1.25f : 2.0f;
    t.q_cell_ss = a->q_cell_ss; t.e2pref = a->e2pref; t.units_p = units_p; t.K0 = d->K0;
    t.ss_index = a->q_cell_ss_index; t.ss_ld = a->q_cell_ss_index ? a->q_cell_ss_ld : Bp;
    if (a->q_cell_ss_index && a->q_cell_ss_ld <= 0) return KGE_EINVAL;
    t.level = a->level; t.q_dn2 = a->q_dn2; t.q_dn2_index = a->q_dn2_index; t.de2max = a->de2max;
    t.tp_bmax = a->tp_block_max; t.tp_blocks = a->tp_blocks;
    t.emax_out = const_cast<float *>(a->emax0); t.de2max_out = const_cast<float *>(a->de2max);
    if (a->tp_block_max && (a->tp_blocks <= 0 || a->emax1 || a->thr_ready)) return KGE_EINVAL;
    if (lv1) { t.q_cell_ss = nullptr; t.e2pref = nullptr; }
    t.list_count = a->list_count;
    t.overflow = a->overflow;
    if (!a->thr_ready) {    // (the fused query pipeline has already written thr and zeroed list_count)
        hipLaunchKernelGGL(split_thr_kernel, dim3((int)((Bp + 255) / 256)), dim3(256), 0, s, t);
        KGE_CHECK_LAUNCH();
    }

    const void *Es = a->Es, *Qs = a->Qs;
    float *thr = a->thr, *overflow = a->overflow;
    int32_t *list = a->list, *list_count = a->list_count;
    const int32_t cap = a->cap;
    SplitParams p;
    p.Es = reinterpret_cast<const char *>(Es);
    p.Qs = reinterpret_cast<const char *>(Qs);
    p.row_bytes = lv1 ? units_p * 32 : units_p * 64;
    p.units = units;
    p.stages = lv1 ? units_p / 4 : units_p / 2;
    p.B = d->B;
    p.N = d->N;
    p.thr = reinterpret_cast<const float2 *>(thr);
    p.thr4 = reinterpret_cast<const float4 *>(thr);
    p.X = d->scal; p.ldx = d->scal_ld; p.r_idx = d->r_idx; p.yc = d->yc;
    p.raw_count = raw_count;
    p.list = list;
    p.cap = cap;
    p.list_count = list_count;
    p.overflow = overflow;
    p.col_q = nullptr; p.members = nullptr;
    p.c_tiles = (int)((d->N + TC - 1) / TC);
    p.dbg = kge_env_int("KGE_SPLIT_DBG", 0);
    // Query panels interleaved under one sweep of the candidate tiles (work order, see the kernel).  Measured r03
    // (profiles/r03/split_work_order_sweep.txt): at K = 200 (172 KiB per panel) 16 panels per XCD cut the L2-miss
    // traffic from 646 to 295 MB per evaluate and are ~0.5 % FASTER in the sustained, power-capped state (4: 0.819,
    // 8: 0.812, 16: 0.807 ms per evaluate; 32 thrashes the 4 MiB L2 slice); at K = 400 (320 KiB per panel) 4 / 8 / 16
    // are within noise with 4 ahead -> 16 while 16 panels stay below ~3 MiB, else 4.
    p.qg = kge_env_int("KGE_SPLIT_QG", (int64_t)TQ * p.row_bytes * 16 <= (3 << 20) ? 16 : 4);
    const int slots = split_num_cus();
    const int pm = d->mode == KGE_LP_L2_PROJH ? 1 : (d->mode == KGE_LP_L2_PROJD ? 2 : 0);      // threshold form of the epilogue
    if (a->es_frag) {
        // the free-running one-product kernel (lp_hi_stream.hip): fragment-major candidate table, resident query panel
        // long rows: the panel streamed in chunks (lp_hi_chunk.hip)
        const bool chunked = units > kge_hi_stream_max_units();
        const bool grouped = a->members && a->n_multi_p > 0;         // r06: + a second launch over the grouped columns
        if (!lv1 || (chunked && !kge_hi_chunk_supported(units))) return KGE_EINVAL;
        if ((a->members != nullptr) != (a->n_multi_p > 0) || (grouped && (chunked || proj || a->region_count || !a->col_q)))
            return KGE_EINVAL;
        if (grouped && (a->n_multi_p % TQ || GSETS != 4)) return KGE_EINVAL;
        kge_hi_stream_params h;
        h.Ef = reinterpret_cast<const char *>(Es);
        h.Qh = reinterpret_cast<const char *>(Qs);
        h.q_row_bytes = p.row_bytes;
        h.units = units; h.units_p = units_p;
        h.rows_p = kge_lp_split_rows_padded(d->N, 0);
        h.q_rows = a->col_q ? a->n_single_p : Bp;
        if (a->col_q && (a->n_single_p <= 0 || a->n_single_p % TQ)) return KGE_EINVAL;
        h.B = d->B;
        h.thr = p.thr; h.thr4 = p.thr4;
        h.X = p.X; h.ldx = p.ldx; h.r_idx = p.r_idx; h.yc = p.yc;
        h.raw_count = raw_count; h.list = list; h.cap = cap; h.list_count = list_count; h.overflow = overflow;
        h.col_q = a->col_q;
        h.members = nullptr;
        h.region_count = nullptr; h.region_cap = 0;
        if (a->region_count) {      // the list cut into regions (kge_lp_split_recheck_regions takes them)
            if (a->col_q || !kge_lp_split_regions_supported(d)) return KGE_EINVAL;
            const int n_regions = kge_lp_split_regions(d->B);
            h.region_count = a->region_count;
            h.region_cap = cap / n_regions;
            if (h.region_cap <= 0) return KGE_EINVAL;
        }
        h.true_idx = a->true_idx; h.c_base = d->c_base;
        if (chunked) {
            if (pm != 0 || h.region_count) return KGE_EUNSUPPORTED;
            return kge_hi_chunk_launch(h, slots, s);
        }
        if (!grouped) return kge_hi_stream_launch(h, pm, slots, s);
        // columns: the single-query ones (col_q), then the grouped ones (members) -- two launches over the same candidate table
        if (a->n_single_p > 0) {
            rc = kge_hi_stream_launch(h, pm, slots, s);
            if (rc) return rc;
        }
        h.Qh = reinterpret_cast<const char *>(Qs) + a->n_single_p * (int64_t)p.row_bytes;
        h.q_rows = a->n_multi_p;
        h.col_q = nullptr;
        h.members = a->members;
        return kge_hi_stream_launch(h, 0, slots, s);
    }
    if (a->col_q || a->members) {
        // Columns instead of queries: Qs holds n_single_p rows that carry one query each (col_q), then n_multi_p rows
        // that carry up to GSETS queries of one key each (members); both counts multiples of the query panel.
        if (a->n_single_p < 0 || a->n_multi_p < 0 || a->n_single_p % TQ || a->n_multi_p % TQ ||
            (a->n_single_p > 0 && !a->col_q) || (a->n_multi_p > 0 && !a->members))
            return KGE_EINVAL;
        if (a->n_single_p > 0) {
            p.col_q = a->col_q;
            p.q_panels = (int)(a->n_single_p / TQ);
            p.n_items = (int64_t)p.q_panels * p.c_tiles;
            const int grid = (int)(p.n_items < slots ? p.n_items : slots);
            rc = launch_split_for(pm, 0, lv1, false, p, grid, s);
            if (rc) return rc;
        }
        if (a->n_multi_p > 0) {
            p.col_q = nullptr;
            p.members = a->members;
            p.Qs = reinterpret_cast<const char *>(Qs) + a->n_single_p * (int64_t)p.row_bytes;
            p.q_panels = (int)(a->n_multi_p / TQ);
            p.n_items = (int64_t)p.q_panels * p.c_tiles;
            const int grid = (int)(p.n_items < slots ? p.n_items : slots);
            rc = launch_split_for(pm, GSETS, lv1, false, p, grid, s);
        }
        return rc;
    }
    p.q_panels = (int)((d->B + TQ - 1) / TQ);
    p.n_items = (int64_t)p.q_panels * p.c_tiles;
    const int grid = (int)(p.n_items < slots ? p.n_items : slots);
    return launch_split_for(pm, 0, lv1, p.dbg != 0, p, grid, s);      // (the probes: this path only)
}

/* threshold sets per grouped column (kge_split_args.members) */
extern "C" int kge_lp_split_group_sets(void) { return GSETS; }

/* 1 if this device's v_mfma_f32_32x32x16_f16 accumulates as modelled (see mfma_selftest_kernel), 0 if
 * not, negative / positive error codes as usual.  Synchronises; call it once, outside any capture. */
extern "C" int kge_mfma_f16_selftest(void)
{
    constexpr int NT_ = 8;
    float ab[NT_][32], c[NT_], expect[NT_];
    for (int t = 0; t < NT_; ++t) { for (int k = 0; k < 32; ++k) ab[t][k] = 0.f; c[t] = 0.f; }
    auto A = [&](int t, int k) -> float & { return ab[t][k]; };
    auto Bv = [&](int t, int k) -> float & { return ab[t][16 + k]; };
    // 0: [2^24, 1 x15]: exact 2^24+15 -> RNE 2^24+16 (sequential fp32 adds would give 2^24)
    for (int k = 0; k < 16; ++k) { A(0, k) = 1.f; Bv(0, k) = 1.f; } A(0, 0) = 4096.f; Bv(0, 0) = 4096.f; expect[0] = 16777232.f;
    // 1: C = 2^24 + [1,1,1]: 2^24+3 -> RNE 2^24+4 (truncation would give +2)
    A(1, 0) = A(1, 1) = A(1, 2) = 1.f; Bv(1, 0) = Bv(1, 1) = Bv(1, 2) = 1.f; c[1] = 16777216.f; expect[1] = 16777220.f;
    // 2: C = 2^24 + [1]: tie -> even
    A(2, 0) = 1.f; Bv(2, 0) = 1.f; c[2] = 16777216.f; expect[2] = 16777216.f;
    // 3: [2^24, -2^24, 1 x14]: addends 24 bits below the largest survive -> 14
    for (int k = 0; k < 16; ++k) { A(3, k) = 1.f; Bv(3, k) = 1.f; } A(3, 0) = 4096.f; Bv(3, 0) = 4096.f; A(3, 1) = 4096.f; Bv(3, 1) = -4096.f; expect[3] = 14.f;
    // 4: [2^24, -2^24, 0.5 x6 | 0.5 x8]: 25 bits below is cut in the first pass, the second pass is exact -> 4
    for (int k = 0; k < 16; ++k) { A(4, k) = 0.5f; Bv(4, k) = 1.f; } A(4, 0) = 4096.f; Bv(4, 0) = 4096.f; A(4, 1) = 4096.f; Bv(4, 1) = -4096.f; expect[4] = 4.f;
    // 5: [2^24, 1, 0.5]: no sticky bit -> tie to even 2^24
    A(5, 0) = 4096.f; Bv(5, 0) = 4096.f; A(5, 1) = 1.f; Bv(5, 1) = 1.f; A(5, 2) = 0.5f; Bv(5, 2) = 1.f; expect[5] = 16777216.f;
    // 6: C = 2^24, [1 | 0.5]: the second pass aligns to 2^24 as well
    A(6, 0) = 1.f; Bv(6, 0) = 1.f; A(6, 8) = 0.5f; Bv(6, 8) = 1.f; c[6] = 16777216.f; expect[6] = 16777216.f;
    // 7: f16 subnormal input 2^-20 * 2^10: kept
    A(7, 0) = 9.5367431640625e-07f; Bv(7, 0) = 1024.f; expect[7] = 0.0009765625f;
    float *d_ab = nullptr, *d_c = nullptr, *d_out = nullptr, got[NT_];
    hipError_t e = hipMalloc(&d_ab, sizeof(ab));
    if (e == hipSuccess) e = hipMalloc(&d_c, sizeof(c));
    if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(got));
    if (e == hipSuccess) e = hipMemcpy(d_ab, ab, sizeof(ab), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_c, c, sizeof(c), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0, 0, d_ab, d_c, d_out, NT_);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(got, d_out, sizeof(got), hipMemcpyDeviceToHost);
    if (d_ab) (void)hipFree(d_ab);
    if (d_c) (void)hipFree(d_c);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return (int)e;
    for (int t = 0; t < NT_; ++t)
        if (got[t] != expect[t]) return 0;
    return 1;
}
