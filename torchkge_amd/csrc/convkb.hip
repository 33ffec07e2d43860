// ConvKB (models/deep.py:13-154): F conv filters of width 3 over (head, relation, tail), ReLU, a linear layer to two
// logits, softmax.  The contract -- the closed form on D = L[1] - L[0], one accumulator per pair, j outer / f inner -- is
// in include/kge_hip_convkb.h.  Per pair the ReLU sits between two sums: 3 d F VALU operations (fma, max, fma), no
// matrix-core form and no norm expansion.  This file holds
//   - the per-pair sequence, ONCE (ckb_u / ckb_step / ckb_finish): every kernel below that scores a pair calls it;
//   - the preparation of D, its transpose and the packed filters (kge_convkb_prepare);
//   - the hot kernel: register tiles of TQ queries x TC candidates, scores or counts (convkb_tile_kernel<SLOT, COUNT>);
//   - one pair per thread for the pair / filter / scoring_function entries (few pairs, the same sequence);
//   - scoring_function's backward: gradient rows per triple, and the parameter gradients as one reduction over the batch.
// Everything that depends on (f, j) alone -- the packed filter {w0, w1, w2, cb} and Dt[j*F + f] -- is read through
// kernel-argument pointers at block-uniform indices: scalar loads, the inner loop is VALU with SGPR operands.
// Built with -fno-slp-vectorize (build.py): the vectoriser would pack the per-filter FMAs into half-rate v_pk_fma_f32.
#include "kge_common.h"
#include "../../include/kge_hip_convkb.h"

namespace {

constexpr int CKB_MAXD = KGE_CONVKB_MAX_DIM;
constexpr int CKB_TQ = 4;               // queries per thread (the same four for every thread of a block)
constexpr int CKB_TC = 4;               // candidates per thread
constexpr int CKB_THREADS = 256;
constexpr int CKB_CT = CKB_THREADS * CKB_TC;    // candidates per block: 1024
constexpr int CKB_JC = 8;               // columns of the candidate tile staged per round
constexpr int CKB_LD = CKB_CT + 8;      // LDS row stride of the transposed tile [jj][c]: staging stores spread over the banks

// ---- the per-pair sequence of the contract --------------------------------------------------------------------------
__device__ __forceinline__ float ckb_u(float w1, float y1, float w2, float y2, float cb)
{
    return fmaf(w2, y2, fmaf(w1, y1, cb));
}
__device__ __forceinline__ float ckb_step(float acc, float ws, float e, float u, float D)
{
    return fmaf(D, fmaxf(fmaf(ws, e, u), 0.0f), acc);
}
__device__ __forceinline__ float ckb_finish(float acc, float db)
{
    const float z = acc + db;
    return 1.0f / (1.0f + expf(-z));
}

// slot of query i
__device__ __forceinline__ int ckb_slot(const kge_convkb_desc &p, int64_t i)
{
    return p.slot == KGE_CONVKB_SLOT_BOTH ? (i < p.B_tail ? 2 : 0) : p.slot;
}

// One pair, one thread: qe / qr the query's two rows (kge_convkb_desc), e the candidate's.
__device__ float ckb_pair(const float *__restrict__ wp, const float *__restrict__ Dt, float db, int d, int F, int slot,
                          const float *__restrict__ qe, const float *__restrict__ qr, const float *__restrict__ e)
{
    // s1 < s2 the query's slots: s = 2: (qe, qr) = slots (0, 1); s = 0: (qr, qe) = (1, 2); s = 1: (qe, qr) = (0, 2)
    const float *y1 = slot == 0 ? qr : qe, *y2 = slot == 0 ? qe : qr;
    const int s1 = slot == 0 ? 1 : 0, s2 = slot == 2 ? 1 : 2;
    float acc = 0.0f;
    for (int j = 0; j < d; ++j) {
        const float a = y1[j], b = y2[j], ev = e[j];
        const float *Dj = Dt + (int64_t)j * F;
        for (int f = 0; f < F; ++f) {
            const float *w = wp + 4 * f;
            acc = ckb_step(acc, w[slot], ev, ckb_u(w[s1], a, w[s2], b, w[3]), Dj[f]);
        }
    }
    return ckb_finish(acc, db);
}

__device__ __forceinline__ float ckb_desc_pair(const kge_convkb_desc &p, int64_t i, int64_t c)
{
    const int64_t re = p.qe_idx ? p.qe_idx[i] : i, rr = p.qr_idx ? p.qr_idx[i] : i;
    return ckb_pair(p.wp, p.Dt, p.db[0], p.d, p.F, ckb_slot(p, i), p.QE + re * p.ld_qe, p.QR + rr * p.ld_qr,
                    p.T + c * p.ldt);
}

// ---- preparation -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void convkb_prepare_kernel(const float *__restrict__ w, const float *__restrict__ cb,
                                                             const float *__restrict__ L, int64_t ldl,
                                                             const float *__restrict__ lb, int d, int F,
                                                             float *__restrict__ ws)
{
    const int n = d * F;
    float *wp = ws, *db = ws + 4 * F, *D = db + 4, *Dt = D + n;     // (the packed filters first: float4-readable)
    for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        const float v = L[ldl + k] - L[k];
        const int f = k / d, j = k - f * d;
        D[k] = v;
        Dt[(int64_t)j * F + f] = v;
    }
    if (blockIdx.x == 0) {
        for (int f = threadIdx.x; f < F; f += 256) {
            wp[4 * f] = w[3 * f];
            wp[4 * f + 1] = w[3 * f + 1];
            wp[4 * f + 2] = w[3 * f + 2];
            wp[4 * f + 3] = cb[f];
        }
        if (threadIdx.x == 0) {
            db[0] = lb[1] - lb[0];
            db[1] = db[2] = db[3] = 0.0f;
        }
    }
}

// ---- the hot kernel ----------------------------------------------------------------------------------------------------
// Block = 256 threads on one tile of TQ queries x 1024 candidates; thread t owns candidates t, t + 256, t + 512, t + 768
// of the tile (LDS reads without bank conflicts, coalesced score stores) and all TQ queries, so the query rows are
// block-uniform.  The candidate tile goes through LDS transposed, CKB_JC columns per round.  Per (j, f): 2 TQ FMAs for u
// (recomputed, amortised over TC candidates; the B F d query activations are never materialised) + 3 TQ TC for the pairs.
// Queries [q0, q0 + nq) of the descriptor, all of slot SLOT (a both-sides batch is two launches: no tile straddles B_tail).
template <int SLOT, bool COUNT>
__global__ __launch_bounds__(CKB_THREADS) void convkb_tile_kernel(const kge_convkb_desc p, int64_t q0, int64_t nq,
                                                                  int n_ct, float *__restrict__ out, int64_t ldo,
                                                                  const float *__restrict__ s_true,
                                                                  int32_t *__restrict__ raw)
{
    __shared__ float es[CKB_JC * CKB_LD];
    __shared__ float ys[2 * CKB_TQ * CKB_JC];   // the queries' y1 | y2 columns of the round (LDS reads land in VGPRs: as
                                                // block-uniform scalars hipcc copied them into VGPRs once per filter)
    __shared__ int cnt_s[CKB_THREADS / 64][CKB_TQ];
    constexpr int S1 = SLOT == 0 ? 1 : 0, S2 = SLOT == 2 ? 1 : 2;
    const int tid = threadIdx.x;
    const int ct = blockIdx.x % n_ct;
    const int64_t qt = blockIdx.x / n_ct;
    const int64_t c0 = (int64_t)ct * CKB_CT;
    const int64_t qb = q0 + qt * CKB_TQ, qend = q0 + nq;
    const int d = p.d, F = p.F;
    const float *__restrict__ wp = p.wp;
    const float *__restrict__ Dt = p.Dt;

    // threads [0, 2 TQ JC) stage the queries' columns: row 0 .. TQ-1 of ys is y1 of query a, TQ .. 2 TQ-1 is y2
    const float *ysrc = nullptr;
    if (tid < 2 * CKB_TQ * CKB_JC) {
        const int row = tid / CKB_JC, a = row % CKB_TQ;
        const int64_t i = qb + a < qend ? qb + a : qend - 1;    // a padding query repeats the last one (never stored)
        const bool want_qe = (row < CKB_TQ) == (SLOT != 0);     // y1 is the entity row unless s = 0 (header)
        if (want_qe) ysrc = p.QE + (p.qe_idx ? p.qe_idx[i] : i) * p.ld_qe;
        else ysrc = p.QR + (p.qr_idx ? p.qr_idx[i] : i) * p.ld_qr;
        ysrc += tid % CKB_JC;
    }
    float acc[CKB_TQ][CKB_TC];
#pragma unroll
    for (int a = 0; a < CKB_TQ; ++a)
#pragma unroll
        for (int k = 0; k < CKB_TC; ++k) acc[a][k] = 0.0f;

    for (int j0 = 0; j0 < d; j0 += CKB_JC) {
        __syncthreads();
        for (int idx = tid; idx < CKB_CT * CKB_JC; idx += CKB_THREADS) {
            const int c = idx / CKB_JC, jj = idx - c * CKB_JC;
            float v = 0.0f;
            if (c0 + c < p.N && j0 + jj < d) v = p.T[(c0 + c) * p.ldt + j0 + jj];
            es[jj * CKB_LD + c] = v;
        }
        if (tid < 2 * CKB_TQ * CKB_JC) ys[tid] = j0 + tid % CKB_JC < d ? ysrc[j0] : 0.0f;
        __syncthreads();
        const int jn = d - j0 < CKB_JC ? d - j0 : CKB_JC;
        for (int jj = 0; jj < jn; ++jj) {
            const int j = j0 + jj;
            float y1[CKB_TQ], y2[CKB_TQ], e[CKB_TC];
#pragma unroll
            for (int a = 0; a < CKB_TQ; ++a) { y1[a] = ys[a * CKB_JC + jj]; y2[a] = ys[(CKB_TQ + a) * CKB_JC + jj]; }
#pragma unroll
            for (int k = 0; k < CKB_TC; ++k) e[k] = es[jj * CKB_LD + tid + CKB_THREADS * k];
            const float *__restrict__ Dj = Dt + (int64_t)j * F;
            for (int f = 0; f < F; ++f) {
                const float4 w = *reinterpret_cast<const float4 *>(wp + 4 * f);     // {w0, w1, w2, cb}: one scalar load
                const float wv[4] = {w.x, w.y, w.z, w.w};
                const float Dv = Dj[f];
#pragma unroll
                for (int a = 0; a < CKB_TQ; ++a) {
                    const float u = ckb_u(wv[S1], y1[a], wv[S2], y2[a], wv[3]);
#pragma unroll
                    for (int k = 0; k < CKB_TC; ++k) acc[a][k] = ckb_step(acc[a][k], wv[SLOT], e[k], u, Dv);
                }
            }
        }
    }
    const float db = p.db[0];
    int cnt[CKB_TQ];
#pragma unroll
    for (int a = 0; a < CKB_TQ; ++a) {
        cnt[a] = 0;
        const int64_t i = qb + a;
        const bool qok = i < qend;
        const float thr = (COUNT && qok) ? s_true[i] : 0.0f;
#pragma unroll
        for (int k = 0; k < CKB_TC; ++k) {
            const int64_t c = c0 + tid + CKB_THREADS * k;
            const float sc = ckb_finish(acc[a][k], db);
            if (qok && c < p.N) {
                if (COUNT) cnt[a] += sc >= thr ? 1 : 0;
                else out[i * ldo + c] = sc;
            }
        }
    }
    if (COUNT) {    // per-thread counters -> wave -> block: one integer atomic per (query, block)
#pragma unroll
        for (int a = 0; a < CKB_TQ; ++a) {
            const int s = wave_sum_i(cnt[a]);
            if ((tid & 63) == 0) cnt_s[tid >> 6][a] = s;
        }
        __syncthreads();
        if (tid < CKB_TQ && qb + tid < qend) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < CKB_THREADS / 64; ++w) s += cnt_s[w][tid];
            if (s) atomicAdd(raw + qb + tid, s);
        }
    }
}

// ---- one pair per thread: pair scores, filter correction, scoring_function ---------------------------------------------
__global__ __launch_bounds__(256) void convkb_pair_kernel(const kge_convkb_desc p, const int64_t *__restrict__ qi,
                                                          const int64_t *__restrict__ ci, int64_t P,
                                                          float *__restrict__ out)
{
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < P; q += (int64_t)gridDim.x * 256) {
        const int64_t i = qi ? qi[q] : q, c = ci[q] - p.c_base;
        out[q] = (c >= 0 && c < p.N) ? ckb_desc_pair(p, i, c) : 0.0f;
    }
}

// 8 lanes per query stride over its filter segment (rank_filter.hip's filter_sub_kernel on this model's pair score)
__global__ __launch_bounds__(256) void convkb_filter_sub_kernel(const kge_convkb_desc p, const float *__restrict__ s_true,
                                                                const int64_t *__restrict__ true_idx,
                                                                const int64_t *__restrict__ seg_lo,
                                                                const int64_t *__restrict__ seg_hi,
                                                                const int32_t *__restrict__ targets, int32_t *sub_out,
                                                                int32_t *found_out)
{
    constexpr int LPQ = 8;
    const int sub_lane = threadIdx.x & (LPQ - 1);
    const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPQ;
    const int64_t ngroups = (int64_t)gridDim.x * 256 / LPQ;
    const int64_t rounds = (p.B + ngroups - 1) / ngroups;   // uniform trip count: the shuffles need all lanes
    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t i = group + rd * ngroups;
        int sub = 0, found = 0;
        if (i < p.B) {
            const float tv = s_true[i];
            const int64_t ti = true_idx[i];
            const int neg_inf_counts = (-INFINITY >= tv) ? 1 : 0;
            for (int64_t j = seg_lo[i] + sub_lane; j < seg_hi[i]; j += LPQ) {
                const int64_t cg = targets[j];
                const int64_t c = cg - p.c_base;
                if (c < 0 || c >= p.N) continue;
                if (cg == ti) { found = 1; continue; }
                sub += ((ckb_desc_pair(p, i, c) >= tv) ? 1 : 0) - neg_inf_counts;
            }
        }
#pragma unroll
        for (int o = LPQ / 2; o > 0; o >>= 1) {
            sub += __shfl_xor(sub, o, 64);
            found += __shfl_xor(found, o, 64);
        }
        if (i < p.B && sub_lane == 0) { sub_out[i] = sub; found_out[i] = found ? 1 : 0; }
    }
}

// ---- backward of scoring_function -----------------------------------------------------------------------------------
struct BwdParams {
    const float *E, *R;
    int64_t lde, ldr;
    int d, F;
    const float *D, *wp;
    const int64_t *h, *t, *r;
    int64_t B;
    const float *s, *go;
    float *g, *rows;
    int64_t rows_ld;
    float *dL, *dlb, *dw, *dcb;
};

// v of the contract at s = 2 (the forward of scoring_function)
__device__ __forceinline__ float ckb_v(const float *w, float x0, float x1, float x2)
{
    return fmaf(w[2], x2, ckb_u(w[0], x0, w[1], x1, w[3]));
}

// One wavefront per triple, lanes over j: g_i, and the three gradient rows dx_s[j] = g_i sum_f D[f*d+j] [v > 0] w[f][s].
__global__ __launch_bounds__(256) void convkb_bwd_rows_kernel(const BwdParams p)
{
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wv; i < p.B; i += (int64_t)gridDim.x * 4) {
        const float s = p.s[i];
        const float g = p.go[i] * (s * (1.0f - s));
        if (lane == 0) p.g[i] = g;
        if (!p.rows) continue;
        const float *x0 = p.E + p.h[i] * p.lde, *x1 = p.R + p.r[i] * p.ldr, *x2 = p.E + p.t[i] * p.lde;
        float *gh = p.rows + i * p.rows_ld, *gt = p.rows + (p.B + i) * p.rows_ld, *gr = p.rows + (2 * p.B + i) * p.rows_ld;
        for (int j = lane; j < p.d; j += 64) {
            const float a = x0[j], b = x1[j], c = x2[j];
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int f = 0; f < p.F; ++f) {
                const float *w = p.wp + 4 * f;
                const float m = ckb_v(w, a, b, c) > 0.0f ? p.D[(int64_t)f * p.d + j] : 0.0f;
                s0 = fmaf(m, w[0], s0);
                s1 = fmaf(m, w[1], s1);
                s2 = fmaf(m, w[2], s2);
            }
            gh[j] = g * s0;
            gr[j] = g * s1;
            gt[j] = g * s2;
        }
    }
}

// sum of the 256 values of a block as a fixed-shape tree (the same bits on every run)
__device__ __forceinline__ float block_tree_sum(float v, float *sh)
{
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// One block per filter f (and one more for dlb), threads over j: the triples in ascending order, v recomputed.
//   dL[1][k] = sum_i g_i relu(v),  dw[f][s] = sum_j D[k] sum_i g_i [v > 0] x_s[j],  dcb[f] = sum_j D[k] sum_i g_i [v > 0]
__global__ __launch_bounds__(256) void convkb_bwd_params_kernel(const BwdParams p)
{
    __shared__ float sh[256];
    const int tid = threadIdx.x;
    const int f = blockIdx.x;
    if (f == p.F) {     // dlb = (-sum g_i, +sum g_i)
        float part = 0.0f;
        for (int64_t i = tid; i < p.B; i += 256) part += p.g[i];
        const float tot = block_tree_sum(part, sh);
        if (tid == 0) { p.dlb[0] = -tot; p.dlb[1] = tot; }
        return;
    }
    const float *w = p.wp + 4 * f;
    const float w0 = w[0], w1 = w[1], w2 = w[2], cb = w[3];
    const int64_t n = (int64_t)p.F * p.d;
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, tc = 0.0f;       // this thread's share of dw[f][0..2], dcb[f]
    for (int j = tid; j < p.d; j += 256) {
        const int64_t k = (int64_t)f * p.d + j;
        float sm = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, ac = 0.0f;
        for (int64_t i = 0; i < p.B; ++i) {
            const float x0 = p.E[p.h[i] * p.lde + j], x1 = p.R[p.r[i] * p.ldr + j], x2 = p.E[p.t[i] * p.lde + j];
            const float v = fmaf(w2, x2, ckb_u(w0, x0, w1, x1, cb));
            const float g = p.g[i];
            sm = fmaf(g, fmaxf(v, 0.0f), sm);
            const float gm = v > 0.0f ? g : 0.0f;
            a0 = fmaf(gm, x0, a0);
            a1 = fmaf(gm, x1, a1);
            a2 = fmaf(gm, x2, a2);
            ac += gm;
        }
        p.dL[n + k] = sm;
        p.dL[k] = -sm;
        const float Dk = p.D[k];
        t0 = fmaf(Dk, a0, t0);
        t1 = fmaf(Dk, a1, t1);
        t2 = fmaf(Dk, a2, t2);
        tc = fmaf(Dk, ac, tc);
    }
    t0 = block_tree_sum(t0, sh);
    t1 = block_tree_sum(t1, sh);
    t2 = block_tree_sum(t2, sh);
    tc = block_tree_sum(tc, sh);
    if (tid == 0) {
        p.dw[3 * f] = t0;
        p.dw[3 * f + 1] = t1;
        p.dw[3 * f + 2] = t2;
        p.dcb[f] = tc;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
int check_dims(int d, int F)
{
    if (d < 1 || F < 1) return KGE_EINVAL;
    if (d > CKB_MAXD || F > CKB_MAXD) return KGE_EUNSUPPORTED;
    return 0;
}

// 0 and *empty = true: valid, nothing to do
int check_desc(const kge_convkb_desc *p, bool *empty)
{
    *empty = false;
    if (!p) return KGE_EINVAL;
    if (p->slot < 0 || p->slot > KGE_CONVKB_SLOT_BOTH) return KGE_EINVAL;
    if (p->B < 0 || p->N < 0) return KGE_EINVAL;
    if (p->slot == KGE_CONVKB_SLOT_BOTH && (p->B_tail < 0 || p->B_tail > p->B)) return KGE_EINVAL;
    const int rc = check_dims(p->d, p->F);
    if (rc) return rc;
    if (p->B == 0 || p->N == 0) {
        *empty = true;
        return 0;
    }
    if (!p->QE || !p->QR || !p->T || !p->D || !p->Dt || !p->wp || !p->db) return KGE_EINVAL;
    if (p->ld_qe < p->d || p->ld_qr < p->d || p->ldt < p->d) return KGE_EINVAL;
    if (!kge_aligned16(p->wp)) return KGE_EINVAL;
    return 0;
}

inline int grid1d(int64_t items, int per_block, int cap)
{
    const int64_t b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b < cap ? b : cap));
}

template <bool COUNT>
int launch_tiles(const kge_convkb_desc &p, float *out, int64_t ldo, const float *s_true, int32_t *raw, hipStream_t s)
{
    // the query ranges by slot: a both-sides batch is [0, B_tail) at s = 2 and [B_tail, B) at s = 0
    int64_t q0[2] = {0, 0}, nq[2] = {p.B, 0};
    int slot[2] = {p.slot, 0};
    if (p.slot == KGE_CONVKB_SLOT_BOTH) {
        slot[0] = 2;
        nq[0] = p.B_tail;
        q0[1] = p.B_tail;
        nq[1] = p.B - p.B_tail;
    }
    const int64_t n_ct = (p.N + CKB_CT - 1) / CKB_CT;
    for (int part = 0; part < 2; ++part)
        if (nq[part] > 0 && n_ct * ((nq[part] + CKB_TQ - 1) / CKB_TQ) > INT32_MAX) return KGE_EUNSUPPORTED;
    for (int part = 0; part < 2; ++part) {
        if (nq[part] <= 0) continue;
        const dim3 grid((unsigned)(n_ct * ((nq[part] + CKB_TQ - 1) / CKB_TQ)));
#define CKB_LAUNCH(S)                                                                                                  \
    hipLaunchKernelGGL((convkb_tile_kernel<S, COUNT>), grid, dim3(CKB_THREADS), 0, s, p, q0[part], nq[part], (int)n_ct, \
                       out, ldo, s_true, raw)
        if (slot[part] == 0) CKB_LAUNCH(0);
        else if (slot[part] == 1) CKB_LAUNCH(1);
        else CKB_LAUNCH(2);
#undef CKB_LAUNCH
        KGE_CHECK_LAUNCH();
    }
    return 0;
}

void ws_pointers(const float *ws, int d, int F, kge_convkb_desc *p)
{
    if (!ws) return;
    p->wp = ws;
    p->db = ws + 4 * F;
    p->D = ws + 4 * F + 4;
    p->Dt = p->D + (int64_t)d * F;
}

} // namespace

extern "C" int kge_convkb_prepare(const float *w, const float *cb, const float *L, int64_t ldl, const float *lb, int d,
                                  int F, float *ws, kge_stream_t stream)
{
    const int rc = check_dims(d, F);
    if (rc) return rc;
    if (!w || !cb || !L || !lb || !ws || ldl < (int64_t)d * F || !kge_aligned16(ws)) return KGE_EINVAL;
    hipLaunchKernelGGL(convkb_prepare_kernel, dim3(grid1d((int64_t)d * F, 256, 1024)), dim3(256), 0, kge_s(stream), w, cb,
                       L, ldl, lb, d, F, ws);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_convkb_scores(const kge_convkb_desc *desc, float *out, int64_t ldo, kge_stream_t stream)
{
    bool empty;
    const int rc = check_desc(desc, &empty);
    if (rc) return rc;
    if (empty) return 0;
    if (!out || ldo < desc->N) return KGE_EINVAL;
    return launch_tiles<false>(*desc, out, ldo, nullptr, nullptr, kge_s(stream));
}

extern "C" int kge_convkb_count_ge(const kge_convkb_desc *desc, const float *s_true, int32_t *raw_count,
                                   kge_stream_t stream)
{
    bool empty;
    const int rc = check_desc(desc, &empty);
    if (rc) return rc;
    if (empty) return 0;
    if (!s_true || !raw_count) return KGE_EINVAL;
    return launch_tiles<true>(*desc, nullptr, 0, s_true, raw_count, kge_s(stream));
}

extern "C" int kge_convkb_pair_scores(const kge_convkb_desc *desc, const int64_t *qi, const int64_t *ci, int64_t P,
                                      float *out, kge_stream_t stream)
{
    bool empty;
    if (!desc || P < 0) return KGE_EINVAL;
    // (a pair list is scored against an EMPTY candidate range too: every pair lies outside it and scores 0)
    kge_convkb_desc p = *desc;
    const bool none = p.N == 0;
    if (none) p.N = 1;
    if (p.B == 0) p.B = 1;
    const int rc = check_desc(&p, &empty);
    if (rc) return rc;
    if (P == 0) return 0;
    if (!ci || !out) return KGE_EINVAL;
    if (none) p.N = 0;
    hipLaunchKernelGGL(convkb_pair_kernel, dim3(grid1d(P, 256, 256 * 32)), dim3(256), 0, kge_s(stream), p, qi, ci, P, out);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_convkb_filter_sub(const kge_convkb_desc *desc, const float *s_true, const int64_t *true_idx,
                                     const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *targets, int32_t *sub,
                                     int32_t *found, kge_stream_t stream)
{
    bool empty;
    if (!desc) return KGE_EINVAL;
    kge_convkb_desc p = *desc;
    const bool none = p.N == 0;     // (an empty candidate range still owes sub = found = 0)
    if (none) p.N = 1;
    const int rc = check_desc(&p, &empty);
    if (rc) return rc;
    if (p.B == 0) return 0;
    if (!s_true || !true_idx || !seg_lo || !seg_hi || !sub || !found) return KGE_EINVAL;
    if (none) p.N = 0;
    hipLaunchKernelGGL(convkb_filter_sub_kernel, dim3(grid1d(p.B, 32, 256 * 32)), dim3(256), 0, kge_s(stream), p, s_true,
                       true_idx, seg_lo, seg_hi, targets, sub, found);
    KGE_CHECK_LAUNCH();
    return 0;
}

static int check_triples(const float *E, int64_t lde, const float *R, int64_t ldr, int d, int F, const float *ws,
                         const int64_t *h, const int64_t *t, const int64_t *r, int64_t B)
{
    const int rc = check_dims(d, F);
    if (rc) return rc;
    if (B < 0) return KGE_EINVAL;
    if (B > 0 && (!E || !R || !ws || !h || !t || !r || lde < d || ldr < d || !kge_aligned16(ws))) return KGE_EINVAL;
    return 0;
}

extern "C" int kge_convkb_score_triples(const float *E, int64_t lde, const float *R, int64_t ldr, int d, int F,
                                        const float *ws, const int64_t *h, const int64_t *t, const int64_t *r, int64_t B,
                                        float *out, kge_stream_t stream)
{
    const int rc = check_triples(E, lde, R, ldr, d, F, ws, h, t, r, B);
    if (rc) return rc;
    if (B == 0) return 0;
    if (!out) return KGE_EINVAL;
    // the pair entry on (E[h], R[r]) against the whole table E, candidate t: s = 2
    kge_convkb_desc p = {};
    p.slot = 2;
    p.d = d;
    p.F = F;
    p.B = B;
    p.N = INT64_MAX;
    p.QE = E; p.ld_qe = lde; p.qe_idx = h;
    p.QR = R; p.ld_qr = ldr; p.qr_idx = r;
    p.T = E; p.ldt = lde;
    ws_pointers(ws, d, F, &p);
    hipLaunchKernelGGL(convkb_pair_kernel, dim3(grid1d(B, 256, 256 * 32)), dim3(256), 0, kge_s(stream), p, nullptr, t, B,
                       out);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_convkb_score_triples_bwd(const float *E, int64_t lde, const float *R, int64_t ldr, int d, int F,
                                            const float *ws, const int64_t *h, const int64_t *t, const int64_t *r,
                                            int64_t B, const float *s, const float *go, float *g, float *rows,
                                            int64_t rows_ld, float *dL, float *dlb, float *dw, float *dcb,
                                            kge_stream_t stream)
{
    const int rc = check_triples(E, lde, R, ldr, d, F, ws, h, t, r, B);
    if (rc) return rc;
    const int n_par = (dL ? 1 : 0) + (dlb ? 1 : 0) + (dw ? 1 : 0) + (dcb ? 1 : 0);
    if (n_par != 0 && n_par != 4) return KGE_EINVAL;
    if (rows && rows_ld < d) return KGE_EINVAL;
    if (B > 0 && (!s || !go || !g)) return KGE_EINVAL;
    if (n_par && !ws) return KGE_EINVAL;
    kge_convkb_desc wsd = {};
    ws_pointers(ws, d, F, &wsd);
    const BwdParams p{E, R, lde, ldr, d, F, wsd.D, wsd.wp, h, t, r, B, s, go, g, rows, rows_ld, dL, dlb, dw, dcb};
    if (B > 0) {
        hipLaunchKernelGGL(convkb_bwd_rows_kernel, dim3(grid1d(B, 4, 256 * 32)), dim3(256), 0, kge_s(stream), p);
        KGE_CHECK_LAUNCH();
    }
    if (n_par) {    // (B == 0: the sums are empty, the kernel writes zeros)
        hipLaunchKernelGGL(convkb_bwd_params_kernel, dim3(F + 1), dim3(256), 0, kge_s(stream), p);
        KGE_CHECK_LAUNCH();
    }
    return 0;
}
