// RESCAL and HolE: the two bilinear models whose relation acts as a d x d operator B_r on the head row,
//   score(h, r, t) = h . B_r . t,    RESCAL  B_r = M_r = rel_mat[r].view(d, d)   (models/bilinear.py:14-143)
//                                    HolE    B_r[i, j] = R[r, (j - i) mod d]      (the rolling matrix, :326-340)
// Once the query row is transformed (tail side q = x . B_r, head side q = x . B_r^T), the all-candidates score is
// the plain dot product q . E[c] of DistMult: everything downstream (KGE_LP_DOT, the split prefilter, filter, ranks)
// is reused.  This file holds what is specific to these two models:
//   - the query transform of evaluate() (kge_bilinear_query) as an Op of the relation-grouped transform of
//     rel_operator.h: which entity row, which side of B_r, the shard's ownership (HolE: the tile of B_r is generated in LDS
//     from the d floats of R[r]);
//   - the relation-candidate rows of relation prediction (kge_bilinear_relation_rows);
//   - scoring_function forward / backward (reached through kge_score_triples / _bwd); RESCAL's d rel_mat
//     (kge_rescal_rel_grad) is the square case of the per-relation reduction in transr_xform.hip.
// Every sum is an explicit fmaf chain in a fixed order (-ffp-contract=off): a transformed query row depends on
// (entity, relation, side) only, never on the rest of the batch or on where the row sits in a tile.
#include "rel_operator.h"

namespace {

// coefficient of x[k] in output column j: tail side B[k][j], head side B[j][k]; rr = the relation's row
__device__ __forceinline__ float op_coef(int kind, bool head, const float *__restrict__ rr, int d, int k, int j)
{
    if (kind == KGE_RESCAL) return head ? rr[(int64_t)j * d + k] : rr[(int64_t)k * d + j];
    int m = head ? k - j : j - k;
    if (m < 0) m += d;
    return rr[m];
}

// kge_bilinear_query as an Op of rel_query_kernel (rel_operator.h).  A run is one (relation, side): the two sides of a
// relation read B_r in different index orders.  A row whose entity lies outside the shard [ent_lo, ent_lo + ent_n) is
// written as zeros (the owning rank's row is added to it).
struct BilinearOp {
    int K, J;                           // both d
    int kind, side;
    const float *Rt; int64_t ldr;       // relation table: rel_mat (n_rel, d*d) or R (n_rel, d)
    const int64_t *h, *t, *r;
    int64_t n_facts;
    int64_t ent_lo, ent_n;              // ent_n < 0: X is the whole table

    __device__ RelRow row(int64_t pos) const
    {
        const bool second = side == KGE_SIDE_BOTH && pos >= n_facts;
        const bool head = side == KGE_SIDE_HEAD || second;
        const int64_t f = second ? pos - n_facts : pos;
        const int64_t e = (head ? t[f] : h[f]) - ent_lo;
        return RelRow{pos, r[f] * 2 + (head ? 1 : 0), (ent_n < 0 || (e >= 0 && e < ent_n)) ? e : -1, 0.f};
    }
    struct Coefs {
        int kind, d;
        bool head;
        const float *rr;
        __device__ bool k_contiguous() const { return kind == KGE_RESCAL && head; }    // M[j][k]
        __device__ float operator()(int k, int j) const { return op_coef(kind, head, rr, d, k, j); }
    };
    __device__ Coefs coefs(int64_t key) const { return Coefs{kind, K, (key & 1) != 0, Rt + (key >> 1) * ldr}; }
    __device__ float finish(const RelRow &w, int, float acc) const { return w.src >= 0 ? acc : 0.f; }
};

// relation prediction rows: RESCAL out[i, a*d + b] = h_a t_b; HolE out[i, k] = chain_j h_j t_{(j+k) mod d}
__global__ __launch_bounds__(256) void relation_rows_kernel(int kind, const float *__restrict__ H, int64_t ldh,
                                                            const float *__restrict__ T, int64_t ldt, int64_t B, int d,
                                                            float *__restrict__ out, int64_t ldo)
{
    const int64_t w = (kind == KGE_RESCAL) ? (int64_t)d * d : d;
    const int64_t n = B * w;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = x / w;
        const int c = (int)(x - i * w);
        const float *hr = H + i * ldh, *tr = T + i * ldt;
        float v;
        if (kind == KGE_RESCAL) {
            v = hr[c / d] * tr[c % d];
        } else {
            v = 0.f;
            int m = c;
            for (int jj = 0; jj < d; ++jj) {
                v = fmaf(hr[jj], tr[m], v);
                if (++m == d) m = 0;
            }
        }
        out[i * ldo + c] = v;
    }
}

// ---- scoring_function: h^ . B_r . t^ with x^ = x / max(||x||, 1e-12), four triples per block (one per wave) ----
struct BScoreParams {
    int kind;
    const float *E, *Rt;
    int64_t ldr;
    int d;
    const int64_t *h, *t, *r;
    int64_t B;
    float *out;
    // backward
    const float *go;
    float *g0, *g1, *rows;
    int64_t rows_ld;
};

__global__ __launch_bounds__(SC_WAVES * 64) void bilinear_score_fwd_kernel(const BScoreParams p)
{
    __shared__ float hs[SC_WAVES][REL_MAXD], ts[SC_WAVES][REL_MAXD];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, d = p.d;
    for (int64_t base = (int64_t)blockIdx.x * SC_WAVES; base < p.B; base += (int64_t)gridDim.x * SC_WAVES) {
        const int64_t i = base + w;
        const bool ok = i < p.B;
        if (ok) {
            load_normalized(p.E + p.h[i] * d, d, lane, hs[w]);
            load_normalized(p.E + p.t[i] * d, d, lane, ts[w]);
        }
        __syncthreads();
        if (ok) {
            const float *rr = p.Rt + p.r[i] * p.ldr;
            float part = 0.f;
            for (int j = lane; j < d; j += 64) {
                float u = 0.f;
                for (int k = 0; k < d; ++k) u = fmaf(hs[w][k], op_coef(p.kind, false, rr, d, k, j), u);
                part = fmaf(u, ts[w][j], part);
            }
            const float s = wave_sum(part);
            if (lane == 0) p.out[i] = s;
        }
        __syncthreads();
    }
}

// one gradient row: stored as row `stream` of the row mode, or added with fp32 atomics into g[row]
__device__ __forceinline__ void emit_row(const BScoreParams &p, int stream, int64_t i, float *g, int64_t row,
                                         const float *v, int d, int lane)
{
    if (p.rows) {
        float *dst = p.rows + ((int64_t)stream * p.B + i) * p.rows_ld;
        for (int k = lane; k < d; k += 64) dst[k] = v[k];
    } else {
        for (int k = lane; k < d; k += 64)
            if (v[k] != 0.f) atomicAdd(g + row * d + k, v[k]);
    }
}

__global__ __launch_bounds__(SC_WAVES * 64) void bilinear_score_bwd_kernel(const BScoreParams p)
{
    __shared__ float hs[SC_WAVES][REL_MAXD], ts[SC_WAVES][REL_MAXD], gh[SC_WAVES][REL_MAXD], gt[SC_WAVES][REL_MAXD];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, d = p.d;
    for (int64_t base = (int64_t)blockIdx.x * SC_WAVES; base < p.B; base += (int64_t)gridDim.x * SC_WAVES) {
        const int64_t i = base + w;
        const bool ok = i < p.B;
        float nh = 1.f, nt = 1.f;
        if (ok) {
            nh = load_normalized(p.E + p.h[i] * d, d, lane, hs[w]);
            nt = load_normalized(p.E + p.t[i] * d, d, lane, ts[w]);
        }
        __syncthreads();
        if (ok) {
            const float go = p.go[i];
            const float *rr = p.Rt + p.r[i] * p.ldr;
            for (int j = lane; j < d; j += 64) {        // d/dt^_j = go chain_k h^_k B[k][j]
                float u = 0.f;
                for (int k = 0; k < d; ++k) u = fmaf(hs[w][k], op_coef(p.kind, false, rr, d, k, j), u);
                gt[w][j] = go * u;
            }
            for (int k = lane; k < d; k += 64) {        // d/dh^_k = go chain_j B[k][j] t^_j
                float u = 0.f;
                for (int j = 0; j < d; ++j) u = fmaf(op_coef(p.kind, false, rr, d, k, j), ts[w][j], u);
                gh[w][k] = go * u;
            }
            if (p.kind == KGE_RESCAL) {
                // operands of the relation-grouped reduction (kge_rescal_rel_grad): U = go h^, V = t^
                float *U = p.rows + ((int64_t)2 * p.B + i) * p.rows_ld, *V = p.rows + ((int64_t)3 * p.B + i) * p.rows_ld;
                for (int k = lane; k < d; k += 64) { U[k] = go * hs[w][k]; V[k] = ts[w][k]; }
            } else {            // HolE: d/dR[r]_m = go chain_k h^_k t^_{(k+m) mod d}
                float *dst = p.rows ? p.rows + ((int64_t)2 * p.B + i) * p.rows_ld : nullptr;
                for (int m = lane; m < d; m += 64) {
                    float u = 0.f;
                    int q = m;
                    for (int k = 0; k < d; ++k) {
                        u = fmaf(hs[w][k], ts[w][q], u);
                        if (++q == d) q = 0;
                    }
                    u = go * u;
                    if (dst) dst[m] = u;
                    else if (u != 0.f) atomicAdd(p.g1 + p.r[i] * d + m, u);
                }
            }
        }
        __syncthreads();
        if (ok) {           // through the normalisation: (g - x^ (x^ . g)) / n  (x / eps: plain scaling)
            float sh = 0.f, st = 0.f;
            for (int k = lane; k < d; k += 64) { sh = fmaf(hs[w][k], gh[w][k], sh); st = fmaf(ts[w][k], gt[w][k], st); }
            sh = wave_sum(sh); st = wave_sum(st);
            const bool ch = nh <= 1e-12f, ct = nt <= 1e-12f;
            for (int k = lane; k < d; k += 64) {
                gh[w][k] = ch ? gh[w][k] / nh : (gh[w][k] - hs[w][k] * sh) / nh;
                gt[w][k] = ct ? gt[w][k] / nt : (gt[w][k] - ts[w][k] * st) / nt;
            }
            emit_row(p, 0, i, p.g0, p.h[i], gh[w], d, lane);
            emit_row(p, 1, i, p.g0, p.t[i], gt[w], d, lane);
        }
        __syncthreads();
    }
}

int check_operator_kind(int kind, const float *E, const float *Rt, int d_ent, int d_rel)
{
    if (kind != KGE_RESCAL && kind != KGE_HOLE) return KGE_EINVAL;
    if (!E || !Rt || d_ent < 1 || d_ent > REL_MAXD) return KGE_EINVAL;
    if (d_rel != (kind == KGE_RESCAL ? d_ent * d_ent : d_ent)) return KGE_EINVAL;
    return 0;
}

} // namespace

// KGE_RESCAL / KGE_HOLE behind kge_score_triples / kge_score_triples_bwd (declared in kge_common.h)
int kge_bilinear_score_fwd(int kind, const float *t0, const float *t1, int d_ent, int d_rel, const int64_t *h,
                           const int64_t *t, const int64_t *r, int64_t B, float *out, hipStream_t s)
{
    int rc = check_operator_kind(kind, t0, t1, d_ent, d_rel);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!h || !t || !r || !out))) return KGE_EINVAL;
    if (B == 0) return 0;
    BScoreParams p{kind, t0, t1, d_rel, d_ent, h, t, r, B, out, nullptr, nullptr, nullptr, nullptr, 0};
    hipLaunchKernelGGL(bilinear_score_fwd_kernel, dim3(sc_grid(B)), dim3(SC_WAVES * 64), 0, s, p);
    KGE_CHECK_LAUNCH();
    return 0;
}

int kge_bilinear_score_bwd(int kind, const float *t0, const float *t1, int d_ent, int d_rel, const int64_t *h,
                           const int64_t *t, const int64_t *r, int64_t B, const float *go, float *g0, float *g1,
                           float *rows, int64_t rows_ld, hipStream_t s)
{
    int rc = check_operator_kind(kind, t0, t1, d_ent, d_rel);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!h || !t || !r || !go))) return KGE_EINVAL;
    if (B == 0) return 0;
    if (kind == KGE_RESCAL && !rows) return KGE_EINVAL;     // d rel_mat only through kge_rescal_rel_grad
    if (rows && rows_ld < d_ent) return KGE_EINVAL;
    if (!rows && (!g0 || !g1)) return KGE_EINVAL;
    BScoreParams p{kind, t0, t1, d_rel, d_ent, h, t, r, B, nullptr, go, g0, g1, rows, rows_ld};
    hipLaunchKernelGGL(bilinear_score_bwd_kernel, dim3(sc_grid(B)), dim3(SC_WAVES * 64), 0, s, p);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_bilinear_query(int kind, int side, const float *X, int64_t ldx, const float *Rt, int64_t ldr, int d,
                                  const int64_t *h, const int64_t *t, const int64_t *r, int64_t B, int64_t ent_lo,
                                  int64_t ent_n, const int64_t *perm, float *Q, int64_t ldq, kge_stream_t stream)
{
    if (kind != KGE_RESCAL && kind != KGE_HOLE) return KGE_EINVAL;
    if (side != KGE_SIDE_TAIL && side != KGE_SIDE_HEAD && side != KGE_SIDE_BOTH) return KGE_EINVAL;
    if (d < 1 || d > REL_MAXD || B < 0 || ldx < d || ldq < d) return KGE_EINVAL;
    if (ldr < (kind == KGE_RESCAL ? (int64_t)d * d : (int64_t)d)) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!X || !Rt || !r || !Q) return KGE_EINVAL;
    if ((side != KGE_SIDE_HEAD && !h) || (side != KGE_SIDE_TAIL && !t)) return KGE_EINVAL;
    const int64_t rows = side == KGE_SIDE_BOTH ? 2 * B : B;
    if ((rows + QT_ROWS - 1) / QT_ROWS > 0x7fffffffll) return KGE_EINVAL;
    const RelQueryIO io{X, ldx, perm, rows, Q, ldq};
    const BilinearOp op{d, d, kind, side, Rt, ldr, h, t, r, B, ent_lo, ent_n};
    const dim3 grid((unsigned)((rows + QT_ROWS - 1) / QT_ROWS), (unsigned)((d + QT_COLS - 1) / QT_COLS));
    hipStream_t s = kge_s(stream);
    if (d % QT_KC == 0) hipLaunchKernelGGL((rel_query_kernel<BilinearOp, true>), grid, dim3(QT_THREADS), 0, s, io, op);
    else hipLaunchKernelGGL((rel_query_kernel<BilinearOp, false>), grid, dim3(QT_THREADS), 0, s, io, op);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_bilinear_relation_rows(int kind, const float *H, int64_t ldh, const float *T, int64_t ldt, int64_t B,
                                          int d, float *out, int64_t ldo, kge_stream_t stream)
{
    if (kind != KGE_RESCAL && kind != KGE_HOLE) return KGE_EINVAL;
    const int64_t w = kind == KGE_RESCAL ? (int64_t)d * d : d;
    if (d < 1 || d > REL_MAXD || B < 0 || ldh < d || ldt < d || ldo < w) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!H || !T || !out) return KGE_EINVAL;
    const int64_t n = B * w;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(relation_rows_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                       kge_s(stream), kind, H, ldh, T, ldt, B, d, out, ldo);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_rescal_rel_grad(const float *U, const float *V, int64_t ld, int d, const int64_t *r,
                                   const int64_t *perm, int64_t B, int64_t n_rel, float *gM, int64_t ldg,
                                   kge_stream_t stream)
{
    if (d < 1 || d > REL_MAXD || B < 0 || n_rel < 0 || ld < d || ldg < (int64_t)d * d) return KGE_EINVAL;
    if (n_rel == 0) return 0;
    if (!gM || (B > 0 && (!U || !V || !r || !perm))) return KGE_EINVAL;
    if (n_rel > 0x7fffffffll) return KGE_EINVAL;
    return kge_rel_outer_grad(U, ld, V, ld, d, d, r, perm, B, n_rel, gM, ldg, kge_s(stream));     // the square case
}
