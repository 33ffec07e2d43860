// TransR (models/translation.py:287-458): every relation owns a d_r x d_e operator M_r = proj_mat[r].view(d_r, d_e),
//   score(h, r, t) = -|| M_r h + r - M_r t ||^2.
// The reference evaluates it through a (n_rel, n_ent, d_r) cache of every entity projected under every relation.  Here
// the all-candidates score is expanded around the query q_i = M_r e + s R[r] (s = +1 tail side, -1 head side):
//   || q_i - M_r e_c ||^2 = ||q_i||^2 - 2 u_i . e_c + Z[r_i, c],   u_i = M_r^T q_i,   Z[r, c] = || M_r e_c ||^2
// which is the KGE_LP_L2_PROJH problem with A0 = u, T0 = the raw entity table, en = 0, (p_i, z_i) = (1, 0), X = Z.
// This file holds what is specific to TransR:
//   - kge_transr_proj_sqnorm: out[r, j] = || M_r x_j + b_r ||^2 on v_mfma_f32_32x32x2_f32; the projected rows live in
//     accumulators only (the Z table of an evaluation; with x = e_h - e_t and b = rel_emb the relation-prediction scores);
//   - kge_transr_query: q, u of a batch as two Ops of the relation-grouped transform of rel_operator.h (rows grouped by
//     relation with kge_key_sort): M_r read row-wise with the +- R[r] finish, then M_r^T;
//   - scoring_function forward / backward (through kge_score_triples / _bwd, kind KGE_TRANSR);
//   - the per-relation outer-product reduction, rectangular: d proj_mat (kge_transr_rel_grad) and, square, RESCAL's
//     d rel_mat (kge_rescal_rel_grad in bilinear_xform.hip) through kge_rel_outer_grad.
// Every sum has a fixed order (-ffp-contract=off, explicit fmaf): no float atomics, and no result depends on the grid, on
// where a row sits in a tile or on the rest of the batch.
#include "rel_operator.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// ---- a. projected squared norms ------------------------------------------------------------------------------------
// Block: 4 waves, one relation, 128 rows of X; wave w owns rows [32 w, 32 w + 32) for ALL output columns.  The output
// columns are visited in slices of 128 (4 MFMA tiles of 32 per wave, 64 accumulator registers); per slice the inner
// dimension runs in chunks of 32 through LDS (row stride 36 floats: conflict-free b128 reads and writes; the next chunk
// is fetched global -> registers while the MFMAs of the current one run).
// MFMA operands: A = M_r (i = output column), B = X^T (j = row), so lane l holds D[i][j] with j = l & 31 and
// i = 8 (reg >> 2) + 4 (l >> 5) + (reg & 3): a row's columns are spread over 16 registers of two lanes (l, l + 32).
// Order (restated by the tests on the CPU):
//   p_c = chain_k M_r[c, k] x[k] -- one accumulator, 8-blocks of k ascending, inside a block k = 0,4,1,5,2,6,3,7 (the
//         order lp_gemm_mfma.hip feeds the instruction; absent k are zero products) -- then p_c += b_r[c] when b is given;
//   out = chain over ASCENDING c of fmaf(p_c, p_c, out) from 0: the running sum is handed between the two lanes that
//         share a row after every group of four columns (columns >= d_r hold p = 0 and leave the sum unchanged).
constexpr int PN_ROWS = 128, PN_COLS = 128, PN_BK = 32, PN_LD = PN_BK + 4, PN_THREADS = 256;

struct ProjNormParams {
    const float *M; int64_t ldm;        // proj_mat (n_rel, d_r * d_e)
    const float *X; int64_t ldx;        // (n, d_e)
    const float *b; int64_t ldb;        // (n_rel, d_r) or NULL
    const int64_t *rels;                // relation of grid row y (NULL: y)
    int64_t n;
    int d_e, d_r;
    float *out; int64_t os_r, os_j;     // out[rel * os_r + j * os_j]
};

template <bool VEC4>
__global__ __launch_bounds__(PN_THREADS) void proj_sqnorm_kernel(const ProjNormParams p)
{
    __shared__ __attribute__((aligned(16))) float Ms[PN_COLS * PN_LD];
    __shared__ __attribute__((aligned(16))) float Xs[PN_ROWS * PN_LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int64_t rel = p.rels ? p.rels[blockIdx.y] : (int64_t)blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * PN_ROWS;
    const float *Mr = p.M + rel * p.ldm;
    const int d_e = p.d_e, d_r = p.d_r;
    const int srow = tid >> 3, sk = (tid & 7) * 4;      // staging: 32 rows x 8 float4 per pass, 4 passes per tile
    float s = 0.f;
    for (int c0 = 0; c0 < d_r; c0 += PN_COLS) {
        const int nmt = (d_r - c0 + 31) / 32 < 4 ? (d_r - c0 + 31) / 32 : 4;    // tiles of this slice that hold columns
        f32x16 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
        // chunk k0 + 32 is fetched into registers while the MFMAs of chunk k0 run (one chunk: 8 float4 per thread)
        float4 pm[4], px[4];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                const int row = srow + 32 * ps;
                const int k = k0 + sk;
                float4 m = make_float4(0.f, 0.f, 0.f, 0.f), x = m;
                const int c = c0 + row;
                const int64_t j = j0 + row;
                if (c < d_r && row < 32 * nmt) {
                    const float *src = Mr + (int64_t)c * d_e + k;
                    if (VEC4) { if (k < d_e) m = *reinterpret_cast<const float4 *>(src); }
                    else {
                        if (k < d_e) m.x = src[0];
                        if (k + 1 < d_e) m.y = src[1];
                        if (k + 2 < d_e) m.z = src[2];
                        if (k + 3 < d_e) m.w = src[3];
                    }
                }
                if (j < p.n) {
                    const float *src = p.X + j * p.ldx + k;
                    if (VEC4) { if (k < d_e) x = *reinterpret_cast<const float4 *>(src); }
                    else {
                        if (k < d_e) x.x = src[0];
                        if (k + 1 < d_e) x.y = src[1];
                        if (k + 2 < d_e) x.z = src[2];
                        if (k + 3 < d_e) x.w = src[3];
                    }
                }
                pm[ps] = m; px[ps] = x;
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < d_e; k0 += PN_BK) {
            __syncthreads();        // the previous chunk's readers are done
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                const int row = srow + 32 * ps;
                *reinterpret_cast<float4 *>(Ms + row * PN_LD + sk) = pm[ps];
                *reinterpret_cast<float4 *>(Xs + row * PN_LD + sk) = px[ps];
            }
            __syncthreads();
            if (k0 + PN_BK < d_e) fetch(k0 + PN_BK);
            const float *Xb = Xs + (wid * 32 + l31) * PN_LD + half * 4;
            const float *Mb = Ms + l31 * PN_LD + half * 4;
#pragma unroll
            for (int blk = 0; blk < PN_BK / 8; ++blk) {
                const float4 xf = *reinterpret_cast<const float4 *>(Xb + blk * 8);
                float4 mf[4];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    if (mt < nmt) mf[mt] = *reinterpret_cast<const float4 *>(Mb + mt * 32 * PN_LD + blk * 8);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    if (mt < nmt) {
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(mf[mt].x, xf.x, acc[mt], 0, 0, 0);
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(mf[mt].y, xf.y, acc[mt], 0, 0, 0);
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(mf[mt].z, xf.z, acc[mt], 0, 0, 0);
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(mf[mt].w, xf.w, acc[mt], 0, 0, 0);
                    }
            }
        }
        // squares over ascending column: lane l (half 0) takes columns 8g..8g+3 of a tile, lane l + 32 columns 8g+4..8g+7
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            if (mt < nmt) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float pv[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = c0 + mt * 32 + 8 * g + 4 * half + e;
                        const float bias = (p.b && c < d_r) ? p.b[rel * p.ldb + c] : 0.f;
                        pv[e] = p.b ? acc[mt][4 * g + e] + bias : acc[mt][4 * g + e];
                    }
                    float a = s;
#pragma unroll
                    for (int e = 0; e < 4; ++e) a = fmaf(pv[e], pv[e], a);
                    s = half ? s : a;                       // half 0 has added its four columns
                    float o = __shfl_xor(s, 32, 64);
                    s = half ? o : s;                       // ... and hands the sum to half 1
                    a = s;
#pragma unroll
                    for (int e = 0; e < 4; ++e) a = fmaf(pv[e], pv[e], a);
                    s = half ? a : s;
                    o = __shfl_xor(s, 32, 64);
                    s = half ? s : o;                       // back in half 0 (half 1 keeps the same value)
                }
            }
        }
    }
    const int64_t j = j0 + wid * 32 + l31;
    if (half == 0 && j < p.n) p.out[rel * p.os_r + j * p.os_j] = s;
}

// ---- b. query transform ---------------------------------------------------------------------------------------------
// out[pos, j] = chain_k in(pos)[k] * C[k][j]  (+ sgn(pos) * R[rel(pos), j]),  k ascending, one accumulator per output.
//   stage 1 (TO_REL):  in = entity rows (d_e), C[k][j] = M_r[j, k], j < d_r, bias = the relation row (tail +, head -)
//   stage 2 (!TO_REL): in = the q rows of stage 1 (d_r), C[k][j] = M_r[k, j], j < d_e, no bias
// An Op of rel_query_kernel (rel_operator.h); a run is one relation: both sides read M_r in the same index order and
// differ in the sign of the bias only.  Instantiated in the general form alone (no unrolled whole-chunk loop).
struct TransROp {
    int K, J;                           // stage 1: (d_e, d_r), stage 2: (d_r, d_e)
    int side, to_rel;
    const float *M; int64_t ldm;
    const float *R; int64_t ldr;        // stage 1 bias table (n_rel, d_r)
    const int64_t *h, *t, *r;           // h, t: stage 1 over the entity table; NULL: the rows of X by position
    int64_t n_facts;
    int d_e;

    __device__ RelRow row(int64_t pos) const
    {
        const bool second = side == KGE_SIDE_BOTH && pos >= n_facts;
        const bool head = side == KGE_SIDE_HEAD || second;
        const int64_t f = second ? pos - n_facts : pos;
        return RelRow{pos, r[f], (to_rel && h) ? (head ? t[f] : h[f]) : pos, head ? -1.f : 1.f};
    }
    struct Coefs {
        int to_rel, d_e;
        const float *Mr;
        __device__ bool k_contiguous() const { return to_rel != 0; }     // M[j][k]; stage 2 reads M[k][j]
        __device__ float operator()(int k, int j) const { return to_rel ? Mr[(int64_t)j * d_e + k] : Mr[(int64_t)k * d_e + j]; }
    };
    __device__ Coefs coefs(int64_t rel) const { return Coefs{to_rel, d_e, M + rel * ldm}; }
    __device__ float finish(const RelRow &w, int j, float acc) const
    {
        return (to_rel && R) ? fmaf(w.sgn, R[w.key * ldr + j], acc) : acc;
    }
};

// ---- c. scoring_function --------------------------------------------------------------------------------------------
// x^ = x / max(||x||, 1e-12) of the gathered h, t rows, v = h^ - t^, p_c = chain_k M_r[c, k] v_k (k ascending) + r_c,
// score = -sum_c p_c^2 (lanes over c, fmaf per lane in ascending c, then the wavefront tree).  One triple per wave.
struct RScoreParams {
    const float *E, *R, *M;
    int d_e, d_r;
    const int64_t *h, *t, *r;
    int64_t B;
    float *out;
    const float *go;
    float *rows;
    int64_t rows_ld;
};

__global__ __launch_bounds__(SC_WAVES * 64) void transr_score_fwd_kernel(const RScoreParams p)
{
    __shared__ float hs[SC_WAVES][REL_MAXD], ts[SC_WAVES][REL_MAXD];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, d_e = p.d_e, d_r = p.d_r;
    for (int64_t base = (int64_t)blockIdx.x * SC_WAVES; base < p.B; base += (int64_t)gridDim.x * SC_WAVES) {
        const int64_t i = base + w;
        const bool ok = i < p.B;
        if (ok) {
            load_normalized(p.E + p.h[i] * d_e, d_e, lane, hs[w]);
            load_normalized(p.E + p.t[i] * d_e, d_e, lane, ts[w]);
        }
        __syncthreads();
        if (ok) {
            for (int k = lane; k < d_e; k += 64) hs[w][k] = hs[w][k] - ts[w][k];
        }
        __syncthreads();
        if (ok) {
            const float *Mr = p.M + p.r[i] * (int64_t)d_r * d_e, *rr = p.R + p.r[i] * d_r;
            float part = 0.f;
            for (int c = lane; c < d_r; c += 64) {
                const float *mc = Mr + (int64_t)c * d_e;
                float u = 0.f;
                for (int k = 0; k < d_e; ++k) u = fmaf(mc[k], hs[w][k], u);
                u = u + rr[c];
                part = fmaf(u, u, part);
            }
            const float sc = wave_sum(part);
            if (lane == 0) p.out[i] = -sc;
        }
        __syncthreads();
    }
}

// backward (row mode): g = -2 go p;  streams 0 / 1: d h / d t (through the normalisation), 2: g (d rel_emb, and the
// left operand of kge_transr_rel_grad), 3: v = h^ - t^ (its right operand)
__global__ __launch_bounds__(SC_WAVES * 64) void transr_score_bwd_kernel(const RScoreParams p)
{
    __shared__ float hs[SC_WAVES][REL_MAXD], ts[SC_WAVES][REL_MAXD], vs[SC_WAVES][REL_MAXD], gs[SC_WAVES][REL_MAXD];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, d_e = p.d_e, d_r = p.d_r;
    for (int64_t base = (int64_t)blockIdx.x * SC_WAVES; base < p.B; base += (int64_t)gridDim.x * SC_WAVES) {
        const int64_t i = base + w;
        const bool ok = i < p.B;
        float nh = 1.f, nt = 1.f;
        if (ok) {
            nh = load_normalized(p.E + p.h[i] * d_e, d_e, lane, hs[w]);
            nt = load_normalized(p.E + p.t[i] * d_e, d_e, lane, ts[w]);
        }
        __syncthreads();
        if (ok) {
            for (int k = lane; k < d_e; k += 64) vs[w][k] = hs[w][k] - ts[w][k];
        }
        __syncthreads();
        const float *Mr = ok ? p.M + p.r[i] * (int64_t)d_r * d_e : nullptr;
        if (ok) {
            const float go = p.go[i];
            const float *rr = p.R + p.r[i] * d_r;
            for (int c = lane; c < d_r; c += 64) {
                const float *mc = Mr + (int64_t)c * d_e;
                float u = 0.f;
                for (int k = 0; k < d_e; ++k) u = fmaf(mc[k], vs[w][k], u);
                u = u + rr[c];
                gs[w][c] = -2.f * go * u;
            }
        }
        __syncthreads();
        if (ok) {
            float *G = p.rows + ((int64_t)2 * p.B + i) * p.rows_ld, *V = p.rows + ((int64_t)3 * p.B + i) * p.rows_ld;
            for (int c = lane; c < d_r; c += 64) G[c] = gs[w][c];
            for (int k = lane; k < d_e; k += 64) V[k] = vs[w][k];
            // d v_k = chain_c M_r[c, k] g_c;  d h^ = d v, d t^ = -d v
            float sh = 0.f, st = 0.f;
            float dv[REL_MAXD / 64];
#pragma unroll
            for (int q = 0; q < REL_MAXD / 64; ++q) {
                const int k = lane + 64 * q;
                float u = 0.f;
                if (k < d_e) {
                    for (int c = 0; c < d_r; ++c) u = fmaf(Mr[(int64_t)c * d_e + k], gs[w][c], u);
                    sh = fmaf(hs[w][k], u, sh);
                    st = fmaf(ts[w][k], -u, st);
                }
                dv[q] = u;
            }
            sh = wave_sum(sh); st = wave_sum(st);
            const bool ch = nh <= 1e-12f, ct = nt <= 1e-12f;
            float *DH = p.rows + i * p.rows_ld, *DT = p.rows + ((int64_t)p.B + i) * p.rows_ld;
#pragma unroll
            for (int q = 0; q < REL_MAXD / 64; ++q) {
                const int k = lane + 64 * q;
                if (k < d_e) {
                    DH[k] = ch ? dv[q] / nh : (dv[q] - hs[w][k] * sh) / nh;
                    DT[k] = ct ? -dv[q] / nt : (-dv[q] - ts[w][k] * st) / nt;
                }
            }
        }
        __syncthreads();
    }
}

// ---- d. the per-relation outer-product reduction --------------------------------------------------------------------
// d proj_mat, and with d_r = d_e RESCAL's d rel_mat (kge_rel_outer_grad): gM[rho][a * d_e + b] = sum over the triples of
// rho, in sorted order, of U_i[a] V_i[b] (a < d_r, b < d_e) -- a GEMM whose K is the relation's triples.  One block per
// (relation, 64 x 64 tile); rho's segment of perm by binary search.
constexpr int RG_KC = 16;       // triples staged per step

__global__ __launch_bounds__(256) void rel_outer_grad_kernel(const float *__restrict__ U, int64_t ldu,
                                                             const float *__restrict__ V, int64_t ldv, int d_r, int d_e,
                                                             const int64_t *__restrict__ r,
                                                             const int64_t *__restrict__ perm, int64_t B,
                                                             float *__restrict__ gM, int64_t ldg)
{
    __shared__ float Us[RG_KC][QT_COLS + 1], Vs[RG_KC][QT_COLS + 1];
    __shared__ int64_t seg[2];
    __shared__ int64_t rowid[RG_KC];
    const int64_t rho = blockIdx.x;
    const int ntb = (d_e + QT_COLS - 1) / QT_COLS;
    const int a0 = (blockIdx.y / ntb) * QT_COLS, b0 = (blockIdx.y % ntb) * QT_COLS;
    const int tid = threadIdx.x;
    if (tid < 2) {
        int64_t lo = 0, hi = B;
        const int64_t key = rho + tid;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (r[perm[mid]] < key) lo = mid + 1;
            else hi = mid;
        }
        seg[tid] = lo;
    }
    __syncthreads();
    const int64_t s0 = seg[0], s1 = seg[1];
    const int col = tid & (QT_COLS - 1), rg = tid / QT_COLS;
    float acc[QT_PER_THREAD];
#pragma unroll
    for (int s = 0; s < QT_PER_THREAD; ++s) acc[s] = 0.f;
    for (int64_t j0 = s0; j0 < s1; j0 += RG_KC) {
        const int kn = (s1 - j0) < RG_KC ? (int)(s1 - j0) : RG_KC;
        if (tid < RG_KC) rowid[tid] = tid < kn ? perm[j0 + tid] : -1;
        __syncthreads();
        for (int idx = tid; idx < RG_KC * QT_COLS; idx += 256) {
            const int kk = idx / QT_COLS, cc = idx % QT_COLS;
            const int64_t i = rowid[kk];
            Us[kk][cc] = (i >= 0 && a0 + cc < d_r) ? U[i * ldu + a0 + cc] : 0.f;
            Vs[kk][cc] = (i >= 0 && b0 + cc < d_e) ? V[i * ldv + b0 + cc] : 0.f;
        }
        __syncthreads();
        for (int kk = 0; kk < kn; ++kk) {
            const float v = Vs[kk][col];
#pragma unroll
            for (int s = 0; s < QT_PER_THREAD; ++s) acc[s] = fmaf(Us[kk][rg + 4 * s], v, acc[s]);
        }
        __syncthreads();
    }
    const int b = b0 + col;
    if (b < d_e) {
#pragma unroll
        for (int s = 0; s < QT_PER_THREAD; ++s) {
            const int a = a0 + rg + 4 * s;
            if (a < d_r) gM[rho * ldg + (int64_t)a * d_e + b] = acc[s];
        }
    }
}

inline int check_dims(int d_e, int d_r)
{
    if (d_e < 1 || d_r < 1) return KGE_EINVAL;
    if (d_e > REL_MAXD || d_r > REL_MAXD) return KGE_EUNSUPPORTED;
    return 0;
}

} // namespace

// the reduction behind kge_transr_rel_grad and kge_rescal_rel_grad (declared in kge_common.h): arguments validated by
// the caller, n_rel in [1, 2^31)
int kge_rel_outer_grad(const float *U, int64_t ldu, const float *V, int64_t ldv, int d_r, int d_e, const int64_t *r,
                       const int64_t *perm, int64_t B, int64_t n_rel, float *gM, int64_t ldg, hipStream_t s)
{
    const int nta = (d_r + QT_COLS - 1) / QT_COLS, ntb = (d_e + QT_COLS - 1) / QT_COLS;
    hipLaunchKernelGGL(rel_outer_grad_kernel, dim3((unsigned)n_rel, (unsigned)(nta * ntb)), dim3(256), 0, s,
                       U, ldu, V, ldv, d_r, d_e, r, perm, B, gM, ldg);
    KGE_CHECK_LAUNCH();
    return 0;
}

// KGE_TRANSR behind kge_score_triples / kge_score_triples_bwd (declared in kge_common.h)
int kge_transr_score_fwd(const float *E, const float *R, const float *M, int d_ent, int d_rel, const int64_t *h,
                         const int64_t *t, const int64_t *r, int64_t B, float *out, hipStream_t s)
{
    int rc = check_dims(d_ent, d_rel);
    if (rc) return rc;
    if (!E || !R || !M || B < 0 || (B > 0 && (!h || !t || !r || !out))) return KGE_EINVAL;
    if (B == 0) return 0;
    RScoreParams p{E, R, M, d_ent, d_rel, h, t, r, B, out, nullptr, nullptr, 0};
    hipLaunchKernelGGL(transr_score_fwd_kernel, dim3(sc_grid(B)), dim3(SC_WAVES * 64), 0, s, p);
    KGE_CHECK_LAUNCH();
    return 0;
}

int kge_transr_score_bwd(const float *E, const float *R, const float *M, int d_ent, int d_rel, const int64_t *h,
                         const int64_t *t, const int64_t *r, int64_t B, const float *go, float *rows, int64_t rows_ld,
                         hipStream_t s)
{
    int rc = check_dims(d_ent, d_rel);
    if (rc) return rc;
    if (!E || !R || !M || B < 0 || (B > 0 && (!h || !t || !r || !go))) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!rows || rows_ld < d_ent || rows_ld < d_rel) return KGE_EINVAL;     // row mode only: d proj_mat is never scattered
    RScoreParams p{E, R, M, d_ent, d_rel, h, t, r, B, nullptr, go, rows, rows_ld};
    hipLaunchKernelGGL(transr_score_bwd_kernel, dim3(sc_grid(B)), dim3(SC_WAVES * 64), 0, s, p);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_transr_proj_sqnorm(const float *M, int64_t ldm, const float *X, int64_t ldx, const float *b,
                                      int64_t ldb, const int64_t *rels, int64_t n_list, int64_t n, int d_e, int d_r,
                                      float *out, int64_t os_r, int64_t os_j, kge_stream_t stream)
{
    int rc = check_dims(d_e, d_r);
    if (rc) return rc;
    if (n < 0 || n_list < 0 || ldx < d_e || ldm < (int64_t)d_e * d_r || (b && ldb < d_r)) return KGE_EINVAL;
    if (n == 0 || n_list == 0) return 0;
    if (!M || !X || !out) return KGE_EINVAL;
    const int64_t tiles = (n + PN_ROWS - 1) / PN_ROWS;
    if (tiles > 0x7fffffffll || n_list > 65535) return KGE_EINVAL;
    ProjNormParams p{M, ldm, X, ldx, b, ldb, rels, n, d_e, d_r, out, os_r, os_j};
    const dim3 grid((unsigned)tiles, (unsigned)n_list);
    const bool vec4 = d_e % 4 == 0 && ldx % 4 == 0 && ldm % 4 == 0 && kge_aligned16(M) && kge_aligned16(X);
    if (vec4) hipLaunchKernelGGL(proj_sqnorm_kernel<true>, grid, dim3(PN_THREADS), 0, kge_s(stream), p);
    else hipLaunchKernelGGL(proj_sqnorm_kernel<false>, grid, dim3(PN_THREADS), 0, kge_s(stream), p);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_transr_query(int side, const float *X, int64_t ldx, const float *M, int64_t ldm, const float *R,
                                int64_t ldr, int d_e, int d_r, const int64_t *h, const int64_t *t, const int64_t *r,
                                int64_t B, const int64_t *perm, float *Q, int64_t ldq, float *U, int64_t ldu,
                                kge_stream_t stream)
{
    int rc = check_dims(d_e, d_r);
    if (rc) return rc;
    if (side != KGE_SIDE_TAIL && side != KGE_SIDE_HEAD && side != KGE_SIDE_BOTH) return KGE_EINVAL;
    if (B < 0 || (X && ldx < d_e) || ldq < d_r || ldm < (int64_t)d_e * d_r || (R && ldr < d_r) || (U && ldu < d_e)) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!M || !r || !Q || (!X && !U)) return KGE_EINVAL;
    if ((h == nullptr) != (t == nullptr)) return KGE_EINVAL;    // both index vectors, or gathered rows by position
    const int64_t rows = side == KGE_SIDE_BOTH ? 2 * B : B;
    const int64_t tiles = (rows + QT_ROWS - 1) / QT_ROWS;
    if (tiles > 0x7fffffffll) return KGE_EINVAL;
    hipStream_t s = kge_s(stream);
    if (X) {            // X NULL: Q is given (a query already in relation space), only U is computed
        const RelQueryIO io{X, ldx, perm, rows, Q, ldq};
        const TransROp op{d_e, d_r, side, 1, M, ldm, R, ldr, h, t, r, B, d_e};
        hipLaunchKernelGGL((rel_query_kernel<TransROp, false>), dim3((unsigned)tiles, (unsigned)((d_r + QT_COLS - 1) / QT_COLS)),
                           dim3(QT_THREADS), 0, s, io, op);
        KGE_CHECK_LAUNCH();
    }
    if (U) {
        const RelQueryIO io{Q, ldq, perm, rows, U, ldu};
        const TransROp op{d_r, d_e, side, 0, M, ldm, nullptr, 0, nullptr, nullptr, r, B, d_e};
        hipLaunchKernelGGL((rel_query_kernel<TransROp, false>), dim3((unsigned)tiles, (unsigned)((d_e + QT_COLS - 1) / QT_COLS)),
                           dim3(QT_THREADS), 0, s, io, op);
        KGE_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int kge_transr_rel_grad(const float *U, int64_t ldu, const float *V, int64_t ldv, int d_r, int d_e,
                                   const int64_t *r, const int64_t *perm, int64_t B, int64_t n_rel, float *gM,
                                   int64_t ldg, kge_stream_t stream)
{
    int rc = check_dims(d_e, d_r);
    if (rc) return rc;
    if (B < 0 || n_rel < 0 || ldu < d_r || ldv < d_e || ldg < (int64_t)d_r * d_e) return KGE_EINVAL;
    if (n_rel == 0) return 0;
    if (!gM || (B > 0 && (!U || !V || !r || !perm))) return KGE_EINVAL;
    if (n_rel > 0x7fffffffll) return KGE_EINVAL;
    return kge_rel_outer_grad(U, ldu, V, ldv, d_r, d_e, r, perm, B, n_rel, gM, ldg, kge_s(stream));
}
