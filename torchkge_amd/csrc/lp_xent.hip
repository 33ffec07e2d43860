// 1-vs-all training (include/kge_hip_xent.h): softmax cross-entropy of every query row of a KGE_LP_DOT problem over
// all N candidates, and its gradients, without the (B, N) score matrix (gfx950).
//
// Every kernel recomputes the score tile it needs with score_tile(): the 32x32x2 fp32 MFMA loop of lp_gemm_mfma.hip in
// the same k-order (8-blocks ascending, k = 0,4,1,5,2,6,3,7 inside, segment 1 continuing segment 0's accumulator), so a
// score here has the bits of kge_lp_scores / kge_lp_pair_scores (kge_common.h: lp_chain_dot).
//
// Structure
//  * tile 64 queries x 64 candidates, 4 waves as 2 x 2 of one 32x32 MFMA tile each, BK = 32 per step; operands staged
//    global -> VGPR -> LDS (row stride 36 floats, the conflict-free b128 pattern of lp_gemm_mfma.hip), the global loads
//    of step s + 1 in flight under the MFMAs of step s.  Rows beyond B / N are clamped DUPLICATES, as there -- and
//    unlike there they would enter a sum, so every epilogue here masks them;
//  * xent_stats_kernel: block = (row panel, candidate chunk); the S tile goes through LDS to a row-wise pass (4 threads
//    per row, 16 candidates each) that keeps (m, l, sum s) online across the chunk; one partial per (row, chunk);
//  * xent_finish_kernel: one block per panel merges the chunks in ascending order, writes lse / row_loss;
//  * xent_grad_kernel<TR>: S tile -> G tile in LDS -> MFMA operand.  TR = false (dA = G.T): block = (row panel, chunk,
//    column slice), G rows are the MFMA's A operand, T rows come straight from global (a lane reads 32 consecutive
//    floats of one row: whole 128-byte lines, used by both 32-row halves), the partial panel goes to the workspace.
//    TR = true (dT = G^T.A): block = (candidate tile, column slice) walks all row panels, G columns are the A operand,
//    the query rows come from global, the result is stored once.  Up to 512 output columns per block: 2 x 4 MFMA tiles
//    = 128 accumulator VGPRs per lane; K0 + K1 > 512 takes a second slice (and recomputes S for it);
//  * xent_sum_chunks_kernel: dA = the partial panels added in ascending chunk order.
#include "kge_common.h"
#include "../../include/kge_hip_xent.h"

#ifndef KGE_BUILD_NO_SLP
#error "build with -fno-slp-vectorize -DKGE_BUILD_NO_SLP=1 (torchkge_amd/csrc/build.py): VALU epilogues beside co-executing MFMAs (DESIGN.md 3.6)"
#endif

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int BM = KGE_XENT_BM, BN = KGE_XENT_BN, BK = 32, LDS_LD = BK + 4, G_LD = BN + 1;
constexpr int NTHREADS = 256;
constexpr int SLICE_TILES = KGE_XENT_KSLICE / 32;   // 32-column MFMA tiles of one slice
constexpr int CT = SLICE_TILES / 4;                 // ... per wave (tile 4 ct + wave)
constexpr int XG = 8;                               // MFMA steps per prefetch group of the product phase
static_assert((32 / XG) % 2 == 0, "the product phase alternates two register sets");
static_assert(BM == 64 && BN == 64, "2 x 2 waves of one 32x32 tile each");

struct XentParams {
    kge_lp_desc d;
    const int64_t *target;
    const float *lse_in, *g;
    float one_m_eps, eps, eps_n, q_t;   // q_t = (1 - eps) + eps / N: what the target's probability is compared with
    int chunks, col_tiles, row_panels;
    // workspace
    double *ws_ss;      // [B][chunks] sum of scores
    float2 *ws_ml;      // [B][chunks] (m, l)
    float *ws_st;       // [B] s(i, t_i)
    float *ws_da;       // [chunks][B][K0 + K1]
    // outputs
    float *lse, *row_loss;
    float *o0, *o1;     // gradient group of the launch (dA: unused, the workspace is written)
    int64_t ldo0, ldo1;
};

// S tile (64 x 64 at (row0, col0)) of the descriptor's DOT score: this wave's 32x32 part in acc (row r of the MFMA
// layout: (r & 3) + 8 (r >> 2) + 4 half, column l31).  Block-uniform; starts and ends with LDS free for the caller.
template <bool VEC4>
__device__ __forceinline__ void score_tile(const kge_lp_desc &d, int64_t row0, int64_t col0, float *As, float *Bs,
                                           f32x16 &acc)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    const int srow = tid >> 3, spc = tid & 7;     // staging: 16-byte piece spc of rows srow, srow + 32
    int64_t ra[2], rb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ra[j] = min(row0 + srow + 32 * j, d.B - 1);
        rb[j] = min(col0 + srow + 32 * j, d.N - 1);
    }
    const int steps0 = (d.K0 + BK - 1) / BK, steps1 = (d.K1 + BK - 1) / BK, S = steps0 + steps1;
    float4 sa[2], sb[2];
    auto load_step = [&](int s) {   // unconditional loads from clamped addresses; k >= K zeroed
        const bool seg1 = s >= steps0;
        const float *A = seg1 ? d.A1 : d.A0, *T = seg1 ? d.T1 : d.T0;
        const int64_t lda = seg1 ? d.lda1 : d.lda0, ldt = seg1 ? d.ldt1 : d.ldt0;
        const int K = seg1 ? d.K1 : d.K0;
        const int k = (seg1 ? s - steps0 : s) * BK + spc * 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float *pa = A + ra[j] * lda, *pb = T + rb[j] * ldt;
            if (VEC4) {
                const int kc = k < K ? k : 0;
                float4 a = *reinterpret_cast<const float4 *>(pa + kc), b = *reinterpret_cast<const float4 *>(pb + kc);
                if (k >= K) { a = make_float4(0.f, 0.f, 0.f, 0.f); b = a; }
                sa[j] = a; sb[j] = b;
            } else {
                float a[4], b[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kc = k + e < K ? k + e : 0;
                    a[e] = pa[kc]; b[e] = pb[kc];
                    if (k + e >= K) { a[e] = 0.f; b[e] = 0.f; }
                }
                sa[j] = make_float4(a[0], a[1], a[2], a[3]);
                sb[j] = make_float4(b[0], b[1], b[2], b[3]);
            }
        }
    };
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    load_step(0);
    for (int s = 0; s < S; ++s) {
        __syncthreads();    // the previous step's (or the caller's) LDS reads are done
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            *reinterpret_cast<float4 *>(As + (srow + 32 * j) * LDS_LD + spc * 4) = sa[j];
            *reinterpret_cast<float4 *>(Bs + (srow + 32 * j) * LDS_LD + spc * 4) = sb[j];
        }
        __syncthreads();
        if (s + 1 < S) load_step(s + 1);
        const bool seg1 = s >= steps0;
        const int K = seg1 ? d.K1 : d.K0, kb = (seg1 ? s - steps0 : s) * BK;
        const int nblk = min(4, (K - kb + 7) >> 3);
        const float *Ab = As + (wr * 32 + l31) * LDS_LD + half * 4;
        const float *Bb = Bs + (wc * 32 + l31) * LDS_LD + half * 4;
        for (int blk = 0; blk < nblk; ++blk) {
            const float4 af = *reinterpret_cast<const float4 *>(Ab + blk * 8);
            const float4 bf = *reinterpret_cast<const float4 *>(Bb + blk * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, acc, 0, 0, 0);
        }
    }
}

// merge of online-softmax partials in the given order: (M, L) <- (m[0..n), l[0..n))
__device__ __forceinline__ void merge_ml(const float *m, const float *l, int n, float &M, float &L)
{
    M = m[0];
    for (int q = 1; q < n; ++q) M = fmaxf(M, m[q]);
    L = 0.f;
    for (int q = 0; q < n; ++q) L += l[q] * expf(m[q] - M);     // an empty partial is (-inf, 0): adds 0
}

template <bool VEC4>
__global__ __launch_bounds__(NTHREADS) void xent_stats_kernel(const XentParams p)
{
    __shared__ __attribute__((aligned(16))) float As[BM * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LDS_LD];
    __shared__ float Ss[BM * G_LD];
    __shared__ float m_s[BM * 4], l_s[BM * 4];
    __shared__ double ss_s[BM * 4];
    const kge_lp_desc &d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    const int chunk = blockIdx.x;
    const int64_t row0 = (int64_t)blockIdx.y * BM;
    const int t0 = (int)((int64_t)p.col_tiles * chunk / p.chunks), t1 = (int)((int64_t)p.col_tiles * (chunk + 1) / p.chunks);

    const int prow = tid >> 2, pq = tid & 3;      // row-wise pass: candidates 16 pq .. 16 pq + 15 of row prow
    const int64_t row = row0 + prow;
    const int64_t tgt = row < d.B ? p.target[row] : -1;
    float m = -INFINITY, l = 0.f;
    double ss = 0.0;

    for (int t = t0; t < t1; ++t) {
        const int64_t col0 = (int64_t)t * BN;
        f32x16 acc;
        score_tile<VEC4>(d, row0, col0, As, Bs, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            Ss[(wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * G_LD + wc * 32 + l31] = acc[r];
        __syncthreads();
        const int nvalid = (int)min((int64_t)BN, d.N - col0), c_lo = pq * 16;
        if (c_lo < nvalid) {    // candidates >= N never enter
            const int cnt = min(16, nvalid - c_lo);
            float v[16];
            float tmax = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                v[e] = Ss[prow * G_LD + c_lo + e];
                if (e < cnt) tmax = fmaxf(tmax, v[e]);
            }
            const float mn = fmaxf(m, tmax);
            float sum = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (e < cnt) {
                    sum += expf(v[e] - mn);
                    ss += (double)v[e];
                }
            l = l * expf(m - mn) + sum;
            m = mn;
            const int64_t tc = tgt - col0;
            if (tc >= c_lo && tc < c_lo + cnt) p.ws_st[row] = Ss[prow * G_LD + (int)tc];
        }
        // (the next score_tile synchronises before anything overwrites Ss)
    }
    m_s[tid] = m; l_s[tid] = l; ss_s[tid] = ss;
    __syncthreads();
    if (pq == 0 && row < d.B) {
        float M, L;
        merge_ml(m_s + tid, l_s + tid, 4, M, L);
        const double SS = ((ss_s[tid] + ss_s[tid + 1]) + ss_s[tid + 2]) + ss_s[tid + 3];
        p.ws_ml[row * p.chunks + chunk] = make_float2(M, L);
        p.ws_ss[row * p.chunks + chunk] = SS;
    }
}

__global__ __launch_bounds__(BM) void xent_finish_kernel(const XentParams p)
{
    const int64_t row = (int64_t)blockIdx.x * BM + threadIdx.x;
    if (row >= p.d.B) return;
    const float2 *ml = p.ws_ml + row * p.chunks;
    float M = ml[0].x, L = 0.f;     // merge_ml over the chunks, from global
    for (int c = 1; c < p.chunks; ++c) M = fmaxf(M, ml[c].x);
    double SS = 0.0;
    for (int c = 0; c < p.chunks; ++c) {
        L += ml[c].y * expf(ml[c].x - M);
        SS += p.ws_ss[row * p.chunks + c];
    }
    const float lse = M + logf(L);
    const float st = p.ws_st[row];
    float loss = lse - st;
    if (p.eps != 0.f) {
        const float mean = (float)(SS / (double)p.d.N);
        const float a = p.one_m_eps * loss, b = p.eps * (lse - mean);
        loss = a + b;
    }
    p.lse[row] = lse;
    p.row_loss[row] = loss;
}

template <bool VEC4, bool TR>
__global__ __launch_bounds__(NTHREADS) void xent_grad_kernel(const XentParams p)
{
    __shared__ __attribute__((aligned(16))) float As[BM * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LDS_LD];
    __shared__ float Gs[BM * G_LD];
    __shared__ float lse_s[BM], g_s[BM];
    __shared__ int64_t tgt_s[BM];
    const kge_lp_desc &d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    const int Ktot = d.K0 + d.K1;
    const int chunk = TR ? 0 : (int)blockIdx.x;

    // the walk: candidate tiles of the chunk (dA) or all row panels (dT)
    int it0, it1;
    if (TR) { it0 = 0; it1 = p.row_panels; }
    else {
        it0 = (int)((int64_t)p.col_tiles * chunk / p.chunks);
        it1 = (int)((int64_t)p.col_tiles * (chunk + 1) / p.chunks);
    }
    const int64_t own0 = TR ? (int64_t)blockIdx.x * BN : (int64_t)blockIdx.y * BM;    // first candidate / row owned
    const int64_t own_n = TR ? d.N : d.B;

    // output columns: tile 4 ct + wid of the slice, column l31 of it.  X = the walked side's operand rows.
    const int j0 = (int)blockIdx.z * KGE_XENT_KSLICE;
    const float *xp[CT];
    int64_t xld[CT];
    bool xok[CT];
    int nct = 0;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int jt = j0 + (4 * ct + wid) * 32, j = jt + l31;
        if (jt < Ktot) nct = ct + 1;    // wave-uniform
        xok[ct] = j < Ktot;
        const int jc = xok[ct] ? j : 0;
        const bool s1 = jc >= d.K0;
        xp[ct] = s1 ? (TR ? d.A1 : d.T1) + (jc - d.K0) : (TR ? d.A0 : d.T0) + jc;
        xld[ct] = s1 ? (TR ? d.lda1 : d.ldt1) : (TR ? d.lda0 : d.ldt0);
    }

    f32x16 oacc[2][CT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[rt][ct][r] = 0.f;

    for (int it = it0; it < it1; ++it) {
        const int64_t row0 = TR ? (int64_t)it * BM : own0, col0 = TR ? own0 : (int64_t)it * BN;
        if ((TR || it == it0) && tid < BM) {    // (the previous epilogue's reads are behind the barrier before its MFMA phase)
            const int64_t row = row0 + tid;
            const bool ok = row < d.B;
            lse_s[tid] = ok ? p.lse_in[row] : 0.f;
            g_s[tid] = ok ? p.g[row] : 0.f;
            tgt_s[tid] = ok ? p.target[row] : -1;
        }
        f32x16 acc;
        score_tile<VEC4>(d, row0, col0, As, Bs, acc);   // (its barriers publish the panel vectors)
        // The product phase walks the tile's 64 rows of X in groups of XG MFMA steps (2 rows each), and the global
        // loads of group g + 1 are issued before the MFMAs of group g: a lane's XG x CT dwords are in flight under
        // 2 x CT x XG MFMAs.  The first group is issued here, under the epilogue's expf work.
        const int64_t x0 = TR ? row0 : col0, xn = TR ? d.B : d.N;
        auto load_group = [&](int grp, float (&xv)[XG][CT]) {
#pragma unroll
            for (int s = 0; s < XG; ++s) {
                const int64_t xr = min(x0 + 2 * (grp * XG + s) + half, xn - 1);     // clamped duplicate: its G is zero
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const float x = xp[ct][xr * xld[ct]];
                    xv[s][ct] = xok[ct] ? x : 0.f;
                }
            }
        };
        auto mma_group = [&](int grp, const float (&xv)[XG][CT]) {
#pragma unroll
            for (int s = 0; s < XG; ++s) {
                const int kk = 2 * (grp * XG + s) + half;
                float gv[2];
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
                    gv[rt] = TR ? Gs[kk * G_LD + 32 * rt + l31] : Gs[(32 * rt + l31) * G_LD + kk];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    if (ct < nct) {
#pragma unroll
                        for (int rt = 0; rt < 2; ++rt)
                            oacc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[rt], xv[s][ct], oacc[rt][ct], 0, 0, 0);
                    }
            }
        };
        float xa[XG][CT], xb[XG][CT];
        if (nct > 0) load_group(0, xa);
        const int cloc = wc * 32 + l31;
        const int64_t col = col0 + cloc;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rloc = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const float pe = expf(acc[r] - lse_s[rloc]);
            const float v = pe - (col == tgt_s[rloc] ? p.q_t : p.eps_n);
            const float G = g_s[rloc] * v;
            Gs[rloc * G_LD + cloc] = (row0 + rloc < d.B && col < d.N) ? G : 0.f;    // padded rows / columns: exact zeros
        }
        __syncthreads();
        if (nct > 0) {
#pragma unroll
            for (int grp = 0; grp < 32 / XG; grp += 2) {
                load_group(grp + 1, xb);
                mma_group(grp, xa);
                if (grp + 2 < 32 / XG) load_group(grp + 2, xa);
                mma_group(grp + 1, xb);
            }
        }
        // (the next score_tile synchronises before As / Bs change; Gs changes only after it)
    }

#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        if (!xok[ct]) continue;
        const int j = j0 + (4 * ct + wid) * 32 + l31;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t o = own0 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (o >= own_n) continue;
                if (TR) {
                    if (j < d.K0) p.o0[o * p.ldo0 + j] = oacc[rt][ct][r];
                    else p.o1[o * p.ldo1 + (j - d.K0)] = oacc[rt][ct][r];
                } else {
                    p.ws_da[((int64_t)chunk * d.B + o) * Ktot + j] = oacc[rt][ct][r];
                }
            }
    }
}

__global__ __launch_bounds__(256) void xent_sum_chunks_kernel(const XentParams p)
{
    const int Ktot = p.d.K0 + p.d.K1;
    const int64_t n = p.d.B * Ktot;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / Ktot;
        const int j = (int)(e - i * Ktot);
        float s = p.ws_da[e];
        for (int c = 1; c < p.chunks; ++c) s += p.ws_da[(int64_t)c * n + e];
        if (j < p.d.K0) p.o0[i * p.ldo0 + j] = s;
        else p.o1[i * p.ldo1 + (j - p.d.K0)] = s;
    }
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// shared validation of both entries; fills the geometry and the workspace pointers
int xent_setup(const kge_lp_desc *d, const int64_t *target, float eps, void *ws, size_t ws_bytes, XentParams &p, bool &vec4)
{
    if (!d) return KGE_EINVAL;
    if (d->mode != KGE_LP_DOT || d->c_base != 0) return KGE_EUNSUPPORTED;
    if (int e = kge_lp_desc_check(d)) return e;
    if ((int64_t)d->K0 + d->K1 > KGE_XENT_MAX_K) return KGE_EUNSUPPORTED;
    if (d->B >= ((int64_t)1 << 31) || d->N >= ((int64_t)1 << 31) || d->B > (int64_t)65535 * BM) return KGE_EUNSUPPORTED;
    if (!(eps >= 0.f && eps <= 1.f)) return KGE_EINVAL;
    if (d->B == 0) return 0;
    if (d->N <= 0 || !target) return KGE_EINVAL;
    if (d->lda0 < d->K0 && d->B > 1) return KGE_EINVAL;
    const size_t need = kge_lp_xent_ws_bytes(d->B, d->N, d->K0, d->K1);
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || need == 0 || ws_bytes < need) return KGE_EINVAL;
    p.d = *d;
    p.target = target;
    p.eps = eps;
    p.one_m_eps = 1.0f - eps;
    p.eps_n = eps / (float)d->N;
    p.q_t = p.one_m_eps + p.eps_n;
    p.chunks = kge_lp_xent_chunks(d->N);
    p.col_tiles = (int)((d->N + BN - 1) / BN);
    p.row_panels = (int)((d->B + BM - 1) / BM);
    char *w = static_cast<char *>(ws);
    p.ws_ss = reinterpret_cast<double *>(w);
    p.ws_ml = reinterpret_cast<float2 *>(w + (size_t)8 * d->B * p.chunks);
    p.ws_st = reinterpret_cast<float *>(w + (size_t)16 * d->B * p.chunks);
    p.ws_da = reinterpret_cast<float *>(w + (size_t)16 * d->B * p.chunks + align16((size_t)4 * d->B));
    vec4 = (d->K0 % 4 == 0) && (d->lda0 % 4 == 0) && (d->ldt0 % 4 == 0) && kge_aligned16(d->A0) && kge_aligned16(d->T0);
    if (d->K1 > 0)
        vec4 = vec4 && (d->K1 % 4 == 0) && (d->lda1 % 4 == 0) && (d->ldt1 % 4 == 0) && kge_aligned16(d->A1) &&
               kge_aligned16(d->T1);
    return 0;
}

} // namespace

extern "C" int kge_lp_xent_chunks(int64_t N)
{
    if (N <= 0) return 0;
    const int64_t tiles = (N + BN - 1) / BN;
    const int64_t c = (tiles + KGE_XENT_MIN_TILES_PER_CHUNK - 1) / KGE_XENT_MIN_TILES_PER_CHUNK;
    return (int)(c < KGE_XENT_MAX_CHUNKS ? c : KGE_XENT_MAX_CHUNKS);
}

extern "C" size_t kge_lp_xent_ws_bytes(int64_t B, int64_t N, int K0, int K1)
{
    if (B <= 0 || N <= 0 || K0 <= 0 || K1 < 0 || (int64_t)K0 + K1 > KGE_XENT_MAX_K) return 0;
    if (B >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31)) return 0;
    const size_t chunks = (size_t)kge_lp_xent_chunks(N);
    return (size_t)16 * B * chunks + align16((size_t)4 * B) + (size_t)4 * chunks * B * (size_t)(K0 + K1);
}

extern "C" int kge_lp_xent_fwd(const kge_lp_desc *desc, const int64_t *target, float label_smoothing, float *lse,
                               float *row_loss, void *ws, size_t ws_bytes, kge_stream_t stream)
{
    XentParams p = {};
    bool vec4 = false;
    if (!lse || !row_loss) return KGE_EINVAL;
    if (int e = xent_setup(desc, target, label_smoothing, ws, ws_bytes, p, vec4)) return e;
    if (desc->B == 0) return 0;
    p.lse = lse;
    p.row_loss = row_loss;
    hipStream_t s = kge_s(stream);
    const dim3 grid(p.chunks, p.row_panels);
    if (vec4) hipLaunchKernelGGL(xent_stats_kernel<true>, grid, dim3(NTHREADS), 0, s, p);
    else hipLaunchKernelGGL(xent_stats_kernel<false>, grid, dim3(NTHREADS), 0, s, p);
    KGE_CHECK_LAUNCH();
    hipLaunchKernelGGL(xent_finish_kernel, dim3(p.row_panels), dim3(BM), 0, s, p);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_lp_xent_bwd(const kge_lp_desc *desc, const int64_t *target, float label_smoothing, const float *lse,
                               const float *g, float *dA0, int64_t ldda0, float *dA1, int64_t ldda1, float *dT0,
                               int64_t lddt0, float *dT1, int64_t lddt1, void *ws, size_t ws_bytes, kge_stream_t stream)
{
    XentParams p = {};
    bool vec4 = false;
    if (!lse || !g) return KGE_EINVAL;
    if (int e = xent_setup(desc, target, label_smoothing, ws, ws_bytes, p, vec4)) return e;
    const bool want_a = dA0 != nullptr, want_t = dT0 != nullptr;
    if ((!want_a && dA1) || (!want_t && dT1)) return KGE_EINVAL;
    if (desc->K1 > 0 && ((want_a && !dA1) || (want_t && !dT1))) return KGE_EINVAL;
    if (want_a && ((ldda0 < desc->K0 && desc->B > 1) || (desc->K1 > 0 && ldda1 < desc->K1 && desc->B > 1))) return KGE_EINVAL;
    if (want_t && ((lddt0 < desc->K0 && desc->N > 1) || (desc->K1 > 0 && lddt1 < desc->K1 && desc->N > 1))) return KGE_EINVAL;
    if (desc->B == 0) return 0;
    p.lse_in = lse;
    p.g = g;
    hipStream_t s = kge_s(stream);
    const int slices = (desc->K0 + desc->K1 + KGE_XENT_KSLICE - 1) / KGE_XENT_KSLICE;
    if (want_t) {
        p.o0 = dT0; p.ldo0 = lddt0; p.o1 = dT1; p.ldo1 = lddt1;
        const dim3 grid(p.col_tiles, 1, slices);
        if (vec4) hipLaunchKernelGGL((xent_grad_kernel<true, true>), grid, dim3(NTHREADS), 0, s, p);
        else hipLaunchKernelGGL((xent_grad_kernel<false, true>), grid, dim3(NTHREADS), 0, s, p);
        KGE_CHECK_LAUNCH();
    }
    if (want_a) {
        p.o0 = dA0; p.ldo0 = ldda0; p.o1 = dA1; p.ldo1 = ldda1;
        const dim3 grid(p.chunks, p.row_panels, slices);
        if (vec4) hipLaunchKernelGGL((xent_grad_kernel<true, false>), grid, dim3(NTHREADS), 0, s, p);
        else hipLaunchKernelGGL((xent_grad_kernel<false, false>), grid, dim3(NTHREADS), 0, s, p);
        KGE_CHECK_LAUNCH();
        const int64_t n = desc->B * (int64_t)(desc->K0 + desc->K1);
        hipLaunchKernelGGL(xent_sum_chunks_kernel, dim3(grid1d(n, 256)), dim3(256), 0, s, p);
        KGE_CHECK_LAUNCH();
    }
    return 0;
}
