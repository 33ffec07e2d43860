// 1-vs-all training (include/kge_hip_xent.h): softmax cross-entropy of every query row of a KGE_LP_DOT problem over
// all N candidates, and its gradients, without the (B, N) score matrix (gfx950).
//
// Every kernel recomputes the score tile it needs with score_tile() of lp_tile64.h -- the skeleton this criterion shares
// with lp_bce.hip: the bit-defined 64 x 64 score tile, the gradient walk (S tile -> G tile in LDS -> MFMA operand, dA per
// (row panel, chunk, column slice) into the workspace, dT per (candidate tile, column slice) stored once) and the chunk
// sum of dA.  What is this criterion's own:
//  * xent_stats_kernel: block = (row panel, candidate chunk); the S tile goes through LDS to a row-wise pass (4 threads
//    per row, 16 candidates each) that keeps (m, l, sum s) online across the chunk; one partial per (row, chunk);
//  * xent_finish_kernel: one block per panel merges the chunks in ascending order, writes lse / row_loss;
//  * XentCrit: G(i, c) = g_i (expf(s - lse_i) - q(i, c)) from the panel's (lse, g, target) in LDS.
#include "kge_common.h"
#include "../../include/kge_hip_xent.h"
#include "lp_tile64.h"

namespace {

using namespace tile64;
static_assert(BM == KGE_XENT_BM && BN == KGE_XENT_BN && KSLICE == KGE_XENT_KSLICE, "the geometry the header publishes");

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

// the softmax criterion of grad_walk(): the panel's (lse, g, target) in LDS, one expf and one subtraction per element
struct XentCrit {
    const XentParams &p;
    float *lse_s, *g_s;
    int64_t *tgt_s;
    __device__ __forceinline__ void panel(int64_t row0, int64_t)
    {
        const int tid = threadIdx.x;
        if (tid < BM) {     // (the previous epilogue's reads are behind the barrier before its MFMA phase)
            const int64_t row = row0 + tid;
            const bool ok = row < p.d.B;
            lse_s[tid] = ok ? p.lse_in[row] : 0.f;
            g_s[tid] = ok ? p.g[row] : 0.f;
            tgt_s[tid] = ok ? p.target[row] : -1;
        }
    }
    __device__ __forceinline__ void tile(int64_t) {}
    __device__ __forceinline__ float G(int rloc, int, int64_t col, float s) const
    {
        const float pe = expf(s - lse_s[rloc]);
        const float v = pe - (col == tgt_s[rloc] ? p.q_t : p.eps_n);
        return g_s[rloc] * v;
    }
};

template <bool VEC4, bool TR>
__global__ __launch_bounds__(NTHREADS) void xent_grad_kernel(const XentParams p)
{
    __shared__ __attribute__((aligned(16))) float As[BM * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LDS_LD];
    __shared__ float Gs[BM * G_LD];
    __shared__ float lse_s[BM], g_s[BM];
    __shared__ int64_t tgt_s[BM];
    XentCrit crit = {p, lse_s, g_s, tgt_s};
    grad_walk<VEC4, TR>(p, crit, As, Bs, Gs);
}

__global__ __launch_bounds__(256) void xent_sum_chunks_kernel(const XentParams p) { sum_chunks(p); }

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
    vec4 = operands_vec4(d);
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
    if (int e = grad_groups_check(desc, dA0, ldda0, dA1, ldda1, dT0, lddt0, dT1, lddt1)) return e;
    const bool want_a = dA0 != nullptr, want_t = dT0 != nullptr;
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
