// 1-vs-all training (include/kge_hip_xent.h): softmax cross-entropy of every query row of a KGE_LP_DOT problem over
// all N candidates, and its gradients, without the (B, N) score matrix (gfx950).
//
// Every kernel recomputes the score tile it needs with score_tile() of lp_tile64.h -- the skeleton this criterion shares
// with lp_bce.hip: the bit-defined 64 x 64 score tile, the chunk arithmetic, the statistics walk (block = (row panel,
// candidate chunk), S tile through LDS to a row-wise pass, one partial per (row, chunk)), the gradient walk (S tile -> G
// tile in LDS -> MFMA operand, dA per (row panel, chunk, column slice) into the workspace, dT per (candidate tile, column
// slice) stored once), the chunk sum of dA, the entries' shared checks and the two launch sequences.  The kernels here
// are one-line bodies around it.  What is this criterion's own:
//  * XentStat: a thread's 16 candidates of a row keep (m, l, sum s) online across the chunk; the row's four threads
//    merge in LDS into the (row, chunk) partial; the thread that meets the target writes s(i, t_i);
//  * xent_finish_kernel: one block per panel merges the chunks in ascending order, writes lse / row_loss;
//  * XentCrit: G(i, c) = g_i (expf(s - lse_i) - q(i, c)) from the panel's (lse, g, target) in LDS;
//  * the parameter block, the workspace layout and the four extern "C" entries.
#include "kge_common.h"
#include "../../include/kge_hip_xent.h"
#include "lp_tile64.h"

namespace {

using namespace tile64;
static_assert(BM == KGE_XENT_BM && BN == KGE_XENT_BN && KSLICE == KGE_XENT_KSLICE &&
              MIN_TILES_PER_CHUNK == KGE_XENT_MIN_TILES_PER_CHUNK && MAX_CHUNKS == KGE_XENT_MAX_CHUNKS &&
              MAX_K == KGE_XENT_MAX_K, "the geometry the header publishes");

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

// the softmax statistics of stats_walk(): (m, l) online and the fp64 sum of the scores, per thread
struct XentStat {
    const XentParams &p;
    float *m_s, *l_s;
    double *ss_s;
    int64_t tgt;
    float m, l;
    double ss;
    __device__ __forceinline__ void start(int64_t row, bool ok, int64_t)
    {
        tgt = ok ? p.target[row] : -1;
        m = -INFINITY; l = 0.f; ss = 0.0;
    }
    __device__ __forceinline__ void tile(int64_t) {}
    __device__ __forceinline__ void add(const float *s, int64_t row, int64_t col0, int c_lo, int cnt)
    {
        float v[16];
        float tmax = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            v[e] = s[c_lo + e];
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
        if (tc >= c_lo && tc < c_lo + cnt) p.ws_st[row] = s[(int)tc];
    }
    __device__ __forceinline__ void publish(int tid) { m_s[tid] = m; l_s[tid] = l; ss_s[tid] = ss; }
    __device__ __forceinline__ void write(int64_t row, int chunk, int tid) const
    {
        float M, L;
        merge_ml(m_s + tid, l_s + tid, 4, M, L);
        const double SS = ((ss_s[tid] + ss_s[tid + 1]) + ss_s[tid + 2]) + ss_s[tid + 3];
        p.ws_ml[row * p.chunks + chunk] = make_float2(M, L);
        p.ws_ss[row * p.chunks + chunk] = SS;
    }
};

// (NTHREADS, 4): the block's LDS lets four blocks share a CU -- four waves per SIMD -- and the registers are held to that
template <bool VEC4>
__global__ __launch_bounds__(NTHREADS, 4) void xent_stats_kernel(const XentParams p)
{
    __shared__ __attribute__((aligned(16))) float As[BM * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LDS_LD];
    __shared__ float Ss[BM * G_LD];
    __shared__ float m_s[BM * 4], l_s[BM * 4];
    __shared__ double ss_s[BM * 4];
    XentStat stat = {p, m_s, l_s, ss_s};
    stats_walk<VEC4>(p, stat, As, Bs, Ss);
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

// validation of both entries (tile64::setup) and what is this criterion's own of the parameter block
int xent_setup(const kge_lp_desc *d, const int64_t *target, float eps, void *ws, size_t ws_bytes, XentParams &p)
{
    if (int e = setup(d, target != nullptr, eps, ws, ws_bytes, kge_lp_xent_ws_bytes, p)) return e;
    if (d->B == 0) return 0;
    p.target = target;
    p.eps = eps;
    p.one_m_eps = 1.0f - eps;
    p.eps_n = eps / (float)d->N;
    p.q_t = p.one_m_eps + p.eps_n;
    char *w = static_cast<char *>(ws);
    p.ws_ss = reinterpret_cast<double *>(w);
    p.ws_ml = reinterpret_cast<float2 *>(w + (size_t)8 * d->B * p.chunks);
    p.ws_st = reinterpret_cast<float *>(w + (size_t)16 * d->B * p.chunks);
    p.ws_da = reinterpret_cast<float *>(w + (size_t)16 * d->B * p.chunks + align16((size_t)4 * d->B));
    return 0;
}

} // namespace

extern "C" int kge_lp_xent_chunks(int64_t N) { return chunk_count(N); }

extern "C" size_t kge_lp_xent_ws_bytes(int64_t B, int64_t N, int K0, int K1)
{
    if (B <= 0 || N <= 0 || K0 <= 0 || K1 < 0 || (int64_t)K0 + K1 > MAX_K) return 0;
    if (B >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31)) return 0;
    const size_t chunks = (size_t)chunk_count(N);
    return (size_t)16 * B * chunks + align16((size_t)4 * B) + (size_t)4 * chunks * B * (size_t)(K0 + K1);
}

extern "C" int kge_lp_xent_fwd(const kge_lp_desc *desc, const int64_t *target, float label_smoothing, float *lse,
                               float *row_loss, void *ws, size_t ws_bytes, kge_stream_t stream)
{
    XentParams p = {};
    if (!lse || !row_loss) return KGE_EINVAL;
    if (int e = xent_setup(desc, target, label_smoothing, ws, ws_bytes, p)) return e;
    p.lse = lse;
    p.row_loss = row_loss;
    return launch_fwd(xent_stats_kernel<false>, xent_stats_kernel<true>, xent_finish_kernel, p, kge_s(stream));
}

extern "C" int kge_lp_xent_bwd(const kge_lp_desc *desc, const int64_t *target, float label_smoothing, const float *lse,
                               const float *g, float *dA0, int64_t ldda0, float *dA1, int64_t ldda1, float *dT0,
                               int64_t lddt0, float *dT1, int64_t lddt1, void *ws, size_t ws_bytes, kge_stream_t stream)
{
    XentParams p = {};
    if (!lse || !g) return KGE_EINVAL;
    if (int e = xent_setup(desc, target, label_smoothing, ws, ws_bytes, p)) return e;
    p.lse_in = lse;
    p.g = g;
    return launch_bwd(xent_grad_kernel<false, true>, xent_grad_kernel<true, true>, xent_grad_kernel<false, false>,
                      xent_grad_kernel<true, false>, xent_sum_chunks_kernel, p, dA0, ldda0, dA1, ldda1, dT0, lddt0, dT1, lddt1,
                      kge_s(stream));
}
