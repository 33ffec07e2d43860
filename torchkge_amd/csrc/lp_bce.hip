// K-vs-all training (include/kge_hip_bce.h): binary cross-entropy with logits of every query row of a KGE_LP_DOT problem
// over all N candidates against a CSR of true candidates, and its gradients, without the (B, N) score, label or gradient
// matrix (gfx950).
//
// The skeleton is lp_tile64.h's, shared with lp_xent.hip: the bit-defined 64 x 64 score tile, the chunk arithmetic, the
// statistics walk, the gradient walk, the chunk sum of dA, the entries' shared checks and the two launch sequences; the
// kernels here are one-line bodies around it.  What is this criterion's own:
//  * LabelCursor: a row's position in its sorted label segment.  Where a block walks candidate tiles in ascending order
//    (the stats sweep, dA) it is set by ONE lower_bound at the block's first tile and then only advances; in dT, where a
//    block owns one tile and walks the row panels, every (row, tile) takes one binary search.  The next label is kept in
//    a register, so a tile without labels of the row costs no load, and a hub segment costs O(log len + labels in the
//    tile), never O(len).  Both run BEFORE score_tile(), so the loads retire under its staging and MFMAs;
//  * BceStat (stats_walk's functor): each of a row's four threads keeps the row's cursor and its 64-bit membership mask
//    of the tile in registers and adds softplus(s), s over the labels and s over all candidates of its 16 in fp64; the
//    four meet in LDS in one partial per (row, chunk);
//  * bce_finish_kernel: adds the chunks in ascending order, combines in fp64, rounds once;
//  * BceCrit: G(i, c) = g_i (sigma(s) - y(i, c)); one thread per row writes the tile's 64-bit membership mask to LDS
//    (64 x 8 bytes), the MFMA-layout epilogue reads it;
//  * the parameter block, the workspace layout and the four extern "C" entries.
// No read-modify-write on global memory anywhere: every output element and every partial has one writer.
#include "kge_common.h"
#include "../../include/kge_hip_bce.h"
#include "lp_tile64.h"

namespace {

using namespace tile64;
static_assert(BM == KGE_BCE_BM && BN == KGE_BCE_BN && KSLICE == KGE_BCE_KSLICE &&
              MIN_TILES_PER_CHUNK == KGE_BCE_MIN_TILES_PER_CHUNK && MAX_CHUNKS == KGE_BCE_MAX_CHUNKS &&
              MAX_K == KGE_BCE_MAX_K, "the geometry the header publishes");

typedef unsigned long long u64;

struct BceParams {
    kge_lp_desc d;
    const int64_t *seg_lo, *seg_hi;
    const int32_t *labels;
    const float *g;
    float eps, y_pos, y_neg;    // y_pos = (1 - eps) + eps / N, y_neg = eps / N: rounded once, here
    int chunks, col_tiles, row_panels;
    // workspace
    double *ws_sp, *ws_spos, *ws_sall;  // [B][chunks] each: sum softplus(s), sum of s over the labels, sum of s
    float *ws_da;                       // [chunks][B][K0 + K1]
    // outputs
    float *row_loss;
    float *o0, *o1;     // gradient group of the launch (dA: unused, the workspace is written)
    int64_t ldo0, ldo1;
};

struct LabelCursor {
    int64_t cur, hi, nxt;   // nxt = labels[cur], or past every candidate when the segment is used up
    static constexpr int64_t DONE = INT64_MAX;
    // position at the first label >= col0 of labels[lo .. hi_): lower_bound (an empty or inverted range reads nothing)
    __device__ __forceinline__ void start(const int32_t *labels, int64_t lo, int64_t hi_, int64_t col0)
    {
        hi = hi_;
        int64_t a = lo, b = hi_;
        while (a < b) {
            const int64_t m = a + ((b - a) >> 1);
            if (labels[m] < col0) a = m + 1;
            else b = m;
        }
        cur = a;
        nxt = cur < hi ? (int64_t)labels[cur] : DONE;
    }
    // membership mask of the tile [col0, col0 + BN); advances past its labels.  Reads labels inside [cur, hi) only; a
    // label below col0 (a segment that is not ascending) sets no bit.
    __device__ __forceinline__ u64 take(const int32_t *labels, int64_t col0)
    {
        u64 m = 0;
        const int64_t end = col0 + BN;
        while (nxt < end) {
            const int64_t o = nxt - col0;
            if (o >= 0) m |= (u64)1 << o;
            ++cur;
            nxt = cur < hi ? (int64_t)labels[cur] : DONE;
        }
        return m;
    }
};

__device__ __forceinline__ float sigmoid_f(float s)
{
    const float e = expf(-fabsf(s));
    return (s >= 0.f ? 1.f : e) / (1.f + e);
}

// the multi-label statistics of stats_walk(): three fp64 sums per thread, the row's cursor and the tile's mask
struct BceStat {
    const BceParams &p;
    double (*sum_s)[BM * 4];
    LabelCursor lc;     // (the four threads of a row walk the same cursor: the same addresses in one wave)
    u64 mask;
    double sp, spos, sall;
    __device__ __forceinline__ void start(int64_t row, bool ok, int64_t col0)
    {
        lc.start(p.labels, ok ? p.seg_lo[row] : 0, ok ? p.seg_hi[row] : 0, col0);
        sp = 0.0; spos = 0.0; sall = 0.0;
    }
    // issued before the tile: retires under its loads and MFMAs
    __device__ __forceinline__ void tile(int64_t col0) { mask = lc.take(p.labels, col0); }
    __device__ __forceinline__ void add(const float *s, int64_t, int64_t, int c_lo, int cnt)
    {
        const unsigned mine = (unsigned)(mask >> c_lo) & 0xffffu;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float v = s[c_lo + e];
            if (e < cnt) {
                // the two terms of softplus enter the fp64 sum one by one: rounded together to fp32, log1pf(.) would
                // lose its low bits beside a large s -- which the label sum then cancels
                sp += (double)fmaxf(v, 0.f);
                sp += (double)log1pf(expf(-fabsf(v)));
                sall += (double)v;
                if ((mine >> e) & 1u) spos += (double)v;
            }
        }
    }
    __device__ __forceinline__ void publish(int tid) { sum_s[0][tid] = sp; sum_s[1][tid] = spos; sum_s[2][tid] = sall; }
    __device__ __forceinline__ void write(int64_t row, int chunk, int tid) const
    {
        double r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = ((sum_s[k][tid] + sum_s[k][tid + 1]) + sum_s[k][tid + 2]) + sum_s[k][tid + 3];
        p.ws_sp[row * p.chunks + chunk] = r[0];
        p.ws_spos[row * p.chunks + chunk] = r[1];
        p.ws_sall[row * p.chunks + chunk] = r[2];
    }
};

template <bool VEC4>
__global__ __launch_bounds__(NTHREADS) void bce_stats_kernel(const BceParams p)
{
    __shared__ __attribute__((aligned(16))) float As[BM * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LDS_LD];
    __shared__ float Ss[BM * G_LD];
    __shared__ double sum_s[3][BM * 4];
    BceStat stat = {p, sum_s};
    stats_walk<VEC4>(p, stat, As, Bs, Ss);
}

__global__ __launch_bounds__(BM) void bce_finish_kernel(const BceParams p)
{
    const int64_t row = (int64_t)blockIdx.x * BM + threadIdx.x;
    if (row >= p.d.B) return;
    double SP = 0.0, SPOS = 0.0, SALL = 0.0;
    for (int c = 0; c < p.chunks; ++c) {
        SP += p.ws_sp[row * p.chunks + c];
        SPOS += p.ws_spos[row * p.chunks + c];
        SALL += p.ws_sall[row * p.chunks + c];
    }
    double loss = SP - SPOS;
    if (p.eps != 0.f) loss = SP - ((double)p.y_pos * SPOS + (double)p.y_neg * (SALL - SPOS));
    p.row_loss[row] = (float)loss;
}

// the multi-label criterion of grad_walk(): thread i < BM owns row i of the panel -- its weight, its cursor, its mask
struct BceCrit {
    const BceParams &p;
    float *g_s;
    u64 *mask_s;
    LabelCursor lc;
    __device__ __forceinline__ void panel(int64_t row0, int64_t col0)
    {
        const int tid = threadIdx.x;
        if (tid < BM) {     // (the previous epilogue's reads are behind the barrier before its MFMA phase)
            const int64_t row = row0 + tid;
            const bool ok = row < p.d.B;
            g_s[tid] = ok ? p.g[row] : 0.f;
            lc.start(p.labels, ok ? p.seg_lo[row] : 0, ok ? p.seg_hi[row] : 0, col0);
        }
    }
    __device__ __forceinline__ void tile(int64_t col0)
    {
        if (threadIdx.x < BM) mask_s[threadIdx.x] = lc.take(p.labels, col0);
    }
    __device__ __forceinline__ float G(int rloc, int cloc, int64_t, float s) const
    {
        const float y = ((mask_s[rloc] >> cloc) & 1) ? p.y_pos : p.y_neg;
        const float v = sigmoid_f(s) - y;
        return g_s[rloc] * v;
    }
};

template <bool VEC4, bool TR>
__global__ __launch_bounds__(NTHREADS) void bce_grad_kernel(const BceParams p)
{
    __shared__ __attribute__((aligned(16))) float As[BM * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LDS_LD];
    __shared__ float Gs[BM * G_LD];
    __shared__ float g_s[BM];
    __shared__ u64 mask_s[BM];
    BceCrit crit = {p, g_s, mask_s, {0, 0, LabelCursor::DONE}};
    grad_walk<VEC4, TR>(p, crit, As, Bs, Gs);
}

__global__ __launch_bounds__(256) void bce_sum_chunks_kernel(const BceParams p) { sum_chunks(p); }

// validation of both entries (tile64::setup) and what is this criterion's own of the parameter block
int bce_setup(const kge_lp_desc *d, const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *labels, float eps, void *ws,
              size_t ws_bytes, BceParams &p)
{
    if (int e = setup(d, seg_lo && seg_hi && labels, eps, ws, ws_bytes, kge_lp_bce_ws_bytes, p)) return e;
    if (d->B == 0) return 0;
    p.seg_lo = seg_lo;
    p.seg_hi = seg_hi;
    p.labels = labels;
    p.eps = eps;
    p.y_neg = eps / (float)d->N;
    p.y_pos = (1.0f - eps) + p.y_neg;
    const size_t part = (size_t)8 * d->B * p.chunks;
    char *w = static_cast<char *>(ws);
    p.ws_sp = reinterpret_cast<double *>(w);
    p.ws_spos = reinterpret_cast<double *>(w + part);
    p.ws_sall = reinterpret_cast<double *>(w + 2 * part);
    p.ws_da = reinterpret_cast<float *>(w + 3 * part);
    return 0;
}

} // namespace

extern "C" int kge_lp_bce_chunks(int64_t N) { return chunk_count(N); }

extern "C" size_t kge_lp_bce_ws_bytes(int64_t B, int64_t N, int K0, int K1)
{
    if (B <= 0 || N <= 0 || K0 <= 0 || K1 < 0 || (int64_t)K0 + K1 > MAX_K) return 0;
    if (B >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31)) return 0;
    const size_t chunks = (size_t)chunk_count(N);
    return (size_t)24 * B * chunks + (size_t)4 * chunks * B * (size_t)(K0 + K1);
}

extern "C" int kge_lp_bce_fwd(const kge_lp_desc *desc, const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *labels,
                              float label_smoothing, float *row_loss, void *ws, size_t ws_bytes, kge_stream_t stream)
{
    BceParams p = {};
    if (!row_loss) return KGE_EINVAL;
    if (int e = bce_setup(desc, seg_lo, seg_hi, labels, label_smoothing, ws, ws_bytes, p)) return e;
    p.row_loss = row_loss;
    return launch_fwd(bce_stats_kernel<false>, bce_stats_kernel<true>, bce_finish_kernel, p, kge_s(stream));
}

extern "C" int kge_lp_bce_bwd(const kge_lp_desc *desc, const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *labels,
                              float label_smoothing, const float *g, float *dA0, int64_t ldda0, float *dA1, int64_t ldda1,
                              float *dT0, int64_t lddt0, float *dT1, int64_t lddt1, void *ws, size_t ws_bytes,
                              kge_stream_t stream)
{
    BceParams p = {};
    if (!g) return KGE_EINVAL;
    if (int e = bce_setup(desc, seg_lo, seg_hi, labels, label_smoothing, ws, ws_bytes, p)) return e;
    p.g = g;
    return launch_bwd(bce_grad_kernel<false, true>, bce_grad_kernel<true, true>, bce_grad_kernel<false, false>,
                      bce_grad_kernel<true, false>, bce_sum_chunks_kernel, p, dA0, ldda0, dA1, ldda1, dT0, lddt0, dT1, lddt1,
                      kge_s(stream));
}
