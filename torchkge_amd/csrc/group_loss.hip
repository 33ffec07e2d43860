// The grouped training criteria (include/kge_hip_group.h): B facts with K negatives each, the negatives of a fact weighed
// against each other (self-adversarial weights, or a softmax of the fact against its negatives), closed-form gradients.
//
// neg is (K, B): lanes own consecutive facts -- 4 each, one 16-byte quad -- so a wavefront's load of row k is one
// contiguous KiB and the reduction over k never crosses a lane.  B alone gives too few blocks (B = 1,024: 4 panels on
// 256 CUs), so K is split over the four wavefronts of a block (slices) and over chunk blocks (grid.y).
//
// group_stats_kernel<KIND>   grid (panels, chunks): per (fact, chunk, slice) the running (m, l, t) in ascending k, to the
//                            workspace.
// group_finish_kernel<KIND>  the first stage of the fp64 tree of loss_common.h over the B facts: a thread merges the
//                            partials of its four facts in ascending (chunk, slice) order, writes row_loss, dpos and the
//                            final (m, l) -- SOFTMAX: (M, l') with the fact itself in -- and its four row terms enter the tree.  B <= 1024: one block, *loss written.
// st_final_kernel            B > 1024 only: the tree's second stage.
// group_grad_kernel<KIND>    grid (panels, chunks): neg again with the final (m, l) per fact, dneg out.
// Two reads and one write of B K floats; the workspace holds no B K-sized term.  -ffp-contract=off: the arithmetic is the
// source's.  No MFMA and nothing runs beside one: the file needs no -fno-slp-vectorize (see build.py).
#include <float.h>
#include "kge_common.h"
#include "../../include/kge_hip_group.h"
#include "loss_common.h"

namespace {

constexpr int GL_THREADS = 64 * KGE_GROUP_SLICES;
constexpr int GL_ROWS = KGE_GROUP_ROWS;
constexpr int GL_SLICES = KGE_GROUP_SLICES;
constexpr int64_t GL_MAX_BK = 0x7fffffffll;
static_assert(GL_ROWS == 4 * 64, "a lane owns one quad of facts");
static_assert(GL_THREADS == ST_THREADS, "the finish step is the tree's first stage");
static_assert(KGE_GROUP_MIN_K_PER_CHUNK / 2 >= KGE_GROUP_SLICES, "only a single short chunk may have empty slices");

enum { VEC_POS = 1, VEC_NEG = 2, VEC_RW = 4, VEC_ROWLOSS = 8, VEC_DPOS = 16, VEC_DNEG = 32 };

struct GroupLoss {
    const float *pos, *neg, *rw;
    float *loss, *acc_io, *row_loss, *dpos, *dneg;
    double *part;       // workspace: the tree's partials,
    double *stats_lt;   // the (chunk, slice, {l, t}, Bp) partials in fp64,
    float *stats_m;     // their (chunk, slice, Bp) maxima,
    float *fin;         // ({m, l}, Bp) finals
    int64_t ld_neg, ld_dneg, B, K, Bp, Bq;      // Bp: B rounded up to 4, Bq: to GL_ROWS
    float margin, alpha;
    int chunks;
    int vec;            // VEC_* bits: which operands are accessed in quads
};

inline int gl_chunks(int64_t K)
{
    if (K < 1) return 0;
    const int64_t c = (K + KGE_GROUP_MIN_K_PER_CHUNK - 1) / KGE_GROUP_MIN_K_PER_CHUNK;
    return (int)(c < KGE_GROUP_MAX_CHUNKS ? c : KGE_GROUP_MAX_CHUNKS);
}

// the negatives [ka, kb) of slice s of chunk c
__host__ __device__ __forceinline__ void gl_slice(int64_t K, int chunks, int c, int s, int64_t &ka, int64_t &kb)
{
    const int64_t k0 = c * K / chunks, k1 = (c + 1) * K / chunks, len = k1 - k0;
    ka = k0 + s * len / GL_SLICES;
    kb = k0 + (s + 1) * len / GL_SLICES;
}

// is slice s of chunk c empty?  Only a single chunk shorter than the slice count has empty slices (a chunk of several
// holds KGE_GROUP_MIN_K_PER_CHUNK / 2 negatives at least): no 64-bit division where the finish step asks per partial
__device__ __forceinline__ bool gl_slice_empty(int64_t K, int s)
{
    if (K >= GL_SLICES) return false;
    const int k = (int)K;
    return (s + 1) * k / GL_SLICES <= s * k / GL_SLICES;
}

__device__ __forceinline__ float gl_u(float alpha, float x)
{
    return fminf(fmaxf(alpha * x, -FLT_MAX), FLT_MAX);
}

__device__ __forceinline__ float *gl_stat_m(const GroupLoss &a, int c, int s)
{
    return a.stats_m + (int64_t)(c * GL_SLICES + s) * a.Bp;
}

// comp 0: l, 1: t
__device__ __forceinline__ double *gl_stat_lt(const GroupLoss &a, int c, int s, int comp)
{
    return a.stats_lt + ((int64_t)(c * GL_SLICES + s) * 2 + comp) * a.Bq;
}

// The fp32 quad of the facts j .. j + 3 (j a multiple of 4) in the workspace: always whole and on 16 bytes (Bp is a
// multiple of 4) -- no bound and no scalar path, so that nothing stands between the loads of consecutive partials
__device__ __forceinline__ void load_quad_ws(const float *__restrict__ x, int64_t j, float (&v)[4])
{
    const float4 q = *reinterpret_cast<const float4 *>(x + j);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}

__device__ __forceinline__ void store_quad_ws(float *__restrict__ x, int64_t j, const float (&v)[4])
{
    *reinterpret_cast<float4 *>(x + j) = make_float4(v[0], v[1], v[2], v[3]);
}

// The fp64 quad of the facts j .. j + 3 (j a multiple of 4) in the workspace.  Within a panel of GL_ROWS facts the two
// 16-byte halves of a lane's quad lie GL_ROWS / 2 doubles apart, lane after lane: each of a wavefront's two accesses is
// one contiguous KiB (32 bytes per lane in fact order would be two accesses of 16 bytes at a stride of 32).
__device__ __forceinline__ int64_t gl_q64(int64_t j)
{
    return (j / GL_ROWS) * GL_ROWS + ((j % GL_ROWS) / 4) * 2;
}

__device__ __forceinline__ void load_quad64(const double *__restrict__ x, int64_t j, double (&v)[4])
{
    const double2 lo = *reinterpret_cast<const double2 *>(x + gl_q64(j));
    const double2 hi = *reinterpret_cast<const double2 *>(x + gl_q64(j) + GL_ROWS / 2);
    v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
}

__device__ __forceinline__ void store_quad64(double *__restrict__ x, int64_t j, const double (&v)[4])
{
    *reinterpret_cast<double2 *>(x + gl_q64(j)) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2 *>(x + gl_q64(j) + GL_ROWS / 2) = make_double2(v[2], v[3]);
}

template <int KIND>
__global__ __launch_bounds__(GL_THREADS) void group_stats_kernel(const GroupLoss a)
{
    const int s = threadIdx.x >> 6, c = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * GL_ROWS + 4 * (threadIdx.x & 63);
    int64_t ka, kb;
    gl_slice(a.K, a.chunks, c, s, ka, kb);
    if (i0 >= a.B || ka >= kb) return;
    const bool vec = a.vec & VEC_NEG;
    float m[4], x[4];
    double l[4], t[4];      // the running sums are carried in fp64: their rounding does not grow with K
    load_quad(a.neg + ka * a.ld_neg, i0, a.B, vec, x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float sp = 0.f, sg;
        if (KIND == KGE_GROUP_NSSA) softplus_sigma(a.margin + x[e], sp, sg);
        m[e] = KIND == KGE_GROUP_NSSA ? gl_u(a.alpha, x[e]) : x[e];
        l[e] = 1.0;
        t[e] = (double)sp;
    }
#pragma unroll 2
    for (int64_t k = ka + 1; k < kb; ++k) {
        load_quad(a.neg + k * a.ld_neg, i0, a.B, vec, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float sp = 0.f, sg;
            if (KIND == KGE_GROUP_NSSA) softplus_sigma(a.margin + x[e], sp, sg);
            const float u = KIND == KGE_GROUP_NSSA ? gl_u(a.alpha, x[e]) : x[e];
            // one expf for both cases: u - m and m - u differ in sign only, so expf(-|u - m|) is the header's factor
            const float d = u - m[e];
            const double f = (double)expf(-fabsf(d));
            const bool up = d > 0.f;
            l[e] = up ? l[e] * f + 1.0 : l[e] + f;
            t[e] = up ? t[e] * f + (double)sp : t[e] + f * (double)sp;
            m[e] = up ? u : m[e];
        }
    }
    // (Bp is a multiple of 4 and the workspace lies on 16 bytes: whole quads, the entries from B on are scratch)
    store_quad_ws(gl_stat_m(a, c, s), i0, m);
    store_quad64(gl_stat_lt(a, c, s, 0), i0, l);
    if (KIND == KGE_GROUP_NSSA) store_quad64(gl_stat_lt(a, c, s, 1), i0, t);
}

template <int KIND, bool GRAD>
__global__ __launch_bounds__(ST_THREADS) void group_finish_kernel(const GroupLoss a)
{
    __shared__ double sh[ST_THREADS / 64];
    const double acc = st_thread_sum(a.B, [&](int64_t j, float (&term)[4]) {
        // Two passes over the fact's partials, both in ascending (chunk, slice) order: the maximum first, then the sums
        // rescaled to it.  No step waits for the one before it except the additions themselves, so the loads of many
        // partials are in flight at once -- a running merge would pay a load's latency per partial, on one CU.
        // The loops hold no branch and no store, so the loads of several chunks' partials are issued together.
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        double l[4] = {0.0, 0.0, 0.0, 0.0}, t[4] = {0.0, 0.0, 0.0, 0.0};
        auto max_in = [&](int c, int s) {
            float m2[4];
            load_quad_ws(gl_stat_m(a, c, s), j, m2);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], m2[e]);
        };
        auto add_in = [&](int c, int s) {
            float m2[4];
            double l2[4], t2[4] = {0.0, 0.0, 0.0, 0.0};
            load_quad_ws(gl_stat_m(a, c, s), j, m2);
            load_quad64(gl_stat_lt(a, c, s, 0), j, l2);
            if (KIND == KGE_GROUP_NSSA) load_quad64(gl_stat_lt(a, c, s, 1), j, t2);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double f = (double)expf(m2[e] - m[e]);
                l[e] = l[e] + l2[e] * f;
                t[e] = t[e] + t2[e] * f;
            }
        };
        if (a.K >= GL_SLICES) {         // every slice of every chunk holds a negative
#pragma unroll 4
            for (int c = 0; c < a.chunks; ++c) {
#pragma unroll
                for (int s = 0; s < GL_SLICES; ++s) max_in(c, s);
            }
#pragma unroll 2
            for (int c = 0; c < a.chunks; ++c) {
#pragma unroll
                for (int s = 0; s < GL_SLICES; ++s) add_in(c, s);
            }
        } else {                        // one chunk of fewer negatives than slices
            for (int s = 0; s < GL_SLICES; ++s)
                if (!gl_slice_empty(a.K, s)) max_in(0, s);
            for (int s = 0; s < GL_SLICES; ++s)
                if (!gl_slice_empty(a.K, s)) add_in(0, s);
        }
        float p[4], w[4] = {1.f, 1.f, 1.f, 1.f}, gp[4], lf[4];
        load_quad(a.pos, j, a.B, a.vec & VEC_POS, p);
        if (a.rw) load_quad(a.rw, j, a.B, a.vec & VEC_RW, w);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (KIND == KGE_GROUP_NSSA) {
                float sp, sg;
                softplus_sigma(-(a.margin + p[e]), sp, sg);
                term[e] = sp + (float)(t[e] / l[e]);
                gp[e] = -sg;
                lf[e] = (float)l[e];
            } else {
                // lse = M + log(l') is never formed: at scores of 1e4 its fp32 rounding (1e-3) would sit in every
                // gradient.  M - p is exact where it matters, -n / l' has no cancellation where the fact dominates.
                const float M = fmaxf(m[e], p[e]);
                const double n = l[e] * (double)expf(m[e] - M);
                const double lp = n + (double)expf(p[e] - M);
                term[e] = (float)((double)(M - p[e]) + log(lp));
                gp[e] = -(float)(n / lp);
                m[e] = M;
                lf[e] = (float)lp;
            }
            if (a.rw) {
                term[e] = term[e] * w[e];
                gp[e] = gp[e] * w[e];
            }
        }
        if (a.row_loss) store_quad(a.row_loss, j, a.B, a.vec & VEC_ROWLOSS, term);
        if (GRAD) {
            store_quad(a.dpos, j, a.B, a.vec & VEC_DPOS, gp);
            store_quad_ws(a.fin, j, m);
            store_quad_ws(a.fin + a.Bp, j, lf);
        }
    });
    st_finish_block(acc, sh, a.part, a.loss, a.acc_io);
}

template <int KIND>
__global__ __launch_bounds__(GL_THREADS) void group_grad_kernel(const GroupLoss a)
{
    const int s = threadIdx.x >> 6, c = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * GL_ROWS + 4 * (threadIdx.x & 63);
    int64_t ka, kb;
    gl_slice(a.K, a.chunks, c, s, ka, kb);
    if (i0 >= a.B || ka >= kb) return;
    float m[4], l[4], w[4] = {1.f, 1.f, 1.f, 1.f}, x[4], g[4];
    load_quad_ws(a.fin, i0, m);
    load_quad_ws(a.fin + a.Bp, i0, l);
    if (a.rw) load_quad(a.rw, i0, a.B, a.vec & VEC_RW, w);
#pragma unroll 2
    for (int64_t k = ka; k < kb; ++k) {
        load_quad(a.neg + k * a.ld_neg, i0, a.B, a.vec & VEC_NEG, x);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (KIND == KGE_GROUP_NSSA) {
                float sp, sg;
                softplus_sigma(a.margin + x[e], sp, sg);
                g[e] = (expf(gl_u(a.alpha, x[e]) - m[e]) / l[e]) * sg;
            } else {
                g[e] = expf(x[e] - m[e]) / l[e];
            }
            if (a.rw) g[e] = g[e] * w[e];
        }
        store_quad(a.dneg + k * a.ld_dneg, i0, a.B, a.vec & VEC_DNEG, g);
    }
}

inline size_t gl_part_bytes(int64_t B)
{
    return ((size_t)st_grid(B) * sizeof(double) + 15) & ~(size_t)15;
}

inline int64_t gl_bp(int64_t B) { return (B + 3) & ~(int64_t)3; }
inline int64_t gl_bq(int64_t B) { return (B + GL_ROWS - 1) / GL_ROWS * GL_ROWS; }

template <int KIND>
void gl_launch(const GroupLoss &a, bool grad, hipStream_t s)
{
    const dim3 grid((unsigned)((a.B + GL_ROWS - 1) / GL_ROWS), (unsigned)a.chunks);
    hipLaunchKernelGGL((group_stats_kernel<KIND>), grid, dim3(GL_THREADS), 0, s, a);
    const int G = st_grid(a.B);
    if (grad) hipLaunchKernelGGL((group_finish_kernel<KIND, true>), dim3(G), dim3(ST_THREADS), 0, s, a);
    else hipLaunchKernelGGL((group_finish_kernel<KIND, false>), dim3(G), dim3(ST_THREADS), 0, s, a);
    if (G > 1) hipLaunchKernelGGL(st_final_kernel, dim3(1), dim3(ST_THREADS), 0, s, a.part, G, a.loss, a.acc_io);
    if (grad) hipLaunchKernelGGL((group_grad_kernel<KIND>), grid, dim3(GL_THREADS), 0, s, a);
}

} // namespace

extern "C" int kge_group_loss_chunks(int64_t K)
{
    return gl_chunks(K);
}

extern "C" size_t kge_group_loss_ws_bytes(int64_t B, int64_t K)
{
    if (B <= 0 || K < 1 || K > GL_MAX_BK || B > GL_MAX_BK / K) return 0;
    // per (fact, chunk, slice) l and t in fp64 (whole panels) and m in fp32; per fact the final (m, l) in fp32
    const size_t cs = GL_SLICES * (size_t)gl_chunks(K);
    return gl_part_bytes(B) + (size_t)gl_bq(B) * cs * 2 * sizeof(double) +
           (size_t)gl_bp(B) * (cs * sizeof(float) + 2 * sizeof(float));
}

extern "C" int kge_group_loss(int kind, float margin, float temperature, const float *pos, const float *neg, int64_t ld_neg,
                              const float *row_weight, int64_t B, int64_t K, float *loss, float *acc_io, float *row_loss,
                              float *dpos, float *dneg, int64_t ld_dneg, void *ws, size_t ws_bytes, kge_stream_t stream)
{
    if ((kind != KGE_GROUP_NSSA && kind != KGE_GROUP_SOFTMAX) || B < 0 || !loss || (dpos == nullptr) != (dneg == nullptr))
        return KGE_EINVAL;
    if (kind == KGE_GROUP_NSSA && !(temperature >= 0.f && temperature <= FLT_MAX)) return KGE_EINVAL;
    hipStream_t s = kge_s(stream);
    if (B == 0) {
        hipError_t e = hipMemsetAsync(loss, 0, sizeof(float), s);
        return e == hipSuccess ? 0 : (int)e;
    }
    const size_t need = kge_group_loss_ws_bytes(B, K);      // 0: K < 1 or B * K >= 2^31
    if (need == 0 || !pos || !neg || ld_neg < B || (dneg && ld_dneg < B) || !ws || !kge_aligned16(ws) || ws_bytes < need)
        return KGE_EINVAL;
    GroupLoss a{};
    a.pos = pos; a.neg = neg; a.rw = row_weight; a.loss = loss; a.acc_io = acc_io; a.row_loss = row_loss;
    a.dpos = dpos; a.dneg = dneg; a.ld_neg = ld_neg; a.ld_dneg = ld_dneg; a.B = B; a.K = K; a.Bp = gl_bp(B); a.Bq = gl_bq(B);
    a.margin = margin; a.alpha = temperature; a.chunks = gl_chunks(K);
    a.part = static_cast<double *>(ws);
    a.stats_lt = reinterpret_cast<double *>(static_cast<char *>(ws) + gl_part_bytes(B));
    a.stats_m = reinterpret_cast<float *>(a.stats_lt + (size_t)a.chunks * GL_SLICES * 2 * a.Bq);
    a.fin = a.stats_m + (size_t)a.chunks * GL_SLICES * a.Bp;
    a.vec = (kge_aligned16(pos) ? VEC_POS : 0) | (kge_aligned16(neg) && ld_neg % 4 == 0 ? VEC_NEG : 0) |
            (row_weight && kge_aligned16(row_weight) ? VEC_RW : 0) | (row_loss && kge_aligned16(row_loss) ? VEC_ROWLOSS : 0) |
            (dpos && kge_aligned16(dpos) ? VEC_DPOS : 0) | (dneg && kge_aligned16(dneg) && ld_dneg % 4 == 0 ? VEC_DNEG : 0);
    const bool grad = dpos != nullptr;
    if (kind == KGE_GROUP_NSSA) gl_launch<KGE_GROUP_NSSA>(a, grad, s);
    else gl_launch<KGE_GROUP_SOFTMAX>(a, grad, s);
    KGE_CHECK_LAUNCH();
    return 0;
}
