// The embedding regularizers (include/kge_hip_penalty.h): the Lp penalty, p = 2 or 3, of the table rows a batch names,
// and its gradient rows.
//
// penalty_terms_kernel<P>   one wavefront per (stream, row), grid-stride over the M rows of up to 8 streams whose
//                           descriptors ride in the kernel arguments; the wavefront finds its stream from the prefix
//                           offsets, streams the row once (nothing of it is kept: any width) and lane 0 writes the term.
// penalty_sum_kernel        the fp64 tree of loss_common.h over the M terms (st_final_kernel behind it for G > 1).
// penalty_bwd_kernel<P>     the same walk, the row gathered again, the gradient row(s) written: no atomic.
// The order of a row's additions is fixed by row_walk(): lane l owns the aligned groups of four l, l + 64, ..., in
// ascending order; the load path (16-byte quads or scalars) only changes how a group's four floats arrive.
// Pure streaming behind a gather: 4 d bytes read per row forward, 4 d read and written backward; at a training batch the
// cost is the launches, which is why there are at most three forward and one backward.  -ffp-contract=off: the arithmetic
// is the source's.
#include "kge_common.h"
#include "../../include/kge_hip_penalty.h"
#include "loss_common.h"

namespace {

constexpr int RP_WAVES = KGE_PENALTY_WAVES;
constexpr int RP_THREADS = RP_WAVES * KGE_WAVE;
constexpr int RP_MAX_BLOCKS = KGE_PENALTY_MAX_BLOCKS;
constexpr int RP_MAX_STREAMS = KGE_PENALTY_MAX_STREAMS;
constexpr int64_t RP_MAX_M = 0x7fffffffll;

struct PenaltyArgs {
    kge_penalty_stream s[RP_MAX_STREAMS];
    int64_t off[RP_MAX_STREAMS + 1];    // prefix sums of n: stream q owns the terms [off[q], off[q + 1])
    int64_t row_off[RP_MAX_STREAMS];    // float offset of stream q's block in the rows buffer
    float cf[RP_MAX_STREAMS];           // p * factor, rounded once on the host
    int vec[RP_MAX_STREAMS];            // bit 0: the tables are read in 16-byte quads; bit 1: the rows are written so
    int n_streams;
    int64_t M;
    float *terms;
    const float *go;
    float *rows;
};

inline int rp_grid(int64_t M)
{
    const int64_t g = (M + RP_WAVES - 1) / RP_WAVES;
    return (int)(g < RP_MAX_BLOCKS ? g : RP_MAX_BLOCKS);
}

// four consecutive floats of a row from column c on: one quad where the path allows it and the group lies inside the
// row, scalars with entries past d as 0 otherwise
__device__ __forceinline__ void load_group(const float *__restrict__ x, int c, int d, bool vec, float (&v)[4])
{
    if (vec && c + 4 <= d) {
        const float4 q = *reinterpret_cast<const float4 *>(x + c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < d ? x[c + e] : 0.f;
    }
}

__device__ __forceinline__ void store_group(float *__restrict__ x, int c, int d, bool vec, const float (&v)[4])
{
    if (vec && c + 4 <= d) {
        *reinterpret_cast<float4 *>(x + c) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < d) x[c + e] = v[e];
    }
}

// |x|^P of a real element and of a complex coordinate; both are 0 at 0
template <int P>
__device__ __forceinline__ float real_term(float x)
{
    const float x2 = x * x;
    return P == 2 ? x2 : fabsf(x) * x2;
}
template <int P>
__device__ __forceinline__ float cplx_term(float re, float im)
{
    const float m2 = fmaf(im, im, re * re);
    return P == 2 ? m2 : m2 * sqrtf(m2);
}
// the factor of the element in its gradient: c |x|^(P - 2)
template <int P>
__device__ __forceinline__ float real_scale(float c, float x) { return P == 2 ? c : c * fabsf(x); }
template <int P>
__device__ __forceinline__ float cplx_scale(float c, float re, float im)
{
    return P == 2 ? c : c * sqrtf(fmaf(im, im, re * re));
}

// The walk of one row by one wavefront: lane l takes the aligned groups of four l, l + 64, ... in ascending order and
// hands each to group(c, v0, v1) -- c the group's first column, v0 its floats of t0, v1 those of t1 (SPLIT) -- whose
// return value enters the lane's accumulator.  Returns the lane's sum.
template <bool SPLIT, class Group>
__device__ __forceinline__ float row_walk(const float *__restrict__ x0, const float *__restrict__ x1, int d, bool vec,
                                          Group group)
{
    const int lane = threadIdx.x & (KGE_WAVE - 1);
    float acc = 0.f;
    for (int c = 4 * lane; c < d; c += 4 * KGE_WAVE) {
        float v0[4], v1[4] = {0.f, 0.f, 0.f, 0.f};
        load_group(x0, c, d, vec, v0);
        if (SPLIT) load_group(x1, c, d, vec, v1);
        acc = acc + group(c, v0, v1);
    }
    return acc;
}

template <int P>
__device__ __forceinline__ float row_terms(const kge_penalty_stream &st, int64_t id, bool vec)
{
    const float *x0 = st.t0 + id * st.ld;
    if (st.layout == KGE_PENALTY_SPLIT) {
        return row_walk<true>(x0, st.t1 + id * st.ld, st.d, vec, [](int, const float (&a)[4], const float (&b)[4]) {
            return (cplx_term<P>(a[0], b[0]) + cplx_term<P>(a[1], b[1])) + (cplx_term<P>(a[2], b[2]) + cplx_term<P>(a[3], b[3]));
        });
    }
    if (st.layout == KGE_PENALTY_INTERLEAVED) {
        return row_walk<false>(x0, nullptr, st.d, vec, [](int, const float (&a)[4], const float (&)[4]) {
            return cplx_term<P>(a[0], a[1]) + cplx_term<P>(a[2], a[3]);
        });
    }
    return row_walk<false>(x0, nullptr, st.d, vec, [](int, const float (&a)[4], const float (&)[4]) {
        return (real_term<P>(a[0]) + real_term<P>(a[1])) + (real_term<P>(a[2]) + real_term<P>(a[3]));
    });
}

template <int P>
__device__ __forceinline__ void row_grads(const kge_penalty_stream &st, int64_t id, int64_t i, bool vec, bool vec_out,
                                          float c, float *__restrict__ block)
{
    const float *x0 = st.t0 + id * st.ld;
    const int d = st.d;
    float *g0 = block + i * d;
    if (st.layout == KGE_PENALTY_SPLIT) {
        float *g1 = block + (st.n + i) * d;
        row_walk<true>(x0, st.t1 + id * st.ld, d, vec, [=](int col, const float (&a)[4], const float (&b)[4]) {
            float ga[4], gb[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float s = cplx_scale<P>(c, a[e], b[e]);
                ga[e] = s * a[e];
                gb[e] = s * b[e];
            }
            store_group(g0, col, d, vec_out, ga);
            store_group(g1, col, d, vec_out, gb);
            return 0.f;
        });
    } else if (st.layout == KGE_PENALTY_INTERLEAVED) {
        row_walk<false>(x0, nullptr, d, vec, [=](int col, const float (&a)[4], const float (&)[4]) {
            const float s0 = cplx_scale<P>(c, a[0], a[1]), s1 = cplx_scale<P>(c, a[2], a[3]);
            const float g[4] = {s0 * a[0], s0 * a[1], s1 * a[2], s1 * a[3]};
            store_group(g0, col, d, vec_out, g);
            return 0.f;
        });
    } else {
        row_walk<false>(x0, nullptr, d, vec, [=](int col, const float (&a)[4], const float (&)[4]) {
            float g[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = real_scale<P>(c, a[e]) * a[e];
            store_group(g0, col, d, vec_out, g);
            return 0.f;
        });
    }
}

// the stream of term m (wave-uniform): the last q with off[q] <= m
__device__ __forceinline__ int stream_of(const PenaltyArgs &a, int64_t m)
{
    int q = 0;
    while (q + 1 < a.n_streams && m >= a.off[q + 1]) ++q;
    return q;
}

template <int P>
__global__ __launch_bounds__(RP_THREADS) void penalty_terms_kernel(const PenaltyArgs a)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t step = (int64_t)gridDim.x * RP_WAVES;
    for (int64_t m = (int64_t)blockIdx.x * RP_WAVES + wave; m < a.M; m += step) {
        const int q = stream_of(a, m);
        const kge_penalty_stream &st = a.s[q];
        const int64_t i = m - a.off[q];
        const float sum = wave_sum(row_terms<P>(st, st.ids[i], a.vec[q] & 1));
        if ((threadIdx.x & (KGE_WAVE - 1)) == 0) a.terms[m] = st.factor * sum;
    }
}

template <int P>
__global__ __launch_bounds__(RP_THREADS) void penalty_bwd_kernel(const PenaltyArgs a)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t step = (int64_t)gridDim.x * RP_WAVES;
    const float go = a.go[0];
    for (int64_t m = (int64_t)blockIdx.x * RP_WAVES + wave; m < a.M; m += step) {
        const int q = stream_of(a, m);
        const kge_penalty_stream &st = a.s[q];
        const int64_t i = m - a.off[q];
        row_grads<P>(st, st.ids[i], i, a.vec[q] & 1, a.vec[q] & 2, a.cf[q] * go, a.rows + a.row_off[q]);
    }
}

__global__ __launch_bounds__(ST_THREADS) void penalty_sum_kernel(const float *terms, int64_t M, bool vec, double *part,
                                                                 float *loss, float *acc_io)
{
    __shared__ double sh[ST_THREADS / 64];
    const double acc = st_thread_sum(M, [&](int64_t j, float (&t)[4]) { load_quad(terms, j, M, vec, t); });
    st_finish_block(acc, sh, part, loss, acc_io);
}

inline int64_t stream_copies(const kge_penalty_stream &st) { return st.layout == KGE_PENALTY_SPLIT ? 2 : 1; }

inline bool streams_countable(const kge_penalty_stream *streams, int n_streams)
{
    if (n_streams < 0 || n_streams > RP_MAX_STREAMS || (n_streams > 0 && !streams)) return false;
    for (int q = 0; q < n_streams; ++q)
        if (streams[q].n < 0) return false;
    return true;
}

// the checks both entries share, and the kernel arguments; 0 or KGE_EINVAL
int penalty_args(const kge_penalty_stream *streams, int n_streams, int p, PenaltyArgs &a)
{
    if ((p != 2 && p != 3) || !streams_countable(streams, n_streams)) return KGE_EINVAL;
    a = PenaltyArgs{};
    a.n_streams = n_streams;
    int64_t M = 0, floats = 0;
    for (int q = 0; q < n_streams; ++q) {
        const kge_penalty_stream &st = streams[q];
        if (st.layout < KGE_PENALTY_REAL || st.layout > KGE_PENALTY_INTERLEAVED || !st.t0 || st.d < 1 || st.ld < st.d ||
            (st.n > 0 && !st.ids))
            return KGE_EINVAL;
        if (st.layout == KGE_PENALTY_SPLIT && !st.t1) return KGE_EINVAL;
        if (st.layout == KGE_PENALTY_INTERLEAVED && (st.d & 1)) return KGE_EINVAL;
        a.s[q] = st;
        a.off[q] = M;
        a.row_off[q] = floats;
        a.cf[q] = (float)p * st.factor;
        a.vec[q] = kge_aligned16(st.t0) && (st.layout != KGE_PENALTY_SPLIT || kge_aligned16(st.t1)) && st.ld % 4 == 0;
        M += st.n;
        if (M > RP_MAX_M) return KGE_EINVAL;
        floats += stream_copies(st) * st.n * st.d;
    }
    for (int q = n_streams; q <= RP_MAX_STREAMS; ++q) a.off[q] = M;
    a.M = M;
    return 0;
}

} // namespace

extern "C" int64_t kge_row_penalty_terms(const kge_penalty_stream *streams, int n_streams)
{
    if (!streams_countable(streams, n_streams)) return -1;
    int64_t M = 0;
    for (int q = 0; q < n_streams; ++q) M += streams[q].n;
    return M;
}

extern "C" size_t kge_row_penalty_ws_bytes(int64_t M)
{
    if (M <= 0 || M > RP_MAX_M) return 0;
    return (size_t)st_grid(M) * sizeof(double);
}

extern "C" int64_t kge_row_penalty_row_offset(const kge_penalty_stream *streams, int n_streams, int s)
{
    if (!streams_countable(streams, n_streams) || s < 0 || s > n_streams) return -1;
    int64_t floats = 0;
    for (int q = 0; q < s; ++q) floats += stream_copies(streams[q]) * streams[q].n * (int64_t)streams[q].d;
    return floats;
}

extern "C" int64_t kge_row_penalty_rows_floats(const kge_penalty_stream *streams, int n_streams)
{
    return kge_row_penalty_row_offset(streams, n_streams, n_streams);
}

extern "C" int kge_row_penalty(const kge_penalty_stream *streams, int n_streams, int p, float *terms, float *loss,
                               float *acc_io, void *ws, size_t ws_bytes, kge_stream_t stream)
{
    PenaltyArgs a;
    if (penalty_args(streams, n_streams, p, a) != 0 || !terms || !loss) return KGE_EINVAL;
    hipStream_t s = kge_s(stream);
    const int64_t M = a.M;
    if (M == 0) {
        hipError_t e = hipMemsetAsync(loss, 0, sizeof(float), s);
        return e == hipSuccess ? 0 : (int)e;
    }
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) != 0 || ws_bytes < kge_row_penalty_ws_bytes(M)) return KGE_EINVAL;
    a.terms = terms;
    if (p == 2) hipLaunchKernelGGL(penalty_terms_kernel<2>, dim3(rp_grid(M)), dim3(RP_THREADS), 0, s, a);
    else hipLaunchKernelGGL(penalty_terms_kernel<3>, dim3(rp_grid(M)), dim3(RP_THREADS), 0, s, a);
    KGE_CHECK_LAUNCH();
    const int G = st_grid(M);
    double *part = static_cast<double *>(ws);
    hipLaunchKernelGGL(penalty_sum_kernel, dim3(G), dim3(ST_THREADS), 0, s, (const float *)terms, M, kge_aligned16(terms),
                       part, loss, acc_io);
    KGE_CHECK_LAUNCH();
    if (G > 1) {
        hipLaunchKernelGGL(st_final_kernel, dim3(1), dim3(ST_THREADS), 0, s, (const double *)part, G, loss, acc_io);
        KGE_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int kge_row_penalty_bwd(const kge_penalty_stream *streams, int n_streams, int p, const float *go, float *rows,
                                   kge_stream_t stream)
{
    PenaltyArgs a;
    if (penalty_args(streams, n_streams, p, a) != 0 || !go || !rows) return KGE_EINVAL;
    if (a.M == 0) return 0;
    // a block's rows lie on 16 bytes when the buffer does, the block starts at a multiple of four floats and so does
    // every row (SPLIT: the imaginary block starts n * d floats in, a multiple of four with d)
    for (int q = 0; q < n_streams; ++q)
        if (kge_aligned16(rows) && a.row_off[q] % 4 == 0 && a.s[q].d % 4 == 0) a.vec[q] |= 2;
    a.go = go;
    a.rows = rows;
    hipStream_t s = kge_s(stream);
    if (p == 2) hipLaunchKernelGGL(penalty_bwd_kernel<2>, dim3(rp_grid(a.M)), dim3(RP_THREADS), 0, s, a);
    else hipLaunchKernelGGL(penalty_bwd_kernel<3>, dim3(rp_grid(a.M)), dim3(RP_THREADS), 0, s, a);
    KGE_CHECK_LAUNCH();
    return 0;
}
