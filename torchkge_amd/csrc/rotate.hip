// RotatE (Sun et al. 2019) on interleaved complex rows, gfx950: the triple scorer behind kge_score_triples /
// kge_score_triples_bwd (KGE_ROTATE) and the query rows of its all-candidates problems (kge_rotate_query).
//
//   score(h, r, t) = - sum_j | h_j r_j - t_j |,   r_j = cos(theta_j) + i sin(theta_j)
//
// E (n_ent, 2d) holds (re_0, im_0, re_1, im_1, ...), P (n_rel, d) the phases.  The all-candidates score is the
// broadcast-subtract mode KGE_LP_CMOD (lp_direct.hip) of the query row q = h o r (tail side) or q = t o conj(r) (head side:
// |h r - t| = |h - t conj(r)| for |r| = 1) against the RAW entity table: nothing is repacked, and the kernels here are
// the only RotatE-specific device code.  The rotation (rotate_cs, rotate_apply) has one definition, used by the query
// kernel and both triple kernels; the modulus (lp_cmod_pair) and the accumulation -- one add per aligned group of four
// floats, ascending -- are those of the mode, so a triple's score has the bits of the mode's score of its query row.
// The contract is include/kge_hip_rotate.h.
#include "kge_common.h"

namespace {

constexpr int WAVES = 4;        // wavefronts per block, one triple each
constexpr int ROTATE_MAX_ROW = 1024;    // floats of an entity row, the bound of every kind of kge_score_triples

__device__ __forceinline__ void rotate_cs(float theta, float &c, float &s) { sincosf(theta, &s, &c); }
// x (c + i s), or with CONJ x (c - i s): one fmaf per component around one rounded product
template <bool CONJ>
__device__ __forceinline__ float2 rotate_apply(float xr, float xi, float c, float s)
{
    if (CONJ) return make_float2(fmaf(xr, c, xi * s), fmaf(xi, c, -(xr * s)));
    return make_float2(fmaf(xr, c, -(xi * s)), fmaf(xr, s, xi * c));
}

// ---- query rows ------------------------------------------------------------------------------------------------------
// one thread per (row, complex coordinate): row i < B is the tail-side query of fact i (SIDE_HEAD: the head-side one), row
// B + i of a both-sides batch the head-side query of fact i
__global__ __launch_bounds__(256) void rotate_query_kernel(int side, const float *__restrict__ E, int64_t lde,
                                                           const float *__restrict__ P, int64_t ldp, int d,
                                                           const int64_t *__restrict__ h, const int64_t *__restrict__ t,
                                                           const int64_t *__restrict__ r, int64_t B, int64_t ent_lo,
                                                           int64_t ent_n, float *__restrict__ Q, int64_t ldq)
{
    const int64_t rows = side == KGE_SIDE_BOTH ? 2 * B : B;
    const int64_t total = rows * d;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t row = idx / d;
        const int j = (int)(idx - row * d);
        const bool head = side == KGE_SIDE_HEAD || row >= B;
        const int64_t f = row >= B ? row - B : row;
        int64_t e = head ? t[f] : h[f];
        float2 q = make_float2(0.f, 0.f);
        if (ent_n >= 0) e -= ent_lo;
        if (ent_n < 0 || (e >= 0 && e < ent_n)) {       // (a row another shard owns stays zero: summed over the shards)
            const float *x = E + e * lde + 2 * j;
            float c, s;
            rotate_cs(P[r[f] * ldp + j], c, s);
            q = head ? rotate_apply<true>(x[0], x[1], c, s) : rotate_apply<false>(x[0], x[1], c, s);
        }
        Q[row * ldq + 2 * j] = q.x;
        Q[row * ldq + 2 * j + 1] = q.y;
    }
}

// ---- triples -----------------------------------------------------------------------------------------------------------
// y = h r - t of complex coordinate j of one triple, and what the backward needs beside it
struct RotY {
    float yr, yi, qr, qi, c, s;
};
__device__ __forceinline__ RotY rotate_y(const float *__restrict__ hrow, const float *__restrict__ trow,
                                         const float *__restrict__ prow, int j)
{
    RotY o;
    rotate_cs(prow[j], o.c, o.s);
    const float2 q = rotate_apply<false>(hrow[2 * j], hrow[2 * j + 1], o.c, o.s);
    o.qr = q.x; o.qi = q.y;
    o.yr = q.x - trow[2 * j];
    o.yi = q.y - trow[2 * j + 1];
    return o;
}

// One wavefront per triple.  Lane l takes the aligned group of four floats g = 64 n + l, that is the complex coordinates
// 2g and 2g + 1, and forms the group's (m_2g + m_2g+1); the groups then enter ONE accumulator in ascending order -- the
// chain of KGE_LP_CMOD -- through 64 v_readlane + v_add on every lane (a group past the row adds +0: the same bits).
__global__ __launch_bounds__(WAVES * 64) void rotate_fwd_kernel(const float *__restrict__ E, const float *__restrict__ P,
                                                                int d, const int64_t *__restrict__ h,
                                                                const int64_t *__restrict__ t, const int64_t *__restrict__ r,
                                                                int64_t B, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * WAVES;
    const int groups = (d + 1) >> 1;
    for (int64_t i = wave; i < B; i += nwaves) {
        const float *hrow = E + h[i] * (2 * (int64_t)d), *trow = E + t[i] * (2 * (int64_t)d), *prow = P + r[i] * (int64_t)d;
        float acc = 0.0f;
        for (int g0 = 0; g0 < groups; g0 += 64) {
            const int g = g0 + lane;
            float gs = 0.0f;
            if (g < groups) {
                const RotY a = rotate_y(hrow, trow, prow, 2 * g);
                float m1 = 0.0f;        // an absent pair counts as m = 0
                if (2 * g + 1 < d) {
                    const RotY b = rotate_y(hrow, trow, prow, 2 * g + 1);
                    m1 = lp_cmod_pair(b.yr, b.yi);
                }
                gs = lp_cmod_pair(a.yr, a.yi) + m1;
            }
#pragma unroll
            for (int l = 0; l < 64; ++l)
                acc = acc + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, gs), l));
        }
        if (lane == 0) out[i] = lp_direct_finish<KGE_LP_CMOD>(acc);
    }
}

// Backward in closed form, lanes over the complex coordinates of the wavefront's triple: with u = y / |y| and u = 0 where
// |y| = 0 (the written-out sqrt(re^2 + im^2) differentiates to NaN there), g = go_i:
//   dt = +g u,   dh = -g u conj(r),   dtheta = -g Re(conj(u) i q) = -g (u_i q_r - u_r q_i),  q = h r
// Gradient rows only (streams 0 (E, h), 1 (E, t), 2 (P, r) of rows[(stream * B + i) * rows_ld ...]): the caller's row
// reduction sums them -- no float atomics here.
__global__ __launch_bounds__(WAVES * 64) void rotate_bwd_kernel(const float *__restrict__ E, const float *__restrict__ P,
                                                                int d, const int64_t *__restrict__ h,
                                                                const int64_t *__restrict__ t, const int64_t *__restrict__ r,
                                                                int64_t B, const float *__restrict__ go,
                                                                float *__restrict__ rows, int64_t rows_ld)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * WAVES;
    for (int64_t i = wave; i < B; i += nwaves) {
        const float *hrow = E + h[i] * (2 * (int64_t)d), *trow = E + t[i] * (2 * (int64_t)d), *prow = P + r[i] * (int64_t)d;
        float *gh = rows + i * rows_ld, *gt = rows + (B + i) * rows_ld, *gp = rows + (2 * B + i) * rows_ld;
        const float g = go[i];
        for (int j = lane; j < d; j += 64) {
            const RotY y = rotate_y(hrow, trow, prow, j);
            const float m = lp_cmod_pair(y.yr, y.yi);
            const float ur = m > 0.0f ? y.yr / m : 0.0f, ui = m > 0.0f ? y.yi / m : 0.0f;
            const float tr = g * ur, ti = g * ui;                               // dt = g u;  dq = -dt
            const float2 dh = rotate_apply<true>(-tr, -ti, y.c, y.s);          // dq conj(r)
            gt[2 * j] = tr; gt[2 * j + 1] = ti;
            gh[2 * j] = dh.x; gh[2 * j + 1] = dh.y;
            gp[j] = fmaf(tr, y.qi, -(ti * y.qr));                               // <dq, i q> = -g (u_r (-q_i) + u_i q_r)
        }
    }
}

inline int rotate_grid(int64_t B)
{
    const int64_t blocks = (B + WAVES - 1) / WAVES, cap = 256 * 32;
    return (int)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

inline int rotate_check(const float *E, const float *P, int d_ent, int d_rel, const int64_t *h, const int64_t *t,
                        const int64_t *r, int64_t B)
{
    if (!E || !P || d_rel < 1 || d_ent != 2 * d_rel || d_ent > ROTATE_MAX_ROW || B < 0) return KGE_EINVAL;
    if (B > 0 && (!h || !t || !r)) return KGE_EINVAL;
    return 0;
}

} // namespace

int kge_rotate_score_fwd(const float *E, const float *P, int d_ent, int d_rel, const int64_t *h, const int64_t *t,
                         const int64_t *r, int64_t B, float *out, hipStream_t s)
{
    if (int rc = rotate_check(E, P, d_ent, d_rel, h, t, r, B)) return rc;
    if (B == 0) return 0;
    if (!out) return KGE_EINVAL;
    hipLaunchKernelGGL(rotate_fwd_kernel, dim3(rotate_grid(B)), dim3(WAVES * 64), 0, s, E, P, d_rel, h, t, r, B, out);
    KGE_CHECK_LAUNCH();
    return 0;
}

int kge_rotate_score_bwd(const float *E, const float *P, int d_ent, int d_rel, const int64_t *h, const int64_t *t,
                         const int64_t *r, int64_t B, const float *go, float *rows, int64_t rows_ld, hipStream_t s)
{
    if (int rc = rotate_check(E, P, d_ent, d_rel, h, t, r, B)) return rc;
    if (B == 0) return 0;
    if (!go || !rows || rows_ld < d_ent) return KGE_EINVAL;     // row mode only: no per-element float atomics
    hipLaunchKernelGGL(rotate_bwd_kernel, dim3(rotate_grid(B)), dim3(WAVES * 64), 0, s, E, P, d_rel, h, t, r, B, go, rows,
                       rows_ld);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_rotate_query(int side, const float *E, int64_t lde, const float *P, int64_t ldp, int d, const int64_t *h,
                                const int64_t *t, const int64_t *r, int64_t B, int64_t ent_lo, int64_t ent_n, float *Q,
                                int64_t ldq, kge_stream_t stream)
{
    if (side != KGE_SIDE_TAIL && side != KGE_SIDE_HEAD && side != KGE_SIDE_BOTH) return KGE_EINVAL;
    if (d < 1 || B < 0 || lde < 2 * (int64_t)d || ldp < d || ldq < 2 * (int64_t)d || (ent_n >= 0 && ent_lo < 0)) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!E || !P || !r || !Q || (side != KGE_SIDE_HEAD && !h) || (side != KGE_SIDE_TAIL && !t)) return KGE_EINVAL;
    const int64_t rows = side == KGE_SIDE_BOTH ? 2 * B : B;
    hipLaunchKernelGGL(rotate_query_kernel, dim3(grid1d(rows * d, 256)), dim3(256), 0, kge_s(stream), side, E, lde, P, ldp,
                       d, h, t, r, B, ent_lo, ent_n, Q, ldq);
    KGE_CHECK_LAUNCH();
    return 0;
}
