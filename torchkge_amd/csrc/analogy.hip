// ANALOGY (models/bilinear.py:559-763): DistMult on d_sc scalar coordinates plus ComplEx on d_c complex ones.
// The all-candidates score is one dot product of width K = d_sc + 2 d_c between a query row and the candidate's
// packed row [sc | re | im] (include/kge_hip_analogy.h), so everything downstream of this file is the one-segment
// KGE_LP_DOT problem of DistMult.  This file holds what is specific to the model:
//   - the packing of three tables' rows into one (kge_analogy_pack_rows);
//   - the query rows of the three sides (kge_analogy_query);
//   - scoring_function forward / backward (kge_analogy_score_triples / _bwd).
// All four are gather / elementwise kernels bound by memory: one wavefront per row, lanes over the columns (each
// wavefront load is a contiguous run of 4-byte elements, whatever the base alignment or the leading dimension: the
// re / im segments of a packed row start at columns d_sc and d_sc + d_c, which are 16-byte aligned only by accident, so
// there is no vector body to guard).  Products and sums are separate roundings (-ffp-contract=off): a query row is
// bit for bit the reference's fp32 expression.
#include "kge_common.h"
#include "../../include/kge_hip_analogy.h"

namespace {

constexpr int AN_WAVES = 4;         // rows per block (one per wavefront)
constexpr int AN_MAXD = 512;

struct Tables3 {
    const float *sc, *re, *im;
    int64_t ld_sc, ld_re, ld_im;
};

inline int an_grid(int64_t rows)
{
    const int64_t blocks = (rows + AN_WAVES - 1) / AN_WAVES;
    return (int)(blocks < 256 * 32 ? (blocks > 0 ? blocks : 1) : 256 * 32);
}

int check_dims(int d_sc, int d_c)
{
    if (d_sc < 0 || d_c < 0 || d_sc + d_c < 1 || d_sc > AN_MAXD || d_c > AN_MAXD) return KGE_EUNSUPPORTED;
    return 0;
}

// pointers present and leading dimensions wide enough for the segments that exist
bool tables_ok(const Tables3 &T, int d_sc, int d_c)
{
    if (d_sc > 0 && (!T.sc || T.ld_sc < d_sc)) return false;
    if (d_c > 0 && (!T.re || !T.im || T.ld_re < d_c || T.ld_im < d_c)) return false;
    return true;
}

__global__ __launch_bounds__(AN_WAVES * 64) void analogy_pack_kernel(const Tables3 S, int d_sc, int d_c,
                                                                     const int64_t *__restrict__ idx, int64_t rows,
                                                                     float *__restrict__ P, int64_t ldp)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t j = (int64_t)blockIdx.x * AN_WAVES + w; j < rows; j += (int64_t)gridDim.x * AN_WAVES) {
        const int64_t i = idx ? idx[j] : j;
        float *dst = P + j * ldp;
        const float *sc = S.sc + i * S.ld_sc, *re = S.re + i * S.ld_re, *im = S.im + i * S.ld_im;
        for (int k = lane; k < d_sc; k += 64) dst[k] = sc[k];
        for (int k = lane; k < d_c; k += 64) {
            dst[d_sc + k] = re[k];
            dst[d_sc + d_c + k] = im[k];
        }
    }
}

struct QueryParams {
    int side;
    Tables3 E, R;
    int d_sc, d_c;
    const int64_t *h, *t, *r;
    int64_t B, n_rows, ent_lo, ent_n;
    float *Q;
    int64_t ldq;
};

// One wavefront per output row.  Every side is a product of two packed operands a, b:
//   tail side       a = entity h, b = relation:  a b        = [ sa sb | ra rb - ia ib | ra ib + ia rb ]
//   head side       a = relation, b = entity t:  conj(a) b  = [ sa sb | ra rb + ia ib | ra ib - ia rb ]
//   relation side   a = entity h, b = entity t:  conj(a) b
__global__ __launch_bounds__(AN_WAVES * 64) void analogy_query_kernel(const QueryParams p)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int d_sc = p.d_sc, d_c = p.d_c;
    const bool gathered = !p.r && !p.h && !p.t;
    for (int64_t pos = (int64_t)blockIdx.x * AN_WAVES + w; pos < p.n_rows; pos += (int64_t)gridDim.x * AN_WAVES) {
        const bool second = p.side == KGE_SIDE_BOTH && pos >= p.B;
        const bool head = p.side == KGE_SIDE_HEAD || second;
        const bool rel = p.side == KGE_ANALOGY_SIDE_REL;
        const int64_t f = second ? pos - p.B : pos;
        float *q = p.Q + pos * p.ldq;
        // rows of the two operands (a: first factor, b: second factor)
        int64_t ea, eb = 0;         // ea: the entity row (relation side: the head's), eb: relation side, the tail's
        bool own = true;
        if (gathered) {
            ea = pos;
            eb = f;
        } else if (rel) {
            ea = p.h[f];
            eb = p.t[f];
        } else {
            ea = (head ? p.t[f] : p.h[f]) - (p.ent_n >= 0 ? p.ent_lo : 0);
            own = p.ent_n < 0 || (ea >= 0 && ea < p.ent_n);
        }
        if (!own) {
            for (int k = lane; k < d_sc + 2 * d_c; k += 64) q[k] = 0.f;
            continue;
        }
        const float *e_sc = p.E.sc + ea * p.E.ld_sc, *e_re = p.E.re + ea * p.E.ld_re, *e_im = p.E.im + ea * p.E.ld_im;
        const float *o_sc, *o_re, *o_im;    // the other operand: a relation's rows, or (relation side) the tail's
        if (rel && !gathered) {
            o_sc = p.E.sc + eb * p.E.ld_sc; o_re = p.E.re + eb * p.E.ld_re; o_im = p.E.im + eb * p.E.ld_im;
        } else {
            const int64_t rr = gathered ? f : p.r[f];
            o_sc = p.R.sc + rr * p.R.ld_sc; o_re = p.R.re + rr * p.R.ld_re; o_im = p.R.im + rr * p.R.ld_im;
        }
        for (int k = lane; k < d_sc; k += 64) q[k] = e_sc[k] * o_sc[k];
        if (rel) {                  // conj(h) t
            for (int k = lane; k < d_c; k += 64) {
                const float rh = e_re[k], ih = e_im[k], rt = o_re[k], it = o_im[k];
                q[d_sc + k] = rh * rt + ih * it;
                q[d_sc + d_c + k] = rh * it - ih * rt;
            }
        } else if (head) {          // conj(r) t
            for (int k = lane; k < d_c; k += 64) {
                const float rt = e_re[k], it = e_im[k], rr = o_re[k], ir = o_im[k];
                q[d_sc + k] = rr * rt + ir * it;
                q[d_sc + d_c + k] = rr * it - ir * rt;
            }
        } else {                    // h r
            for (int k = lane; k < d_c; k += 64) {
                const float rh = e_re[k], ih = e_im[k], rr = o_re[k], ir = o_im[k];
                q[d_sc + k] = rh * rr - ih * ir;
                q[d_sc + d_c + k] = rh * ir + ih * rr;
            }
        }
    }
}

struct ScoreParams {
    Tables3 E, R;
    int d_sc, d_c;
    const int64_t *h, *t, *r;
    int64_t B;
    float *out;
    const float *go;
    float *rows;
    int64_t rows_ld;
};

__global__ __launch_bounds__(AN_WAVES * 64) void analogy_score_fwd_kernel(const ScoreParams p)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * AN_WAVES + w; i < p.B; i += (int64_t)gridDim.x * AN_WAVES) {
        const int64_t h = p.h[i], t = p.t[i], r = p.r[i];
        const float *sh = p.E.sc + h * p.E.ld_sc, *st = p.E.sc + t * p.E.ld_sc, *sr = p.R.sc + r * p.R.ld_sc;
        const float *rh = p.E.re + h * p.E.ld_re, *rt = p.E.re + t * p.E.ld_re, *rr = p.R.re + r * p.R.ld_re;
        const float *ih = p.E.im + h * p.E.ld_im, *it = p.E.im + t * p.E.ld_im, *ir = p.R.im + r * p.R.ld_im;
        float part = 0.f;
        for (int k = lane; k < p.d_sc; k += 64) part += sh[k] * sr[k] * st[k];
        for (int k = lane; k < p.d_c; k += 64) {
            const float a = rr[k] * rt[k] + ir[k] * it[k], b = rr[k] * it[k] - ir[k] * rt[k];
            part += rh[k] * a + ih[k] * b;
        }
        const float s = wave_sum(part);
        if (lane == 0) p.out[i] = s;
    }
}

// the three gradient rows of a triple are its three query formulas scaled by go: d/dh = go (conj(r) t),
// d/dt = go (h r), d/dr = go (conj(h) t)
__global__ __launch_bounds__(AN_WAVES * 64) void analogy_score_bwd_kernel(const ScoreParams p)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int d_sc = p.d_sc, d_c = p.d_c;
    for (int64_t i = (int64_t)blockIdx.x * AN_WAVES + w; i < p.B; i += (int64_t)gridDim.x * AN_WAVES) {
        const int64_t h = p.h[i], t = p.t[i], r = p.r[i];
        const float go = p.go[i];
        const float *sh = p.E.sc + h * p.E.ld_sc, *st = p.E.sc + t * p.E.ld_sc, *sr = p.R.sc + r * p.R.ld_sc;
        const float *rh = p.E.re + h * p.E.ld_re, *rt = p.E.re + t * p.E.ld_re, *rr = p.R.re + r * p.R.ld_re;
        const float *ih = p.E.im + h * p.E.ld_im, *it = p.E.im + t * p.E.ld_im, *ir = p.R.im + r * p.R.ld_im;
        float *gh = p.rows + i * p.rows_ld, *gt = p.rows + (p.B + i) * p.rows_ld, *gr = p.rows + (2 * p.B + i) * p.rows_ld;
        for (int k = lane; k < d_sc; k += 64) {
            const float a = sh[k], b = st[k], c = sr[k];
            gh[k] = go * (c * b);
            gt[k] = go * (a * c);
            gr[k] = go * (a * b);
        }
        for (int k = lane; k < d_c; k += 64) {
            const float a = rh[k], b = ih[k], c = rt[k], d = it[k], e = rr[k], f = ir[k];
            gh[d_sc + k] = go * (e * c + f * d);
            gh[d_sc + d_c + k] = go * (e * d - f * c);
            gt[d_sc + k] = go * (a * e - b * f);
            gt[d_sc + d_c + k] = go * (a * f + b * e);
            gr[d_sc + k] = go * (a * c + b * d);
            gr[d_sc + d_c + k] = go * (a * d - b * c);
        }
    }
}

} // namespace

extern "C" int kge_analogy_pack_rows(const float *sc, int64_t ld_sc, const float *re, int64_t ld_re, const float *im,
                                     int64_t ld_im, int d_sc, int d_c, const int64_t *idx, int64_t rows, float *P,
                                     int64_t ldp, kge_stream_t stream)
{
    int rc = check_dims(d_sc, d_c);
    if (rc) return rc;
    if (rows < 0 || ldp < (int64_t)d_sc + 2 * d_c) return KGE_EINVAL;
    if (rows == 0) return 0;
    const Tables3 S{sc, re, im, ld_sc, ld_re, ld_im};
    if (!tables_ok(S, d_sc, d_c) || !P) return KGE_EINVAL;
    hipLaunchKernelGGL(analogy_pack_kernel, dim3(an_grid(rows)), dim3(AN_WAVES * 64), 0, kge_s(stream), S, d_sc, d_c, idx,
                       rows, P, ldp);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_analogy_query(int side, const float *sc_e, int64_t ld_sce, const float *re_e, int64_t ld_ree,
                                 const float *im_e, int64_t ld_ime, const float *sc_r, int64_t ld_scr, const float *re_r,
                                 int64_t ld_rer, const float *im_r, int64_t ld_imr, int d_sc, int d_c, const int64_t *h,
                                 const int64_t *t, const int64_t *r, int64_t B, int64_t ent_lo, int64_t ent_n, float *Q,
                                 int64_t ldq, kge_stream_t stream)
{
    const bool rel = side == KGE_ANALOGY_SIDE_REL;
    if (side != KGE_SIDE_TAIL && side != KGE_SIDE_HEAD && side != KGE_SIDE_BOTH && !rel) return KGE_EINVAL;
    int rc = check_dims(d_sc, d_c);
    if (rc) return rc;
    if (B < 0 || ldq < (int64_t)d_sc + 2 * d_c) return KGE_EINVAL;
    const bool gathered = !h && !t && !r;
    if (ent_n >= 0 && (rel || gathered)) return KGE_EINVAL;
    if (B == 0) return 0;
    const Tables3 E{sc_e, re_e, im_e, ld_sce, ld_ree, ld_ime}, R{sc_r, re_r, im_r, ld_scr, ld_rer, ld_imr};
    if (!Q || !tables_ok(E, d_sc, d_c)) return KGE_EINVAL;
    if (!(rel && !gathered) && !tables_ok(R, d_sc, d_c)) return KGE_EINVAL;
    if (!gathered) {
        if (rel ? (!h || !t) : !r) return KGE_EINVAL;
        if (!rel && ((side != KGE_SIDE_HEAD && !h) || (side != KGE_SIDE_TAIL && !t))) return KGE_EINVAL;
    }
    const int64_t rows = side == KGE_SIDE_BOTH ? 2 * B : B;
    const QueryParams p{side, E, R, d_sc, d_c, h, t, r, B, rows, ent_lo, ent_n, Q, ldq};
    hipLaunchKernelGGL(analogy_query_kernel, dim3(an_grid(rows)), dim3(AN_WAVES * 64), 0, kge_s(stream), p);
    KGE_CHECK_LAUNCH();
    return 0;
}

static int check_score(const Tables3 &E, const Tables3 &R, int d_sc, int d_c, const int64_t *h, const int64_t *t,
                       const int64_t *r, int64_t B)
{
    int rc = check_dims(d_sc, d_c);
    if (rc) return rc;
    if (B < 0 || (B > 0 && (!h || !t || !r))) return KGE_EINVAL;
    if (B > 0 && (!tables_ok(E, d_sc, d_c) || !tables_ok(R, d_sc, d_c))) return KGE_EINVAL;
    return 0;
}

extern "C" int kge_analogy_score_triples(const float *sc_e, int64_t ld_sce, const float *re_e, int64_t ld_ree,
                                         const float *im_e, int64_t ld_ime, const float *sc_r, int64_t ld_scr,
                                         const float *re_r, int64_t ld_rer, const float *im_r, int64_t ld_imr, int d_sc,
                                         int d_c, const int64_t *h, const int64_t *t, const int64_t *r, int64_t B,
                                         float *out, kge_stream_t stream)
{
    const Tables3 E{sc_e, re_e, im_e, ld_sce, ld_ree, ld_ime}, R{sc_r, re_r, im_r, ld_scr, ld_rer, ld_imr};
    int rc = check_score(E, R, d_sc, d_c, h, t, r, B);
    if (rc) return rc;
    if (B == 0) return 0;
    if (!out) return KGE_EINVAL;
    const ScoreParams p{E, R, d_sc, d_c, h, t, r, B, out, nullptr, nullptr, 0};
    hipLaunchKernelGGL(analogy_score_fwd_kernel, dim3(an_grid(B)), dim3(AN_WAVES * 64), 0, kge_s(stream), p);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_analogy_score_triples_bwd(const float *sc_e, int64_t ld_sce, const float *re_e, int64_t ld_ree,
                                             const float *im_e, int64_t ld_ime, const float *sc_r, int64_t ld_scr,
                                             const float *re_r, int64_t ld_rer, const float *im_r, int64_t ld_imr,
                                             int d_sc, int d_c, const int64_t *h, const int64_t *t, const int64_t *r,
                                             int64_t B, const float *go, float *rows, int64_t rows_ld,
                                             kge_stream_t stream)
{
    const Tables3 E{sc_e, re_e, im_e, ld_sce, ld_ree, ld_ime}, R{sc_r, re_r, im_r, ld_scr, ld_rer, ld_imr};
    int rc = check_score(E, R, d_sc, d_c, h, t, r, B);
    if (rc) return rc;
    if (rows_ld < (int64_t)d_sc + 2 * d_c) return KGE_EINVAL;
    if (B == 0) return 0;
    if (!go || !rows) return KGE_EINVAL;
    const ScoreParams p{E, R, d_sc, d_c, h, t, r, B, nullptr, go, rows, rows_ld};
    hipLaunchKernelGGL(analogy_score_bwd_kernel, dim3(an_grid(B)), dim3(AN_WAVES * 64), 0, kge_s(stream), p);
    KGE_CHECK_LAUNCH();
    return 0;
}
