// K1: fused embedding gather + on-the-fly L2 normalisation + score, one
// wavefront per triple (gfx950).  HBM-bound: every table row is read exactly
// once (16 B per lane, coalesced within the row), nothing but the fp32 score is
// written.  Replaces the 6-10 ATen kernels of Model.scoring_function:
//   TransE   models/translation.py:69-81      -|| h^ + r - t^ ||_p (p=1) or squared L2
//   TransH   models/translation.py:183-206    -|| p_w(h^) + r - p_w(t^) ||^2
//   TransD   models/translation.py:538-568    -|| (h^.hp^) rp^ + h^[:dr] + r^ - ... ||^2
//   DistMult models/bilinear.py:188-199       sum h^ r t^
//   ComplEx  models/bilinear.py:460-473       Re<h, r, conj t>   (no normalisation)
// (x^ = x / max(||x||_2, 1e-12), torch.nn.functional.normalize).
// The backward kernel recomputes the forward intermediates from the same
// gathered rows and writes one gradient row per gathered row (or scatters it
// with fp32 atomics).
#include <type_traits>
#include "kge_common.h"

namespace {

constexpr int WAVES_PER_BLOCK = 4;

template <bool VEC4, int NE>
__device__ __forceinline__ void load_row(const float *__restrict__ p, int d, int lane, float (&x)[NE])
{
    if (VEC4) {
#pragma unroll
        for (int c = 0; c < NE / 4; ++c) {
            const int k = (c * 64 + lane) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < d) v = *reinterpret_cast<const float4 *>(p + k);
            x[4 * c] = v.x; x[4 * c + 1] = v.y; x[4 * c + 2] = v.z; x[4 * c + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int k = e * 64 + lane;
            x[e] = (k < d) ? p[k] : 0.f;
        }
    }
}

template <bool VEC4, int NE>
__device__ __forceinline__ int elem_index(int e, int lane)
{
    return VEC4 ? ((e >> 2) * 64 + lane) * 4 + (e & 3) : e * 64 + lane;
}

// Wavefront sum on the DPP cross-lane path of the VALU (quad permutes, row mirrors, row broadcasts;
// the total lands in lane 63 and is read back as a wave-uniform scalar): ~7 dependent full-rate VALU
// ops instead of 6 ds_bpermute round trips through the LDS crossbar (__shfl_xor).  A triple's score is a
// chain of up to six such reductions (norms, projections, the final sum), so this kernel is bound by
// their latency, not by bytes.  (Summation order differs from wave_sum(): this file only.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum_dpp(float v)
{
    v += dpp_mov<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v += dpp_mov<0x141, 0xf>(v);   // row_half_mirror
    v += dpp_mov<0x140, 0xf>(v);   // row_mirror: every lane holds its row's 16-lane sum
    v += dpp_mov<0x142, 0xa>(v);   // row_bcast15 into rows 1 and 3
    v += dpp_mov<0x143, 0xc>(v);   // row_bcast31 into rows 2 and 3: lane 63 holds the total
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

template <int NE>
__device__ __forceinline__ float sumsq(const float (&x)[NE])
{
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) s = fmaf(x[e], x[e], s);
    return wave_sum_dpp(s);
}
template <int NE>
__device__ __forceinline__ float dotp(const float (&x)[NE], const float (&y)[NE])
{
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) s = fmaf(x[e], y[e], s);
    return wave_sum_dpp(s);
}
// F.normalize: x / max(||x||, eps).  EXACT = true keeps the IEEE division per element (the backward, whose two
// reduction modes are compared bit for bit); the forward multiplies by the reciprocal (one division per row,
// <= 1 ulp per element: far inside the 1e-5 score tolerance, ~40 VALU ops per row cheaper).
template <int NE, bool EXACT = true>
__device__ __forceinline__ float normalize_inplace(float (&x)[NE])
{
    const float n = fmaxf(sqrtf(sumsq<NE>(x)), 1e-12f);
    if (EXACT) {
#pragma unroll
        for (int e = 0; e < NE; ++e) x[e] = x[e] / n;
    } else {
        const float rn = 1.0f / n;
#pragma unroll
        for (int e = 0; e < NE; ++e) x[e] = x[e] * rn;
    }
    return n;
}

struct ScoreParams {
    int kind;
    const float *t0, *t1, *t2, *t3;
    int d_ent, d_rel;
    const int64_t *h, *t, *r;
    int64_t B;
    float *out;
};

// Rows a triple gathers, per model kind -- THE table of this file.  Row j is read from table t<tab> at the id it names
// (a row at h or t is d_ent wide, a row at r d_rel wide) and is L2-normalised or not; the backward's gradient of row j is
// gradient stream j of the header's contract (include/kge_hip.h) and is added into g<tab> at the same id.  gather_rows,
// normalize_rows, emit_row and the zero fill of a triple without gradient all read it from here.
//   TransE / DistMult / TorusE: E[h] E[t] R[r]             TransH: E[h] E[t] R[r] W[r]
//   ComplEx: Re[h] Re[t] Im[h] Im[t] Rre[r] Rim[r]         TransD: E[h] E[t] Ep[h] Ep[t] R[r] Rp[r]
enum { ID_H, ID_T, ID_R };
struct Row {
    int tab, id;
    bool norm;
};
struct Rows {
    int n;
    Row row[6];
};
constexpr Rows row_set(int kind)
{
    switch (kind) {
    case KGE_TRANSE_L1:
    case KGE_TRANSE_L2:
    case KGE_DISTMULT: return {3, {{0, ID_H, true}, {0, ID_T, true}, {1, ID_R, false}}};
    case KGE_TRANSH: return {4, {{0, ID_H, true}, {0, ID_T, true}, {1, ID_R, false}, {2, ID_R, true}}};
    case KGE_COMPLEX:
        return {6, {{0, ID_H, false}, {0, ID_T, false}, {1, ID_H, false}, {1, ID_T, false}, {2, ID_R, false}, {3, ID_R, false}}};
    case KGE_TRANSD:
        return {6, {{0, ID_H, true}, {0, ID_T, true}, {2, ID_H, true}, {2, ID_T, true}, {1, ID_R, true}, {3, ID_R, true}}};
    default: return {3, {{0, ID_H, false}, {0, ID_T, false}, {1, ID_R, false}}};    // the four TorusE kinds: frac, no norm
    }
}
template <int KIND> struct RowSet {
    static constexpr int NR = row_set(KIND).n;
    static constexpr Rows rows() { return row_set(KIND); }
};
// one of four pointers by a table number that is a constant once the caller's loop over the rows is unrolled
template <typename T>
__device__ __forceinline__ T *table_of(int tab, T *a0, T *a1, T *a2, T *a3)
{
    return tab == 0 ? a0 : tab == 1 ? a1 : tab == 2 ? a2 : a3;
}

// TorusE (translation.py:705-721): frac(x) = x - trunc(x) (torch.frac: exact in fp32, keeps the sign) of the gathered
// rows, x = (h + r) - t, score = -diss(x) -- the per-element terms of the all-candidates modes (kge_common.h)
__host__ __device__ inline constexpr bool is_toruse(int kind) { return kind >= KGE_TORUSE_L1 && kind <= KGE_TORUSE_TORUS_EL2; }
__host__ __device__ inline constexpr int toruse_mode(int kind)
{
    return kind == KGE_TORUSE_TORUS_L1 ? KGE_LP_TORUS_L1 : kind == KGE_TORUSE_TORUS_L2 ? KGE_LP_TORUS_L2
         : kind == KGE_TORUSE_TORUS_EL2 ? KGE_LP_TORUS_EL2 : KGE_LP_L1_DIRECT;
}
template <int NE>
__device__ __forceinline__ void frac_inplace(float (&x)[NE])
{
#pragma unroll
    for (int e = 0; e < NE; ++e) x[e] = x[e] - truncf(x[e]);
}
// d score / d x of one element (closed form of torch autograd through the reference's expressions): |x| -> sign(x); a
// min() passes the gradient to the branch it took and, at an exact tie, half to each -- the two halves cancel here
template <int MODE>
__device__ __forceinline__ float toruse_dscore(float x, float go)
{
    const float sg = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
    if (MODE == KGE_LP_TORUS_L1) {          // -2 min(a, 1 - a), a = |x|
        const float a = fabsf(x), b = 1.0f - a;
        const float br = (a < b) ? 1.f : ((a > b) ? -1.f : 0.f);
        return go * (-2.f * br * sg);
    } else if (MODE == KGE_LP_TORUS_L2) {   // -4 min(v, 1 - v), v = x * x, dv/dx = 2x
        const float v = x * x, b = 1.0f - v;
        const float br = (v < b) ? 1.f : ((v > b) ? -1.f : 0.f);
        return br * (go * (-8.f * x));
    } else if (MODE == KGE_LP_TORUS_EL2) {  // -(1/4) 2 (1 - cos(2 pi u)), u = min(x, 1 - x)
        const float b = 1.0f - x;
        const float br = (x < b) ? 1.f : ((x > b) ? -1.f : 0.f);
        const float u = fminf(x, b);
        const float gu = (-(go * 0.5f) * sinf(KGE_TWO_PI_F * u)) * KGE_TWO_PI_F;
        return br * gu;
    }
    return go * -sg;                        // 'L1': -|x|
}

template <int KIND, bool VEC4, int NE>
__device__ __forceinline__ void gather_rows(const ScoreParams &p, int64_t hi, int64_t ti, int64_t ri, int lane,
                                            float (&x)[RowSet<KIND>::NR][NE])
{
    constexpr auto rs = RowSet<KIND>::rows();
    const int64_t id[3] = {hi, ti, ri};
    // the loads are issued id by id -- the rows at h, then at t, then at r -- whatever their place in the row set: the two
    // rows of ComplEx at one entity next to each other measured 4 % faster in the forward than in stream order
#pragma unroll
    for (int k = ID_H; k <= ID_R; ++k) {
        const int d = k == ID_R ? p.d_rel : p.d_ent;
#pragma unroll
        for (int j = 0; j < RowSet<KIND>::NR; ++j)
            if (rs.row[j].id == k) load_row<VEC4, NE>(table_of(rs.row[j].tab, p.t0, p.t1, p.t2, p.t3) + id[k] * d, d, lane, x[j]);
    }
}

// F.normalize of the rows that the kind normalises; n[j] = the clamped norm of row j (normalize_bwd)
template <int KIND, int NE, bool EXACT>
__device__ __forceinline__ void normalize_rows(float (&x)[RowSet<KIND>::NR][NE], float (&n)[RowSet<KIND>::NR])
{
    constexpr auto rs = RowSet<KIND>::rows();
#pragma unroll
    for (int j = 0; j < RowSet<KIND>::NR; ++j) n[j] = rs.row[j].norm ? normalize_inplace<NE, EXACT>(x[j]) : 1.f;
}

template <int KIND, bool VEC4, int NE>
__device__ __forceinline__ float score_rows(const ScoreParams &p, int lane, float (&x)[RowSet<KIND>::NR][NE])
{
    float n[RowSet<KIND>::NR];  // (the forward has no use for the norms)
    normalize_rows<KIND, NE, false>(x, n);
    if (KIND == KGE_TRANSE_L1 || KIND == KGE_TRANSE_L2) {
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float diff = (h[e] + r[e]) - t[e];
            s = (KIND == KGE_TRANSE_L1) ? s + fabsf(diff) : fmaf(diff, diff, s);
        }
        s = wave_sum_dpp(s);
        if (KIND == KGE_TRANSE_L2) { const float n = sqrtf(s); s = n * n; } // norm(p=2)**2
        return -s;
    } else if (is_toruse(KIND)) {
        constexpr int MODE = toruse_mode(KIND);
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2];
        frac_inplace<NE>(h);
        frac_inplace<NE>(t);
        frac_inplace<NE>(r);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) s = s + lp_direct_term<MODE>((h[e] + r[e]) - t[e]);   // (padding: x = 0, term 0)
        return lp_direct_finish<MODE>(wave_sum_dpp(s));
    } else if (KIND == KGE_DISTMULT) {
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) s += (h[e] * r[e]) * t[e];
        return wave_sum_dpp(s);
    } else if (KIND == KGE_COMPLEX) {
        float (&reh)[NE] = x[0], (&ret)[NE] = x[1], (&imh)[NE] = x[2], (&imt)[NE] = x[3], (&rer)[NE] = x[4], (&imr)[NE] = x[5];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e)
            s += reh[e] * (rer[e] * ret[e] + imr[e] * imt[e]) + imh[e] * (rer[e] * imt[e] - imr[e] * ret[e]);
        return wave_sum_dpp(s);
    } else if (KIND == KGE_TRANSH) {
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2], (&w)[NE] = x[3];
        const float hw = dotp<NE>(h, w), tw = dotp<NE>(t, w);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float ph = h[e] - hw * w[e];
            const float pt = t[e] - tw * w[e];
            const float diff = (ph + r[e]) - pt;
            s = fmaf(diff, diff, s);
        }
        s = wave_sum_dpp(s);
        const float n = sqrtf(s);
        return -(n * n);
    } else { // KGE_TRANSD
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&hp)[NE] = x[2], (&tp)[NE] = x[3], (&r)[NE] = x[4], (&rp)[NE] = x[5];
        const float sh = dotp<NE>(h, hp), st = dotp<NE>(t, tp);
        const int dr = p.d_rel;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const bool in = elem_index<VEC4, NE>(e, lane) < dr; // ent[:, :rel_emb_dim]
            const float ph = rp[e] * sh + (in ? h[e] : 0.f);
            const float pt = rp[e] * st + (in ? t[e] : 0.f);
            const float diff = (ph + r[e]) - pt;
            s = fmaf(diff, diff, s);
        }
        s = wave_sum_dpp(s);
        const float n = sqrtf(s);
        return -(n * n);
    }
}

// One wavefront per triple, specialised per model kind, software-pipelined over the wavefront's triples
// (PF): the rows of triple i + nwaves are in flight while triple i is normalised / reduced -- a triple is a
// dependent chain  index load -> row gathers -> up to eight wave reductions, and with a handful of triples
// per wavefront nothing else hides that chain.
template <int KIND, bool VEC4, int NE, bool PF>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void score_fwd_kernel(const ScoreParams p)
{
    constexpr int NR = RowSet<KIND>::NR;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * WAVES_PER_BLOCK;
    if (wave >= p.B) return;
    if (!PF) {
        for (int64_t i = wave; i < p.B; i += nwaves) {
            float x[NR][NE];
            gather_rows<KIND, VEC4, NE>(p, p.h[i], p.t[i], p.r[i], lane, x);
            const float score = score_rows<KIND, VEC4, NE>(p, lane, x);
            if (lane == 0) p.out[i] = score;
        }
        return;
    }
    float a[NR][NE], b[NR][NE];
    gather_rows<KIND, VEC4, NE>(p, p.h[wave], p.t[wave], p.r[wave], lane, a);
    for (int64_t i = wave; i < p.B; i += 2 * nwaves) {
        const int64_t i1 = i + nwaves, i2 = i1 + nwaves;
        if (i1 < p.B) gather_rows<KIND, VEC4, NE>(p, p.h[i1], p.t[i1], p.r[i1], lane, b);
        const float sa = score_rows<KIND, VEC4, NE>(p, lane, a);
        if (lane == 0) p.out[i] = sa;
        if (i1 >= p.B) break;
        if (i2 < p.B) gather_rows<KIND, VEC4, NE>(p, p.h[i2], p.t[i2], p.r[i2], lane, a);
        const float sb = score_rows<KIND, VEC4, NE>(p, lane, b);
        if (lane == 0) p.out[i1] = sb;
    }
}

// ---------------------------------------------------------------------------
// backward: d(sum_i go_i * score_i) / d tables, scattered with fp32 atomics.
// With x^ = x/n, n = max(||x||, eps): d/dx = (g - x^ (x^.g)) / n   (n > eps)
// ---------------------------------------------------------------------------
struct BwdParams {
    ScoreParams f;
    const float *go;
    float *g0, *g1, *g2, *g3;
    // row mode (rows != NULL): no atomics -- every triple stores its gradient rows at
    // rows[(stream * B + i) * rows_ld ...]; kge_segment_sum_rows then reduces them by target
    // row in sorted order.  Streams (target table, index):
    //   TransE / DistMult: 0 (g0,h) 1 (g0,t) 2 (g1,r)          TransH: 0 (g0,h) 1 (g0,t) 2 (g1,r) 3 (g2,r)
    //   ComplEx: 0 (g0,h) 1 (g0,t) 2 (g1,h) 3 (g1,t) 4 (g2,r) 5 (g3,r)
    //   TransD:  0 (g0,h) 1 (g0,t) 2 (g2,h) 3 (g2,t) 4 (g1,r) 5 (g3,r)
    float *rows;
    int64_t rows_ld;
};

template <bool VEC4, int NE>
__device__ __forceinline__ void store_row(float *__restrict__ g, int d, int lane, const float (&x)[NE])
{
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int k = elem_index<VEC4, NE>(e, lane);
        if (k < d) g[k] = x[e];
    }
}

template <bool VEC4, int NE>
__device__ __forceinline__ void scatter_row(float *__restrict__ g, int d, int lane, const float (&x)[NE])
{
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int k = elem_index<VEC4, NE>(e, lane);
        if (k < d && x[e] != 0.f) atomicAdd(g + k, x[e]);
    }
}

// gradient wrt the un-normalised row given gradient wrt the normalised row
template <int NE>
__device__ __forceinline__ void normalize_bwd(const float (&xn)[NE], float n, float (&g)[NE])
{
    const float xg = dotp<NE>(xn, g);
    const bool clamped = n <= 1e-12f; // x/eps: plain scaling
#pragma unroll
    for (int e = 0; e < NE; ++e) g[e] = clamped ? g[e] / n : (g[e] - xn[e] * xg) / n;
}

// Gradient row j of triple i (RowSet<KIND>): stream j of the rows buffer or, in the atomic mode, added into row id[j's id]
// of the gradient table of the table row j was read from
template <int KIND, bool VEC4, int NE>
__device__ __forceinline__ void emit_row(const BwdParams &q, int64_t i, const int64_t (&id)[3], int j, int lane,
                                         const float (&g)[NE])
{
    const Row w = RowSet<KIND>::rows().row[j];
    const int d = w.id == ID_R ? q.f.d_rel : q.f.d_ent;
    if (q.rows) store_row<VEC4, NE>(q.rows + ((int64_t)j * q.f.B + i) * q.rows_ld, d, lane, g);
    else scatter_row<VEC4, NE>(table_of(w.tab, q.g0, q.g1, q.g2, q.g3) + id[w.id] * d, d, lane, g);
}

// The counterpart of score_rows: the gradients of the gathered rows x of triple i, each emitted as soon as it is complete
template <int KIND, bool VEC4, int NE>
__device__ __forceinline__ void bwd_rows(const BwdParams &q, int64_t i, const int64_t (&id)[3], float go, int lane,
                                         float (&x)[RowSet<KIND>::NR][NE])
{
    const int dr = q.f.d_rel;
    auto emit = [&](int j, const float (&g)[NE]) __attribute__((always_inline)) { emit_row<KIND, VEC4, NE>(q, i, id, j, lane, g); };
    float n[RowSet<KIND>::NR];
    normalize_rows<KIND, NE, true>(x, n);
    if (KIND == KGE_TRANSE_L1 || KIND == KGE_TRANSE_L2) {
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2];
        float gd[NE];
        // score = -sum f(diff); dscore/ddiff = -sign(diff) (L1) or -2 diff (L2)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float diff = (h[e] + r[e]) - t[e];
            const float sg = (diff > 0.f) ? 1.f : ((diff < 0.f) ? -1.f : 0.f);
            gd[e] = go * ((KIND == KGE_TRANSE_L1) ? -sg : -2.f * diff);
        }
        emit(2, gd);        // d/dr = gd
        float gh[NE], gt[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) { gh[e] = gd[e]; gt[e] = -gd[e]; }
        normalize_bwd<NE>(h, n[0], gh);
        normalize_bwd<NE>(t, n[1], gt);
        emit(0, gh);
        emit(1, gt);
    } else if (is_toruse(KIND)) {
        // frac is applied to the gathered copies' .data: autograd sees the identity, so d/dh = d/dr = dscore/dx and
        // d/dt = -dscore/dx with x = (frac h + frac r) - frac t
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2];
        float gd[NE], gt[NE];
        frac_inplace<NE>(h);
        frac_inplace<NE>(t);
        frac_inplace<NE>(r);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float g = toruse_dscore<toruse_mode(KIND)>((h[e] + r[e]) - t[e], go);
            gd[e] = g;
            gt[e] = -g;
        }
        emit(2, gd);
        emit(0, gd);
        emit(1, gt);
    } else if (KIND == KGE_DISTMULT) {
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2];
        float gh[NE], gt[NE], gr[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            gh[e] = go * r[e] * t[e];
            gt[e] = go * h[e] * r[e];
            gr[e] = go * h[e] * t[e];
        }
        normalize_bwd<NE>(h, n[0], gh);
        normalize_bwd<NE>(t, n[1], gt);
        emit(0, gh);
        emit(1, gt);
        emit(2, gr);
    } else if (KIND == KGE_COMPLEX) {
        float (&reh)[NE] = x[0], (&ret)[NE] = x[1], (&imh)[NE] = x[2], (&imt)[NE] = x[3], (&rer)[NE] = x[4], (&imr)[NE] = x[5];
        float g[NE];    // one gradient row at a time
        // s = reh(rer ret + imr imt) + imh(rer imt - imr ret)
#pragma unroll
        for (int e = 0; e < NE; ++e) g[e] = go * (rer[e] * ret[e] + imr[e] * imt[e]);
        emit(0, g);     // d/d reh
#pragma unroll
        for (int e = 0; e < NE; ++e) g[e] = go * (rer[e] * imt[e] - imr[e] * ret[e]);
        emit(2, g);     // d/d imh
#pragma unroll
        for (int e = 0; e < NE; ++e) g[e] = go * (reh[e] * rer[e] - imh[e] * imr[e]);
        emit(1, g);     // d/d ret
#pragma unroll
        for (int e = 0; e < NE; ++e) g[e] = go * (reh[e] * imr[e] + imh[e] * rer[e]);
        emit(3, g);     // d/d imt
#pragma unroll
        for (int e = 0; e < NE; ++e) g[e] = go * (reh[e] * ret[e] + imh[e] * imt[e]);
        emit(4, g);     // d/d rer
#pragma unroll
        for (int e = 0; e < NE; ++e) g[e] = go * (reh[e] * imt[e] - imh[e] * ret[e]);
        emit(5, g);     // d/d imr
    } else if (KIND == KGE_TRANSH) {
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2], (&w)[NE] = x[3];
        float gd[NE];
        const float hw = dotp<NE>(h, w), tw = dotp<NE>(t, w);
        // diff = (h - t) - (hw - tw) w + r ; score = -|diff|^2
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float diff = ((h[e] - hw * w[e]) + r[e]) - (t[e] - tw * w[e]);
            gd[e] = go * (-2.f * diff);
        }
        emit(2, gd);    // d/dr
        const float gdw = dotp<NE>(gd, w);
        float gh[NE], gt[NE], gw[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            gh[e] = gd[e] - gdw * w[e];         // d/dh^ = gd - (gd.w) w
            gt[e] = -gh[e];
            // d/dw^ = -(hw - tw) gd - (gd.w)(h - t)
            gw[e] = -(hw - tw) * gd[e] - gdw * (h[e] - t[e]);
        }
        normalize_bwd<NE>(h, n[0], gh);
        normalize_bwd<NE>(t, n[1], gt);
        normalize_bwd<NE>(w, n[3], gw);
        emit(0, gh);
        emit(1, gt);
        emit(3, gw);
    } else { // KGE_TRANSD
        float (&h)[NE] = x[0], (&t)[NE] = x[1], (&hp)[NE] = x[2], (&tp)[NE] = x[3], (&r)[NE] = x[4], (&rp)[NE] = x[5];
        float gd[NE];
        const float sh = dotp<NE>(h, hp), st = dotp<NE>(t, tp);
        // diff_k = (sh - st) rp_k + [k<dr](h_k - t_k) + r_k   (k < dr; zero beyond)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const bool in = elem_index<VEC4, NE>(e, lane) < dr;
            const float diff = ((rp[e] * sh + (in ? h[e] : 0.f)) + r[e]) - (rp[e] * st + (in ? t[e] : 0.f));
            gd[e] = in ? go * (-2.f * diff) : 0.f;
        }
        const float gdrp = dotp<NE>(gd, rp);
        float gr[NE], grp[NE], gh[NE], gt[NE], ghp[NE], gtp[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            gr[e] = gd[e];
            grp[e] = (sh - st) * gd[e];
            gh[e] = gd[e] + gdrp * hp[e];   // via [:dr] slice and via sh = h.hp
            gt[e] = -gd[e] - gdrp * tp[e];
            ghp[e] = gdrp * h[e];
            gtp[e] = -gdrp * t[e];
        }
        normalize_bwd<NE>(r, n[4], gr);
        normalize_bwd<NE>(rp, n[5], grp);
        normalize_bwd<NE>(h, n[0], gh);
        normalize_bwd<NE>(t, n[1], gt);
        normalize_bwd<NE>(hp, n[2], ghp);
        normalize_bwd<NE>(tp, n[3], gtp);
        emit(4, gr);
        emit(5, grp);
        emit(0, gh);
        emit(1, gt);
        emit(2, ghp);
        emit(3, gtp);
    }
}

// One wavefront per triple, specialised per model kind as the forward is: gather the kind's rows, recompute the
// forward's intermediates from them, emit one gradient row per gathered row.
template <int KIND, bool VEC4, int NE>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void score_bwd_kernel(const BwdParams q)
{
    constexpr int NR = RowSet<KIND>::NR;
    const ScoreParams &p = q.f;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * WAVES_PER_BLOCK;

    for (int64_t i = wave; i < p.B; i += nwaves) {
        const int64_t id[3] = {p.h[i], p.t[i], p.r[i]};
        const float go = q.go[i];
        if (go == 0.f) {
            if (q.rows) {   // this triple's rows still have to exist (as zeros) for the reduction
                // (d_ent columns of every stream, a stream of d_rel < d_ent wide rows (TransD) included)
                for (int st = 0; st < NR; ++st)
                    for (int k = lane; k < p.d_ent; k += 64) q.rows[((int64_t)st * p.B + i) * q.rows_ld + k] = 0.f;
            }
            continue;
        }
        float x[NR][NE];
        gather_rows<KIND, VEC4, NE>(p, id[ID_H], id[ID_T], id[ID_R], lane, x);
        bwd_rows<KIND, VEC4, NE>(q, i, id, go, lane, x);
    }
}

inline int grid_for(int64_t B)
{
    int64_t blocks = (B + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    static const int64_t cap = kge_env_int("KGE_K1_BLOCKS", 256 * 32); // one triple per wavefront up to B = 32768 (measured 7-15 % faster than 4 per wave), grid-stride beyond
    return (int)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

// The kinds of this file as compile-time constants: f(std::integral_constant<int, KIND>) of the run-time kind
template <typename F>
int dispatch_kind(int kind, F f)
{
    switch (kind) {
    case KGE_TRANSE_L1: return f(std::integral_constant<int, KGE_TRANSE_L1>{});
    case KGE_TRANSE_L2: return f(std::integral_constant<int, KGE_TRANSE_L2>{});
    case KGE_TRANSH: return f(std::integral_constant<int, KGE_TRANSH>{});
    case KGE_TRANSD: return f(std::integral_constant<int, KGE_TRANSD>{});
    case KGE_DISTMULT: return f(std::integral_constant<int, KGE_DISTMULT>{});
    case KGE_COMPLEX: return f(std::integral_constant<int, KGE_COMPLEX>{});
    case KGE_TORUSE_L1: return f(std::integral_constant<int, KGE_TORUSE_L1>{});
    case KGE_TORUSE_TORUS_L1: return f(std::integral_constant<int, KGE_TORUSE_TORUS_L1>{});
    case KGE_TORUSE_TORUS_L2: return f(std::integral_constant<int, KGE_TORUSE_TORUS_L2>{});
    case KGE_TORUSE_TORUS_EL2: return f(std::integral_constant<int, KGE_TORUSE_TORUS_EL2>{});
    default: return KGE_EINVAL;
    }
}

template <typename P, typename KernelSel>
int dispatch_ne(const P &p, int dmax, bool vec4, int64_t B, hipStream_t s, KernelSel sel)
{
    const int per_lane = vec4 ? ((dmax + 255) / 256) * 4 : (dmax + 63) / 64;
    if (per_lane <= 4) return sel(p, std::integral_constant<int, 4>{}, vec4, B, s);
    if (per_lane <= 8) return sel(p, std::integral_constant<int, 8>{}, vec4, B, s);
    if (per_lane <= 16) return sel(p, std::integral_constant<int, 16>{}, vec4, B, s);
    return KGE_EINVAL; // d > 1024 (vec4) / 1024 (scalar) not supported by the register-resident kernel
}

int check_common(int kind, const float *t0, const float *t1, const float *t2, const float *t3,
                 int d_ent, int d_rel, const int64_t *h, const int64_t *t, const int64_t *r, int64_t B)
{
    if (kind < KGE_TRANSE_L1 || (kind > KGE_COMPLEX && !is_toruse(kind))) return KGE_EINVAL;
    if (!t0 || !t1 || d_ent <= 0 || d_rel <= 0 || B < 0) return KGE_EINVAL;
    if (B > 0 && (!h || !t || !r)) return KGE_EINVAL;
    if ((kind == KGE_TRANSH || kind == KGE_TRANSD || kind == KGE_COMPLEX) && !t2) return KGE_EINVAL;
    if ((kind == KGE_TRANSD || kind == KGE_COMPLEX) && !t3) return KGE_EINVAL;
    if (kind != KGE_TRANSD && d_ent != d_rel) return KGE_EINVAL;
    if (kind == KGE_TRANSD && d_ent < d_rel) return KGE_EINVAL;
    return 0;
}

bool tables_vec4(const float *t0, const float *t1, const float *t2, const float *t3, int d_ent, int d_rel)
{
    bool v = (d_ent % 4 == 0) && (d_rel % 4 == 0) && kge_aligned16(t0) && kge_aligned16(t1);
    if (t2) v = v && kge_aligned16(t2);
    if (t3) v = v && kge_aligned16(t3);
    return v;
}

} // namespace

extern "C" int kge_score_triples(int kind, const float *t0, const float *t1, const float *t2,
                                 const float *t3, int d_ent, int d_rel, const int64_t *h,
                                 const int64_t *t, const int64_t *r, int64_t B, float *out,
                                 kge_stream_t stream)
{
    if (kind == KGE_RESCAL || kind == KGE_HOLE)
        return kge_bilinear_score_fwd(kind, t0, t1, d_ent, d_rel, h, t, r, B, out, kge_s(stream));
    if (kind == KGE_TRANSR) return kge_transr_score_fwd(t0, t1, t2, d_ent, d_rel, h, t, r, B, out, kge_s(stream));
    int rc = check_common(kind, t0, t1, t2, t3, d_ent, d_rel, h, t, r, B);
    if (rc) return rc;
    if (B == 0) return 0;
    if (!out) return KGE_EINVAL;
    ScoreParams p{kind, t0, t1, t2, t3, d_ent, d_rel, h, t, r, B, out};
    const bool vec4 = tables_vec4(t0, t1, t2, t3, d_ent, d_rel);
    auto sel = [](const ScoreParams &pp, auto ne, bool v4, int64_t b, hipStream_t s) -> int {
        constexpr int NE = decltype(ne)::value;
        constexpr bool PF = NE <= 8;    // two row sets in registers (6 rows x 16 floats x 2 would not fit)
        const dim3 grid(grid_for(b)), block(WAVES_PER_BLOCK * 64);
        return dispatch_kind(pp.kind, [&](auto k) -> int {
            constexpr int K = decltype(k)::value;
            if (v4) hipLaunchKernelGGL((score_fwd_kernel<K, true, NE, PF>), grid, block, 0, s, pp);
            else hipLaunchKernelGGL((score_fwd_kernel<K, false, NE, PF>), grid, block, 0, s, pp);
            KGE_CHECK_LAUNCH();
            return 0;
        });
    };
    return dispatch_ne(p, d_ent, vec4, B, kge_s(stream), sel);
}

extern "C" int kge_score_triples_bwd(int kind, const float *t0, const float *t1, const float *t2,
                                     const float *t3, int d_ent, int d_rel, const int64_t *h,
                                     const int64_t *t, const int64_t *r, int64_t B, const float *go,
                                     float *g0, float *g1, float *g2, float *g3, float *rows, int64_t rows_ld,
                                     kge_stream_t stream)
{
    if (kind == KGE_RESCAL || kind == KGE_HOLE)
        return kge_bilinear_score_bwd(kind, t0, t1, d_ent, d_rel, h, t, r, B, go, g0, g1, rows, rows_ld, kge_s(stream));
    if (kind == KGE_TRANSR)
        return kge_transr_score_bwd(t0, t1, t2, d_ent, d_rel, h, t, r, B, go, rows, rows_ld, kge_s(stream));
    int rc = check_common(kind, t0, t1, t2, t3, d_ent, d_rel, h, t, r, B);
    if (rc) return rc;
    if (B == 0) return 0;
    if (!go || (!rows && (!g0 || !g1))) return KGE_EINVAL;
    if (rows && rows_ld < d_ent) return KGE_EINVAL;
    if (!rows && (kind == KGE_TRANSH || kind == KGE_TRANSD || kind == KGE_COMPLEX) && !g2) return KGE_EINVAL;
    if (!rows && (kind == KGE_TRANSD || kind == KGE_COMPLEX) && !g3) return KGE_EINVAL;
    BwdParams q{{kind, t0, t1, t2, t3, d_ent, d_rel, h, t, r, B, nullptr}, go, g0, g1, g2, g3, rows, rows_ld};
    const bool vec4 = tables_vec4(t0, t1, t2, t3, d_ent, d_rel);
    auto sel = [](const BwdParams &qq, auto ne, bool v4, int64_t b, hipStream_t s) -> int {
        constexpr int NE = decltype(ne)::value;
        const dim3 grid(grid_for(b)), block(WAVES_PER_BLOCK * 64);
        return dispatch_kind(qq.f.kind, [&](auto k) -> int {
            constexpr int K = decltype(k)::value;
            if (v4) hipLaunchKernelGGL((score_bwd_kernel<K, true, NE>), grid, block, 0, s, qq);
            else hipLaunchKernelGGL((score_bwd_kernel<K, false, NE>), grid, block, 0, s, qq);
            KGE_CHECK_LAUNCH();
            return 0;
        });
    };
    return dispatch_ne(q, d_ent, vec4, B, kge_s(stream), sel);
}
