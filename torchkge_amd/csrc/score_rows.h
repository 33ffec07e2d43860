// The per-kind device code of the fused triple scorers, shared by score_triples.hip (one wavefront per triple) and
// score_fact_groups.hip (one workgroup per fact and its K negatives): the rows a triple gathers per model kind, their
// loads, the L2 normalisation, the wavefront sum, the score of a prepared row set and the TorusE helpers.  Both
// translation units inline the same functions under the same flags, which is what makes their scores the same bits.
#pragma once
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
// their latency, not by bytes.  (Summation order differs from wave_sum(): the fused triple scorers only.)
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

// Rows a triple gathers, per model kind -- THE table of the fused triple scorers.  Row j is read from table t<tab> at the id it names
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

// Does the kind's score go through two per-triple scalars, one of the head side and one of the tail side (TransH: h.w and
// t.w, TransD: h.hp and t.tp)?  A scalar of one side depends on that side's entity rows and the relation rows alone.
__host__ __device__ inline constexpr bool has_side_dots(int kind) { return kind == KGE_TRANSH || kind == KGE_TRANSD; }
template <int KIND, int NE>
__device__ __forceinline__ float side_dot(const float (&x)[RowSet<KIND>::NR][NE], int side)
{
    if (KIND == KGE_TRANSH) return dotp<NE>(x[side], x[3]);     // h.w / t.w
    if (KIND == KGE_TRANSD) return dotp<NE>(x[side], x[2 + side]);      // h.hp / t.tp
    return 0.f;
}

// The score of a PREPARED row set: the rows normalised (normalize_rows), for TorusE reduced to their fractional parts,
// and the two side scalars of the kinds that have them (side_dot; ignored otherwise).
template <int KIND, bool VEC4, int NE>
__device__ __forceinline__ float score_prepared(int d_rel, int lane, const float (&x)[RowSet<KIND>::NR][NE], float dot_h, float dot_t)
{
    if (KIND == KGE_TRANSE_L1 || KIND == KGE_TRANSE_L2) {
        const float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2];
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
        const float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) s = s + lp_direct_term<MODE>((h[e] + r[e]) - t[e]);   // (padding: x = 0, term 0)
        return lp_direct_finish<MODE>(wave_sum_dpp(s));
    } else if (KIND == KGE_DISTMULT) {
        const float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) s += (h[e] * r[e]) * t[e];
        return wave_sum_dpp(s);
    } else if (KIND == KGE_COMPLEX) {
        const float (&reh)[NE] = x[0], (&ret)[NE] = x[1], (&imh)[NE] = x[2], (&imt)[NE] = x[3], (&rer)[NE] = x[4], (&imr)[NE] = x[5];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e)
            s += reh[e] * (rer[e] * ret[e] + imr[e] * imt[e]) + imh[e] * (rer[e] * imt[e] - imr[e] * ret[e]);
        return wave_sum_dpp(s);
    } else if (KIND == KGE_TRANSH) {
        const float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[2], (&w)[NE] = x[3];
        const float hw = dot_h, tw = dot_t;
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
        const float (&h)[NE] = x[0], (&t)[NE] = x[1], (&r)[NE] = x[4], (&rp)[NE] = x[5];
        const float sh = dot_h, st = dot_t;
        const int dr = d_rel;
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

// The score of the gathered rows x of one triple: normalise, (TorusE) take the fractional parts, the side scalars, the sum
template <int KIND, bool VEC4, int NE>
__device__ __forceinline__ float score_rows(const ScoreParams &p, int lane, float (&x)[RowSet<KIND>::NR][NE])
{
    float n[RowSet<KIND>::NR];  // (the forward has no use for the norms)
    normalize_rows<KIND, NE, false>(x, n);
    if (is_toruse(KIND)) {
        frac_inplace<NE>(x[0]);
        frac_inplace<NE>(x[1]);
        frac_inplace<NE>(x[2]);
    }
    const float dot_h = side_dot<KIND, NE>(x, 0), dot_t = side_dot<KIND, NE>(x, 1);
    return score_prepared<KIND, VEC4, NE>(p.d_rel, lane, x, dot_h, dot_t);
}

template <bool VEC4, int NE>
__device__ __forceinline__ void store_row(float *__restrict__ g, int d, int lane, const float (&x)[NE])
{
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int k = elem_index<VEC4, NE>(e, lane);
        if (k < d) g[k] = x[e];
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

// The kinds of the fused triple scorers as compile-time constants: f(std::integral_constant<int, KIND>) of the run-time kind
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

// registers per lane a row of dmax floats takes on the float4 / the scalar load path (the NE bucket is the next of 4, 8, 16)
inline int row_regs_per_lane(int dmax, bool vec4) { return vec4 ? ((dmax + 255) / 256) * 4 : (dmax + 63) / 64; }

inline int check_common(int kind, const float *t0, const float *t1, const float *t2, const float *t3,
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

inline bool tables_vec4(const float *t0, const float *t1, const float *t2, const float *t3, int d_ent, int d_rel)
{
    bool v = (d_ent % 4 == 0) && (d_rel % 4 == 0) && kge_aligned16(t0) && kge_aligned16(t1);
    if (t2) v = v && kge_aligned16(t2);
    if (t3) v = v && kge_aligned16(t3);
    return v;
}

} // namespace
