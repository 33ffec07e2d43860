// A fact and its K negatives in one pass (include/kge_hip_factgroup.h): one workgroup per fact (the forward: per fact and
// chunk of its negatives), its WAVES_PER_BLOCK wavefronts split the negatives into consecutive slices.  Every wavefront
// gathers and normalises the fact's rows once and keeps them in registers; per negative it loads only the replaced entity's
// row(s) -- one, or two for ComplEx and TransD -- with the next negative's rows in flight while the current one is reduced.
// The scores come out of the functions of score_rows.h that kge_score_triples inlines, on the same prepared values: the
// same bits.
//
// The backward accumulates, per wavefront, the gradient with respect to the PREPARED (normalised) fact rows over its slice
// (wavefront 0: the positive first), combines the four partials through the LDS in ascending wavefront order, applies
// normalize_bwd once per row (it is linear in the incoming gradient) and stores ONE row per fact row; the replaced rows'
// gradients go out one per negative.  No float atomic; the order of the additions depends on (K, d) alone.
#include "score_rows.h"
#include "../../include/kge_hip_factgroup.h"

namespace {

struct FactParams {
    ScoreParams f;              // tables, widths, the facts (f.out: pos)
    const int64_t *neg_h, *neg_t;
    int64_t K;
    int chunks;                 // forward: the blocks a fact's K negatives are cut into (gridDim.y)
    float *neg;
    int64_t ld_neg;
    // backward
    const float *go_pos, *go_neg;
    int64_t ld_go;
    float *rows;
    int64_t rows_ld;
    int64_t *ids;
};

// entity tables of a kind (the rows at h and t come in pairs: rows 2 s and 2 s + 1 of the row set belong to entity slot s)
template <int KIND> struct Slots {
    static constexpr int NR = RowSet<KIND>::NR;
    static constexpr int NENT = (KIND == KGE_COMPLEX || KIND == KGE_TRANSD) ? 2 : 1;
    static constexpr bool ent_norm() { return RowSet<KIND>::rows().row[0].norm; }
};

// The replaced entity's rows of one negative, as loaded: the rows of the head when the negative is head-corrupted
// (neg_h != h), of neg_t otherwise -- a negative that breaks the contract is scored as (neg_h, r, t).
template <int KIND, int NE> struct NegRows {
    float v[Slots<KIND>::NENT][NE];
    int64_t id;
    bool head;
    float go;
};

template <int KIND, bool VEC4, int NE, bool BWD>
__device__ __forceinline__ void load_neg(const FactParams &q, int64_t i, int64_t hi, int64_t k, int lane, NegRows<KIND, NE> &n)
{
    constexpr auto rs = RowSet<KIND>::rows();
    const int64_t at = k * q.f.B + i;
    const int64_t nh = q.neg_h[at];
    n.head = nh != hi;
    n.id = n.head ? nh : q.neg_t[at];
    if (BWD) n.go = q.go_neg[k * q.ld_go + i];
#pragma unroll
    for (int s = 0; s < Slots<KIND>::NENT; ++s)
        load_row<VEC4, NE>(table_of(rs.row[2 * s].tab, q.f.t0, q.f.t1, q.f.t2, q.f.t3) + n.id * q.f.d_ent, q.f.d_ent, lane, n.v[s]);
}

// normalise (or take the fractional part of) the replaced rows as normalize_rows / score_rows do for a gathered row
template <int KIND, int NE, bool EXACT>
__device__ __forceinline__ void prepare_neg(NegRows<KIND, NE> &n, float (&nn)[Slots<KIND>::NENT])
{
#pragma unroll
    for (int s = 0; s < Slots<KIND>::NENT; ++s) {
        nn[s] = Slots<KIND>::ent_norm() ? normalize_inplace<NE, EXACT>(n.v[s]) : 1.f;
        if (is_toruse(KIND)) frac_inplace<NE>(n.v[s]);
    }
}

// the fact's rows: gathered, normalised, for TorusE reduced to their fractional parts; n[j]: the clamped norms
template <int KIND, bool VEC4, int NE, bool EXACT>
__device__ __forceinline__ void prepare_fact(const ScoreParams &p, int64_t hi, int64_t ti, int64_t ri, int lane,
                                             float (&x)[RowSet<KIND>::NR][NE], float (&n)[RowSet<KIND>::NR])
{
    gather_rows<KIND, VEC4, NE>(p, hi, ti, ri, lane, x);
    normalize_rows<KIND, NE, EXACT>(x, n);
    if (is_toruse(KIND)) {
        frac_inplace<NE>(x[0]);
        frac_inplace<NE>(x[1]);
        frac_inplace<NE>(x[2]);
    }
}

// the prepared row set of a negative: the fact's rows with the replaced side's taken from n; the side scalars likewise
template <int KIND, int NE>
__device__ __forceinline__ void negative_rows(const float (&x)[RowSet<KIND>::NR][NE], const NegRows<KIND, NE> &n, float dot_h,
                                              float dot_t, float (&y)[RowSet<KIND>::NR][NE], float &ydot_h, float &ydot_t)
{
    constexpr int NR = RowSet<KIND>::NR;
    constexpr auto rs = RowSet<KIND>::rows();
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const bool mine = rs.row[j].id != ID_R && ((rs.row[j].id == ID_H) == n.head);    // the row this negative replaces
        constexpr int NENT = Slots<KIND>::NENT;
#pragma unroll
        for (int e = 0; e < NE; ++e) y[j][e] = mine ? n.v[j / 2 < NENT ? j / 2 : 0][e] : x[j][e];
    }
    ydot_h = dot_h;
    ydot_t = dot_t;
    if (has_side_dots(KIND)) {
        // (the scalar of the replaced side from the rows it is made of: dotp of the same values as side_dot on y)
        const float nd = KIND == KGE_TRANSH ? dotp<NE>(n.v[0], x[3]) : dotp<NE>(n.v[0], n.v[Slots<KIND>::NENT - 1]);
        ydot_h = n.head ? nd : dot_h;
        ydot_t = n.head ? dot_t : nd;
    }
}

// part s of n of the negatives [lo, hi): [lo + s (hi - lo) / n, lo + (s + 1) (hi - lo) / n)
__device__ __forceinline__ void k_slice(int64_t lo, int64_t hi, int s, int n, int64_t &k0, int64_t &k1)
{
    k0 = lo + (int64_t)s * (hi - lo) / n;
    k1 = lo + (int64_t)(s + 1) * (hi - lo) / n;
}

template <int KIND, bool VEC4, int NE>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void fact_fwd_kernel(const FactParams q)
{
    constexpr int NR = RowSet<KIND>::NR;
    const ScoreParams &p = q.f;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    // the forward has nothing to combine, so a fact's negatives are cut into chunks (blockIdx.y), each a block of its own:
    // K = 1024 on 512 facts would otherwise be 2 wavefronts per SIMD walking 256 negatives each
    const bool first = blockIdx.y == 0 && w == 0;   // ... and this wavefront has the positive
    int64_t c0, c1, k0, k1;
    k_slice(0, q.K, blockIdx.y, q.chunks, c0, c1);
    k_slice(c0, c1, w, WAVES_PER_BLOCK, k0, k1);
    if (!first && k0 == k1) return;     // an empty slice (a chunk of fewer negatives than the wavefronts of a block)
    const int64_t hi = p.h[i];
    float x[NR][NE], n[NR];
    prepare_fact<KIND, VEC4, NE, false>(p, hi, p.t[i], p.r[i], lane, x, n);
    const float dot_h = side_dot<KIND, NE>(x, 0), dot_t = side_dot<KIND, NE>(x, 1);
    NegRows<KIND, NE> a, b;
    if (k0 < k1) load_neg<KIND, VEC4, NE, false>(q, i, hi, k0, lane, a);
    if (first) {
        const float s = score_prepared<KIND, VEC4, NE>(p.d_rel, lane, x, dot_h, dot_t);
        if (lane == 0) p.out[i] = s;
    }
    auto score = [&](NegRows<KIND, NE> &m, int64_t k) __attribute__((always_inline)) {
        float nn[Slots<KIND>::NENT], y[NR][NE], yh, yt;
        prepare_neg<KIND, NE, false>(m, nn);
        negative_rows<KIND, NE>(x, m, dot_h, dot_t, y, yh, yt);
        const float s = score_prepared<KIND, VEC4, NE>(p.d_rel, lane, y, yh, yt);
        if (lane == 0) q.neg[k * q.ld_neg + i] = s;
    };
    for (int64_t k = k0; k < k1; k += 2) {      // two row sets: the next negative's rows are in flight under this one's sums
        if (k + 1 < k1) load_neg<KIND, VEC4, NE, false>(q, i, hi, k + 1, lane, b);
        score(a, k);
        if (k + 1 >= k1) break;
        if (k + 2 < k1) load_neg<KIND, VEC4, NE, false>(q, i, hi, k + 2, lane, a);
        score(b, k + 1);
    }
}

// d (go * score) / d the PREPARED rows y of one triple: bwd_rows' algebra of score_triples.hip before its normalize_bwd
template <int KIND, bool VEC4, int NE>
__device__ __forceinline__ void grad_prepared(int dr, int lane, const float (&y)[RowSet<KIND>::NR][NE], float dot_h, float dot_t,
                                              float go, float (&g)[RowSet<KIND>::NR][NE])
{
    if (KIND == KGE_TRANSE_L1 || KIND == KGE_TRANSE_L2) {
        const float (&h)[NE] = y[0], (&t)[NE] = y[1], (&r)[NE] = y[2];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float diff = (h[e] + r[e]) - t[e];
            const float sg = (diff > 0.f) ? 1.f : ((diff < 0.f) ? -1.f : 0.f);
            const float gd = go * ((KIND == KGE_TRANSE_L1) ? -sg : -2.f * diff);
            g[2][e] = gd;
            g[0][e] = gd;
            g[1][e] = -gd;
        }
    } else if (is_toruse(KIND)) {
        const float (&h)[NE] = y[0], (&t)[NE] = y[1], (&r)[NE] = y[2];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float gd = toruse_dscore<toruse_mode(KIND)>((h[e] + r[e]) - t[e], go);
            g[2][e] = gd;
            g[0][e] = gd;
            g[1][e] = -gd;
        }
    } else if (KIND == KGE_DISTMULT) {
        const float (&h)[NE] = y[0], (&t)[NE] = y[1], (&r)[NE] = y[2];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            g[0][e] = go * r[e] * t[e];
            g[1][e] = go * h[e] * r[e];
            g[2][e] = go * h[e] * t[e];
        }
    } else if (KIND == KGE_COMPLEX) {
        const float (&reh)[NE] = y[0], (&ret)[NE] = y[1], (&imh)[NE] = y[2], (&imt)[NE] = y[3], (&rer)[NE] = y[4], (&imr)[NE] = y[5];
        // s = reh(rer ret + imr imt) + imh(rer imt - imr ret)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            g[0][e] = go * (rer[e] * ret[e] + imr[e] * imt[e]);
            g[2][e] = go * (rer[e] * imt[e] - imr[e] * ret[e]);
            g[1][e] = go * (reh[e] * rer[e] - imh[e] * imr[e]);
            g[3][e] = go * (reh[e] * imr[e] + imh[e] * rer[e]);
            g[4][e] = go * (reh[e] * ret[e] + imh[e] * imt[e]);
            g[5][e] = go * (reh[e] * imt[e] - imh[e] * ret[e]);
        }
    } else if (KIND == KGE_TRANSH) {
        const float (&h)[NE] = y[0], (&t)[NE] = y[1], (&r)[NE] = y[2], (&w)[NE] = y[3];
        const float hw = dot_h, tw = dot_t;
        // diff = (h - t) - (hw - tw) w + r ; score = -|diff|^2
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float diff = ((h[e] - hw * w[e]) + r[e]) - (t[e] - tw * w[e]);
            g[2][e] = go * (-2.f * diff);
        }
        const float gdw = dotp<NE>(g[2], w);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float gd = g[2][e];
            g[0][e] = gd - gdw * w[e];          // d/dh^ = gd - (gd.w) w
            g[1][e] = -g[0][e];
            g[3][e] = -(hw - tw) * gd - gdw * (h[e] - t[e]);    // d/dw^ = -(hw - tw) gd - (gd.w)(h - t)
        }
    } else { // KGE_TRANSD
        const float (&h)[NE] = y[0], (&t)[NE] = y[1], (&hp)[NE] = y[2], (&tp)[NE] = y[3], (&r)[NE] = y[4], (&rp)[NE] = y[5];
        const float sh = dot_h, st = dot_t;
        // diff_k = (sh - st) rp_k + [k<dr](h_k - t_k) + r_k   (k < dr; zero beyond)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const bool in = elem_index<VEC4, NE>(e, lane) < dr;
            const float diff = ((rp[e] * sh + (in ? h[e] : 0.f)) + r[e]) - (rp[e] * st + (in ? t[e] : 0.f));
            g[4][e] = in ? go * (-2.f * diff) : 0.f;
        }
        const float gdrp = dotp<NE>(g[4], rp);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float gd = g[4][e];
            g[5][e] = (sh - st) * gd;
            g[0][e] = gd + gdrp * hp[e];        // via [:dr] slice and via sh = h.hp
            g[1][e] = -gd - gdrp * tp[e];
            g[2][e] = gdrp * h[e];
            g[3][e] = -gdrp * t[e];
        }
    }
}

// The row of the rows buffer (kge_hip_factgroup.h, "The rows buffer"): entity slot s holds (K + 2) B rows -- the B rows at
// h, the B rows at t, the K B replaced rows -- and the relation rows follow, B per relation table.
__device__ __forceinline__ int64_t ent_block(const FactParams &q, int s) { return (int64_t)s * (q.K + 2) * q.f.B; }

template <int KIND, bool VEC4, int NE>
__global__ __launch_bounds__(WAVES_PER_BLOCK * 64) void fact_bwd_kernel(const FactParams q)
{
    constexpr int NR = RowSet<KIND>::NR, NENT = Slots<KIND>::NENT;
    constexpr auto rs = RowSet<KIND>::rows();
    __shared__ float part[WAVES_PER_BLOCK][NR][NE * 64];
    const ScoreParams &p = q.f;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t i = blockIdx.x, B = p.B;
    int64_t k0, k1;
    k_slice(0, q.K, w, WAVES_PER_BLOCK, k0, k1);
    const int64_t hi = p.h[i], ti = p.t[i];
    float x[NR][NE], n[NR], acc[NR][NE];
    prepare_fact<KIND, VEC4, NE, true>(p, hi, ti, p.r[i], lane, x, n);
    const float dot_h = side_dot<KIND, NE>(x, 0), dot_t = side_dot<KIND, NE>(x, 1);
    NegRows<KIND, NE> a, b;
    if (k0 < k1) load_neg<KIND, VEC4, NE, true>(q, i, hi, k0, lane, a);
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[j][e] = 0.f;
    if (w == 0) {       // the positive: every row of the fact
        grad_prepared<KIND, VEC4, NE>(p.d_rel, lane, x, dot_h, dot_t, q.go_pos[i], acc);
        if (lane == 0) {
            q.ids[i] = hi;
            q.ids[B + i] = ti;
        }
    }
    auto negative = [&](NegRows<KIND, NE> &m, int64_t k) __attribute__((always_inline)) {
        float nn[NENT], y[NR][NE], g[NR][NE], yh, yt;
        prepare_neg<KIND, NE, true>(m, nn);
        negative_rows<KIND, NE>(x, m, dot_h, dot_t, y, yh, yt);
        grad_prepared<KIND, VEC4, NE>(p.d_rel, lane, y, yh, yt, m.go, g);
        // the rows this negative shares with the fact
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const bool shared = rs.row[j].id == ID_R || ((rs.row[j].id == ID_H) != m.head);
#pragma unroll
            for (int e = 0; e < NE; ++e) acc[j][e] = shared ? acc[j][e] + g[j][e] : acc[j][e];
        }
        // the rows it replaces: one gradient row per entity table
        const int64_t at = 2 * B + k * B + i;
#pragma unroll
        for (int s = 0; s < NENT; ++s) {
            float gn[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) gn[e] = m.head ? g[2 * s][e] : g[2 * s + 1][e];
            if (Slots<KIND>::ent_norm()) normalize_bwd<NE>(m.v[s], nn[s], gn);
            store_row<VEC4, NE>(q.rows + (ent_block(q, s) + at) * q.rows_ld, p.d_ent, lane, gn);
        }
        if (lane == 0) q.ids[at] = m.id;
    };
    for (int64_t k = k0; k < k1; k += 2) {
        if (k + 1 < k1) load_neg<KIND, VEC4, NE, true>(q, i, hi, k + 1, lane, b);
        negative(a, k);
        if (k + 1 >= k1) break;
        if (k + 2 < k1) load_neg<KIND, VEC4, NE, true>(q, i, hi, k + 2, lane, a);
        negative(b, k + 1);
    }
    // the four partials of every fact row, added in ascending wavefront order; row j is finished by wavefront j mod 4
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int e = 0; e < NE; ++e) part[w][j][e * 64 + lane] = acc[j][e];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        if (j % WAVES_PER_BLOCK != w) continue;
        float g[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            float s = part[0][j][e * 64 + lane];
#pragma unroll
            for (int u = 1; u < WAVES_PER_BLOCK; ++u) s = s + part[u][j][e * 64 + lane];
            g[e] = s;
        }
        if (rs.row[j].norm) normalize_bwd<NE>(x[j], n[j], g);
        const bool rel = rs.row[j].id == ID_R;
        const int64_t row = rel ? ent_block(q, NENT) + (int64_t)(j - 2 * NENT) * B + i
                                : ent_block(q, j / 2) + (rs.row[j].id == ID_T ? B : 0) + i;
        store_row<VEC4, NE>(q.rows + row * q.rows_ld, rel ? p.d_rel : p.d_ent, lane, g);
    }
}

inline bool kind_served(int kind) { return kind >= KGE_TRANSE_L1 && (kind <= KGE_COMPLEX || is_toruse(kind)); }
inline int ent_tables(int kind) { return (kind == KGE_COMPLEX || kind == KGE_TRANSD) ? 2 : 1; }
inline int rel_tables(int kind) { return (kind == KGE_TRANSE_L1 || kind == KGE_TRANSE_L2 || kind == KGE_DISTMULT || is_toruse(kind)) ? 1 : 2; }

int check_groups(int kind, const float *t0, const float *t1, const float *t2, const float *t3, int d_ent, int d_rel,
                 const int64_t *h, const int64_t *t, const int64_t *r, int64_t B, const int64_t *neg_h, const int64_t *neg_t,
                 int64_t K)
{
    int rc = check_common(kind, t0, t1, t2, t3, d_ent, d_rel, h, t, r, B);
    if (rc) return rc;
    if (B == 0) return 0;
    if (K < 1 || K >= ((int64_t)1 << 31) || B >= ((int64_t)1 << 31) || B * K >= ((int64_t)1 << 31)) return KGE_EINVAL;
    if (!neg_h || !neg_t) return KGE_EINVAL;
    return 0;
}

// the register bucket of the rows, or the code that refuses the width: rows beyond 1024 floats as kge_score_triples
// (KGE_EINVAL); the NE = 16 bucket is not served (fact rows, accumulators and a negative in flight do not fit)
template <typename Launch>
int dispatch_groups(const FactParams &q, hipStream_t s, Launch launch)
{
    const ScoreParams &p = q.f;
    const bool vec4 = tables_vec4(p.t0, p.t1, p.t2, p.t3, p.d_ent, p.d_rel);
    const int per_lane = row_regs_per_lane(p.d_ent, vec4);
    if (per_lane > 16) return KGE_EINVAL;
    if (per_lane > 8) return KGE_EUNSUPPORTED;
    const dim3 grid((unsigned)p.B, (unsigned)q.chunks), block(WAVES_PER_BLOCK * 64);
    return dispatch_kind(p.kind, [&](auto k) -> int {
        constexpr int KIND = decltype(k)::value;
        if (per_lane <= 4) {
            if (vec4) launch(std::integral_constant<int, KIND>{}, std::true_type{}, std::integral_constant<int, 4>{}, grid, block, s);
            else launch(std::integral_constant<int, KIND>{}, std::false_type{}, std::integral_constant<int, 4>{}, grid, block, s);
        } else {
            if (vec4) launch(std::integral_constant<int, KIND>{}, std::true_type{}, std::integral_constant<int, 8>{}, grid, block, s);
            else launch(std::integral_constant<int, KIND>{}, std::false_type{}, std::integral_constant<int, 8>{}, grid, block, s);
        }
        KGE_CHECK_LAUNCH();
        return 0;
    });
}

} // namespace

extern "C" int kge_fact_group_forward_chunks(int64_t K)
{
    if (K < 1) return 0;
    const int64_t c = (K + KGE_FACT_GROUP_K_PER_CHUNK - 1) / KGE_FACT_GROUP_K_PER_CHUNK;
    return (int)(c < KGE_FACT_GROUP_MAX_CHUNKS ? c : KGE_FACT_GROUP_MAX_CHUNKS);
}

extern "C" int kge_fact_group_entity_tables(int kind) { return kind_served(kind) ? ent_tables(kind) : 0; }
extern "C" int kge_fact_group_relation_tables(int kind) { return kind_served(kind) ? rel_tables(kind) : 0; }

extern "C" int64_t kge_fact_group_rows_per_fact(int kind, int64_t K)
{
    if (!kind_served(kind) || K < 1) return 0;
    return (int64_t)ent_tables(kind) * (K + 2) + rel_tables(kind);
}

extern "C" int64_t kge_fact_group_rows(int kind, int64_t B, int64_t K)
{
    if (B <= 0 || K < 1 || K >= ((int64_t)1 << 31) || B >= ((int64_t)1 << 31) || B * K >= ((int64_t)1 << 31)) return 0;
    return B * kge_fact_group_rows_per_fact(kind, K);
}

extern "C" size_t kge_fact_group_rows_bytes(int kind, int64_t B, int64_t K, int64_t rows_ld)
{
    if (rows_ld <= 0) return 0;
    return (size_t)kge_fact_group_rows(kind, B, K) * (size_t)rows_ld * sizeof(float);
}

extern "C" int64_t kge_fact_group_ids(int64_t B, int64_t K)
{
    if (B <= 0 || K < 1 || K >= ((int64_t)1 << 31) || B >= ((int64_t)1 << 31) || B * K >= ((int64_t)1 << 31)) return 0;
    return B * (K + 2);
}

extern "C" int kge_score_fact_groups(int kind, const float *t0, const float *t1, const float *t2, const float *t3, int d_ent,
                                     int d_rel, const int64_t *h, const int64_t *t, const int64_t *r, int64_t B,
                                     const int64_t *neg_h, const int64_t *neg_t, int64_t K, float *pos, float *neg,
                                     int64_t ld_neg, kge_stream_t stream)
{
    int rc = check_groups(kind, t0, t1, t2, t3, d_ent, d_rel, h, t, r, B, neg_h, neg_t, K);
    if (rc) return rc;
    if (B == 0) return 0;
    if (!pos || !neg || ld_neg < B) return KGE_EINVAL;
    FactParams q{{kind, t0, t1, t2, t3, d_ent, d_rel, h, t, r, B, pos}, neg_h, neg_t, K, kge_fact_group_forward_chunks(K), neg, ld_neg,
                 nullptr, nullptr, 0, nullptr, 0, nullptr};
    return dispatch_groups(q, kge_s(stream), [&](auto k, auto v4, auto ne, dim3 grid, dim3 block, hipStream_t s) {
        hipLaunchKernelGGL((fact_fwd_kernel<decltype(k)::value, decltype(v4)::value, decltype(ne)::value>), grid, block, 0, s, q);
    });
}

extern "C" int kge_score_fact_groups_bwd(int kind, const float *t0, const float *t1, const float *t2, const float *t3,
                                         int d_ent, int d_rel, const int64_t *h, const int64_t *t, const int64_t *r,
                                         int64_t B, const int64_t *neg_h, const int64_t *neg_t, int64_t K,
                                         const float *go_pos, const float *go_neg, int64_t ld_go, float *rows,
                                         int64_t rows_ld, int64_t *ids, kge_stream_t stream)
{
    int rc = check_groups(kind, t0, t1, t2, t3, d_ent, d_rel, h, t, r, B, neg_h, neg_t, K);
    if (rc) return rc;
    if (B == 0) return 0;
    if (!go_pos || !go_neg || ld_go < B || !rows || rows_ld < d_ent || !ids) return KGE_EINVAL;
    FactParams q{{kind, t0, t1, t2, t3, d_ent, d_rel, h, t, r, B, nullptr}, neg_h, neg_t, K, 1, nullptr, 0,
                 go_pos, go_neg, ld_go, rows, rows_ld, ids};
    return dispatch_groups(q, kge_s(stream), [&](auto k, auto v4, auto ne, dim3 grid, dim3 block, hipStream_t s) {
        hipLaunchKernelGGL((fact_bwd_kernel<decltype(k)::value, decltype(v4)::value, decltype(ne)::value>), grid, block, 0, s, q);
    });
}
