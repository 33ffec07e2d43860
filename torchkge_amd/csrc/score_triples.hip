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
#include "score_rows.h"

namespace {

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
__device__ __forceinline__ void scatter_row(float *__restrict__ g, int d, int lane, const float (&x)[NE])
{
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int k = elem_index<VEC4, NE>(e, lane);
        if (k < d && x[e] != 0.f) atomicAdd(g + k, x[e]);
    }
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

template <typename P, typename KernelSel>
int dispatch_ne(const P &p, int dmax, bool vec4, int64_t B, hipStream_t s, KernelSel sel)
{
    const int per_lane = row_regs_per_lane(dmax, vec4);
    if (per_lane <= 4) return sel(p, std::integral_constant<int, 4>{}, vec4, B, s);
    if (per_lane <= 8) return sel(p, std::integral_constant<int, 8>{}, vec4, B, s);
    if (per_lane <= 16) return sel(p, std::integral_constant<int, 16>{}, vec4, B, s);
    return KGE_EINVAL; // d > 1024 (vec4) / 1024 (scalar) not supported by the register-resident kernel
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
    if (kind == KGE_ROTATE) return kge_rotate_score_fwd(t0, t1, d_ent, d_rel, h, t, r, B, out, kge_s(stream));
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
    if (kind == KGE_ROTATE) return kge_rotate_score_bwd(t0, t1, d_ent, d_rel, h, t, r, B, go, rows, rows_ld, kge_s(stream));
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
