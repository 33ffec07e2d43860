/*
 * kge_hip_convkb.h -- the ConvKB entry points of libkge_hip.so (torchkge/models/deep.py:13-154).
 *
 * ConvKB scores a triple by a CNN: F filters of width 3 over the stacked rows (head, relation, tail), ReLU, one linear
 * layer to two logits, softmax; the score is the second probability.  With x0, x1, x2 the head / relation / tail rows
 * of length d, w[f][0..2] and cb[f] the conv filters, L (2, F*d) and lb (2) the linear layer (flattening index f*d+j):
 *
 *   v[f][j] = w[f][0] x0[j] + w[f][1] x1[j] + w[f][2] x2[j] + cb[f]
 *   o_c     = sum_{f,j} L[c][f*d+j] relu(v[f][j]) + lb[c]
 *   score   = softmax(o)[1] = 1 / (1 + exp(-(o_1 - o_0)))
 *
 * Only o_1 - o_0 matters: the engine works with D = L[1] - L[0] and db = lb[1] - lb[0] (kge_convkb_prepare).  Per pair
 * the ReLU sits between two sums, so there is no matrix-core form: kge_lp_desc, its kernels and the ABI version of
 * kge_hip.h are untouched and these entry points live in a header of their own (as kge_hip_analogy.h).
 *
 * THE fp32 CONTRACT.  s in {0, 1, 2} is the slot the candidates fill (2: tail completion, 0: head completion,
 * 1: relation candidates), s1 < s2 the other two slots with the query's rows y1, y2, e_c the candidate's row:
 *
 *   u     = fmaf(w[f][s2], y2[j], fmaf(w[f][s1], y1[j], cb[f]))        depends on (query, f, j) only
 *   v     = fmaf(w[f][s], e_c[j], u)
 *   acc   = fmaf(D[f*d+j], fmaxf(v, 0), acc)                            ONE accumulator per pair, from 0;
 *           order: j ascending outer, f ascending inner
 *   z     = acc + db
 *   score = 1.0f / (1.0f + expf(-z))                                    ocml expf, IEEE division, -ffp-contract=off
 *
 * with D[k] = L[1][k] - L[0][k] and db = lb[1] - lb[0] fp32 subtractions.  EVERY entry point that scores a pair runs
 * this sequence (one device function in csrc/convkb.hip), so the bits agree between them: a count compares
 * score(i, c) >= s_true[i] on the final fp32 score with s_true from the pair entry, the true candidate counts itself,
 * and the fused counts are what kge_get_rank gives on the engine's own score matrix.  Where fp32 saturates to 0 or 1
 * the ties are the ones an fp32 softmax has as well.  kge_convkb_score_triples uses s = 2: it is bit-equal to the
 * tail-side score at column t.
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising, no allocation;
 * returns 0, KGE_EINVAL (bad argument), KGE_EUNSUPPORTED (d or F above KGE_CONVKB_MAX_DIM, or more tiles than a grid
 * holds) or a positive hipError_t; nothing is launched and no output is touched on a negative code.  Every matrix has
 * its own leading dimension (>= d) and needs 4-byte alignment only.
 */
#ifndef KGE_HIP_CONVKB_H
#define KGE_HIP_CONVKB_H

#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KGE_CONVKB_MAX_DIM 512  /* of each of d and F */
/* kge_convkb_desc.slot of a both-sides batch: queries [0, B_tail) have s = 2, queries [B_tail, B) have s = 0 */
#define KGE_CONVKB_SLOT_BOTH 3

/* Floats of the workspace kge_convkb_prepare fills: [ wp: 4F | db, 3 pads | D: F*d | Dt: F*d ]. */
#define KGE_CONVKB_WS_FLOATS(d, F) (2 * (int64_t)(d) * (F) + 4 * (int64_t)(F) + 4)

/* One all-candidates problem.  The query side is TWO row matrices, each with an optional index vector (NULL: row i):
 *   QE: the query's ENTITY row  -- s = 2: the head (slot 0);  s = 0: the tail (slot 2);  s = 1: the head (slot 0)
 *   QR: the query's OTHER row   -- s = 2, s = 0: the relation (slot 1);              s = 1: the tail (slot 2)
 * so an index-driven both-sides batch is QE = entity table with [h | t], QR = relation table with [r | r], and the
 * already-gathered rows of inference_scoring_function pass NULL indices.  Candidate c (local, 0 <= c < N) is row c of
 * T and stands for the global id c_base + c. */
typedef struct kge_convkb_desc {
    int32_t slot;           /* 0, 1, 2 or KGE_CONVKB_SLOT_BOTH */
    int32_t d, F;
    int32_t reserved;       /* 0 */
    int64_t B, N, c_base;
    int64_t B_tail;         /* KGE_CONVKB_SLOT_BOTH only: where the tail-side queries end (0 <= B_tail <= B) */
    const float *QE;
    int64_t ld_qe;
    const int64_t *qe_idx;
    const float *QR;
    int64_t ld_qr;
    const int64_t *qr_idx;
    const float *T;
    int64_t ldt;
    /* prepared by kge_convkb_prepare (pointers into its workspace) */
    const float *D;         /* D[f*d + j] = L[1][f*d+j] - L[0][f*d+j] */
    const float *Dt;        /* Dt[j*F + f] = D[f*d + j]: the f-inner loop reads contiguous, wave-uniform data */
    const float *wp;        /* wp[4f .. 4f+3] = { w[f][0], w[f][1], w[f][2], cb[f] } */
    const float *db;        /* one float: lb[1] - lb[0] */
} kge_convkb_desc;

/* ws (KGE_CONVKB_WS_FLOATS(d, F) floats, 16-byte aligned) from the layer parameters: conv weight w (F, 3) contiguous,
 * conv bias cb (F), linear weight L (2, F*d) with leading dimension ldl >= F*d, linear bias lb (2). */
int kge_convkb_prepare(const float *w, const float *cb, const float *L, int64_t ldl, const float *lb, int d, int F,
                       float *ws, kge_stream_t stream);

/* out[i*ldo + c] = score(i, c), i < B, c < N; ldo >= N. */
int kge_convkb_scores(const kge_convkb_desc *desc, float *out, int64_t ldo, kge_stream_t stream);

/* out[p] = score(qi[p], ci[p] - c_base), or 0 where ci[p] lies outside [c_base, c_base + N).  qi == NULL: qi[p] = p.
 * ci holds GLOBAL candidate ids (the semantics of kge_lp_pair_scores). */
int kge_convkb_pair_scores(const kge_convkb_desc *desc, const int64_t *qi, const int64_t *ci, int64_t P, float *out,
                           kge_stream_t stream);

/* raw_count[i] += #{c < N : score(i, c) >= s_true[i]} (int32 atomics, one per query and workgroup; the caller zeroes
 * raw_count).  No score is written to memory (the semantics of kge_lp_count_ge). */
int kge_convkb_count_ge(const kge_convkb_desc *desc, const float *s_true, int32_t *raw_count, kge_stream_t stream);

/* The semantics of kge_lp_filter_sub: per query i with filter segment targets[seg_lo[i] : seg_hi[i]) (GLOBAL ids)
 *   sub[i]   = sum over c in the segment, c != true_idx[i], c in [c_base, c_base + N) of
 *              [score(i, c) >= s_true[i]] - [-inf >= s_true[i]]
 *   found[i] = 1 if true_idx[i] occurs in the segment and lies in [c_base, c_base + N). */
int kge_convkb_filter_sub(const kge_convkb_desc *desc, const float *s_true, const int64_t *true_idx,
                          const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *targets, int32_t *sub,
                          int32_t *found, kge_stream_t stream);

/* scoring_function (deep.py:63-77) of B triples from index vectors: out[i] = score with x0 = E[h[i]], x1 = R[r[i]],
 * x2 = E[t[i]], s = 2.  ws: the prepared workspace. */
int kge_convkb_score_triples(const float *E, int64_t lde, const float *R, int64_t ldr, int d, int F, const float *ws,
                             const int64_t *h, const int64_t *t, const int64_t *r, int64_t B, float *out,
                             kge_stream_t stream);

/* Its backward, d(sum_i go[i] * out[i]), with g_i = go_i * s_i * (1 - s_i) (s = out of the forward) and m = relu(v):
 *   g (B)             : g_i (scratch the second kernel reads; also an output)
 *   rows (3B, rows_ld): gradient ROWS of width d, dx_s[j] = g_i sum_f D[f*d+j] [v > 0] w[f][s]; row (s*B + i) with
 *                       s = 0: entity h[i], s = 1: entity t[i], s = 2: relation r[i] -- reduced by the caller with
 *                       kge_key_sort + kge_segment_sum_rows.  NULL: not wanted.
 *   dL (2, F*d) contiguous: dL[1][k] = sum_i g_i m_i[k], dL[0] = -dL[1];   dlb (2) = (-sum g_i, +sum g_i)
 *   dw (F, 3): dw[f][s] = sum_i sum_j g_i D[f*d+j] [v > 0] x_s[j];          dcb (F) = sum_i sum_j g_i D[f*d+j] [v > 0]
 *   The four parameter gradients are reductions over the batch by ONE kernel over (f, j) that loops over the triples in
 *   ascending order and recomputes v (never F*d floats per triple in memory); the sums over j are fixed-shape trees:
 *   two runs give equal bits.  dL, dlb, dw, dcb: all four or none (NULL). */
int kge_convkb_score_triples_bwd(const float *E, int64_t lde, const float *R, int64_t ldr, int d, int F, const float *ws,
                                 const int64_t *h, const int64_t *t, const int64_t *r, int64_t B, const float *s,
                                 const float *go, float *g, float *rows, int64_t rows_ld, float *dL, float *dlb,
                                 float *dw, float *dcb, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_CONVKB_H */
