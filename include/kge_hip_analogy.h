/*
 * kge_hip_analogy.h -- the ANALOGY entry points of libkge_hip.so (torchkge/models/bilinear.py:559-763).
 *
 * ANALOGY is DistMult on d_sc "scalar" coordinates plus ComplEx on d_c complex ones: three entity tables
 * (sc | re | im) and three relation tables.  Its all-candidates score is ONE dot product of width
 *   K = d_sc + 2 * d_c
 * between a query row that depends on (entity, relation, side) only and the candidate's three rows laid end to end:
 *
 *   tail side  q = [ sc_h*sc_r | re_h*re_r - im_h*im_r | re_h*im_r + im_h*re_r ]   . [ sc_c | re_c | im_c ]
 *   head side  q = [ sc_r*sc_t | re_r*re_t + im_r*im_t | re_r*im_t - im_r*re_t ]   . [ sc_c | re_c | im_c ]
 *   relations  q = [ sc_h*sc_t | re_h*re_t + im_h*im_t | re_h*im_t - im_h*re_t ]   . [ sc_rho | re_rho | im_rho ]
 *
 * So the candidate rows are packed once (the pack entry below), the query rows are built by the query entry, and from
 * there on the problem is a one-segment KGE_LP_DOT kge_lp_desc of kge_hip.h: the descriptor, its kernels and the ABI
 * version of kge_hip.h are untouched, which is why these four entry points live in a header of their own (as the
 * collectives do in kge_hip_coll.h).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising, no allocation;
 * returns 0, KGE_EINVAL, KGE_EUNSUPPORTED or a positive hipError_t.  0 <= d_sc <= 512, 0 <= d_c <= 512,
 * d_sc + d_c >= 1; outside that KGE_EUNSUPPORTED.  The pointers of a zero-width segment may be NULL.  Every matrix has
 * its own leading dimension (>= its width) and needs 4-byte alignment only.
 */
#ifndef KGE_HIP_ANALOGY_H
#define KGE_HIP_ANALOGY_H

#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the relation side of the query entry: candidates replace the relation, query = f(h, t) */
#define KGE_ANALOGY_SIDE_REL 5

/* P[j][0:K] = [ sc[i] | re[i] | im[i] ] with i = idx ? idx[j] : j, for j in [0, rows); ldp >= K.  Exactly K columns of
 * each row are written. */
int kge_analogy_pack_rows(const float *sc, int64_t ld_sc, const float *re, int64_t ld_re, const float *im, int64_t ld_im,
                          int d_sc, int d_c, const int64_t *idx, int64_t rows, float *P, int64_t ldp, kge_stream_t stream);

/* Query rows, the three formulas above, element by element the reference's fp32 expression with separate mul and
 * add / sub roundings: a row is bit-identical to the same expression in torch whatever the batch, the row's position
 * or the side grouping.
 * side KGE_SIDE_TAIL / KGE_SIDE_HEAD: B rows; KGE_SIDE_BOTH: 2B rows, [0, B) tail side, [B, 2B) head side;
 * KGE_ANALOGY_SIDE_REL: B rows of the relation formula (the relation tables are not read: pass NULL, 0).
 * h, t, r all NULL: the operands are already-gathered rows -- row i of the entity matrices and row i of the relation
 *   matrices (KGE_SIDE_BOTH: entity rows [0, B) the heads, [B, 2B) the tails, relation rows [0, B));
 *   KGE_ANALOGY_SIDE_REL: the entity matrices hold the heads' rows and the relation-table arguments the TAILS' rows.
 * ent_n >= 0: the entity tables hold only rows [ent_lo, ent_lo + ent_n) (row-sharded, as kge_bilinear_query): a row
 *   whose entity lies outside is written as zeros.  ent_n < 0: whole tables, ent_lo ignored (pass 0).  ent_n >= 0 is
 *   KGE_EINVAL on the relation side and with NULL indices. */
int kge_analogy_query(int side, const float *sc_e, int64_t ld_sce, const float *re_e, int64_t ld_ree, const float *im_e,
                      int64_t ld_ime, const float *sc_r, int64_t ld_scr, const float *re_r, int64_t ld_rer,
                      const float *im_r, int64_t ld_imr, int d_sc, int d_c, const int64_t *h, const int64_t *t,
                      const int64_t *r, int64_t B, int64_t ent_lo, int64_t ent_n, float *Q, int64_t ldq,
                      kge_stream_t stream);

/* scoring_function (bilinear.py:634-650), one fused gather + score launch, no normalisation:
 *   out[i] = sum_k sc_h sc_r sc_t + sum_j re_h (re_r re_t + im_r im_t) + im_h (re_r im_t - im_r re_t)
 * summed over the lanes of a wavefront (the order of the sum is not part of the contract). */
int kge_analogy_score_triples(const float *sc_e, int64_t ld_sce, const float *re_e, int64_t ld_ree, const float *im_e,
                              int64_t ld_ime, const float *sc_r, int64_t ld_scr, const float *re_r, int64_t ld_rer,
                              const float *im_r, int64_t ld_imr, int d_sc, int d_c, const int64_t *h, const int64_t *t,
                              const int64_t *r, int64_t B, float *out, kge_stream_t stream);

/* Its backward, d(sum_i go[i] * out[i]), as gradient ROWS in the packed [sc | re | im] layout (width K, rows_ld >= K),
 * three streams of B rows: row (s * B + i) of `rows` is the gradient of triple i wrt the packed row of
 *   s = 0: entity h[i],   s = 1: entity t[i],   s = 2: relation r[i].
 * kge_key_sort + kge_segment_sum_rows of kge_hip.h reduce streams 0 / 1 into a packed (n_ent, K) gradient and
 * stream 2 into a packed (n_rel, K) one; the per-table gradients are column slices of those. */
int kge_analogy_score_triples_bwd(const float *sc_e, int64_t ld_sce, const float *re_e, int64_t ld_ree, const float *im_e,
                                  int64_t ld_ime, const float *sc_r, int64_t ld_scr, const float *re_r, int64_t ld_rer,
                                  const float *im_r, int64_t ld_imr, int d_sc, int d_c, const int64_t *h,
                                  const int64_t *t, const int64_t *r, int64_t B, const float *go, float *rows,
                                  int64_t rows_ld, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_ANALOGY_H */
