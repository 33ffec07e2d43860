/*
 * kge_hip_triplet.h -- the triplet-classification entry points of libkge_hip.so: the integer half of
 * PositionalNegativeSampler.corrupt_batch (torchkge/sampling.py:428-504) and the two reductions of
 * TripletClassificationEvaluator (torchkge/evaluation.py:513-580).  Scoring is not here: the evaluator calls
 * Model.scoring_function (kge_score_triples of kge_hip.h and its per-model siblings).
 *
 * Three pieces of integer / compare work, no floating-point sum anywhere: every result is a pure function of the
 * inputs, bit for bit the same from launch to launch.  kge_hip.h, its descriptors and its ABI version are untouched,
 * which is why these entry points live in a header of their own (as kge_hip_analogy.h / kge_hip_convkb.h do).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising, no allocation
 * (workspace sizes come from the *_ws_elems functions); returns 0, KGE_EINVAL or a positive hipError_t; on a negative
 * code nothing was launched and no output was touched; a problem of zero elements is a successful no-op that touches no
 * output.  Every array needs the natural alignment of its element type only.
 */
#ifndef KGE_HIP_TRIPLET_H
#define KGE_HIP_TRIPLET_H

#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* int32 elements of the workspace of kge_positional_corrupt for a batch of B positions (0 for B <= 0). */
int64_t kge_positional_ws_elems(int64_t B);

/* Positional corruption of one batch of B facts, as a pure function of the caller's random draws.
 *
 * The two indices are dense per-relation CSRs: the entities seen as head (resp. tail) of relation r occupy
 * values_h[offsets_h[r] .. offsets_h[r + 1]) (resp. values_t / offsets_t), ascending; offsets_* hold n_rel + 1 entries.
 *
 * Position j with mask[j] != 0 is the p-th such position (p = the number of non-zero mask bytes before j); its head is
 * replaced:
 *     neg_tails[j] = tails[j]
 *     r = rels[j], n = offsets_h[r + 1] - offsets_h[r]
 *     n > 0 :  neg_heads[j] = values_h[offsets_h[r] + clamp((int64)floorf((float)n * u_h[p]), 0, n - 1)]
 *     n == 0:  neg_heads[j] = fb_h[p]              (fb_h NULL: heads[j], the position stays as it is)
 * A position with mask[j] == 0 is the (j - p)-th of its kind and has its tail replaced the same way from u_t[j - p],
 * fb_t[j - p] and the tail index; neg_heads[j] = heads[j].
 *
 * The arithmetic is the reference's (n.float() * rand).floor().long(): ONE fp32 multiply of the int -> float conversion
 * of n (round to nearest) by the draw, then floorf.  For every u in [0, 1) that torch.rand returns and n < 2**22 the
 * clamp never fires; it is there so that no draw value (1.0, a negative number, a NaN) can index outside the
 * relation's segment.  A relation id outside [0, n_rel) is treated as a relation with an empty segment.
 *
 * u_h / fb_h need (number of non-zero mask bytes) entries, u_t / fb_t (number of zero ones); a caller that does not
 * know the split passes B-long arrays.  fb_* may be NULL when no relation of the index is empty.  Either index may have
 * zero values in all (values_* then is not dereferenced and may be NULL).
 * Outputs may not alias inputs.  ws: kge_positional_ws_elems(B) int32. */
int kge_positional_corrupt(const int64_t *heads, const int64_t *tails, const int64_t *rels, const uint8_t *mask,
                           const float *u_h, const float *u_t, const int64_t *fb_h, const int64_t *fb_t,
                           const int64_t *offsets_h, const int32_t *values_h, const int64_t *offsets_t,
                           const int32_t *values_t, int64_t n_rel, int64_t B, int64_t *neg_heads, int64_t *neg_tails,
                           int32_t *ws, kge_stream_t stream);

/* int32 elements of the workspace of kge_relation_max (0 for n_rel <= 0). */
int64_t kge_relation_max_ws_elems(int64_t n_rel);

/* thr[r] = max of scores[j] over rels[j] == r, for r in [0, n_rel); a relation that does not occur in rels takes the
 * maximum of ALL n scores (evaluation.py:531-538).  A NaN score makes its relation's threshold NaN and the overall
 * maximum NaN (as torch.max does); -inf is an ordinary value; the maximum starts below -inf, not at 0.  +0.0 ranks
 * above -0.0.  A relation id outside [0, n_rel) contributes to the overall maximum only.
 *
 * Scores are compared through an order-preserving 32-bit integer code: per-workgroup maxima first (in LDS while n_rel
 * fits), then one integer atomic max per touched relation -- max is order-independent, so the result does not depend on
 * the schedule.  n == 0: a no-op, thr is not written.  ws: kge_relation_max_ws_elems(n_rel) int32. */
int kge_relation_max(const float *scores, const int64_t *rels, int64_t n, int64_t n_rel, float *thr, int32_t *ws,
                     kge_stream_t stream);

/* counts[0] = #{j : pos[j] > thr[rels[j]]},  counts[1] = #{j : neg[j] < thr[rels[j]]},  j in [0, n): the two decision
 * counts of accuracy() (evaluation.py:576-580) from one kernel over the three vectors, behind a 16-byte clear of
 * `counts`.  Strict fp32 comparisons on the stored bits: equality and NaN (score or threshold) count for neither, and
 * so does a relation id outside [0, n_rel).  n == 0: a no-op, counts is not written. */
int kge_threshold_count(const float *pos, const float *neg, const int64_t *rels, const float *thr, int64_t n,
                        int64_t n_rel, int64_t *counts, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_TRIPLET_H */
