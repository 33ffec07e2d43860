/*
 * kge_hip_factgroup.h -- the grouped scorer of libkge_hip.so: the scores of B facts and of the K negatives of each, and
 * their backward, for the ten kinds of kge_score_triples' register-resident kernels (TransE-L1 / L2, TransH, TransD,
 * DistMult, ComplEx, the four TorusE kinds).  kge_score_triples over the B (K + 1) concatenated triples gathers,
 * normalises and, in the backward, emits a gradient row for every row of every triple: 3 (K + 1) per fact for TransE.  The
 * K corruptions of a fact share its relation row(s) and either its head or its tail row(s); this entry gathers a fact's
 * rows once, loads per negative only the replaced entity's row(s), and emits one gradient row per fact row (summed over
 * the positive and every negative that shares it) plus one per replaced row: K + 3 for TransE.
 * torchkge_amd.models.interfaces.Model.forward_grouped and a torchkge_amd.utils.training.Trainer whose
 * grouped_forward attribute is set go through it.
 *
 * kge_hip.h, its descriptors and its ABI version are untouched, which is why the entries live in a header of their own
 * (as kge_hip_group.h does).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising or reading back, no
 * allocation; returns 0, KGE_EINVAL, KGE_EUNSUPPORTED or a positive hipError_t; on a negative code nothing was launched
 * and no output was touched.
 */
#ifndef KGE_HIP_FACTGROUP_H
#define KGE_HIP_FACTGROUP_H

#include <stddef.h>
#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The input, where it lies.  kind, t0 .. t3, d_ent, d_rel: as kge_score_triples takes them (the tables of the kind,
 * contiguous rows).  h, t, r: the B facts.  neg_h, neg_t: K * B ids in the tile order of kge_corrupt_batch with n_neg = K:
 * negative k of fact i is at k * B + i.
 *
 * THE CONTRACT: a negative differs from its fact in at most one of head and tail.  Negative (k, i) is HEAD-CORRUPTED iff
 * neg_h[k * B + i] != h[i], otherwise TAIL-CORRUPTED; its replaced entity is neg_h[k * B + i] in the first case and
 * neg_t[k * B + i] in the second (which may equal t[i]: the row is simply loaded again), and its triple is the fact's with
 * that entity in the replaced place.  Input that breaks the contract (both differ) is memory-safe and is taken as
 * head-corrupted: the negative is scored as (neg_h, r[i], t[i]) and neg_t is not read.
 *
 * The geometry.  Backward: one workgroup of KGE_FACT_GROUP_WAVES wavefronts per fact; wavefront w takes the negatives
 * [w K / KGE_FACT_GROUP_WAVES, (w + 1) K / KGE_FACT_GROUP_WAVES) (integer divisions; a slice may be empty).  Forward, which
 * has nothing to combine: the K negatives are first cut into kge_fact_group_forward_chunks(K) =
 * min(ceil(K / KGE_FACT_GROUP_K_PER_CHUNK), KGE_FACT_GROUP_MAX_CHUNKS) chunks, chunk c = [c K / chunks, (c + 1) K / chunks),
 * one workgroup per (fact, chunk), and the wavefronts cut the chunk [k0, k1) likewise, wavefront w taking
 * [k0 + w (k1 - k0) / KGE_FACT_GROUP_WAVES, k0 + (w + 1) (k1 - k0) / KGE_FACT_GROUP_WAVES).  Every
 * wavefront gathers the fact's rows, normalises them once and keeps them in registers; per negative it loads the replaced
 * entity's row(s) only.  The per-fact scalars that do not depend on the replaced row (TransH: h.w / t.w, TransD: h.hp /
 * t.tp) are kept across k.
 *
 * Widths.  Rows of up to 512 floats (the 4- and 8-register buckets of kge_score_triples, on the 16-byte and the scalar load
 * path, TransD with d_rel < d_ent included) are served.  513 .. 1024: KGE_EUNSUPPORTED -- the fact's rows, their gradient
 * accumulators and a negative in flight do not fit the register file -- and the caller scores the concatenated triples
 * with kge_score_triples.  Beyond 1024: KGE_EINVAL, as there. */
#define KGE_FACT_GROUP_WAVES 4
#define KGE_FACT_GROUP_K_PER_CHUNK 128
#define KGE_FACT_GROUP_MAX_CHUNKS 1024

/* Chunks the forward cuts K negatives into; 0 for K < 1.  Host arithmetic only. */
int kge_fact_group_forward_chunks(int64_t K);

/* Entity tables (1; ComplEx and TransD: 2) and relation tables (TransE, DistMult, TorusE: 1; TransH, ComplEx, TransD: 2)
 * of a kind; 0 for a kind outside the ten.  Host arithmetic only. */
int kge_fact_group_entity_tables(int kind);
int kge_fact_group_relation_tables(int kind);

/* Gradient rows a fact of K negatives emits: entity tables * (K + 2) + relation tables -- K + 3 for TransE, DistMult and
 * TorusE, K + 4 for TransH, 2 K + 6 for ComplEx and TransD (kge_score_triples_bwd: 3 (K + 1), 4 (K + 1), 6 (K + 1)).  0 for
 * a kind outside the ten or K < 1.  Host arithmetic only. */
int64_t kge_fact_group_rows_per_fact(int kind, int64_t K);

/* Rows of the rows buffer of B facts (B * rows per fact), its bytes at a leading dimension of rows_ld floats, and the
 * entries of the id vector, B * (K + 2).  0 for B <= 0, K < 1, B * K >= 2^31, a kind outside the ten (or rows_ld <= 0);
 * monotone in B, K and rows_ld.  Host arithmetic only: no GPU call, usable without a device. */
int64_t kge_fact_group_rows(int kind, int64_t B, int64_t K);
size_t kge_fact_group_rows_bytes(int kind, int64_t B, int64_t K, int64_t rows_ld);
int64_t kge_fact_group_ids(int64_t B, int64_t K);

/* pos[i] = the score of fact i; neg[k * ld_neg + i] = the score of its k-th negative (K rows of leading dimension
 * ld_neg >= B: the layout kge_group_loss reads; the columns from B on are never written).
 *
 * EVERY SCORE HAS THE BITS kge_score_triples RETURNS FOR THE SAME TRIPLE: the same normalisation of every row (the
 * reciprocal form of the forward), the same element expressions and the same wavefront sum, inlined from one header into
 * both translation units, which are compiled with the same flags.
 *
 * KGE_EINVAL: what kge_score_triples refuses (a kind outside the ten, a NULL table the kind needs, d_ent != d_rel except
 * TransD with d_rel <= d_ent, non-positive widths, B < 0, for B > 0 a NULL h, t or r), K < 1 with B > 0, B * K >= 2^31,
 * for B > 0 a NULL neg_h, neg_t, pos or neg, ld_neg < B, rows wider than 1024.  B = 0 launches nothing. */
int kge_score_fact_groups(int kind, const float *t0, const float *t1, const float *t2, const float *t3, int d_ent,
                          int d_rel, const int64_t *h, const int64_t *t, const int64_t *r, int64_t B,
                          const int64_t *neg_h, const int64_t *neg_t, int64_t K, float *pos, float *neg, int64_t ld_neg,
                          kge_stream_t stream);

/* The backward: the gradient rows of sum_i go_pos[i] pos[i] + sum_k,i go_neg[k * ld_go + i] neg[k, i] (ld_go >= B).  Row
 * mode only: no float atomic, no table-sized output.
 *
 * The rows buffer.  Every row is rows_ld >= d_ent floats apart; a row of an entity table has d_ent floats, one of a
 * relation table d_rel, the rest of the row is never written.  With E = kge_fact_group_entity_tables(kind) and the
 * kind's tables in the order of kge_score_triples_bwd's gradient streams (kge_hip.h) -- entity tables: t0 (ComplEx:
 * t0, t1; TransD: t0, t2); relation tables: t1 (TransH: t1, t2; ComplEx: t2, t3; TransD: t1, t3) --
 *
 *   entity table s (0 <= s < E) owns the (K + 2) B rows from row s (K + 2) B on:
 *       row i              the gradient of the fact's row at h[i]: the positive and every TAIL-corrupted negative of i
 *       row B + i          ... at t[i]: the positive and every HEAD-corrupted negative of i
 *       row 2 B + k B + i  the gradient of the replaced entity's row of negative (k, i)
 *   relation table q owns the B rows from row E (K + 2) B + q B on: row i, summed over the positive and all K negatives.
 *
 * ids (B (K + 2) int64, written by the kernel): [h | t | the replaced entity of negative (k, i) at 2 B + k B + i] -- the
 * target rows of an entity table's block, whichever table; the relation rows' targets are r.  A table's rows are
 * adjacent, so a caller hands each block on as one view.
 *
 * The order of the additions is a function of (K, d) alone: wavefront w adds the gradients with respect to the NORMALISED
 * fact rows of its negatives in ascending k onto 0 (wavefront 0: onto the positive's), the KGE_FACT_GROUP_WAVES partials
 * are added in ascending w, and the derivative of the normalisation (linear in the incoming gradient) is applied once
 * to the sum.  A fact's rows do not depend on which other facts are in the batch, nor on B.
 *
 * KGE_EINVAL: as the forward, and a NULL go_pos, go_neg, rows or ids, ld_go < B, rows_ld < d_ent. */
int kge_score_fact_groups_bwd(int kind, const float *t0, const float *t1, const float *t2, const float *t3, int d_ent,
                              int d_rel, const int64_t *h, const int64_t *t, const int64_t *r, int64_t B,
                              const int64_t *neg_h, const int64_t *neg_t, int64_t K, const float *go_pos,
                              const float *go_neg, int64_t ld_go, float *rows, int64_t rows_ld, int64_t *ids,
                              kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_FACTGROUP_H */
