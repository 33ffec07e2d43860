/*
 * kge_hip_relation.h -- the relation-side entry point of libkge_hip.so: the integer half of
 * BernoulliRelationNegativeSampler.corrupt_batch (torchkge/sampling.py:526-553), the sampler that corrupts either the
 * relation of a fact or, Bernoulli-style, one of its entities.  RelationInference needs no entry point of its own: it
 * ranks the (b, n_rel) relation scores of the models with kge_topk_chunk of kge_hip.h.
 *
 * Integer work only: the result is a pure function of the inputs, bit for bit the same from launch to launch; every
 * store is an ordinary vector store and nothing takes an atomic.  kge_hip.h, its descriptors and its ABI version are
 * untouched, which is why this entry point lives in a header of its own (as kge_hip_triplet.h does).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising, no allocation
 * (the workspace size comes from kge_relation_corrupt_ws_elems); returns 0, KGE_EINVAL or a positive hipError_t; on a
 * negative code nothing was launched and no output was touched; a problem of zero elements is a successful no-op that
 * touches no output.  Every array needs the natural alignment of its element type only.
 */
#ifndef KGE_HIP_RELATION_H
#define KGE_HIP_RELATION_H

#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* int32 elements of the workspace of kge_relation_corrupt for n = B * n_neg positions (0 for n <= 0). */
int64_t kge_relation_corrupt_ws_elems(int64_t n);

/* Relation / entity corruption of n = B * n_neg positions, as a pure function of the caller's random draws.
 * Position j reads fact j % B (the batch repeated n_neg times).
 *
 *   p = the number of non-zero mask_ent bytes before j
 *   mask_ent[j] == 0:  the relation is corrupted
 *       neg_rels[j] = draws_r[j - p],  neg_heads[j] = heads[j % B],  neg_tails[j] = tails[j % B]
 *   mask_ent[j] != 0:  an entity is corrupted, neg_rels[j] = rels[j % B]; which one says mask_head[p] -- mask_head is
 *       COMPACT: one byte per entity position, consumed in position order
 *       q = the number of entity positions before j whose mask_head byte is non-zero
 *       mask_head[p] != 0:  neg_heads[j] = draws_h[q],      neg_tails[j] = tails[j % B]
 *       mask_head[p] == 0:  neg_tails[j] = draws_t[p - q],  neg_heads[j] = heads[j % B]
 *
 * The second rank q depends on the first (mask_head is indexed by p): two dependent prefix counts.  The first runs over
 * mask_ent, the second over the derived byte mask  mask_ent[j] && mask_head[p_j]  that the first leaves in the
 * workspace.
 *
 * mask_head needs (number of non-zero mask_ent bytes) entries, draws_r (number of zero ones), draws_h (number of head
 * positions), draws_t (number of tail positions); a caller that does not know the split passes n-long arrays.  Any of
 * the three draw arrays, and mask_head, may be empty or NULL when its branch cannot be taken; a position whose branch
 * meets a NULL array keeps the fact's own value (a NULL mask_head reads as all zero).
 * Outputs may not alias inputs.  ws: kge_relation_corrupt_ws_elems(B * n_neg) int32.
 * KGE_EINVAL: B < 0, n_neg < 1, or (for n > 0) a NULL heads / tails / rels / mask_ent / output / ws. */
int kge_relation_corrupt(const int64_t *heads, const int64_t *tails, const int64_t *rels, const uint8_t *mask_ent,
                         const uint8_t *mask_head, const int64_t *draws_r, const int64_t *draws_h,
                         const int64_t *draws_t, int64_t B, int64_t n_neg, int64_t *neg_heads, int64_t *neg_tails,
                         int64_t *neg_rels, int32_t *ws, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_RELATION_H */
