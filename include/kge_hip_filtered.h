/*
 * kge_hip_filtered.h -- filtered negative sampling of libkge_hip.so: a replacement entity drawn EXACTLY over the
 * entities that are neither a known answer of the fact's key nor the replaced entity itself, as a pure function of the
 * caller's random draws, and the diagnostic that says which triples of a batch are known facts.
 * torchkge_amd.sampling.FilteredNegativeSampler goes through both.
 *
 * The known answers are segments of the ascending int32 ``targets`` of a sorted-key CSR (torchkge_amd.filter_index.
 * FilterIndex: keys, offsets, targets); kge_filter_lookup of kge_hip.h finds a batch's segments.
 *
 * Integer work only: no float operation, no atomic; the output is a pure function of the inputs, bit for bit the same
 * from launch to launch, and every store is an ordinary vector store.  kge_hip.h, its descriptors and its ABI version
 * are untouched, which is why the entries live in a header of their own (as kge_hip_relation.h does).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising or reading back, no
 * allocation; returns 0, KGE_EINVAL or a positive hipError_t; on a negative code nothing was launched and no output was
 * touched; a problem of zero elements is a successful no-op.  Every array needs the natural alignment of its element
 * type only.
 */
#ifndef KGE_HIP_FILTERED_H
#define KGE_HIP_FILTERED_H

#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The filtered corruption of B facts, n_neg negatives each, in the tile order of kge_corrupt_batch: negative k of fact i
 * is position p = k * B + i of mask, draws, neg_h, neg_t and exhausted.
 *
 * Fact i brings two lists: tail_targets[tail_lo[i] .. tail_hi[i]), the known tails of (h[i], r_i), and
 * head_targets[head_lo[i] .. head_hi[i]), the known heads of (t[i], r_i); each ascending, distinct, its values in
 * [0, n_ent); hi <= lo is the empty list (a key absent from the index).  h[i], t[i] are in [0, n_ent).  Position p:
 *
 *   1. x = the entity being replaced: h[i] if mask[p] != 0, else t[i];  L = the list of that side (mask[p] != 0: the
 *      heads), m = |L|.
 *   2. in = (x is in L), by binary search;  c = n_ent - m - (in ? 0 : 1): the entities that are neither known answers
 *      nor x itself -- a negative never equals its fact, also for a fact that is not in the index.
 *   3. c <= 0: neg_h[p] = h[i], neg_t[p] = t[i], exhausted[p] = 1.  Otherwise exhausted[p] = 0 and
 *   4. v = (uint64) draws[p] mod c -- every bit pattern of a draw is memory-safe;
 *   5. if !in:  rho = x - #{l in L : l < x} (the rank of x in the complement of L),  v += (v >= rho);
 *   6. j = #{j : L[j] - j <= v}, by one binary search (L[j] - j is non-decreasing);  e = v + j: the v-th entity of the
 *      complement of L in ascending order;
 *   7. e goes to the replaced place, the other place keeps the fact's entity.
 *
 * With draws[p] uniform over [0, 2^62) the replacement is uniform over the c free entities up to a modulo bias below
 * c / 2^62.
 *
 * Geometry: ONE launch, one thread per position, i = p mod B -- neighbouring lanes read neighbouring facts, masks and
 * draws and write neighbouring outputs; a position costs two binary searches of at most ceil(log2(m + 1)) steps each
 * (the membership search also gives #{l in L : l < x}).
 *
 * exhausted may be NULL (a caller that knows no list leaves fewer than two entities free).  Outputs may not alias
 * inputs.  The list of the side a position does not replace is not read.
 *
 * KGE_EINVAL: B < 0, n_ent < 1 or n_ent >= 2^31, n_neg < 1 with B > 0, B * n_neg >= 2^31, for B > 0 a NULL h, t, mask,
 * draws, one of the four bounds, one of the two target arrays, neg_h or neg_t.  B = 0 launches nothing. */
int kge_filtered_corrupt(const int64_t *h, const int64_t *t, int64_t B, int64_t n_neg, const uint8_t *mask,
                         const int64_t *draws, const int64_t *tail_lo, const int64_t *tail_hi,
                         const int32_t *tail_targets, const int64_t *head_lo, const int64_t *head_hi,
                         const int32_t *head_targets, int64_t n_ent, int64_t *neg_h, int64_t *neg_t,
                         uint8_t *exhausted, kge_stream_t stream);

/* out[p] = 1 iff value[p] is in the list of the key (key1[p], key2[p]) of one index, else 0 (an absent key: 0), for n
 * triples: a search of key1[p] * key_span + key2[p] among the n_keys ascending keys, then a search of the key's segment
 * targets[offsets[q] .. offsets[q + 1]).  One launch, one thread per triple.  The diagnostic that counts how many
 * negatives of ANY sampler are known facts: key1 = heads, key2 = relations, value = tails against the (h, r) -> tails
 * index.
 *
 * KGE_EINVAL: n < 0 or n >= 2^31, n_keys < 0, key_span < 1, for n > 0 a NULL key1, key2, value or out, for n > 0 and
 * n_keys > 0 a NULL keys, offsets or targets.  n = 0 launches nothing. */
int kge_triples_known(const int64_t *keys, int64_t n_keys, const int64_t *offsets, const int32_t *targets,
                      int64_t key_span, const int64_t *key1, const int64_t *key2, const int64_t *value, int64_t n,
                      uint8_t *out, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_FILTERED_H */
