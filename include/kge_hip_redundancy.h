/*
 * kge_hip_redundancy.h -- the data-redundancy analytics of libkge_hip.so: what torchkge/utils/data_redundancy.py
 * (Akrami et al., SIGMOD 2020) computes with one Python set per relation and R^2 set intersections, restated as ONE
 * co-occurrence count over sorted 64-bit keys.
 *
 * For two fact lists A and B (each a list of (h, t, r)) and n_rel relations:
 *
 *   same[ra][rb] = number of distinct pairs (h, t) with (h, t, ra) in A and (h, t, rb) in B
 *   rev [ra][rb] = number of distinct pairs (h, t) with (h, t, ra) in A and (t, h, rb) in B
 *
 * With B = A:  len(T[r1] & T[r2]) = same[r1][r2],  len(T[r1] & T_inv[r2]) = rev[r1][r2],  same[r][r] = |T[r]|.
 *
 * Integer work only: every result is an integer or a comparison of two integers (the thresholds of kge_overlap_select
 * are compared in IEEE double, as Python's `/` does).  The pair counts are int32 atomic adds whose results are unused:
 * integer addition commutes, so the matrices are the same bit for bit from launch to launch.
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising, no allocation (each
 * entry point has a workspace size query); returns 0, KGE_EINVAL, KGE_EUNSUPPORTED or a positive hipError_t; on a
 * negative code nothing was launched and no output was touched.  Ids outside [0, n_ent) / [0, n_rel) are the caller's
 * contract.  kge_hip.h, its descriptors and its ABI version are untouched.
 */
#ifndef KGE_HIP_REDUNDANCY_H
#define KGE_HIP_REDUNDANCY_H

#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of kge_relation_overlap for n_a facts in A and n_b facts in B (n_b = 0 when B = A);
 * 0 for n_a + n_b <= 0 or n_a + n_b >= 2^31. */
int64_t kge_relation_overlap_ws_bytes(int64_t n_a, int64_t n_b);

/* same / rev of the lists A = (hA, tA, rA)[nA] and B = (hB, tB, rB)[nB].  hB == NULL means B = A (tB, rB, nB are
 * then ignored).  same and rev are int32 (n_rel, ld), ld >= n_rel: the entry point zeroes columns [0, n_rel) of every
 * row itself and never touches columns >= n_rel.  rev may be NULL.  nA == 0 or nB == 0 gives zero matrices.
 *
 * Key of a fact: lo = min(h, t), hi = max(h, t), orient = (h > t), tag = (fact of B);
 *     key = (lo * n_ent + hi) << (2 + rbits) | orient << (1 + rbits) | tag << rbits | r
 * with rbits = bits(n_rel - 1).  One radix sort over exactly those bits; adjacent equal keys count once.  A group is a
 * run of equal (lo, hi): every ordered pair (x of A, y of B) of it adds 1 to same[r_x][r_y] when orient_x == orient_y,
 * to rev[r_x][r_y] when they differ, and to both when lo == hi.
 *
 * KGE_EUNSUPPORTED: bits(n_ent^2 - 1) + 2 + bits(n_rel - 1) > 64 (the rule of kge_filter_index_build).
 * KGE_EINVAL: nA < 0, nB < 0, nA + nB >= 2^31, n_ent <= 0, n_rel <= 0, n_rel >= 2^31, ld < n_rel, a NULL same or ws,
 * a NULL array of a non-empty list, ws_bytes < kge_relation_overlap_ws_bytes(nA, hB ? nB : 0). */
int kge_relation_overlap(const int64_t *hA, const int64_t *tA, const int64_t *rA, int64_t nA, const int64_t *hB,
                         const int64_t *tB, const int64_t *rB, int64_t nB, int64_t n_ent, int64_t n_rel,
                         int32_t *same, int32_t *rev, int64_t ld, void *ws, int64_t ws_bytes, kge_stream_t stream);

/* Bytes of the workspace of kge_relation_stats for n facts (0 for n <= 0 or n >= 2^31). */
int64_t kge_relation_stats_ws_bytes(int64_t n);

/* out: int64 (3, n_rel), contiguous: facts per relation WITH repeats, distinct heads per relation, distinct tails per
 * relation.  Two sorts of (r * n_ent + e) keys and run-head counts, one integer atomic per (wave, relation).
 * n == 0 gives zeros.  KGE_EUNSUPPORTED: n_rel * n_ent does not fit 64 bits.
 * KGE_EINVAL: n < 0, n >= 2^31, n_ent <= 0, n_rel <= 0, a NULL out, (n > 0) a NULL h / t / r / ws or a short ws. */
int kge_relation_stats(const int64_t *h, const int64_t *t, const int64_t *r, int64_t n, int64_t n_ent, int64_t n_rel,
                       int64_t *out, void *ws, int64_t ws_bytes, kge_stream_t stream);

/* Bytes of the workspace of kge_overlap_select for n_rel relations (0 for n_rel <= 0 or n_rel^2 >= 2^31). */
int64_t kge_overlap_select_ws_bytes(int64_t n_rel);

/* The pairs r1 < r2 of the strict upper triangle of counts (int32 (n_rel, ld)), in row-major order, with
 *     (double)c / (double)lengths[r1] > theta1  &&  (double)c / (double)lengths[r2] > theta2,   c = counts[r1][r2];
 * a zero length never qualifies.  lengths: int64 (n_rel).  The survivors are compacted in order into pairs
 * (int32 (cap, 2)); n_out (one int64) receives the TRUE count, also when it exceeds cap (pairs then holds the first
 * cap of them).  KGE_EUNSUPPORTED: n_rel^2 >= 2^31.
 * KGE_EINVAL: n_rel <= 0, ld < n_rel, cap < 0, a NULL counts / lengths / n_out / ws, a NULL pairs with cap > 0, a
 * short ws. */
int kge_overlap_select(const int32_t *counts, int64_t ld, const int64_t *lengths, int64_t n_rel, double theta1,
                       double theta2, int32_t *pairs, int64_t cap, int64_t *n_out, void *ws, int64_t ws_bytes,
                       kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_REDUNDANCY_H */
