/*
 * kge_hip_rotate.h -- RotatE (Sun et al. 2019, "RotatE: Knowledge Graph Embedding by Relational Rotation in Complex
 * Space") on libkge_hip.so: one mode of kge_lp_desc, one kind of kge_score_triples / kge_score_triples_bwd and one
 * entry point for the query rows.  The reference (torchkge v0.17.7) has no RotatE.
 *
 *   score(h, r, t) = - sum_j | h_j r_j - t_j |,   h_j, t_j complex,  r_j = cos(theta_j) + i sin(theta_j)
 *
 * Additive: the two numbers below continue the enums of kge_hip.h, which -- with its descriptors, its prototypes and ABI
 * version 33 -- is untouched; that is why they live in a header of their own (as kge_hip_triplet.h does).  Conventions of
 * kge_hip.h: device pointers, launches on the given stream without synchronising, no allocation; returns 0, KGE_EINVAL or a
 * positive hipError_t; on a negative code nothing was launched.
 *
 * LAYOUT.  An entity row is d complex numbers stored INTERLEAVED, (re_0, im_0, re_1, im_1, ...): one table E of width
 * 2d.  A complex coordinate is then an aligned pair of floats inside the aligned group of four k that the L1 / torus modes
 * accumulate by, the raw parameter table is the candidate table (one segment, K1 = 0, nothing repacked), and
 * torch.view_as_complex(weight.view(N, d, 2)) is its torch view.  P (n_rel, d) holds the phases in radians.
 */
#ifndef KGE_HIP_ROTATE_H
#define KGE_HIP_ROTATE_H

#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kge_lp_desc.mode, after KGE_LP_TORUS_EL2 = 8: complex modulus of interleaved rows, broadcast-subtract on the fp32 VALU.
 *   Preconditions: K0 even (an odd K0 is KGE_EINVAL), K1 = 0, no Wq (KGE_EINVAL otherwise).
 *   x_k = A0[i,k] - T0[c,k];  m_j = sqrtf(fmaf(x_2j+1, x_2j+1, x_2j * x_2j))  with the correctly rounded fp32 square root;
 *   one accumulator, acc += (m_2g + m_2g+1) per aligned group of four k (g = 0, 1, ...; an absent pair at k >= K0 counts
 *   as m = 0);  s = -acc.
 * m = 0 where both differences are 0 and never NaN for finite operands.  Not an MFMA mode (KGE_LP_IS_MFMA is false for
 * it); no prefilter, no rank-1 term.  kge_lp_scores, kge_lp_pair_scores, kge_lp_count_ge, kge_lp_filter_sub* and
 * kge_lp_scores' chunks under kge_topk_chunk give the same bits for a pair: the term has one definition
 * (torchkge_amd/csrc/kge_common.h: lp_cmod_pair).  kge_lp_scores_batched takes the mode too (K even; its own summation
 * order, as for every mode). */
#define KGE_LP_CMOD 9

/* model kind of kge_score_triples / kge_score_triples_bwd, after KGE_TRANSR = 12: tables {E (n_ent, 2d interleaved),
 * P (n_rel, d phases)}, d_ent = 2d, d_rel = d, 2d <= 1024 (the bound of every kind; KGE_EINVAL beyond it).
 * Forward, per triple and complex coordinate j:  (c, s) = sincosf(P[r][j]),
 *   q_re = fmaf(h_re, c, -(h_im * s)),  q_im = fmaf(h_re, s, h_im * c)        (q = h (c + i s))
 *   y = q - t,  score = -sum_j |y_j|  with the modulus and the accumulation order of KGE_LP_CMOD: a triple's score has
 *   the bits of the KGE_LP_CMOD score of the tail-side row of kge_rotate_query against row t of E.
 * Backward: rows != NULL only (KGE_EINVAL without: no per-element float atomics), streams 0 (g0, h) 1 (g0, t) 2 (g1, r) at
 * rows[(stream * B + i) * rows_ld ...], rows_ld >= 2d; stream 2 fills the first d floats of its rows.  Closed form with
 * g = go_i, u = y / |y| and u = 0 WHERE |y| = 0 (finite where the written-out sqrt(re^2 + im^2) differentiates to NaN):
 *   dt = +g u,   dh = -g u conj(r),   dtheta = -g Re(conj(u) i h r) */
#define KGE_ROTATE 13

/* Query rows of a KGE_LP_CMOD problem against E, interleaved as E's rows, in one launch:
 *   tail side  Q[i] = E[h_i] o r_i        q_re = fmaf(x_re, c, -(x_im * s)),  q_im = fmaf(x_re, s, x_im * c)
 *   head side  Q[i] = E[t_i] o conj(r_i)  q_re = fmaf(x_re, c, x_im * s),     q_im = fmaf(x_im, c, -(x_re * s))
 * with (c, s) = sincosf(P[r_i][j]) by the device function the triple kernels use -- |h o r - t| = |h - t o conj(r)|
 * because |r| = 1.  side KGE_SIDE_TAIL / _HEAD: B rows; KGE_SIDE_BOTH: 2B rows, [0, B) tail side, [B, 2B) head side.
 * ent_n >= 0: E holds only the entity rows [ent_lo, ent_lo + ent_n) (row-sharded, as kge_lp_prep_sharded): rows of
 * entities outside it are written as zeros, to be summed over the shards.  ent_n < 0: whole table.
 * lde >= 2d, ldp >= d, ldq >= 2d, d >= 1; rows need the alignment of a float only. */
int kge_rotate_query(int side, const float *E, int64_t lde, const float *P, int64_t ldp, int d, const int64_t *h,
                     const int64_t *t, const int64_t *r, int64_t B, int64_t ent_lo, int64_t ent_n, float *Q,
                     int64_t ldq, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_ROTATE_H */
