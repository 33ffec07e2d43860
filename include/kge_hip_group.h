/*
 * kge_hip_group.h -- the grouped training criteria of libkge_hip.so: the loss of B facts, each with its own K negatives,
 * where the K negatives of one fact are weighed against each other -- self-adversarial negative sampling (Sun et al.
 * 2019) and a sampled softmax of the fact against its negatives -- with closed-form gradients.  Written out in torch such
 * a criterion is a softmax, a logsigmoid, a product, two reductions and their backward over (K, B) scores: about a dozen
 * elementwise launches and the usual NaN where exp saturates.  torchkge_amd.utils.group_losses and
 * torchkge_amd.utils.training.Trainer(n_neg=K) go through this entry.
 *
 * kge_hip.h, its descriptors and its ABI version are untouched, which is why the entry lives in a header of its own
 * (as kge_hip_train.h does).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising or reading back, no
 * allocation (the workspace size comes from kge_group_loss_ws_bytes); returns 0, KGE_EINVAL or a positive hipError_t; on
 * a negative code nothing was launched and no output was touched.
 */
#ifndef KGE_HIP_GROUP_H
#define KGE_HIP_GROUP_H

#include <stddef.h>
#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KGE_GROUP_NSSA 0
#define KGE_GROUP_SOFTMAX 1

/* The geometry.  A block of the two sweeps takes a panel of KGE_GROUP_ROWS consecutive facts and one chunk of the K
 * negatives: lane l of every wavefront owns the facts 4 l .. 4 l + 3 of the panel (a load of row k is one contiguous run
 * of the panel), and the block's KGE_GROUP_SLICES wavefronts split the chunk's negatives into that many consecutive
 * k-slices.  K is cut into kge_group_loss_chunks(K) = min(ceil(K / KGE_GROUP_MIN_K_PER_CHUNK), KGE_GROUP_MAX_CHUNKS)
 * chunks, chunk c holding the negatives [c K / chunks, (c + 1) K / chunks); slice s of a chunk [k0, k1) holds
 * [k0 + s (k1 - k0) / KGE_GROUP_SLICES, k0 + (s + 1) (k1 - k0) / KGE_GROUP_SLICES) (integer divisions; a slice may be
 * empty, a chunk never is). */
#define KGE_GROUP_ROWS 256
#define KGE_GROUP_SLICES 4
#define KGE_GROUP_MIN_K_PER_CHUNK 32
#define KGE_GROUP_MAX_CHUNKS 16

/* Chunks K negatives are cut into; 0 for K < 1.  Host arithmetic only. */
int kge_group_loss_chunks(int64_t K);

/* Bytes of workspace kge_group_loss needs for B facts of K negatives: the fp64 partials of the row sum, (m, l, t) per
 * fact, chunk and slice (m in fp32, l and t in fp64: 20 bytes; the fp64 ones for whole panels of KGE_GROUP_ROWS facts),
 * two floats per fact.  Host arithmetic only: no GPU call, usable without a device.  0 for B <= 0, K < 1 or
 * B * K >= 2^31; otherwise a multiple of 16, monotone in B and in K, and at most a constant
 * (20 * KGE_GROUP_SLICES * KGE_GROUP_MAX_CHUNKS + 8 bytes) per fact of B rounded up to a panel, whatever K. */
size_t kge_group_loss_ws_bytes(int64_t B, int64_t K);

/* *loss = sum over the B facts of L_i, and its partial derivatives when dpos and dneg are given.
 *
 * pos: B scores.  neg: K rows of B scores with leading dimension ld_neg >= B -- neg[k * ld_neg + i] is the k-th negative
 * of fact i, the tile order of heads.repeat(n_neg).  row_weight: B weights or NULL (all 1).  dneg: K rows of leading
 * dimension ld_dneg >= B, laid out like neg; the columns from B on of neg are never read, those of dneg never written.
 *
 * Per fact i, p = pos[i], x_k = neg[k * ld_neg + i], without contraction, with softplus and sigma the closed forms of
 * kge_hip_train.h (from one e = exp(-|x|) <= 1).  Every term -- expf, softplus, sigma, the weights, the gradients -- is
 * fp32; the running sums l and t alone are carried in fp64 (their rounding does not grow with K) and rounded to fp32
 * once, t / l as a quotient, l for the gradient sweep:
 *
 *   KGE_GROUP_NSSA     u_k = temperature * x_k (clamped to the finite range), m = max_k u_k,
 *                      l = sum_k expf(u_k - m), t = sum_k expf(u_k - m) * softplus(margin + x_k);
 *                      L_i = softplus(-(margin + p)) + t / l;   dpos[i] = -sigma(-(margin + p));
 *                      dneg[k, i] = (expf(u_k - m) / l) * sigma(margin + x_k).
 *                      The weights w_k = expf(u_k - m) / l are constants of the gradient, as in the paper; temperature 0
 *                      gives w_k = 1 / K through the same code (the uniform average).
 *   KGE_GROUP_SOFTMAX  m = max_k x_k, l = sum_k expf(x_k - m); with M = max(m, p), n = l * expf(m - M) and
 *                      l' = n + expf(p - M), so that lse = log(expf(p) + sum_k expf(x_k)) = M + log(l'):
 *                      L_i = lse - p = (M - p) + log(l')  (the logarithm and this sum in fp64, rounded once);
 *                      dpos[i] = expf(p - lse) - 1 = -n / l';   dneg[k, i] = expf(x_k - lse) = expf(x_k - M) / l'.
 *                      lse itself is never rounded to fp32: at scores of 1e4 that rounding (1e-3) would sit in every
 *                      gradient, and -n / l' has no cancellation where the fact dominates its negatives.
 *                      margin and temperature are ignored.
 *
 * row_weight[i] multiplies L_i, dpos[i] and every dneg[k, i] (the last operation of each).  row_loss[i] = L_i (weighted)
 * when row_loss is given.  All outputs are finite for finite inputs: scores of +-1e4, a spread of temperature * x beyond
 * 200 (weights that underflow are exactly 0, l >= 1 always).
 *
 * The order of the additions is a function of (B, K) alone -- no float atomic, nothing depends on the device's CU count
 * or the scheduling -- and what is added into a fact's m, l, t depends on K alone: the row_loss, dpos and dneg bits of a
 * fact do not depend on which other facts are in the batch.
 *   - the stats sweep: per (fact, chunk, slice) a running (m, l, t) over the slice's negatives in ascending k.  The first
 *     negative sets (u, 1, s); a later one with u <= m adds e = expf(u - m) to l and e * s to t; one with u > m rescales,
 *     (m, l, t) <- (u, l * f + 1, t * f + s) with f = expf(m - u)  (s = softplus(margin + x_k); SOFTMAX keeps no t;
 *     e, f and s widened, the products and sums in fp64);
 *   - the finish step merges a fact's partials (m_q, l_q, t_q), q = (chunk, slice) ascending, the empty slices
 *     skipped: m = max_q m_q, then l = sum_q l_q * expf(m_q - m) and t likewise, each added in ascending q onto 0 in
 *     fp64 (the online-softmax merge with every partial rescaled once, to the final maximum); then L_i, dpos[i] and
 *     the fact's final (m, l), for SOFTMAX (M, l');
 *   - the B row terms are added on the fp64 tree of kge_pair_loss (kge_hip_train.h, "The sum", with n = B): the finish
 *     step IS that tree's first stage, so *loss comes out of it for B <= KGE_PAIR_LOSS_CHUNK and out of the tree's second
 *     launch beyond;
 *   - the gradient sweep reads neg again with the final (m, l) of each fact and writes dneg.
 * Two reads and one write of B * K floats; three launches (four for B > KGE_PAIR_LOSS_CHUNK), two without gradients.
 *
 * *acc_io += *loss when acc_io is not NULL, with the semantics of kge_pair_loss.  dpos and dneg: both given or both NULL
 * (the value only: no gradient sweep, neither is written).  B = 0 writes *loss = 0, leaves *acc_io alone and launches
 * nothing else.
 *
 * Every vector needs 4-byte alignment only.  A matrix whose base lies on 16 bytes with a leading dimension that is a
 * multiple of 4, and a vector whose base lies on 16 bytes, is accessed in 16-byte quads, anything else in scalars, each
 * operand by itself; the assignment of facts to lanes and the arithmetic are the same on both paths, so are the bits.
 *
 * ws: kge_group_loss_ws_bytes(B, K) bytes, 16-byte aligned; its contents are scratch.  KGE_EINVAL: a kind outside the
 * two, B < 0, K < 1 with B > 0, B * K >= 2^31, for KGE_GROUP_NSSA a temperature that is negative or not finite, loss
 * NULL, for B > 0 pos or neg NULL, ld_neg < B, one of dpos / dneg NULL and the other not, ld_dneg < B with gradients, a
 * NULL or misaligned workspace or ws_bytes below the bound. */
int kge_group_loss(int kind, float margin, float temperature, const float *pos, const float *neg, int64_t ld_neg,
                   const float *row_weight, int64_t B, int64_t K, float *loss, float *acc_io, float *row_loss,
                   float *dpos, float *dneg, int64_t ld_dneg, void *ws, size_t ws_bytes, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_GROUP_H */
