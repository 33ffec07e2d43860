/*
 * kge_hip_train.h -- the training criterion of libkge_hip.so: the loss of a batch of (positive, negative) score pairs and
 * its closed-form gradients in one pass.  It stands beside the written-out criteria of torchkge_amd/utils/losses.py,
 * which cost a handful of elementwise launches forward and backward and lose their gradient where sigmoid / exp
 * saturate in fp32; torchkge_amd.utils.fused_losses and torchkge_amd.utils.training.Trainer go through this entry.
 *
 * kge_hip.h, its descriptors and its ABI version are untouched, which is why the entry lives in a header of its own
 * (as kge_hip_det.h / kge_hip_rows.h do).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising or reading back, no
 * allocation (the workspace size comes from kge_pair_loss_ws_bytes); returns 0, KGE_EINVAL or a positive hipError_t; on
 * a negative code nothing was launched and no output was touched.
 */
#ifndef KGE_HIP_TRAIN_H
#define KGE_HIP_TRAIN_H

#include <stddef.h>
#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KGE_LOSS_MARGIN 0
#define KGE_LOSS_LOGISTIC 1
#define KGE_LOSS_BCE 2

/* Pairs one block of the first stage takes per turn: 256 threads of 4 consecutive pairs each. */
#define KGE_PAIR_LOSS_CHUNK 1024

/* Bytes of workspace kge_pair_loss needs for n pairs: one fp64 partial per block of the first stage.  Host arithmetic
 * only: no GPU call, usable without a device.  0 for n <= 0 or n >= 2^31; otherwise at least 8 and monotone in n. */
size_t kge_pair_loss_ws_bytes(int64_t n);

/* The grid cap of the first stage.  Host constant.  Beyond kge_pair_loss_max_blocks() * KGE_PAIR_LOSS_CHUNK pairs every
 * block takes several chunks (a grid-stride loop). */
int kge_pair_loss_max_blocks(void);

/* *loss = sum over the n pairs (pos[j], neg[j]) of the term of `kind`, and, when dpos and dneg are given, its partial
 * derivatives dpos[j] = d loss / d pos[j], dneg[j] = d loss / d neg[j].
 *
 * Per pair, in fp32 without contraction, with softplus(x) = max(x, 0) + log1p(exp(-|x|)) and
 * sigma(x) = 1 / (1 + e) for x >= 0, e / (1 + e) otherwise, e = exp(-|x|) <= 1 (no inf / inf, no 0 / 0):
 *
 *   KGE_LOSS_MARGIN    term max(0, a), a = margin - (pos[j] - neg[j]);  dpos = -1, dneg = +1 where a >= 0, else both 0
 *                      (clamp_min's subgradient: a hinge of exactly zero passes the gradient)
 *   KGE_LOSS_LOGISTIC  term softplus(-pos[j]) + softplus(neg[j]);       dpos = -sigma(-pos[j]), dneg = sigma(neg[j])
 *   KGE_LOSS_BCE       term min(softplus(-pos[j]), 100) + min(softplus(neg[j]), 100); the gradients of the logistic
 *                      kind where the softplus does not exceed 100, exactly 0 where it does (the cut-off of BCELoss's
 *                      logarithms at -100)
 *
 * The sum.  No float atomic, at most two launches, and the order of the additions is a function of n alone -- not of
 * the device's CU count, the scheduling or earlier launches: the same inputs give the same bits.  The tree:
 *   - G = min(ceil(n / KGE_PAIR_LOSS_CHUNK), kge_pair_loss_max_blocks()) blocks of 256 threads.  Thread t of block b
 *     owns the pairs (k * G + b) * KGE_PAIR_LOSS_CHUNK + 4 t + {0, 1, 2, 3} for k = 0, 1, ...; the four fp32 terms of a
 *     turn are widened to fp64 and added as (t0 + t1) + (t2 + t3) (pairs from n on count 0), the turns in ascending k
 *     onto the thread's fp64 accumulator;
 *   - the 64 accumulators of a wavefront by the xor butterfly (lane distances 32, 16, 8, 4, 2, 1); the four wavefronts
 *     of a block through LDS as (w0 + w1) + (w2 + w3): the block's partial, in fp64;
 *   - G = 1: that block rounds its partial to fp32 and writes *loss -- one launch.  G > 1: the partials go to the
 *     workspace and a second launch of one block adds them the same way (thread t takes the partials t, t + 256, ... in
 *     ascending order; butterfly; LDS) and rounds to fp32 once.
 * Every addition of the tree is in fp64; the terms and the gradients are fp32.
 *
 * *acc_io += *loss when acc_io is not NULL: one plain read-modify-write in fp32 by the one thread that writes *loss (a
 * running sum of a training epoch that never visits the host).  dpos and dneg: both given or both NULL (the value
 * only; nothing else is written).  n = 0 writes *loss = 0, leaves *acc_io alone and launches nothing else.
 *
 * pos, neg, dpos and dneg need 4-byte alignment only (the two halves of one score vector: neg = pos + n).  A vector
 * whose base lies on 16 bytes is accessed in 16-byte quads, any other in scalars, each of the four by itself; the
 * assignment of pairs to threads and the arithmetic are the same on both paths, so are the bits.
 *
 * ws: kge_pair_loss_ws_bytes(n) bytes, 8-byte aligned; its contents are scratch.  KGE_EINVAL: a kind outside the three,
 * n < 0 or n >= 2^31, loss NULL, for n > 0 pos or neg NULL, one of dpos / dneg NULL and the other not, a NULL or
 * misaligned workspace or ws_bytes below the bound. */
int kge_pair_loss(int kind, float margin, const float *pos, const float *neg, int64_t n, float *loss, float *acc_io,
                  float *dpos, float *dneg, void *ws, size_t ws_bytes, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_TRAIN_H */
