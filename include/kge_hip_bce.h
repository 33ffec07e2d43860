/*
 * kge_hip_bce.h -- K-vs-all training on libkge_hip.so: the binary cross-entropy with logits of every query row of a
 * KGE_LP_DOT problem over ALL N candidates against a multi-label target given as a CSR of true candidates, and its
 * gradients, without ever writing the (B, N) score matrix, a (B, N) label matrix or the (B, N) gradient.  The scores are
 * the descriptor's own: s(i, c) = chain(A0[i], T0[c], K0) then chain(A1[i], T1[c], K1) of kge_hip.h, the bits
 * kge_lp_scores / kge_lp_pair_scores give, so a model trains on exactly the scores the evaluator ranks.
 * torchkge_amd.utils.k_vs_all goes through these entries.
 *
 * kge_hip.h, its descriptors and its ABI version are untouched, which is why the entries live in a header of their own
 * (as kge_hip_xent.h does).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising or reading back, no
 * allocation (the workspace size comes from kge_lp_bce_ws_bytes); returns 0, a negative KGE_E* code or a positive
 * hipError_t; on a negative code nothing was launched and no output was touched.
 *
 * The problem: an ordinary kge_lp_desc with mode == KGE_LP_DOT, one or two segments, c_base == 0, any leading
 * dimensions, bases aligned to 4 bytes (rows that are 16-byte aligned with K and ld multiples of 4 are fetched in
 * 16-byte pieces; the bits do not depend on which).  KGE_EUNSUPPORTED: any other mode, c_base != 0, K0 + K1 >
 * KGE_BCE_MAX_K, B or N >= 2^31, B > 65535 * KGE_BCE_BM.
 *
 * Labels.  Row i's true set is labels[seg_lo[i] .. seg_hi[i]): int32 candidate ids.  These are the two vectors
 * FilterIndex.lookup returns (or slices of the index's offsets) and the index's targets: no label is copied or
 * densified.  PRECONDITION: every segment is strictly ascending with values in [0, N).  Segments may be empty
 * (seg_lo[i] >= seg_hi[i]), shared by several rows, lie anywhere in labels, and be longer than a tile.  A segment that
 * violates the precondition gives undefined values of that row's loss and gradients; the kernels still read labels only
 * inside [seg_lo[i], seg_hi[i]) and write nothing outside the outputs.  A tile costs a row O(labels of the row in the
 * tile) where a block walks the tiles in ascending order (one lower_bound at the block's first tile), and one binary
 * search of the segment, O(log len + labels in the tile), in the table gradient; there is no per-(row, tile) table.
 *
 * Criterion.  With eps = label_smoothing in [0, 1]:
 *   y(i, c) = y_pos = (1 - eps) + eps / N  for c in row i's set,  y_neg = eps / N  otherwise
 * -- both rounded once, on the host, in fp32 (as kge_hip_xent.h's q).  This is the smoothing convention of
 * kge_hip_xent.h carried over to multi-label targets: every label is mixed with the uniform distribution over the N
 * candidates, y = (1 - eps) * [c in set] + eps / N.  (It is not the y * (1 - eps) + eps / 2 some binary-label code uses.)
 *
 * Geometry (published because the tests pick their shapes from it): that of kge_hip_xent.h.  Rows are cut into panels of
 * KGE_BCE_BM queries, candidates into tiles of KGE_BCE_BN; the tiles into kge_lp_bce_chunks(N) contiguous chunks,
 *   chunks(N) = min(KGE_BCE_MAX_CHUNKS, ceil(ceil(N / KGE_BCE_BN) / KGE_BCE_MIN_TILES_PER_CHUNK)),
 * chunk j holding the tiles [T * j / chunks, T * (j + 1) / chunks) of the T = ceil(N / KGE_BCE_BN): a function of N
 * alone, capped, so the workspace -- per (row, chunk) partials and the partial dA panels only -- is bounded over all N
 * for fixed B, K0, K1.
 *
 * Order.  No float atomic anywhere, and the order of every addition is a function of (B, N, K0, K1) alone -- not of the
 * CU count, the scheduling, the label layout or earlier launches: the same inputs give the same bits.  A row's loss and
 * its dA row do not depend on which other rows are in the batch.  Rows >= B and candidates >= N of a last partial tile
 * never enter a sum.
 */
#ifndef KGE_HIP_BCE_H
#define KGE_HIP_BCE_H

#include <stddef.h>
#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KGE_BCE_BM 64                   /* queries per row panel */
#define KGE_BCE_BN 64                   /* candidates per tile */
#define KGE_BCE_MIN_TILES_PER_CHUNK 4   /* a second chunk starts to exist at N = 4 * KGE_BCE_BN + 1 */
#define KGE_BCE_MAX_CHUNKS 32           /* the cap of kge_lp_bce_chunks */
#define KGE_BCE_MAX_K 1024              /* K0 + K1 */
#define KGE_BCE_KSLICE 512              /* gradient columns (of the K0 + K1) one backward block accumulates in registers */

/* Host arithmetic only: no GPU call, usable without a device. */
int kge_lp_bce_chunks(int64_t N);       /* 0 for N <= 0; equals kge_lp_xent_chunks(N) */
/* Bytes of workspace either entry needs: 24 * B * chunks (three fp64 partial sums per (row, chunk)) +
 * 4 * chunks * B * (K0 + K1) (the partial dA panels).  0 for B <= 0, N <= 0, K0 <= 0, K1 < 0 or K0 + K1 >
 * KGE_BCE_MAX_K; otherwise monotone in B and constant in N from
 * N = KGE_BCE_BN * KGE_BCE_MIN_TILES_PER_CHUNK * (KGE_BCE_MAX_CHUNKS - 1) + 1 on. */
size_t kge_lp_bce_ws_bytes(int64_t B, int64_t N, int K0, int K1);

/* Forward.  With s = s(i, c) the descriptor's DOT score:
 *
 *   softplus(s) = fmaxf(s, 0) + log1pf(expf(-fabsf(s)))                    (both terms fp32, their sum in fp64)
 *   row_loss[i] = fp32( SP_i - (y_pos * SPOS_i + y_neg * (SALL_i - SPOS_i)) )  = sum_c [ softplus(s) - y(i, c) * s ]
 *                 SP = sum_c softplus(s), SPOS = sum over the row's labels of s, SALL = sum_c s: three fp64 sums of
 *                 fp32 terms, the combination in fp64, ONE rounding to fp32; for eps == 0 exactly fp32(SP - SPOS).
 *                 The two terms of softplus are added to SP one after the other (fmaxf(s, 0), then log1pf(.)), never
 *                 rounded together to fp32: beside a large positive s the log1pf term would lose its low bits, and for
 *                 a label the s then cancels against SPOS -- the loss of a well-fitted row IS the sum of those terms.
 *
 * Stats sweep: one block per (row panel, chunk) walks its tiles in ascending order.  Inside a tile thread q = 0..3 of a
 * row owns the candidates 16 q .. 16 q + 15 of the tile and keeps its three sums over them across the chunk (tiles
 * ascending, candidates ascending inside); the four of a row add as ((q0 + q1) + q2) + q3, which is the partial of
 * (row, chunk); the finish kernel adds the chunks in ascending order.
 *
 * seg_lo, seg_hi: B int64 each; labels: int32 (see above).  label_smoothing in [0, 1].  row_loss: B floats, 4-byte
 * aligned.  ws: kge_lp_bce_ws_bytes(B, N, K0, K1) bytes, 16-byte aligned; contents are scratch.
 * B == 0: returns 0, nothing launched.  KGE_EINVAL: desc NULL or malformed (B < 0, N <= 0 with B > 0, K0 <= 0, NULL
 * operands), seg_lo / seg_hi / labels / row_loss NULL, label_smoothing outside [0, 1], a NULL or misaligned workspace
 * or ws_bytes below the bound. */
int kge_lp_bce_fwd(const kge_lp_desc *desc, const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *labels,
                   float label_smoothing, float *row_loss, void *ws, size_t ws_bytes, kge_stream_t stream);

/* Backward.  Scores are recomputed from the operands (the same bits as forward); nothing forward wrote is needed:
 *
 *   e = expf(-fabsf(s)),  sigma(s) = 1 / (1 + e) for s >= 0,  e / (1 + e) otherwise          (fp32, overflow-free)
 *   G(i, c) = g[i] * (sigma(s(i, c)) - y(i, c))                                   (ONE subtraction, one product)
 *   dA = G . T   (B, K), OVERWRITTEN: dA0 (B, K0) with leading dimension ldda0, dA1 (B, K1) with ldda1
 *   dT = G^T . A (N, K), OVERWRITTEN: dT0 (N, K0) with lddt0, dT1 (N, K1) with lddt1
 *
 * Either group may be NULL (dA0 == NULL: no query gradient; dT0 == NULL: no table gradient) and its work is then not
 * launched; with K1 > 0 a wanted group needs both of its pointers.  Both products run on the 32x32x2 fp32 MFMA, one
 * fmaf chain per output element, in the orders of kge_hip_xent.h (the same code):
 *   dT: one block per (candidate tile, column slice) walks the row panels in ascending order, rows ascending inside:
 *       one writer and one chain per element;
 *   dA: one block per (row panel, chunk, column slice) walks its candidate tiles in ascending order, candidates
 *       ascending inside, and writes its partial panel to the workspace; a finish kernel adds the chunks of an element
 *       in ascending chunk order.
 * A column slice is KGE_BCE_KSLICE of the K0 + K1 output columns (segment 1 follows segment 0).
 *
 * KGE_EINVAL: as forward (row_loss aside), and g NULL, one pointer of a wanted group NULL while K1 > 0 (or dA1 / dT1
 * given with the group's first pointer NULL), a leading dimension of a wanted output below its K. */
int kge_lp_bce_bwd(const kge_lp_desc *desc, const int64_t *seg_lo, const int64_t *seg_hi, const int32_t *labels,
                   float label_smoothing, const float *g, float *dA0, int64_t ldda0, float *dA1, int64_t ldda1,
                   float *dT0, int64_t lddt0, float *dT1, int64_t lddt1, void *ws, size_t ws_bytes, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_BCE_H */
