/*
 * kge_hip_xent.h -- 1-vs-all training on libkge_hip.so: the softmax cross-entropy of every query row of a KGE_LP_DOT
 * problem over ALL N candidates, and its gradients, without ever writing the (B, N) score matrix, its softmax or its
 * gradient.  The scores are the descriptor's own: s(i, c) = chain(A0[i], T0[c], K0) then chain(A1[i], T1[c], K1) of
 * kge_hip.h, the bits kge_lp_scores / kge_lp_pair_scores give (the same 32x32x2 fp32 MFMA k-order), so a model trains
 * on exactly the scores the evaluator ranks.  torchkge_amd.utils.one_vs_all goes through these entries.
 *
 * kge_hip.h, its descriptors and its ABI version are untouched, which is why the entries live in a header of their own
 * (as kge_hip_train.h / kge_hip_rows.h do).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising or reading back, no
 * allocation (the workspace size comes from kge_lp_xent_ws_bytes); returns 0, a negative KGE_E* code or a positive
 * hipError_t; on a negative code nothing was launched and no output was touched.
 *
 * The problem: an ordinary kge_lp_desc with mode == KGE_LP_DOT, one or two segments, c_base == 0, any leading
 * dimensions, bases aligned to 4 bytes (rows that are 16-byte aligned with K and ld multiples of 4 are fetched in
 * 16-byte pieces; the bits do not depend on which).  KGE_EUNSUPPORTED: any other mode, c_base != 0, K0 + K1 >
 * KGE_XENT_MAX_K, B or N >= 2^31, B > 65535 * KGE_XENT_BM.
 *
 * Geometry (published because the tests pick their shapes from it).  Rows are cut into panels of KGE_XENT_BM queries,
 * candidates into tiles of KGE_XENT_BN; the tiles into kge_lp_xent_chunks(N) contiguous chunks,
 *   chunks(N) = min(KGE_XENT_MAX_CHUNKS, ceil(ceil(N / KGE_XENT_BN) / KGE_XENT_MIN_TILES_PER_CHUNK)),
 * chunk j holding the tiles [T * j / chunks, T * (j + 1) / chunks) of the T = ceil(N / KGE_XENT_BN): a function of N
 * alone, capped, so the workspace -- per (row, chunk) partials only -- is bounded over all N for fixed B, K0, K1.
 *
 * Order.  No float atomic anywhere, and the order of every addition is a function of (B, N, K0, K1) alone -- not of the
 * CU count, the scheduling or earlier launches: the same inputs give the same bits.  A row's lse / row_loss do not
 * depend on which other rows are in the batch.  Rows >= B and candidates >= N of a last partial tile never enter a sum.
 */
#ifndef KGE_HIP_XENT_H
#define KGE_HIP_XENT_H

#include <stddef.h>
#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KGE_XENT_BM 64                   /* queries per row panel */
#define KGE_XENT_BN 64                   /* candidates per tile */
#define KGE_XENT_MIN_TILES_PER_CHUNK 4   /* a second chunk starts to exist at N = 4 * KGE_XENT_BN + 1 */
#define KGE_XENT_MAX_CHUNKS 32           /* the cap of kge_lp_xent_chunks */
#define KGE_XENT_MAX_K 1024              /* K0 + K1 */
#define KGE_XENT_KSLICE 512              /* gradient columns (of the K0 + K1) one backward block accumulates in registers */

/* Host arithmetic only: no GPU call, usable without a device. */
int kge_lp_xent_chunks(int64_t N);      /* 0 for N <= 0 */
/* Bytes of workspace either entry needs: 16 * B * chunks (the (m, l, sum s) partials) + 4 * B (the target scores,
 * rounded up to 16 bytes) + 4 * chunks * B * (K0 + K1) (the partial dA panels).  0 for B <= 0, N <= 0, K0 <= 0,
 * K1 < 0 or K0 + K1 > KGE_XENT_MAX_K; otherwise monotone in B and constant in N from
 * N = KGE_XENT_BN * KGE_XENT_MIN_TILES_PER_CHUNK * (KGE_XENT_MAX_CHUNKS - 1) + 1 on. */
size_t kge_lp_xent_ws_bytes(int64_t B, int64_t N, int K0, int K1);

/* Forward.  With s(i, c) the descriptor's DOT score and eps = label_smoothing:
 *
 *   lse[i]      = m_i + logf(l_i),  m_i = max_c s(i, c),  l_i = sum_c expf(s(i, c) - m_i)     (online softmax)
 *   row_loss[i] = lse[i] - s(i, t_i)                                                 for eps == 0 (ONE fp32 subtraction)
 *               = (1 - eps) * (lse[i] - s(i, t_i)) + eps * (lse[i] - mean_i)          otherwise,
 *                 mean_i = fp32(sum_c s(i, c) / N), the sum in fp64   (torch's definition of label_smoothing)
 *
 * Stats sweep: one block per (row panel, chunk) walks its tiles in ascending order.  Inside a tile thread q = 0..3 of a
 * row owns the candidates 16 q .. 16 q + 15 of the tile and keeps (m, l, sum s) over them across the chunk: per tile
 * m' = max(m, tile max), l = l * expf(m - m') + sum_e expf(s_e - m') (e ascending), sum s += s_e in fp64 (e ascending).
 * The four of a row merge as q = 0, 1, 2, 3 (M = max m_q, L = sum_q l_q * expf(m_q - M)), which is the partial of
 * (row, chunk); the finish kernel merges the chunks the same way in ascending chunk order.  s(i, t_i) is taken from the
 * tile that holds the target.
 *
 * target: int64 in [0, N) -- a PRECONDITION: a target outside leaves row_loss[i] undefined (nothing is written out of
 * bounds; lse[i] is still right).  label_smoothing in [0, 1].  lse, row_loss: B floats each, 4-byte aligned.
 * ws: kge_lp_xent_ws_bytes(B, N, K0, K1) bytes, 16-byte aligned; contents are scratch.
 * B == 0: returns 0, nothing launched.  KGE_EINVAL: desc NULL or malformed (B < 0, N <= 0 with B > 0, K0 <= 0, NULL
 * operands), target / lse / row_loss NULL, label_smoothing outside [0, 1], a NULL or misaligned workspace or ws_bytes
 * below the bound. */
int kge_lp_xent_fwd(const kge_lp_desc *desc, const int64_t *target, float label_smoothing, float *lse, float *row_loss,
                    void *ws, size_t ws_bytes, kge_stream_t stream);

/* Backward.  Scores are recomputed from the operands (the same bits as forward), with lse as forward wrote it:
 *
 *   G(i, c) = g[i] * (expf(s(i, c) - lse[i]) - q(i, c)),  q(i, c) = (1 - eps) + eps / N for c == t_i, eps / N otherwise
 *             (fp32; the two values of q are rounded once, on the host: ONE subtraction per element, and N = 1 gives
 *             exactly 0 as it must)
 *   dA = G . T   (B, K), OVERWRITTEN: dA0 (B, K0) with leading dimension ldda0, dA1 (B, K1) with ldda1
 *   dT = G^T . A (N, K), OVERWRITTEN: dT0 (N, K0) with lddt0, dT1 (N, K1) with lddt1
 *
 * Either group may be NULL (dA0 == NULL: no query gradient; dT0 == NULL: no table gradient) and its work is then not
 * launched; with K1 > 0 a wanted group needs both of its pointers.  Both products run on the 32x32x2 fp32 MFMA, one
 * fmaf chain per output element:
 *   dT: one block per (candidate tile, column slice) walks the row panels in ascending order, rows ascending inside:
 *       one writer and one chain per element;
 *   dA: one block per (row panel, chunk, column slice) walks its candidate tiles in ascending order, candidates
 *       ascending inside, and writes its partial panel to the workspace; a finish kernel adds the chunks of an element
 *       in ascending chunk order.
 * A column slice is KGE_XENT_KSLICE of the K0 + K1 output columns (segment 1 follows segment 0).
 *
 * KGE_EINVAL: as forward, and target / lse / g NULL, one pointer of a wanted group NULL while K1 > 0 (or dA1 / dT1 given
 * with the group's first pointer NULL), a leading dimension of a wanted output below its K. */
int kge_lp_xent_bwd(const kge_lp_desc *desc, const int64_t *target, float label_smoothing, const float *lse,
                    const float *g, float *dA0, int64_t ldda0, float *dA1, int64_t ldda1, float *dT0, int64_t lddt0,
                    float *dT1, int64_t lddt1, void *ws, size_t ws_bytes, kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_XENT_H */
