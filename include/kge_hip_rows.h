/*
 * kge_hip_rows.h -- row gradients of libkge_hip.so: coalescing the uncoalesced (id, gradient row) pairs a backward
 * emits in row-gradient mode (torchkge_amd.set_row_gradients(True)), and optimizer updates that touch only the rows
 * that have a gradient.  No (n_rows, d) gradient table is ever written or read.
 *
 * kge_hip.h, its descriptors and its ABI version are untouched, which is why the entries live in a header of their own
 * (as kge_hip_det.h / kge_hip_analogy.h / kge_hip_convkb.h do).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising or reading back, no
 * allocation (the workspace size comes from kge_rows_coalesce_ws_bytes); returns 0, KGE_EINVAL or a positive
 * hipError_t; on a negative code nothing was launched and no output was touched.
 */
#ifndef KGE_HIP_ROWS_H
#define KGE_HIP_ROWS_H

#include <stddef.h>
#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace kge_rows_coalesce needs for M rows of d columns (ids of up to 32 bits).  No GPU work and no
 * read-back.  0 for M <= 0, M >= 2^31 or d < 1; otherwise positive and monotone in M and in d (d > 1024 is reduced in
 * column chunks of 1024 and needs what d = 1024 needs). */
size_t kge_rows_coalesce_ws_bytes(int64_t M, int d);

/* The distinct ids of `ids` (M of them, each in [0, n_rows), n_rows <= 2^32), ascending, in uniq[0 .. U); their number
 * U in *count (a device int64); and out[j, 0:d] = the sum of the rows rows[i * ld + 0 .. d) over all i with
 * ids[i] == uniq[j], for j < U.
 *
 * The sum is kge_segment_sum_ordered's (kge_hip_det.h) with each id's dense rank as its key: that reduction compares
 * keys for equality and sign only, so its summation order is a function of M and the run boundaries alone, and row j of
 * `out` equals BIT FOR BIT row uniq[j] of what kge_segment_sum_ordered writes into a zeroed (n_rows, d) table for the
 * same ids under their stable ascending order.  No float atomic; the same inputs give the same bits.
 *
 * `uniq` and `out` have room for M entries / rows (out_ld >= d floats apart; the columns d .. out_ld - 1 are not
 * touched); the entries and rows from U on are unspecified.  ld >= d; the columns d .. ld - 1 of `rows` are not read.
 * ws: kge_rows_coalesce_ws_bytes(M, d) bytes, 16-byte aligned; its contents are scratch.  M = 0 writes *count = 0 and
 * nothing else.  Bad arguments, a NULL or misaligned workspace or ws_bytes below the bound: KGE_EINVAL. */
int kge_rows_coalesce(const float *rows, int64_t ld, int d, const int64_t *ids, int64_t M, int64_t n_rows,
                      int64_t *uniq, float *out, int64_t out_ld, int64_t *count, void *ws, size_t ws_bytes,
                      kge_stream_t stream);

/* The row updates: for j < *count (a device int64, 0 <= *count <= M; M is the host-known bound that sizes the grid), the
 * row uniq[j] of the parameter `p` (rows p_ld floats apart, d columns) -- and of the optimizer's state tables, which
 * share p's layout -- is updated in place from the gradient row g[j * g_ld + 0 .. d).  `uniq` must be free of
 * duplicates below *count: every row has one writer, there is no atomic.  Rows that are not named, and the columns from
 * d on, keep every bit.  p_ld >= d, g_ld >= d, d >= 1.  M = 0: a successful no-op.
 *
 * The rules are those of torch's sparse branches, in fp32 without contraction:
 *   kge_row_sgd       p -= lr * g
 *   kge_row_adagrad   sum += g * g;  p -= clr * (g / (sqrt(sum) + eps))         (clr: lr after its decay)
 *   kge_row_adam      SparseAdam's lazy update: m += (g - m) * om_beta1;  v += (g * g - v) * om_beta2;
 *                     p -= step * (m / (sqrt(v) + eps)),  step = lr * sqrt(bias2) / bias1
 *                     with om_beta = 1 - beta and bias = 1 - beta^t of the GLOBAL step t; the moments of rows without a
 *                     gradient do not decay. */
int kge_row_sgd(float *p, int64_t p_ld, int d, const int64_t *uniq, const int64_t *count, int64_t M, const float *g,
                int64_t g_ld, float lr, kge_stream_t stream);
int kge_row_adagrad(float *p, float *sum, int64_t p_ld, int d, const int64_t *uniq, const int64_t *count, int64_t M,
                    const float *g, int64_t g_ld, float clr, float eps, kge_stream_t stream);
int kge_row_adam(float *p, float *exp_avg, float *exp_avg_sq, int64_t p_ld, int d, const int64_t *uniq,
                 const int64_t *count, int64_t M, const float *g, int64_t g_ld, float lr, float om_beta1, float om_beta2,
                 float eps, float bias1, float bias2, kge_stream_t stream);

/* The most wavefronts a row update launches: beyond that many rows every wavefront walks several (a grid-stride loop).
 * Host constant. */
int kge_row_update_max_waves(void);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_ROWS_H */
