/*
 * kge_hip_penalty.h -- the embedding regularizers of libkge_hip.so: the Lp penalty (p = 2: squared L2, p = 3: N3 of
 * Lacroix et al. 2018 and the L3 of the RotatE code base) of the table rows a batch names, and its gradient ROWS.  A
 * penalty written in torch on `table[ids]` hands the table a dense gradient, which the row optimizers refuse and the
 * ordered reduction of the deterministic mode does not cover; this entry gathers the penalised rows once, sums their
 * powers in a fixed order, and its backward emits one gradient row per occurrence -- what every other backward of the
 * library hands to kge_segment_sum_rows / kge_segment_sum_ordered or on to a row optimizer.
 * torchkge_amd.utils.regularizers goes through it.
 *
 * kge_hip.h, its descriptors and its ABI version are untouched, which is why the entries live in a header of their own
 * (as kge_hip_group.h does).
 *
 * Conventions of kge_hip.h: device pointers (the stream descriptors themselves are host memory, read during the call),
 * launches on the given stream without synchronising or reading back, no allocation (the workspace size comes from
 * kge_row_penalty_ws_bytes); returns 0, KGE_EINVAL or a positive hipError_t; on a negative code nothing was launched and
 * no output was touched.
 */
#ifndef KGE_HIP_PENALTY_H
#define KGE_HIP_PENALTY_H

#include <stddef.h>
#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How a stream's rows hold their coordinates.
 *   KGE_PENALTY_REAL         one table t0 of d floats per row, penalised element by element.
 *   KGE_PENALTY_SPLIT        t0 holds the real parts, t1 the imaginary parts of d complex coordinates (two tables of
 *                            equal shape and leading dimension); the penalty is on the modulus of a coordinate.
 *   KGE_PENALTY_INTERLEAVED  one table t0 whose row holds d / 2 pairs (re, im); d is even. */
#define KGE_PENALTY_REAL 0
#define KGE_PENALTY_SPLIT 1
#define KGE_PENALTY_INTERLEAVED 2

#define KGE_PENALTY_MAX_STREAMS 8
/* The geometry of both kernels: one wavefront per (stream, row), KGE_PENALTY_WAVES wavefronts per block, at most
 * KGE_PENALTY_MAX_BLOCKS blocks; beyond KGE_PENALTY_MAX_BLOCKS * KGE_PENALTY_WAVES rows the wavefronts stride. */
#define KGE_PENALTY_WAVES 4
#define KGE_PENALTY_MAX_BLOCKS 2048

/* One stream: the rows ids[0 .. n) of one table (SPLIT: of a pair of tables), rows ld >= d floats apart, each penalised
 * once per occurrence.  factor = w / n, the stream's weight over its length, rounded to fp32 by the caller. */
typedef struct kge_penalty_stream {
    const float *t0, *t1;       /* t1: KGE_PENALTY_SPLIT only */
    int64_t ld;
    int d;
    int layout;
    const int64_t *ids;
    int64_t n;
    float factor;
} kge_penalty_stream;

/* Host arithmetic only: no GPU call, usable without a device.
 *   kge_row_penalty_terms        M = the sum of n over the streams; -1 for n_streams outside [0, KGE_PENALTY_MAX_STREAMS],
 *                                NULL streams with n_streams > 0, or a negative n.
 *   kge_row_penalty_ws_bytes     bytes of workspace kge_row_penalty needs for M terms (the fp64 partials of the sum); 0
 *                                for M <= 0 or M >= 2^31.
 *   kge_row_penalty_rows_floats  floats of kge_row_penalty_bwd's rows buffer: the sum of c * n * d over the streams,
 *                                c = 2 for KGE_PENALTY_SPLIT and 1 otherwise; -1 as above.
 *   kge_row_penalty_row_offset   the float offset of stream s's block in that buffer: the same sum over the streams
 *                                before s (s = n_streams: the whole buffer); -1 as above or for s outside [0, n_streams]. */
int64_t kge_row_penalty_terms(const kge_penalty_stream *streams, int n_streams);
size_t kge_row_penalty_ws_bytes(int64_t M);
int64_t kge_row_penalty_rows_floats(const kge_penalty_stream *streams, int n_streams);
int64_t kge_row_penalty_row_offset(const kge_penalty_stream *streams, int n_streams, int s);

/* terms[off_s + i] = factor_s * sum_k |x_k|^p of row ids_s[i] of stream s (off_s = the sum of n over the streams before
 * s), p = 2 or 3, and *loss = the sum of the M terms.  The rows are read as stored.
 *
 * The element expressions, without contraction:
 *   REAL      p = 2: x * x                          p = 3: fabsf(x) * (x * x)
 *   complex   m2 = fmaf(im, im, re * re);  p = 2: m2;   p = 3: m2 * sqrtf(m2)
 * A row's sum is a function of (layout, p, d) alone -- not of the load path, the alignment, ld or the batch: with the row
 * cut into aligned groups of four floats (SPLIT: of four coordinates), lane l of the row's wavefront owns the groups
 * l, l + 64, ...; a group's terms are added (t0 + t1) + (t2 + t3) (INTERLEAVED: its two pairs, t0 + t1), entries past d
 * counting 0; the group sums enter the lane's fp32 accumulator in ascending group; the 64 accumulators are added by the
 * xor butterfly 32, 16, ..., 1; the factor multiplies last.  Rows of any width are served: nothing of a row is kept.
 * A table whose base lies on 16 bytes with ld a multiple of 4 is read in 16-byte quads, any other in scalars.
 *
 * The sum: the fixed fp64 tree of kge_pair_loss over the M terms (kge_hip_train.h, "The sum", with n = M), *loss its
 * value rounded to fp32 once; *acc_io += *loss when acc_io is not NULL, with the semantics of kge_pair_loss.  Two
 * launches, three for M > KGE_PAIR_LOSS_CHUNK.  M = 0 writes *loss = 0, leaves *acc_io alone and launches nothing else.
 *
 * ws: kge_row_penalty_ws_bytes(M) bytes, 8-byte aligned; its contents are scratch.  KGE_EINVAL: p outside {2, 3},
 * n_streams outside [0, KGE_PENALTY_MAX_STREAMS], NULL streams with n_streams > 0, a layout outside the three, a NULL t0,
 * SPLIT without t1, INTERLEAVED with an odd d, d < 1, ld < d, n < 0, NULL ids with n > 0, M >= 2^31, terms or loss NULL,
 * for M > 0 a NULL or misaligned workspace or ws_bytes below the bound. */
int kge_row_penalty(const kge_penalty_stream *streams, int n_streams, int p, float *terms, float *loss, float *acc_io,
                    void *ws, size_t ws_bytes, kge_stream_t stream);

/* The backward: the gradient rows of go[0] * (*loss), one launch.  Every wavefront gathers its row again and writes
 *   REAL      p = 2: c * x                          p = 3: (c * fabsf(x)) * x
 *   complex   p = 2: (c * re, c * im)               p = 3: ((c * m) * re, (c * m) * im),  m = sqrtf(m2)
 * with c = (p * factor_s) * go[0] -- p * factor_s rounded once on the host, go read on the device.  No division: the
 * gradient of a zero row or a zero coordinate is exactly 0.
 *
 * The rows buffer (kge_row_penalty_rows_floats floats): stream s's block starts at kge_row_penalty_row_offset(.., s),
 * its rows are d_s floats apart, row i belongs to ids_s[i]; SPLIT: the n_s rows of the real parts first, then the n_s rows
 * of the imaginary parts.  No float atomic, no table-sized output.
 *
 * KGE_EINVAL: as kge_row_penalty for p and the streams, and a NULL go or rows. */
int kge_row_penalty_bwd(const kge_penalty_stream *streams, int n_streams, int p, const float *go, float *rows,
                        kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_PENALTY_H */
