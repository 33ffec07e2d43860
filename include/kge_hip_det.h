/*
 * kge_hip_det.h -- the deterministic gradient reduction of libkge_hip.so: a segmented row sum whose result is the same
 * bit pattern on every run.  It stands beside kge_segment_sum_rows (kge_hip.h), which flushes its runs with fp32 atomics
 * and therefore sums in arrival order; torchkge_amd.set_deterministic(True) routes every backward through this entry.
 *
 * kge_hip.h, its descriptors and its ABI version are untouched, which is why the entry lives in a header of its own
 * (as kge_hip_analogy.h / kge_hip_convkb.h / kge_hip_triplet.h do).
 *
 * Conventions of kge_hip.h: device pointers, launches on the given stream without synchronising or reading back, no
 * allocation (the workspace size comes from kge_segment_sum_ordered_ws_bytes); returns 0, KGE_EINVAL or a positive
 * hipError_t; on a negative code nothing was launched and no output was touched.
 */
#ifndef KGE_HIP_DET_H
#define KGE_HIP_DET_H

#include <stddef.h>
#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace kge_segment_sum_ordered needs for M = n0 + n1 entries of d columns.  Host arithmetic only: no GPU
 * call, usable without a device.  0 for M <= 0, M > 2^48 or d outside [1, 1024]; otherwise at least 16 (so a caller can allocate
 * and pass a pointer for every M > 0), monotone in M and in d: about (M / 16) * (4 d + 8) bytes. */
size_t kge_segment_sum_ordered_ws_bytes(int64_t M, int d);

/* out[key, 0:d] += sum of the rows of that key, in a FIXED order.
 *
 * The arguments are those of kge_segment_sum_rows: the keys are [k0 (n0 of them) | k1 (n1, may be NULL with n1 = 0)],
 * all >= 0; `perm` (M = n0 + n1 entries) is their stable ascending order (kge_key_sort); entry j of the sorted sequence
 * has key keys[perm[j]] and contributes rows[perm[j] * ld + 0 .. d).  1 <= d <= 1024, ld >= d, out_ld >= d.
 *
 * The contract:
 *   - no float atomic anywhere: every row of `out` has exactly one writer, which does one plain read-modify-write per
 *     element (out[k] = out[k] + sum);
 *   - the order in which the rows of a run are added is a function of (M, the sorted key sequence) only -- not of the
 *     grid, the scheduling, the number of CUs or earlier launches: the same inputs give the same bits;
 *   - rows of `out` whose key does not occur, the columns d .. out_ld - 1 of `out` and the columns d .. ld - 1 of
 *     `rows` are neither read nor written;
 *   - a run of n entries is summed as a tree: 32 consecutive sorted entries per wavefront, the partial rows of the runs
 *     that reach a chunk's ends go through the workspace to the next level, 16 times shorter, in separate launches on
 *     the stream (about log16 M of them: 6 at M = 4 M) -- a long run is not one wavefront's serial loop.
 *
 * ws: kge_segment_sum_ordered_ws_bytes(M, d) bytes, 8-byte aligned; its contents are scratch.  M = 0: a successful
 * no-op.  Bad arguments, a NULL or misaligned workspace or ws_bytes below the bound: KGE_EINVAL. */
int kge_segment_sum_ordered(const float *rows, int64_t ld, int d, const int64_t *k0, int64_t n0, const int64_t *k1,
                            int64_t n1, const int64_t *perm, float *out, int64_t out_ld, void *ws, size_t ws_bytes,
                            kge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_DET_H */
