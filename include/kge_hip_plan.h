/*
 * kge_hip_plan.h -- the work split of the exact all-candidates kernels of libkge_hip.so, as pure host functions.
 *
 * kge_lp_scores / kge_lp_count_ge run one of two persistent tile kernels (kge_hip.h, kge_lp_desc):
 *
 *   MFMA modes (KGE_LP_DOT, _L2_EXPAND, _L2_PROJH, _L2_PROJD; lp_gemm_mfma.hip): the (row panel, candidate tile) items
 *     item = panel * col_tiles + tile of KGE_LP_GEMM_BM x KGE_LP_GEMM_BN scores are cut into `grid` contiguous ranges
 *     of equal length (+-1); the block with blockIdx.x = bid walks range number lid(bid), where the blocks of one XCD
 *     (equal bid % 8) own neighbouring ranges.
 *   VALU modes (KGE_LP_L1_DIRECT, _L2_DIRECT, the torus modes; lp_direct.hip): a block owns ONE row panel of
 *     KGE_LP_DIRECT_BM_PLAIN (no rank-1 term) or KGE_LP_DIRECT_BM_AXPY (rank-1 term) queries and walks
 *     `tiles_per_block` consecutive candidate tiles of KGE_LP_DIRECT_BN.
 *
 * The functions here answer "which block walks what" with the very arithmetic the kernels and their launchers use (one
 * definition each, shared with the device code), so that a test can assert the premise it was built for -- several items
 * per block, a panel change inside a range, a counter flush -- instead of restating the launch arithmetic.  They launch
 * nothing, allocate nothing and touch no device memory; kge_lp_gemm_plan with grid = 0 asks the current device for its
 * compute-unit count exactly as the launcher does (256 when there is no device).  The environment knobs of the
 * launchers (KGE_LP_ROUNDS, KGE_LP_WAVES, KGE_LP_TARGET_BLOCKS) are read at every call, as the launchers read them.
 *
 * kge_hip.h, its descriptors and its ABI version are untouched.
 */
#ifndef KGE_HIP_PLAN_H
#define KGE_HIP_PLAN_H

#include "kge_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KGE_LP_GEMM_BM 128          /* queries per row panel, MFMA kernel */
#define KGE_LP_GEMM_BN 128          /* candidates per tile, MFMA kernel */
#define KGE_LP_DIRECT_BM_PLAIN 128  /* queries per row panel, VALU kernels without the rank-1 term */
#define KGE_LP_DIRECT_BM_AXPY 64    /* ... with it */
#define KGE_LP_DIRECT_BN 128        /* candidates per tile, VALU kernels */

/* The split of a (B, N) problem of an MFMA mode over `grid` blocks; grid = 0: the grid the launcher picks on the current
 * device, min(items, 2 * compute units * KGE_LP_ROUNDS).  Returns the grid (0 for B == 0 or N == 0), KGE_EINVAL for
 * B < 0, N < 0, grid < 0 or more than 2^31 - 1 items.
 *   dims   (may be NULL): int64 [2] = row_panels, col_tiles
 *   blocks (may be NULL): int64 [grid][3] = lid, item_begin, item_end of the block with blockIdx.x = index; a block
 *          with item_begin == item_end returns at once (only when grid > items). */
int kge_lp_gemm_plan(int64_t B, int64_t N, int grid, int64_t *dims, int64_t *blocks);

/* Candidate tiles of ONE row panel after which a block of the MFMA count kernel flushes its 8-bit per-lane rank
 * counters (a lane's counter gains at most 32x32-tiles-per-wave-along-N per tile: 255 / that), for the wave layout
 * KGE_LP_WAVES selects. */
int kge_lp_gemm_flush_interval(void);

/* The split of a (B, N) problem of a VALU mode; axpy != 0: with the rank-1 term.  Returns 0, KGE_EINVAL for B < 0,
 * N < 0 or NULL plan.
 *   plan:   int64 [4] = row_panels, col_tiles, tiles_per_block, grid (all 0 for B == 0 or N == 0)
 *   blocks (may be NULL): int64 [grid][3] = row panel, tile_begin, tile_end of the block with blockIdx.x = index. */
int kge_lp_direct_plan(int64_t B, int64_t N, int axpy, int64_t *plan, int64_t *blocks);

#ifdef __cplusplus
}
#endif
#endif /* KGE_HIP_PLAN_H */
