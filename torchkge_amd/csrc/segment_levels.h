// Chunk size, grid and argument check of the two segmented row sums (segment_sum_rows.hip, segment_sum_ordered.hip) and
// the level plan of kge_segment_sum_ordered: plain host arithmetic, no HIP in here, so that it can be compiled into a
// stand-alone program and checked on the CPU.
//
// Level 0 is the caller's M sorted entries.  A level of m entries is cut into chunks of KGE_DET_CH; unless it is a
// single chunk it leaves two slots per chunk -- (key, partial row) of the chunk's first and last run -- which are the
// next level's entries.  The workspace holds the levels >= 1: all their keys first (int64), then all their rows (d
// floats each).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int KGE_DET_CH = 32;          // sorted entries per wavefront chunk
constexpr int64_t KGE_DET_MAX_M = (int64_t)1 << 48;     // entries accepted: m + 31 and slot * d stay far from 2^63
constexpr int KGE_DET_MAX_LEVELS = 16;  // 2 * ceil(m / 32) from m = 2^48 reaches one chunk in 12 steps

// What kge_segment_sum_rows (segment_sum_rows.hip) and kge_segment_sum_ordered share beside the chunk size.
// Workgroups of 4 wavefronts, one chunk per wavefront and turn, for the m entries of a launch:
static inline int kge_seg_grid(int64_t m)
{
    const int64_t chunks = (m + KGE_DET_CH - 1) / KGE_DET_CH, blocks = (chunks + 3) / 4;
    return (int)(blocks < 256 * 8 ? blocks : 256 * 8);
}
// Their common arguments: -1 invalid, 0 no entry (nothing to do, whatever the pointers), 1 a reduction to run
static inline int kge_seg_check_args(const float *rows, int64_t ld, int d, const int64_t *k0, int64_t n0, const int64_t *k1,
                                     int64_t n1, const int64_t *perm, const float *out, int64_t out_ld)
{
    if (n0 < 0 || n1 < 0 || d <= 0 || d > 1024 || ld < d || out_ld < d) return -1;
    if (n0 == 0 && n1 == 0) return 0;
    if (!rows || (n0 > 0 && !k0) || (n1 > 0 && !k1) || !perm || !out) return -1;
    return 1;
}

struct kge_det_plan {
    int n_levels;                           // launches: levels 0 .. n_levels - 1, the last one a single chunk
    int64_t m[KGE_DET_MAX_LEVELS];          // entries of each level (m[0] = M)
    int64_t key_off[KGE_DET_MAX_LEVELS];    // of levels >= 1: first key, in int64 elements from the workspace's start
    int64_t row_off[KGE_DET_MAX_LEVELS];    // of levels >= 1: first row, in ROWS (d floats) from the rows' start
    int64_t slots;                          // entries of all levels >= 1
    size_t bytes;                           // of the workspace; 0: M <= 0, M > KGE_DET_MAX_M, bad d, or it does not fit size_t
};

static inline kge_det_plan kge_det_make_plan(int64_t M, int d)
{
    kge_det_plan p{};
    if (M <= 0 || M > KGE_DET_MAX_M || d < 1 || d > 1024) return p;
    int64_t m = M;
    for (;;) {
        p.m[p.n_levels] = m;
        p.key_off[p.n_levels] = p.row_off[p.n_levels] = p.n_levels ? p.slots : 0;
        if (p.n_levels) p.slots += m;
        ++p.n_levels;
        const int64_t chunks = m / KGE_DET_CH + (m % KGE_DET_CH != 0);
        if (chunks == 1) break;
        if (p.n_levels == KGE_DET_MAX_LEVELS) { p = kge_det_plan{}; return p; }     // (not reachable for an int64 M)
        m = 2 * chunks;
    }
    // slots < M / 15 + 2 * n_levels <= 2^45, times at most 4104 bytes: below 2^57
    const uint64_t per = 8u + 4u * (uint64_t)d;
    if ((uint64_t)p.slots > (uint64_t)(SIZE_MAX / 2) / per) { p = kge_det_plan{}; return p; }      // (a 32-bit size_t)
    const uint64_t need = (uint64_t)p.slots * per;
    p.bytes = (size_t)(need < 16 ? 16 : need);
    return p;
}
