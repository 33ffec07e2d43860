// kge_segment_sum_ordered (include/kge_hip_det.h): the segmented row sum of the backward with a FIXED summation order
// and no float atomic -- the reduction behind torchkge_amd.set_deterministic(True).
//
// kge_segment_sum_rows (segment_sum_rows.hip) walks the sorted entries in chunks of 32 per wavefront and flushes every run
// with an atomic row-add: runs that cross chunks are summed in arrival order.  Here the chunk walk is the same, but a
// row of `out` is only ever written by ONE wavefront of ONE launch:
//
//   level 0   a wavefront takes 32 consecutive sorted entries and sums their runs in registers, in entry order.  A run
//             that is neither the chunk's first nor its last has both neighbours inside the chunk, so it is the WHOLE
//             run of its key: the wavefront adds it to out[key] with a plain read-modify-write (the old row is loaded
//             beside the run's first rows, not when the run ends).  The first and the last run may continue in the
//             neighbouring chunks: they go, with their key, into the workspace slots (chunk, 0) and (chunk, 1); an
//             unused slot takes key -1.
//   level l   the slots of level l - 1, in (chunk, slot) order, are again a list of (key, row) sorted by key -- empty
//             slots are skipped without ending a run -- and 16 times shorter.  The same kernel runs on it.
//   last      a level of one chunk writes all its runs to `out`.
//
// The levels are separate launches on the caller's stream: the stream orders them, there is no flag, fence or spin
// between workgroups.  A key's pieces either all stay in the slot list or (once they form a middle run) are all in one
// chunk, so `out[key]` has exactly one writer, and what it adds is ((r0 + r1) + ...) within chunks, chunk partials in
// chunk order within the next level's chunks, and so on: a function of (M, the sorted keys) alone.  The grid only
// decides WHICH wavefront sums a chunk, never what it sums.  A run of n entries takes ceil(n / 32) wavefronts at level
// 0: the 10^5-entry relation rows of a large batch are spread over the chip as any other run is.
#include "kge_common.h"
#include "segment_levels.h"
#include "../../include/kge_hip_det.h"

namespace {

struct SegLevel {
    // level 0: the caller's arguments
    const float *rows;
    int64_t ld;
    const int64_t *k0, *k1, *perm;
    int64_t n0;
    // level >= 1: this level's (key, row) list in the workspace (rows of d floats)
    const int64_t *keys;
    // both
    int64_t m;              // entries of this level
    int d;
    int last;               // a single chunk: every run goes to `out`
    float *out;
    int64_t out_ld;
    int64_t *slot_keys;     // the next level's list: 2 entries per chunk of this one (unused when `last`)
    float *slot_rows;
};

template <int NE>
__device__ __forceinline__ void store_slot(const SegLevel &p, int64_t slot, int64_t key, const float (&acc)[NE], int lane)
{
    if (lane == 0) p.slot_keys[slot] = key;
    if (key < 0) return;                    // an empty slot's row is never read
    float *o = p.slot_rows + slot * p.d;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int k = lane + 64 * e;
        if (k < p.d) o[k] = acc[e];
    }
}

// A run of the chunk is complete: its key's slot, or -- the one writer of that row of `out` -- old row + sum.  `prev` is
// the old row, loaded when the run opened: a load issued here would stall the wavefront for a memory round trip per
// run (20 and more runs in a chunk of entity ids), where the atomic reduction fires and forgets.
template <int NE>
__device__ __forceinline__ void close_run(const SegLevel &p, int64_t c, int64_t key, int64_t s0, int64_t s1,
                                          const float (&acc)[NE], const float (&prev)[NE], int lane)
{
    if (key == s0) return store_slot<NE>(p, 2 * c, key, acc, lane);
    if (key == s1) return store_slot<NE>(p, 2 * c + 1, key, acc, lane);
    float *o = p.out + key * p.out_ld;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int k = lane + 64 * e;
        if (k < p.d) o[k] = prev[e] + acc[e];
    }
}

template <int NE, bool L0>
__global__ __launch_bounds__(256) void segment_sum_ordered_kernel(const SegLevel p)
{
    // rows in flight per step (each with the old `out` row it may open): 64 registers of loads whatever the width.  A chunk
    // is CH / UN dependent memory round trips, and the upper levels are a few chunks each -- latency, not bandwidth
    constexpr int CH = KGE_DET_CH, UN = 32 / NE;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t chunks = (p.m + CH - 1) / CH;
    for (int64_t c = wave; c < chunks; c += nwaves) {
        const int64_t j0 = c * CH;
        const int n = (int)min((int64_t)CH, p.m - j0);
        // the chunk's (row, key) pairs: one coalesced load, then broadcast by shuffle
        const int64_t jl = j0 + min(lane, n - 1);
        int64_t my_row, my_key;
        if (L0) {
            my_row = p.perm[jl];
            my_key = my_row < p.n0 ? p.k0[my_row] : p.k1[my_row - p.n0];
        } else {
            my_row = jl;
            my_key = p.keys[jl];
        }
        // keys of the chunk's first and last run (-1: the chunk holds no entry): they go to the slots (chunk, 0 | 1);
        // every other run lies wholly inside the chunk and goes to `out`.  A single-chunk level has no slots (-2: no key).
        const unsigned long long live = __ballot(lane < n && my_key >= 0);
        const int64_t first_key = live ? __shfl(my_key, __ffsll((long long)live) - 1, 64) : -1;
        const int64_t last_key = live ? __shfl(my_key, 63 - __clzll((long long)live), 64) : -1;
        const int64_t s0 = p.last ? -2 : first_key, s1 = p.last ? -2 : last_key;
        const float *base = p.rows;
        const int64_t ld = p.ld;
        float acc[NE], prev[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] = prev[e] = 0.f;
        int64_t cur = -1;       // key of the open run (-1: none yet)
        for (int j = 0; j < n; j += UN) {
            float v[UN][NE], pre[UN][NE];
            int64_t kk[UN];
            int64_t pk = cur;
#pragma unroll
            for (int u = 0; u < UN; ++u) {      // UN independent row loads in flight ...
                const int ju = min(j + u, n - 1);
                kk[u] = j + u < n ? __shfl(my_key, ju, 64) : -1;        // wave-uniform
                const float *row = base + __shfl(my_row, ju, 64) * ld;
                // ... and, for a run that OPENS here and will be written to `out`, the row it adds to
                const bool direct = kk[u] >= 0 && kk[u] != pk && kk[u] != s0 && kk[u] != s1;
                if (kk[u] >= 0) pk = kk[u];
                const float *old = p.out + (direct ? kk[u] : 0) * p.out_ld;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int k = lane + 64 * e;
                    v[u][e] = (k < p.d && kk[u] >= 0) ? row[k] : 0.f;   // an empty slot's row is not read
                    pre[u][e] = (k < p.d && direct) ? old[k] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                if (kk[u] < 0) continue;        // past the end, or an empty slot: does not end a run
                if (kk[u] != cur) {
                    if (cur >= 0) close_run<NE>(p, c, cur, s0, s1, acc, prev, lane);
#pragma unroll
                    for (int e = 0; e < NE; ++e) { acc[e] = 0.f; prev[e] = pre[u][e]; }
                    cur = kk[u];
                }
#pragma unroll
                for (int e = 0; e < NE; ++e) acc[e] += v[u][e];
            }
        }
        if (cur >= 0) close_run<NE>(p, c, cur, s0, s1, acc, prev, lane);
        if (!p.last) {                          // the slots no run took are empty
            if (first_key < 0) store_slot<NE>(p, 2 * c, -1, acc, lane);
            if (first_key < 0 || first_key == last_key) store_slot<NE>(p, 2 * c + 1, -1, acc, lane);
        }
    }
}

template <int NE>
void launch_level(const SegLevel &p, bool level0, hipStream_t s)
{
    const int grid = kge_seg_grid(p.m);
    if (level0) hipLaunchKernelGGL((segment_sum_ordered_kernel<NE, true>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((segment_sum_ordered_kernel<NE, false>), dim3(grid), dim3(256), 0, s, p);
}

} // namespace

extern "C" size_t kge_segment_sum_ordered_ws_bytes(int64_t M, int d)
{
    return kge_det_make_plan(M, d).bytes;
}

extern "C" int kge_segment_sum_ordered(const float *rows, int64_t ld, int d, const int64_t *k0, int64_t n0,
                                       const int64_t *k1, int64_t n1, const int64_t *perm, float *out, int64_t out_ld,
                                       void *ws, size_t ws_bytes, kge_stream_t stream)
{
    const int todo = kge_seg_check_args(rows, ld, d, k0, n0, k1, n1, perm, out, out_ld);
    if (todo <= 0) return todo < 0 ? KGE_EINVAL : 0;
    if (n0 > INT64_MAX - n1) return KGE_EINVAL;
    const int64_t M = n0 + n1;
    const kge_det_plan plan = kge_det_make_plan(M, d);
    if (plan.n_levels == 0 || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < plan.bytes) return KGE_EINVAL;
    int64_t *ws_keys = static_cast<int64_t *>(ws);
    float *ws_rows = reinterpret_cast<float *>(ws_keys + plan.slots);
    hipStream_t s = kge_s(stream);
    for (int l = 0; l < plan.n_levels; ++l) {
        SegLevel p{};
        p.m = plan.m[l];
        p.d = d;
        p.last = l == plan.n_levels - 1;
        p.out = out;
        p.out_ld = out_ld;
        if (l == 0) {
            p.rows = rows; p.ld = ld; p.k0 = k0; p.k1 = k1; p.perm = perm; p.n0 = n0;
        } else {
            p.keys = ws_keys + plan.key_off[l];
            p.rows = ws_rows + plan.row_off[l] * d;
            p.ld = d;
        }
        if (!p.last) {
            p.slot_keys = ws_keys + plan.key_off[l + 1];
            p.slot_rows = ws_rows + plan.row_off[l + 1] * d;
        }
        if (d <= 256) launch_level<4>(p, l == 0, s);
        else if (d <= 512) launch_level<8>(p, l == 0, s);
        else launch_level<16>(p, l == 0, s);
        KGE_CHECK_LAUNCH();
    }
    return 0;
}
