// Data-redundancy analytics (gfx950) -- include/kge_hip_redundancy.h, SURVEY row 19.
//
//   kge_relation_overlap   the two relation x relation co-occurrence matrices (same orientation / reversed) of two fact
//                          lists: pack 64-bit keys (pair | orient | tag | r), ONE rocPRIM radix sort, then one thread per
//                          sorted element walks its run of equal (lo, hi) and adds 1 per partner
//   kge_relation_stats     facts / distinct heads / distinct tails per relation: two sorts of (r, e) keys + run-head counts
//   kge_overlap_select     threshold the strict upper triangle and compact the survivors in row-major order (the
//                          prefix-count scheme of mask_scan.h over a byte mask of the n_rel^2 cells)
//
// Integer arithmetic throughout, except the two IEEE double divisions of kge_overlap_select.  The atomics are integer adds
// whose results are unused: the sums do not depend on arrival order.
#include "kge_common.h"
#include "mask_scan.h"
#include "../../include/kge_hip_redundancy.h"
#include <rocprim/device/device_radix_sort.hpp>

namespace {

typedef unsigned long long u64;

inline size_t a256(size_t x) { return (x + 255) / 256 * 256; }
inline int grid_for(int64_t n, int cap = 4096) { const int64_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g < cap ? g : cap)); }
inline int bits_of(u64 x) { int b = 0; while (x) { ++b; x >>= 1; } return b < 1 ? 1 : b; }

#define KGE_GRID_STRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

size_t sort_keys_temp(int64_t n, int bits)
{
    size_t b = 0;
    u64 *nul = nullptr;
    (void)rocprim::radix_sort_keys(nullptr, b, nul, nul, (size_t)n, 0u, (unsigned)bits);
    return b;
}

// ---- relation overlap ----------------------------------------------------------------------------------------
// columns [0, n_rel) of every row of the (n_rel, ld) matrices; b may be NULL
__global__ void ro_zero_kernel(int32_t *__restrict__ a, int32_t *__restrict__ b, int64_t n_rel, int64_t ld)
{
    KGE_GRID_STRIDE(i, n_rel * n_rel) {
        const int64_t cell = (i / n_rel) * ld + i % n_rel;
        a[cell] = 0;
        if (b) b[cell] = 0;
    }
}

// elements [0, nA) from A (tag 0), [nA, nA + nB) from B (tag 1)
__global__ void ro_pack_kernel(const int64_t *__restrict__ hA, const int64_t *__restrict__ tA, const int64_t *__restrict__ rA,
                               int64_t nA, const int64_t *__restrict__ hB, const int64_t *__restrict__ tB,
                               const int64_t *__restrict__ rB, int64_t nB, u64 n_ent, int rbits, u64 *__restrict__ key)
{
    KGE_GRID_STRIDE(j, nA + nB) {
        const bool b = j >= nA;
        const int64_t f = b ? j - nA : j;
        const u64 h = (u64)(b ? hB[f] : hA[f]), t = (u64)(b ? tB[f] : tA[f]), r = (u64)(b ? rB[f] : rA[f]);
        const u64 lo = h < t ? h : t, hi = h < t ? t : h;
        key[j] = ((lo * n_ent + hi) << (rbits + 2)) | ((h > t ? 1ull : 0ull) << (rbits + 1)) | ((b ? 1ull : 0ull) << rbits) | r;
    }
}

// One thread per sorted element x: a first occurrence of its key that belongs to A (any element when B = A) visits every
// first occurrence y of B in its run of equal (lo, hi) -- backwards to the run's start, forwards to its end.  The work of
// a group of m distinct elements is m per thread on m threads, never m^2 on one lane.
// Plain adds: a form that stepped the lanes of a wave through their runs together and combined the lanes of a step that
// target one cell (match-any over the cell index, one atomic per distinct cell) gave the same matrices and took 11.8 ms
// against 2.1 ms for the whole entry point at FB15k's shape (profiles/r09/redundancy.txt); it was deleted.
__global__ __launch_bounds__(256) void ro_count_kernel(const u64 *__restrict__ keys, int64_t n, u64 n_ent, int rbits, int self_mode,
                                                       int32_t *same, int32_t *rev, int64_t ld)
{
    const u64 rmask = (1ull << rbits) - 1ull;
    const int pshift = rbits + 2;
    KGE_GRID_STRIDE(x, n) {
        const u64 kx = keys[x];
        if (x > 0 && keys[x - 1] == kx) continue;               // a repeated fact counts once
        if (!self_mode && ((kx >> rbits) & 1ull)) continue;     // x ranges over A
        const u64 px = kx >> pshift;
        const bool loop = px / n_ent == px % n_ent;             // lo == hi: (a, a) lies in T and in T_inv
        const u64 ox = (kx >> (rbits + 1)) & 1ull;
        const int64_t row = (int64_t)(kx & rmask) * ld;
        auto visit = [&](u64 ky) {
            if (!self_mode && !((ky >> rbits) & 1ull)) return;  // y ranges over B
            const int64_t cell = row + (int64_t)(ky & rmask);
            const bool eq = ((ky >> (rbits + 1)) & 1ull) == ox;
            if (loop || eq) atomicAdd(&same[cell], 1);
            if (rev && (loop || !eq)) atomicAdd(&rev[cell], 1);
        };
        // backwards: y is a first occurrence when keys[y - 1] differs (or y == 0)
        int64_t y = x - 1;
        u64 ky = y >= 0 ? keys[y] : 0ull;
        while (y >= 0 && (ky >> pshift) == px) {
            const u64 kp = y > 0 ? keys[y - 1] : ~ky;
            if (kp != ky) visit(ky);
            ky = kp;
            --y;
        }
        // forwards, x itself included
        visit(kx);
        u64 kprev = kx;
        for (y = x + 1; y < n; ++y) {
            const u64 k = keys[y];
            if ((k >> pshift) != px) break;
            if (k != kprev) visit(k);
            kprev = k;
        }
    }
}

// ---- relation stats --------------------------------------------------------------------------------------------
__global__ void rs_zero_kernel(int64_t *__restrict__ out, int64_t n) { KGE_GRID_STRIDE(i, n) out[i] = 0; }

__global__ void rs_pack_kernel(const int64_t *__restrict__ e, const int64_t *__restrict__ r, int64_t n, u64 n_ent,
                               u64 *__restrict__ key)
{
    KGE_GRID_STRIDE(j, n) key[j] = (u64)r[j] * n_ent + (u64)e[j];
}

// sorted (r, e) keys: distinct[r] += run heads of relation r, facts[r] += elements of relation r (facts may be NULL).
// Inside a wave the relation is non-decreasing: the first lane of every relation adds its segment's two popcounts, one
// integer atomic per (wave, relation).
__global__ __launch_bounds__(256) void rs_count_kernel(const u64 *__restrict__ keys, int64_t n, u64 n_ent, u64 *facts, u64 *distinct)
{
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {     // (uniform trip count)
        const int64_t j = base + threadIdx.x;
        const bool valid = j < n;
        const u64 k = valid ? keys[j] : 0ull;
        const bool head = valid && (j == 0 || keys[j - 1] != k);
        const long long r = valid ? (long long)(k / n_ent) : -1ll;
        const long long rp = __shfl_up(r, 1, 64);
        const bool leader = valid && (lane == 0 || rp != r);
        const u64 lead_mask = __ballot(leader), head_mask = __ballot(head), valid_mask = __ballot(valid);
        if (leader) {
            const u64 higher = lane == 63 ? 0ull : (lead_mask & (~0ull << (lane + 1)));
            const int end = higher ? __ffsll((long long)higher) - 1 : 64;        // the next relation's first lane
            const u64 seg = (end == 64 ? ~0ull : ((1ull << end) - 1ull)) & (~0ull << lane) & valid_mask;
            atomicAdd(&distinct[r], (u64)__popcll(seg & head_mask));
            if (facts) atomicAdd(&facts[r], (u64)__popcll(seg));
        }
    }
}

// ---- overlap select --------------------------------------------------------------------------------------------
// mask[p] of cell p = r1 * n_rel + r2: r1 < r2 and both ratios above their thresholds (a row-major walk of all cells
// meets the strict upper triangle in the order of itertools.combinations)
__global__ void os_mask_kernel(const int32_t *__restrict__ counts, int64_t ld, const int64_t *__restrict__ lengths, int64_t n_rel,
                               double theta1, double theta2, uint8_t *__restrict__ mask)
{
    KGE_GRID_STRIDE(p, n_rel * n_rel) {
        const int64_t r1 = p / n_rel, r2 = p % n_rel;
        bool keep = false;
        if (r1 < r2) {
            const int64_t l1 = lengths[r1], l2 = lengths[r2];
            if (l1 > 0 && l2 > 0) {
                const double c = (double)counts[r1 * ld + r2];
                keep = c / (double)l1 > theta1 && c / (double)l2 > theta2;
            }
        }
        mask[p] = keep ? 1 : 0;
    }
}

__global__ __launch_bounds__(MS_CT) void os_emit_kernel(const uint8_t *__restrict__ mask, int64_t n, int64_t n_rel,
                                                        const int32_t *__restrict__ block_base, int32_t *__restrict__ pairs,
                                                        int64_t cap, int64_t *__restrict__ n_out)
{
    int m[MS_CE];
    int64_t idx = mask_thread_prefix(mask, n, block_base, m);
    const int64_t first = (int64_t)blockIdx.x * MS_CB + threadIdx.x * MS_CE;
#pragma unroll
    for (int e = 0; e < MS_CE; ++e) {
        if (!m[e]) continue;
        if (idx < cap) {
            pairs[2 * idx] = (int32_t)((first + e) / n_rel);
            pairs[2 * idx + 1] = (int32_t)((first + e) % n_rel);
        }
        ++idx;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == MS_CT - 1) *n_out = idx;      // the last thread has seen every cell
}

} // namespace

extern "C" int64_t kge_relation_overlap_ws_bytes(int64_t n_a, int64_t n_b)
{
    if (n_a < 0 || n_b < 0) return 0;
    const int64_t n = n_a + n_b;
    if (n <= 0 || n > 0x7fffffffll) return 0;
    return (int64_t)(2 * a256((size_t)n * 8) + a256(sort_keys_temp(n, 64)));
}

extern "C" int kge_relation_overlap(const int64_t *hA, const int64_t *tA, const int64_t *rA, int64_t nA, const int64_t *hB,
                                    const int64_t *tB, const int64_t *rB, int64_t nB, int64_t n_ent, int64_t n_rel,
                                    int32_t *same, int32_t *rev, int64_t ld, void *ws, int64_t ws_bytes, kge_stream_t stream)
{
    const bool self_mode = hB == nullptr;
    if (self_mode) nB = 0;
    if (nA < 0 || nB < 0 || nA > 0x7fffffffll || nB > 0x7fffffffll || nA + nB > 0x7fffffffll) return KGE_EINVAL;
    if (n_ent <= 0 || n_rel <= 0 || n_rel > 0x7fffffffll || ld < n_rel || !same) return KGE_EINVAL;
    if (nA > 0 && (!hA || !tA || !rA)) return KGE_EINVAL;
    if (nB > 0 && (!tB || !rB)) return KGE_EINVAL;
    if ((u64)n_ent > 0x100000000ull) return KGE_EUNSUPPORTED;
    const int rbits = bits_of((u64)n_rel - 1), pbits = bits_of((u64)n_ent * (u64)n_ent - 1);
    if (pbits + 2 + rbits > 64) return KGE_EUNSUPPORTED;
    const int64_t n = nA + nB;
    const bool empty = nA == 0 || (!self_mode && nB == 0);
    size_t a = 0, temp_bytes = 0;
    if (!empty) {
        a = a256((size_t)n * 8);
        if (!ws || ws_bytes < kge_relation_overlap_ws_bytes(nA, nB)) return KGE_EINVAL;
        temp_bytes = (size_t)ws_bytes - 2 * a;
        if (sort_keys_temp(n, pbits + 2 + rbits) > temp_bytes) return KGE_EINVAL;
    }
    hipStream_t s = kge_s(stream);
    hipLaunchKernelGGL(ro_zero_kernel, dim3(grid_for(n_rel * n_rel)), dim3(256), 0, s, same, rev, n_rel, ld);
    KGE_CHECK_LAUNCH();
    if (empty) return 0;
    char *w = reinterpret_cast<char *>(ws);
    u64 *k_in = (u64 *)w, *k_out = (u64 *)(w + a);
    const int g = grid_for(n);
    hipLaunchKernelGGL(ro_pack_kernel, dim3(g), dim3(256), 0, s, hA, tA, rA, nA, hB, tB, rB, nB, (u64)n_ent, rbits, k_in);
    KGE_CHECK_LAUNCH();
    hipError_t e = rocprim::radix_sort_keys(w + 2 * a, temp_bytes, k_in, k_out, (size_t)n, 0u, (unsigned)(pbits + 2 + rbits), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ro_count_kernel, dim3(g), dim3(256), 0, s, k_out, n, (u64)n_ent, rbits, self_mode ? 1 : 0, same, rev, ld);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t kge_relation_stats_ws_bytes(int64_t n)
{
    if (n <= 0 || n > 0x7fffffffll) return 0;
    return (int64_t)(2 * a256((size_t)n * 8) + a256(sort_keys_temp(n, 64)));
}

extern "C" int kge_relation_stats(const int64_t *h, const int64_t *t, const int64_t *r, int64_t n, int64_t n_ent,
                                  int64_t n_rel, int64_t *out, void *ws, int64_t ws_bytes, kge_stream_t stream)
{
    if (n < 0 || n > 0x7fffffffll || n_ent <= 0 || n_rel <= 0 || !out) return KGE_EINVAL;
    if ((u64)n_rel > (~0ull) / (u64)n_ent) return KGE_EUNSUPPORTED;
    const int bits = bits_of((u64)n_rel * (u64)n_ent - 1);
    size_t a = 0, temp_bytes = 0;
    if (n > 0) {
        if (!h || !t || !r || !ws || ws_bytes < kge_relation_stats_ws_bytes(n)) return KGE_EINVAL;
        a = a256((size_t)n * 8);
        temp_bytes = (size_t)ws_bytes - 2 * a;
        if (sort_keys_temp(n, bits) > temp_bytes) return KGE_EINVAL;
    }
    hipStream_t s = kge_s(stream);
    hipLaunchKernelGGL(rs_zero_kernel, dim3(grid_for(3 * n_rel)), dim3(256), 0, s, out, 3 * n_rel);
    KGE_CHECK_LAUNCH();
    if (n == 0) return 0;
    char *w = reinterpret_cast<char *>(ws);
    u64 *k_in = (u64 *)w, *k_out = (u64 *)(w + a);
    u64 *o = reinterpret_cast<u64 *>(out);
    const int g = grid_for(n);
    for (int side = 0; side < 2; ++side) {
        hipLaunchKernelGGL(rs_pack_kernel, dim3(g), dim3(256), 0, s, side == 0 ? h : t, r, n, (u64)n_ent, k_in);
        KGE_CHECK_LAUNCH();
        size_t tb = temp_bytes;
        hipError_t e = rocprim::radix_sort_keys(w + 2 * a, tb, k_in, k_out, (size_t)n, 0u, (unsigned)bits, s);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(rs_count_kernel, dim3(g), dim3(256), 0, s, k_out, n, (u64)n_ent, side == 0 ? o : (u64 *)nullptr,
                           o + (side + 1) * n_rel);
        KGE_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int64_t kge_overlap_select_ws_bytes(int64_t n_rel)
{
    if (n_rel <= 0 || n_rel > 46340) return 0;                  // n_rel^2 < 2^31: the block bases are int32
    const int64_t cells = n_rel * n_rel;
    return (int64_t)(a256((size_t)cells) + a256((size_t)mask_scan_ws_elems(cells) * 4));
}

extern "C" int kge_overlap_select(const int32_t *counts, int64_t ld, const int64_t *lengths, int64_t n_rel, double theta1,
                                  double theta2, int32_t *pairs, int64_t cap, int64_t *n_out, void *ws, int64_t ws_bytes,
                                  kge_stream_t stream)
{
    if (n_rel <= 0 || ld < n_rel || cap < 0 || !counts || !lengths || !n_out || !ws || (cap > 0 && !pairs)) return KGE_EINVAL;
    if (n_rel > 46340) return KGE_EUNSUPPORTED;
    if (ws_bytes < kge_overlap_select_ws_bytes(n_rel)) return KGE_EINVAL;
    const int64_t cells = n_rel * n_rel;
    hipStream_t s = kge_s(stream);
    uint8_t *mask = reinterpret_cast<uint8_t *>(ws);
    int32_t *bases = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(ws) + a256((size_t)cells));
    hipLaunchKernelGGL(os_mask_kernel, dim3(grid_for(cells)), dim3(256), 0, s, counts, ld, lengths, n_rel, theta1, theta2, mask);
    KGE_CHECK_LAUNCH();
    const int rc = mask_scan_launch(mask, cells, bases, s);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(os_emit_kernel, dim3((unsigned)mask_scan_blocks(cells)), dim3(MS_CT), 0, s, mask, cells, n_rel, bases, pairs,
                       cap, n_out);
    KGE_CHECK_LAUNCH();
    return 0;
}
