// What the two free-running count kernels of the one-product level share (lp_hi_stream.hip: resident query panel;
// lp_hi_chunk.hip: the panel streamed through a two-slot chunk ring): the work order, a wave's candidate fragments, the
// per-lane thresholds, the compare of one 32-query sub-tile, the list / count flushes and the launch.  What differs between
// them -- how the query operand reaches the MFMA, the K sweep and its interleave, grouped columns, the projection term --
// stays in the two files.  Included by those two only.
#pragma once
#include "kge_common.h"
#ifndef KGE_BUILD_NO_SLP
#error "build with -fno-slp-vectorize -DKGE_BUILD_NO_SLP=1 (torchkge_amd/csrc/build.py): SLP-packed v_pk_fma_f32 with a lane-crossing op_sel misreads beside co-executing MFMAs (profiles/r06/slp_bisect.txt)"
#endif

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int SW_MT = 2;                        // 32-row MFMA tiles per wave: ...
constexpr int SW_WROWS = 32 * SW_MT;            // ... its 64 candidate rows
constexpr int SW_WLIST = 384;                   // uncertain pairs buffered per wave (int2 entries), one sub-list per 32-query sub-tile

// ---- work order: as lp_split_count_kernel -- QG panels interleaved under a sweep of the candidate tiles, XCD x owns an
// eighth of the item list, its blocks take stride-nbx positions (nbx a multiple of QG: a block keeps its panel).
// IDX: the width of an item index (lp_hi_stream_kernel: int; lp_hi_chunk_kernel: int64_t)
template <typename IDX>
struct sw_work_order {
    int nitems;             // items of this block (<= 0: none)
    int qg, q_panels, c_tiles, nbx;
    int64_t item_begin;

    __device__ __forceinline__ explicit sw_work_order(const kge_hi_stream_params &p)
        : qg(p.qg), q_panels(p.q_panels), c_tiles(p.c_tiles)
    {
        const int nb = gridDim.x, bid = blockIdx.x;
        const int xcd = bid & 7, loc = bid >> 3;
        nbx = (nb - xcd + 7) >> 3;
        const int nx = nb < 8 ? nb : 8;
        const int64_t x_begin = p.n_items * xcd / nx, x_end = p.n_items * (xcd + 1) / nx;
        item_begin = x_begin + loc;
        nitems = item_begin < x_end ? (int)((x_end - item_begin + nbx - 1) / nbx) : 0;
    }
    // item -> (query panel, candidate tile).  Panels are grouped: floor(P / QG) groups of QG panels, then one group per set
    // bit of the remainder (sizes QG/2 .. 1); inside a group the items run (panel 0, tile 0) (panel 1, tile 0) .. so
    // that a block stepping by nbx -- a multiple of every group size -- keeps ITS panel while the blocks of the XCD sweep
    // the candidate tiles together (every tile enters the L2 once per group).
    __device__ __forceinline__ void item(int i, int &qp, int &ct) const
    {
        const int full_panels = (q_panels / qg) * qg;
        const IDX full_items = (IDX)full_panels * c_tiles;
        IDX idx = (IDX)item_begin + (IDX)i * nbx;
        int base = 0, gsz = qg;
        if (idx < full_items) {
            const IDX per = (IDX)qg * c_tiles;
            const int grp = (int)(idx / per);
            idx -= grp * per;
            base = grp * qg;
        } else {
            idx -= full_items;
            base = full_panels;
            const int rem = q_panels - full_panels;
            gsz = 1;
            for (int sz = qg >> 1; sz >= 1; sz >>= 1) {
                if (rem & sz) {
                    if (idx < (IDX)sz * c_tiles) { gsz = sz; break; }
                    idx -= (IDX)sz * c_tiles;
                    base += sz;
                }
            }
        }
        ct = (int)(idx / gsz);
        qp = base + (int)(idx - (IDX)ct * gsz);
    }
};

// ---- candidate fragments of one wave: 32-row groups g, g + 1 of the fragment-major table, NW waves x 64 rows per tile
template <int NW>
struct sw_candidates {
    const char *Ef;
    int n_groups32, wid;
    int64_t gstride;                            // bytes per 32-row group
    unsigned lane16;

    __device__ __forceinline__ sw_candidates(const kge_hi_stream_params &p, int wid_, int lane)
        : Ef(p.Ef), n_groups32((int)(p.rows_p >> 5)), wid(wid_), gstride((int64_t)p.units_p << 10), lane16(lane * 16) {}
    __device__ __forceinline__ const char *tile_ptr(int ct, bool &active) const
    {
        int g = ct * (NW * 2) + wid * 2;
        active = g + 1 < n_groups32;
        g = min(g, n_groups32 - 2);             // (past the table: valid rows, results dropped)
        return Ef + g * gstride;
    }
    __device__ __forceinline__ void load_A(f16x8 (&dst)[SW_MT], const char *tp, int u) const
    {
#pragma unroll
        for (int mt = 0; mt < SW_MT; ++mt)
            dst[mt] = *reinterpret_cast<const f16x8 *>(tp + mt * gstride + (u << 10) + lane16);
    }
    // first candidate row of this wave in tile ct
    __device__ __forceinline__ int64_t first_row(int ct) const { return (int64_t)ct * (NW * SW_WROWS) + wid * SW_WROWS; }
};

// ---- per-lane thresholds of the panel's NT sub-tiles: lane l31 of sub-tile nt owns column q0 + nt * 32 + l31.
// THR4: (a_lo, a_hi) are the first half of p.thr4[q] (projection modes) instead of p.thr[q]
template <int NT, bool THR4>
__device__ __forceinline__ void sw_load_thresholds(const kge_hi_stream_params &p, int64_t q0, int l31, float (&alo)[NT],
                                                   float (&ahi)[NT], int (&qid)[NT], int (&tru)[NT])
{
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int64_t col = q0 + nt * 32 + l31;
        int64_t q = -1;
        if (col < p.q_rows) q = p.col_q ? (int64_t)p.col_q[col] : col;
        if (q >= p.B) q = -1;
        float2 t = make_float2(INFINITY, INFINITY);
        if (q >= 0) {
            if (THR4) { const float4 t4 = p.thr4[q]; t = make_float2(t4.x, t4.y); }
            else t = p.thr[q];
        }
        alo[nt] = t.x; ahi[nt] = t.y; qid[nt] = (int)q;
        // the pair (query, its true entity) scores s_true exactly: it is counted (acc >= a_lo) and a re-score could
        // never take it back -- it need not be listed (a tenth of a fitted model's list)
        tru[nt] = (p.true_idx && q >= 0) ? (int)(p.true_idx[q] - p.c_base) : -1;
    }
}

// the band [a_lo, a_hi] as the bit pattern of its width: 0 <= w <= a_hi - a_lo is ONE unsigned compare of w's bits
__device__ __forceinline__ unsigned sw_band_bits(float a_lo, float a_hi)
{
    const float hwf = a_hi - a_lo;
    return hwf >= 0.f ? __float_as_uint(hwf) : 0u;
}

struct sw_no_adjust {
    __device__ __forceinline__ void operator()(float (&)[4], int, int) const {}
};

// ---- the compare of one 32-query sub-tile (as lp_split_count_kernel: w = v - a_lo, sign bits -> popcount, band test on
// the bits).  acc[mt][nt]: this wave's 64 candidates x the sub-tile's 32 queries; c0: the wave's first candidate;
// sub / nl: the wave's sub-list of this sub-tile and its wave-uniform fill count.
// adjust(v, mt, g4) may change the 4 values of quad g4 of tile mt before the subtraction; it is called for g4 = 0 .. 3 in order.
// Appends the uncertain pairs (query qid, candidate) other than (qid, tru); returns #{v >= a_lo} of this lane's column.
template <int SUBn, int NT, class ADJUST>
__device__ __forceinline__ int sw_compare_subtile(const f32x16 (&acc)[SW_MT][NT], int nt, float a_lo, unsigned hwb, int qid,
                                                  int tru, int c0, int half, int2 *sub, int &nl, ADJUST adjust)
{
    // (opaque, and per sub-tile: candidate indices the optimiser can see through are formed ahead of the ballots, shared between
    // the sub-tiles and held in registers -- with one pin in front of all sub-tiles the 128-query kernel went from 235 to 256
    // VGPRs at 13 units and spilled 124 bytes with runtime units)
    int cl_base = 4 * half;
    asm volatile("" : "+v"(cl_base));
    unsigned smask = 0u;
#pragma unroll
    for (int mt = 0; mt < SW_MT; ++mt) {
#pragma unroll
        for (int gh = 0; gh < 2; ++gh) {
            unsigned bq[2][4];          // bit patterns of w = v - a_lo of the two quads of this half tile
#pragma unroll
            for (int g4 = 2 * gh; g4 < 2 * gh + 2; ++g4) {
                float vq[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) vq[e] = acc[mt][nt][g4 * 4 + e];
                adjust(vq, mt, g4);
                // four v_sub_f32 (a packed add per pair of elements is the slower form: profiles/r05/hi_stream_epilogue_variants.txt)
#pragma unroll
                for (int e = 0; e < 4; ++e) bq[g4 & 1][e] = __float_as_uint(vq[e] - a_lo);
#pragma unroll
                for (int e = 0; e < 4; ++e) smask = __builtin_amdgcn_alignbit(smask, bq[g4 & 1][e], 31);
            }
            // uncertain pairs (0 <= w <= band width, as unsigned bit patterns), tested per PAIR of quads: half the ballots and
            // branches of a test per quad
            const unsigned mq0 = min(min(min(bq[0][0], bq[0][1]), bq[0][2]), bq[0][3]);
            const unsigned mq1 = min(min(min(bq[1][0], bq[1][1]), bq[1][2]), bq[1][3]);
            if (__ballot(min(mq0, mq1) <= hwb)) {       // some lane holds an uncertain pair among these 8 rows
                // (kept SMALL: unrolled 12 / 16 times; capacity is checked once per tile by sw_clamp_sublist -- an entry
                // past the buffer raises the overflow flag, like UNC_CAP of lp_split_count_kernel)
#pragma unroll
                for (int qq = 0; qq < 2; ++qq) {
                    const int g4 = 2 * gh + qq;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int cand = c0 + cl_base + mt * 32 + e + 8 * g4;
                        const bool unc = bq[qq][e] <= hwb && cand != tru;
                        const unsigned long long m = __ballot(unc);
                        if (m) {
                            const int pos = nl + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                                           __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                            if (unc && pos < SUBn) sub[pos] = make_int2(qid, cand);
                            nl += __popcll(m);
                        }
                    }
                }
            }
        }
    }
    return 32 - __popc(smask);
}

// ---- the wave's list buffer.  A sub-list that a tile outran raises the overflow flag (the caller redoes the count on the
// next level down)
template <int SUBn>
__device__ __forceinline__ void sw_clamp_sublist(const kge_hi_stream_params &p, int lane, int &nl)
{
    if (nl > SUBn) {
        if (lane == 0) *p.overflow = 1.0f;
        nl = SUBn;
    }
}

// the one global list: the sub-lists behind ONE atomic (a returning same-address atomic per sub-list tripled the
// waves' stalls: 0.50 -> 0.55 ms per evaluate, profiles/r05/region_recheck_ab.txt)
template <int NT>
__device__ __forceinline__ void sw_flush_all(const kge_hi_stream_params &p, int lane, const int2 *wlist, int (&nl)[NT])
{
    constexpr int SUBn = SW_WLIST / NT;
    int total = 0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) total += nl[nt];
    if (total > 0) {
        int base = 0;
        if (lane == 0) base = atomicAdd(p.list_count, total);
        base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            for (int i = lane; i < nl[nt]; i += 64) {
                const int pos = base + i;
                if ((unsigned)pos < (unsigned)p.cap) reinterpret_cast<int2 *>(p.list)[pos] = wlist[nt * SUBn + i];
                else *p.overflow = 1.0f;
            }
            base += nl[nt];
            nl[nt] = 0;
        }
    }
}

// per-lane counts of a panel's sweep -> raw_count (the two k-halves of a column first)
template <int NT>
__device__ __forceinline__ void sw_flush_counts(const kge_hi_stream_params &p, int half, int (&cnt)[NT], const int (&qid)[NT])
{
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int v = cnt[nt] + __shfl_xor(cnt[nt], 32, 64);
        if (half == 0 && v != 0 && qid[nt] >= 0) atomicAdd(&p.raw_count[qid[nt]], v);
        cnt[nt] = 0;
    }
}

__device__ __forceinline__ f32x16 sw_zero16()
{
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// ---- launch of one kernel instantiation with `smem` bytes of dynamic LDS
template <auto KERNEL, int NTHREADS>
int sw_launch(const kge_hi_stream_params &p, int grid, int smem, hipStream_t s)
{
    static int attr_dev[16];    // per instantiation, per device
    if (int e = kge_ensure_dyn_smem(reinterpret_cast<const void *>(KERNEL), smem, attr_dev)) return e;
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(NTHREADS), smem, s, p);
    KGE_CHECK_LAUNCH();
    return 0;
}

} // namespace
