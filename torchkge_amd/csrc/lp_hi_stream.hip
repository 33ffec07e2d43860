// The one-product level of the split prefilter as FREE-RUNNING wavefronts (r05).
//
// Same arithmetic as lp_split_count_kernel<.., LV = 1> (lp_split_mfma.hip): acc = sum over the k16 units of
// hi(q) . hi(e) on v_mfma_f32_32x32x16_f16, compared with the two per-query thresholds (a_lo, a_hi); raw_count +=
// #{acc >= a_lo}, pairs inside the band go to the list that kge_lp_split_recheck re-scores exactly.  What is different
// is who waits for whom.  The r04 kernel stages both operands through a double-buffered LDS stage that all eight waves
// of the block fill and read, one barrier per stage: the two waves of a SIMD run the same phase at the same time (MFMA
// group, LDS-DMA issue, fragment wait, compare epilogue) and the matrix pipe idles through every phase but one
// (profiles/r04/lv1_stall_counters.txt: 28-34 % busy, VALU and MFMA co-executing 3.7 % of the time).  Here
//
//   * the QUERY panel (96 queries x all k16 units, 32 B per unit + 16 B row padding: conflict-free ds_read_b128) is
//     RESIDENT in LDS for a whole sweep of the candidate tiles -- loaded once per panel, read-only in between;
//   * every wave owns 64 CANDIDATE rows of the tile and reads their MFMA fragments straight from global memory into
//     registers: the candidate table is laid out FRAGMENT-MAJOR ([32-row group][k16 unit][lane][16 B], kge_lp_hi_rows
//     with frag = 1), so one global_load_dwordx4 per (32 rows, unit) is a fully coalesced 1-KiB read that lands in the
//     exact register layout of the A operand -- no LDS staging, no ds_read, no LDS-DMA for the streamed operand;
//   * hence NO barrier in the tile loop: a wave's only dependencies are its own loads (vmcnt / lgkmcnt, placed by the
//     compiler -- without LDS-DMA in the kernel hipcc's wait insertion is exact).  The waves drift apart, and while one
//     wave of a SIMD runs its compare epilogue (VALU) or waits for fragments, its partner's MFMAs have the pipe;
//   * uncertain pairs go to a per-WAVE list in LDS (ballot + mbcnt positions: no LDS atomics), flushed by the wave
//     itself; the only block-wide synchronisation is the change of the query panel.
//
// Wave tile 64 candidates x 96 queries (2 x 3 MFMA tiles, 96 accumulator VGPRs) as before; a workgroup is NW waves x 64
// rows of ONE panel: NW = 4 (256 threads, TWO workgroups per CU, panel <= 22 units) or NW = 8 (512 threads, one per CU).
#include "kge_common.h"
#ifndef KGE_BUILD_NO_SLP
#error "build with -fno-slp-vectorize -DKGE_BUILD_NO_SLP=1 (torchkge_amd/csrc/build.py): SLP-packed v_pk_fma_f32 with a lane-crossing op_sel misreads beside co-executing MFMAs (profiles/r06/slp_bisect.txt)"
#endif
#include "lp_hi_sweep.h"

namespace {

constexpr int HS_PF = 3, HS_RING = 4;           // candidate fragments: units in flight / ring slots
constexpr int HS_GS = 4;        // queries per grouped column (= kge_lp_split_group_sets(), the layout of kge_split_args.members)
// per-query LDS entries behind the wave lists -- PM: (a_lo, a_hi, p_i, z_i) + relation row per query of the panel; grouped
// columns: (a_lo, a_hi, query id, true candidate) + count per (column, member).  The kernel's layout and the launch's LDS size
constexpr int HS_ENTRY_BYTES = sizeof(float4) + sizeof(int);
constexpr int hs_entries(int tq, int gs) { return tq * (gs > 0 ? gs : 1); }

// GS > 0 (r06; PM = 0 only): the panel's 96 rows are GROUPED columns -- one query row shared by up to GS queries of the same key
// (p.members[column * GS + s], < 0: unused), which differ only in their thresholds: the matrix sweep runs once per column,
// the compare epilogue once per member (thresholds, per-member counters and the sub-tiles' pass counts live in LDS).
// NT (r06): 32-query sub-tiles per panel -- 3 (96 queries, 96 accumulator VGPRs) or 4 (128 queries, 128 accumulators: every
// candidate fragment feeds four MFMAs instead of three; PM = 0, GS = 0 only)
template <int NW, int UNITS /* 0: runtime (<= 32) */, int PM, int GS = 0, int NT = 3>
__global__ __launch_bounds__(64 * NW, 2) void lp_hi_stream_kernel(const kge_hi_stream_params p)
{
    static_assert(GS == 0 || PM == 0, "grouped columns: plain thresholds only");
    static_assert(NT == 3 || (NT == 4 && GS == 0), "128-query panels: one query per column");
    constexpr int TQn = 32 * NT, SUBn = SW_WLIST / NT;
    constexpr int NTHREADS = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int units = UNITS ? UNITS : p.units;
    const int RS = units * 32 + 16;                                 // panel row stride (bytes): (2 units + 1) chunks, odd
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    char *panel = smem;
    int2 *wlist = reinterpret_cast<int2 *>(smem + p.panel_bytes) + wid * SW_WLIST;
    float4 *pthr = reinterpret_cast<float4 *>(smem + p.panel_bytes + NW * SW_WLIST * 8);     // PM: per query of the panel
    int *prow = reinterpret_cast<int *>(pthr + hs_entries(TQn, 0));
    // GS: per (column, member) (a_lo, a_hi, query id, its true candidate) and the member's count of this panel's sweep
    [[maybe_unused]] float4 *mthr = pthr;
    [[maybe_unused]] int *mcnt = reinterpret_cast<int *>(mthr + hs_entries(TQn, GS));
    [[maybe_unused]] int npass[NT] = {};                                   // GS: compare passes of a sub-tile = its fullest column's members

    const sw_work_order<int> work(p);
    const int nitems = work.nitems;
    if (nitems <= 0) return;
    const sw_candidates<NW> cand(p, wid, lane);

    f32x16 acc[SW_MT][NT];
    f16x8 A[HS_RING][SW_MT], Bf[2][NT];
    int cnt[NT] = {};
    float alo[NT], ahi[NT];
    int qid[NT], tru[NT];                                     // query id / its true candidate (local index; -1: none)
    // This wave's LDS list: one sub-list per 32-query sub-tile of the panel (wave-uniform fill counts).  Flushed into the
    // global list -- or, with p.region_count, into the REGION of (panel, sub-tile): the exact recheck then takes a region
    // at a time with the sub-tile's 32 query rows resident in LDS (kge_lp_split_recheck_regions: half the row fetches).
    int nl[NT] = {};

    auto flush_sub = [&](int nt, int qp) __attribute__((always_inline)) {
        if (nl[nt] > 0) {
            int32_t *ctr = p.list_count;
            int2 *dst = reinterpret_cast<int2 *>(p.list);
            unsigned lim = (unsigned)p.cap;
            if (p.region_count) {
                const int reg = qp * NT + nt;
                ctr = p.region_count + reg;
                dst += (int64_t)reg * p.region_cap;
                lim = (unsigned)p.region_cap;
            }
            int base = 0;
            if (lane == 0) base = atomicAdd(ctr, nl[nt]);
            base = __builtin_amdgcn_readfirstlane(base);
            for (int i = lane; i < nl[nt]; i += 64) {
                const int pos = base + i;
                if ((unsigned)pos < lim) dst[pos] = wlist[nt * SUBn + i];
                else *p.overflow = 1.0f;
            }
            nl[nt] = 0;
        }
    };
    [[maybe_unused]] bool first_panel = true;
    auto load_panel = [&](int64_t q0) __attribute__((always_inline)) {
        // rows of the planar query operand -> LDS rows of stride RS
        const int cpr = 2 * units;                                  // 16-byte chunks per row
        const int total = TQn * cpr;
        for (int n = tid; n < total; n += NTHREADS) {
            const int row = n / cpr, c = n - row * cpr;
            // (a 128-query panel may reach past the operand's rows, padded to 96s: its last row again -- thresholds +inf)
            const uint4 v = *reinterpret_cast<const uint4 *>(p.Qh + min(q0 + row, p.q_rows - 1) * p.q_row_bytes + c * 16);
            *reinterpret_cast<uint4 *>(panel + row * RS + c * 16) = v;
        }
        if (PM) {
            if (tid < TQn) {
                int64_t q = -1;
                if (q0 + tid < p.q_rows) q = p.col_q ? (int64_t)p.col_q[q0 + tid] : q0 + tid;
                // (p_i, z_i) pre-multiplied by -2^23, the accumulators' scale (exact): the epilogue's projection term is then two
                // FMAs per element, v + x (x z' + p'), instead of fma, mul, fma (r06; one rounding fewer than before -- inside the
                // band's 9 x 2^-22 allowance for this term either way)
                float4 t4 = q >= 0 ? p.thr4[q] : make_float4(INFINITY, INFINITY, 0.f, 0.f);
                t4.z *= -8388608.0f; t4.w *= -8388608.0f;
                pthr[tid] = t4;
                prow[tid] = (int)p.r_idx[min(max(q, (int64_t)0), p.B - 1)];
            }
        }
        if constexpr (GS > 0) {
            // (called between two block barriers: thread idx owns entry idx of mthr / mcnt -- the previous panel's counts
            // leave through it before the entry is rewritten)
            for (int idx = tid; idx < TQn * GS; idx += NTHREADS) {
                if (!first_panel) {
                    const int c = mcnt[idx], oq = __float_as_int(mthr[idx].z);
                    if (c != 0 && oq >= 0) atomicAdd(&p.raw_count[oq], c);
                }
                const int64_t col = q0 + idx / GS;
                int64_t q = col < p.q_rows ? (int64_t)p.members[col * GS + (idx % GS)] : -1;
                if (q >= p.B) q = -1;
                float2 t = make_float2(INFINITY, INFINITY);
                int tr = -1;
                if (q >= 0) {
                    t = p.thr[q];
                    if (p.true_idx) tr = (int)(p.true_idx[q] - p.c_base);
                }
                mthr[idx] = make_float4(t.x, t.y, __int_as_float((int)q), __int_as_float(tr));
                mcnt[idx] = 0;
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {    // members of this lane's column -> the sub-tile's maximum (wave-uniform)
                const int64_t col = q0 + nt * 32 + l31;
                int m = 0;
                if (col < p.q_rows) {
#pragma unroll
                    for (int s = 0; s < GS; ++s) {
                        const int q = p.members[col * GS + s];
                        m += (q >= 0 && q < p.B) ? 1 : 0;
                    }
                }
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
                npass[nt] = __builtin_amdgcn_readfirstlane(m);
            }
            first_panel = false;
            return;
        }
        sw_load_thresholds<NT, PM != 0>(p, q0, l31, alo, ahi, qid, tru);
    };
    auto flush_counts = [&]() __attribute__((always_inline)) {
        if constexpr (GS > 0) return;       // (grouped columns count in LDS: mcnt, flushed by load_panel / at the end)
        sw_flush_counts<NT>(p, half, cnt, qid);
    };

    // fragment addresses inside the panel: row nt * 32 + l31, unit u, k-half `half`
    const unsigned b_lane = (unsigned)(l31 * RS + half * 16);
    auto load_B = [&](f16x8 (&dst)[NT], int u) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            dst[nt] = *reinterpret_cast<const f16x8 *>(panel + b_lane + nt * 32 * RS + u * 32);
    };
    const f32x16 zero16 = sw_zero16();

    int qp_cur, ct_cur;
    work.item(0, qp_cur, ct_cur);
    int64_t cur_q0 = (int64_t)qp_cur * TQn;
    load_panel(cur_q0);
    bool act_cur;
    const char *tp_cur = cand.tile_ptr(ct_cur, act_cur);
#pragma unroll
    for (int u = 0; u < HS_PF; ++u)
        if (u < units) cand.load_A(A[u], tp_cur, u);
    __syncthreads();
    load_B(Bf[0], 0);

    for (int it = 0; it < nitems; ++it) {
        // ---- the K sweep of one wave tile: per unit 6 MFMAs, 3 ds_read_b128 (queries of the next unit), 2 global loads
        // (candidates three units ahead) -- all register-to-register dependencies, waits placed by the compiler
        if constexpr (UNITS != 0) {
#pragma unroll
            for (int u = 0; u < UNITS; ++u) {
                if (u + 1 < UNITS) load_B(Bf[(u + 1) & 1], u + 1);
                if (u + HS_PF < UNITS) cand.load_A(A[(u + HS_PF) % HS_RING], tp_cur, u + HS_PF);
#pragma unroll
                for (int mt = 0; mt < SW_MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[u % HS_RING][mt], Bf[u & 1][nt],
                                                                            u == 0 ? zero16 : acc[mt][nt], 0, 0, 0);
                // interleave: one load behind each of the first NT + 2 MFMAs of the unit (NT query fragments, 2 candidate loads)
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
#pragma unroll
                for (int i = 0; i < NT - 2; ++i) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            }
        } else {
            // any number of units: a runtime loop over groups of four (the ring's period), guards on the tail
#pragma unroll
            for (int mt = 0; mt < SW_MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = zero16;
            for (int u0 = 0; u0 < units; u0 += HS_RING) {
#pragma unroll
                for (int j = 0; j < HS_RING; ++j) {
                    const int u = u0 + j;
                    if (u < units) {
                        if (u + 1 < units) load_B(Bf[(j + 1) & 1], u + 1);
                        if (u + HS_PF < units) cand.load_A(A[(j + HS_PF) % HS_RING], tp_cur, u + HS_PF);
#pragma unroll
                        for (int mt = 0; mt < SW_MT; ++mt)
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt)
                                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[j][mt], Bf[j & 1][nt], acc[mt][nt], 0, 0, 0);
                    }
                }
            }
        }

        // ---- the next item: its first candidate fragments fly under this tile's epilogue
        const bool more = it + 1 < nitems;
        int qp_next = qp_cur, ct_next = ct_cur;
        if (more) work.item(it + 1, qp_next, ct_next);
        bool act_next;
        const char *tp_next = cand.tile_ptr(ct_next, act_next);
        const bool switching = qp_next != qp_cur;
#pragma unroll
        for (int u = 0; u < HS_PF; ++u)
            if (u < units) cand.load_A(A[u], tp_next, u);
        if (!switching) load_B(Bf[0], 0);

        // ---- compare epilogue, one sub-tile of 32 queries at a time
        if (act_cur) {
            const int64_t c0 = cand.first_row(ct_cur);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                int2 *sub = wlist + nt * SUBn;
                if constexpr (GS > 0) {
                    // grouped columns: once per MEMBER of the column (thresholds from LDS, runtime pass count)
                    for (int s = 0; s < npass[nt]; ++s) {
                        const float4 t4 = mthr[(nt * 32 + l31) * GS + s];
                        const int qid_s = __float_as_int(t4.z), tru_s = __float_as_int(t4.w);
                        const int c = sw_compare_subtile<SUBn>(acc, nt, t4.x, sw_band_bits(t4.x, t4.y), qid_s, tru_s, (int)c0, half,
                                                               sub, nl[nt], sw_no_adjust{});
                        if (c != 0 && qid_s >= 0) atomicAdd(&mcnt[(nt * 32 + l31) * GS + s], c);
                        // (a sub-list that fills up inside the member loop leaves at once: up to GS passes append to it per tile)
                        if (nl[nt] >= SUBn / 2) {
                            sw_clamp_sublist<SUBn>(p, lane, nl[nt]);
                            sw_flush_all<NT>(p, lane, wlist, nl);
                        }
                    }
                } else if constexpr (PM != 0) {
                    // projection modes: v += x (x z' + p') (PM = 1) or y (y z' + p' - 2^24 x) (PM = 2), x = X[relation][candidate],
                    // y = yc[candidate], gathered in front of every even quad for two quads at a time (register budget)
                    const float4 t4 = pthr[nt * 32 + l31];
                    const float p_n = t4.z, z_n = t4.w;
                    const float *xrow = p.X + (int64_t)prow[nt * 32 + l31] * p.ldx + c0 + 4 * half;
                    float4 x4[4], y4[4];
                    auto project = [&](float (&vq)[4], int mt, int g4) __attribute__((always_inline)) {
                        if ((g4 & 1) == 0) {
#pragma unroll
                            for (int g = g4; g < g4 + 2; ++g) {
                                x4[g] = *reinterpret_cast<const float4 *>(xrow + mt * 32 + 8 * g);
                                if (PM == 2) y4[g] = *reinterpret_cast<const float4 *>(p.yc + c0 + 4 * half + mt * 32 + 8 * g);
                            }
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float xe = e == 0 ? x4[g4].x : (e == 1 ? x4[g4].y : (e == 2 ? x4[g4].z : x4[g4].w));
                            if (PM == 1) {
                                vq[e] = fmaf(xe, fmaf(xe, z_n, p_n), vq[e]);
                            } else {
                                const float ye = e == 0 ? y4[g4].x : (e == 1 ? y4[g4].y : (e == 2 ? y4[g4].z : y4[g4].w));
                                vq[e] = fmaf(ye, fmaf(ye, z_n, fmaf(-16777216.0f, xe, p_n)), vq[e]);
                            }
                        }
                    };
                    cnt[nt] += sw_compare_subtile<SUBn>(acc, nt, alo[nt], sw_band_bits(alo[nt], ahi[nt]), qid[nt], tru[nt], (int)c0,
                                                        half, sub, nl[nt], project);
                } else {
                    cnt[nt] += sw_compare_subtile<SUBn>(acc, nt, alo[nt], sw_band_bits(alo[nt], ahi[nt]), qid[nt], tru[nt], (int)c0,
                                                        half, sub, nl[nt], sw_no_adjust{});
                }
            }
        }

        // the list buffer: a tile that outran it raises the overflow flag (the caller redoes the count on the next level down);
        // flushed while >= 2/3 of it is free for the next tile (a density of 4 % of the tile's pairs: UNC_CAP's)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) sw_clamp_sublist<SUBn>(p, lane, nl[nt]);
        if (p.region_count) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                if (nl[nt] >= SUBn / 3 || switching) flush_sub(nt, qp_cur);   // (a region belongs to ONE panel)
        } else {
            int nl_max = 0;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) nl_max = max(nl_max, nl[nt]);
            if (nl_max >= SUBn / 3) sw_flush_all<NT>(p, lane, wlist, nl);
        }

        // ---- query panel change (block-uniform): the only block-wide synchronisation of the sweep
        if (switching) {
            flush_counts();
            __syncthreads();                    // every wave is done reading the old panel
            cur_q0 = (int64_t)qp_next * TQn;
            load_panel(cur_q0);
            __syncthreads();
            load_B(Bf[0], 0);
        }
        qp_cur = qp_next; ct_cur = ct_next; tp_cur = tp_next; act_cur = act_next;
    }
    flush_counts();
    if constexpr (GS > 0) {
        __syncthreads();        // every wave's LDS counts of the last panel are in
        for (int idx = tid; idx < TQn * GS; idx += NTHREADS) {
            const int c = mcnt[idx], oq = __float_as_int(mthr[idx].z);
            if (c != 0 && oq >= 0) atomicAdd(&p.raw_count[oq], c);
        }
    }
    if (p.region_count) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) flush_sub(nt, qp_cur);
    } else {
        sw_flush_all<NT>(p, lane, wlist, nl);
    }
}

constexpr int HS_NT_DEFAULT = 4;

template <int NW, int PM, int GS, int NT>
int hs_launch_units(const kge_hi_stream_params &p, int grid, int smem, hipStream_t s)
{
    if (p.units == 13) return sw_launch<lp_hi_stream_kernel<NW, 13, PM, GS, NT>, 64 * NW>(p, grid, smem, s);
    if (p.units == 26) return sw_launch<lp_hi_stream_kernel<NW, 26, PM, GS, NT>, 64 * NW>(p, grid, smem, s);
    return sw_launch<lp_hi_stream_kernel<NW, 0, PM, GS, NT>, 64 * NW>(p, grid, smem, s);
}

template <int NW, int PM>
int hs_dispatch(const kge_hi_stream_params &p, int grid, int smem, int nt, hipStream_t s)
{
    if constexpr (PM == 0) {
        if (nt == 4) return hs_launch_units<NW, 0, 0, 4>(p, grid, smem, s);            // 128-query panels, one query per column
        if (p.members) return hs_launch_units<NW, 0, HS_GS, 3>(p, grid, smem, s);      // grouped columns
    } else if (nt == 4 || p.members) {
        return KGE_EUNSUPPORTED;        // (plain thresholds only: checked by kge_hi_stream_launch)
    }
    return hs_launch_units<NW, PM, 0, 3>(p, grid, smem, s);
}

} // namespace

int kge_hi_stream_max_units(void) { return 32; }

// p.units, p.units_p, p.rows_p, p.B, pointers filled by the caller (kge_lp_split_count); this fills the work order
int kge_hi_stream_launch(kge_hi_stream_params p, int pm, int num_cus, hipStream_t s)
{
    if (p.units <= 0 || p.units > 32 || p.rows_p % 64 != 0 || p.rows_p < 64) return KGE_EINVAL;
    if (p.members && (pm != 0 || p.col_q || p.region_count)) return KGE_EINVAL;
    const int RS = p.units * 32 + 16;
    // (r06) 128-query panels for plain thresholds, one query per column: every candidate fragment feeds four MFMAs instead of three
    // (KGE_HS_NT=3: the 96-query panels of r05)
    const int nt = (pm == 0 && !p.members &&
                    kge_env_int("KGE_HS_NT", HS_NT_DEFAULT) == 4 &&
                    128 * RS + 8 * SW_WLIST * 8 + hs_entries(128, 0) * HS_ENTRY_BYTES <= 160 * 1024) ? 4 : 3;
    const int tq = 32 * nt;
    p.panel_bytes = (tq * RS + 15) / 16 * 16;
    // two 4-wave workgroups per CU while two panels (+ lists) fit the LDS; else one 8-wave workgroup
    const int extra = hs_entries(tq, p.members ? HS_GS : 0) * HS_ENTRY_BYTES;
    const int smem4 = p.panel_bytes + 4 * SW_WLIST * 8 + extra, smem8 = p.panel_bytes + 8 * SW_WLIST * 8 + extra;
    int nw = 2 * smem4 <= 160 * 1024 - 2048 ? 4 : 8;
    const int force = kge_env_int("KGE_HS_WAVES", 0);
    if (force == 4 && smem4 <= 160 * 1024) nw = 4;
    if (force == 8) nw = 8;
    if (nw == 8 && smem8 > 160 * 1024) return KGE_EUNSUPPORTED;
    const int tile_rows = nw * SW_WROWS;
    p.q_panels = (int)((p.q_rows + tq - 1) / tq);
    p.c_tiles = (int)((p.rows_p + tile_rows - 1) / tile_rows);
    p.n_items = (int64_t)p.q_panels * p.c_tiles;
    if (p.n_items == 0) return 0;
    const int per_cu = nw == 4 ? 2 : 1;
    const int64_t slots = (int64_t)num_cus * per_cu;
    int grid = (int)(p.n_items < slots ? p.n_items : slots);
    // panels interleaved under one candidate sweep: the largest power of two (<= 64) dividing the blocks per XCD, so that
    // a block keeps its panel for a whole sweep; small launches run panel-major
    p.qg = 1;
    if (grid >= 8 && p.n_items >= slots) {
        grid -= grid % 8;
        const int nbx = grid / 8;
        while (p.qg < 64 && nbx % (p.qg * 2) == 0) p.qg *= 2;
        const int cap_qg = kge_env_int("KGE_HS_QG", 64);
        while (p.qg > cap_qg && p.qg > 1) p.qg /= 2;
    }
    const int smem = nw == 4 ? smem4 : smem8;
    if (nw == 4) {
        if (pm == 1) return hs_dispatch<4, 1>(p, grid, smem, nt, s);
        if (pm == 2) return hs_dispatch<4, 2>(p, grid, smem, nt, s);
        return hs_dispatch<4, 0>(p, grid, smem, nt, s);
    }
    if (pm == 1) return hs_dispatch<8, 1>(p, grid, smem, nt, s);
    if (pm == 2) return hs_dispatch<8, 2>(p, grid, smem, nt, s);
    return hs_dispatch<8, 0>(p, grid, smem, nt, s);
}
