// The 64 x 64 skeleton behind the all-candidates training criteria (lp_xent.hip: softmax cross-entropy, lp_bce.hip:
// multi-label BCE): ONE definition of the bit-defined score tile, of the chunk arithmetic, of the statistics walk (S tile
// through LDS to a row-wise pass, one partial per (row, chunk)), of the gradient walk (recompute S, G through LDS,
// dA = G.T / dT = G^T.A on the fp32 MFMA), of the chunk sum of dA, and of the host side around them: the entries'
// shared checks and the two launch sequences.  A criterion plugs in as functors: what it keeps per row and adds per
// candidate in the statistics walk; what it loads per row panel, prepares per tile, and G(i, c) from s(i, c) in the
// gradient walk.  Nothing here branches on which criterion called it.
//
// score_tile(): the 32x32x2 fp32 MFMA loop of lp_gemm_mfma.hip in the same k-order (8-blocks ascending,
// k = 0,4,1,5,2,6,3,7 inside, segment 1 continuing segment 0's accumulator), so a score here has the bits of
// kge_lp_scores / kge_lp_pair_scores (kge_common.h: lp_chain_dot).
//
// Structure
//  * tile 64 queries x 64 candidates, 4 waves as 2 x 2 of one 32x32 MFMA tile each, BK = 32 per step; operands staged
//    global -> VGPR -> LDS (row stride 36 floats, the conflict-free b128 pattern of lp_gemm_mfma.hip), the global loads
//    of step s + 1 in flight under the MFMAs of step s.  Rows beyond B / N are clamped DUPLICATES, as there -- and
//    unlike there they would enter a sum, so every epilogue masks them;
//  * grad_walk<TR>: S tile -> G tile in LDS -> MFMA operand.  TR = false (dA = G.T): block = (row panel, chunk,
//    column slice), G rows are the MFMA's A operand, T rows come straight from global (a lane reads 32 consecutive
//    floats of one row: whole 128-byte lines, used by both 32-row halves), the partial panel goes to the workspace.
//    TR = true (dT = G^T.A): block = (candidate tile, column slice) walks all row panels, G columns are the A operand,
//    the query rows come from global, the result is stored once.  Up to 512 output columns per block: 2 x 4 MFMA tiles
//    = 128 accumulator VGPRs per lane; K0 + K1 > 512 takes a second slice (and recomputes S for it);
//  * stats_walk: block = (row panel, candidate chunk); the S tile goes through LDS in the MFMA layout to a row-wise
//    pass, 4 threads per row and 16 candidates each, candidates >= N never entering; the four threads' sums meet in LDS
//    and thread 0 of the row writes the (row, chunk) partial -- single-writer, no read-modify-write on global memory;
//  * sum_chunks: dA = the partial panels added in ascending chunk order;
//  * chunk_count / chunk_tiles: how many chunks an N-candidate problem has and which tiles chunk c walks -- the one
//    definition behind stats_walk, grad_walk and both exported kge_lp_*_chunks;
//  * setup / launch_fwd / launch_bwd: the host half of an entry (the checks in their order, the geometry, the grids).
//
// The parameter block P of a criterion carries at least: kge_lp_desc d; int chunks, col_tiles, row_panels (setup fills
// these four); float *ws_da ([chunks][B][K0 + K1]); float *o0, *o1; int64_t ldo0, ldo1 (the gradient group of the
// launch: launch_bwd fills these four).
//
// The geometry (column slices, wave tiles per slice, staging steps, the chunk partition and the chunk-sum order) is held
// to tests/tile64_table.py by tests/test_gpu_tile64_matrix.py, through both criteria.
#ifndef KGE_LP_TILE64_H
#define KGE_LP_TILE64_H

#include "kge_common.h"

#ifndef KGE_BUILD_NO_SLP
#error "build with -fno-slp-vectorize -DKGE_BUILD_NO_SLP=1 (torchkge_amd/csrc/build.py): VALU epilogues beside co-executing MFMAs (DESIGN.md 3.6)"
#endif

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace tile64 {

constexpr int BM = 64, BN = 64, BK = 32, LDS_LD = BK + 4, G_LD = BN + 1;
constexpr int NTHREADS = 256;
constexpr int KSLICE = 512;                 // gradient columns one backward block accumulates in registers
constexpr int SLICE_TILES = KSLICE / 32;    // 32-column MFMA tiles of one slice
constexpr int CT = SLICE_TILES / 4;         // ... per wave (tile 4 ct + wave)
constexpr int XG = 8;                       // MFMA steps per prefetch group of the product phase
static_assert((32 / XG) % 2 == 0, "the product phase alternates two register sets");
static_assert(BM == 64 && BN == 64, "2 x 2 waves of one 32x32 tile each");
constexpr int MIN_TILES_PER_CHUNK = 4;      // a chunk walks at least this many candidate tiles ...
constexpr int MAX_CHUNKS = 32;              // ... and there are at most this many (the workspace is bounded over N)
constexpr int MAX_K = 1024;                 // K0 + K1 of a problem: two column slices

// candidate chunks of an N-candidate problem
static inline int chunk_count(int64_t N)
{
    if (N <= 0) return 0;
    const int64_t tiles = (N + BN - 1) / BN;
    const int64_t c = (tiles + MIN_TILES_PER_CHUNK - 1) / MIN_TILES_PER_CHUNK;
    return (int)(c < MAX_CHUNKS ? c : MAX_CHUNKS);
}

// the candidate tiles [t0, t1) of chunk `chunk`
template <typename P>
__device__ __forceinline__ void chunk_tiles(const P &p, int chunk, int &t0, int &t1)
{
    t0 = (int)((int64_t)p.col_tiles * chunk / p.chunks);
    t1 = (int)((int64_t)p.col_tiles * (chunk + 1) / p.chunks);
}

// S tile (64 x 64 at (row0, col0)) of the descriptor's DOT score: this wave's 32x32 part in acc (row r of the MFMA
// layout: (r & 3) + 8 (r >> 2) + 4 half, column l31).  Block-uniform; starts and ends with LDS free for the caller.
template <bool VEC4>
__device__ __forceinline__ void score_tile(const kge_lp_desc &d, int64_t row0, int64_t col0, float *As, float *Bs,
                                           f32x16 &acc)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    const int srow = tid >> 3, spc = tid & 7;     // staging: 16-byte piece spc of rows srow, srow + 32
    int64_t ra[2], rb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ra[j] = min(row0 + srow + 32 * j, d.B - 1);
        rb[j] = min(col0 + srow + 32 * j, d.N - 1);
    }
    const int steps0 = (d.K0 + BK - 1) / BK, steps1 = (d.K1 + BK - 1) / BK, S = steps0 + steps1;
    float4 sa[2], sb[2];
    auto load_step = [&](int s) {   // unconditional loads from clamped addresses; k >= K zeroed
        const bool seg1 = s >= steps0;
        const float *A = seg1 ? d.A1 : d.A0, *T = seg1 ? d.T1 : d.T0;
        const int64_t lda = seg1 ? d.lda1 : d.lda0, ldt = seg1 ? d.ldt1 : d.ldt0;
        const int K = seg1 ? d.K1 : d.K0;
        const int k = (seg1 ? s - steps0 : s) * BK + spc * 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float *pa = A + ra[j] * lda, *pb = T + rb[j] * ldt;
            if (VEC4) {
                const int kc = k < K ? k : 0;
                float4 a = *reinterpret_cast<const float4 *>(pa + kc), b = *reinterpret_cast<const float4 *>(pb + kc);
                if (k >= K) { a = make_float4(0.f, 0.f, 0.f, 0.f); b = a; }
                sa[j] = a; sb[j] = b;
            } else {
                float a[4], b[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kc = k + e < K ? k + e : 0;
                    a[e] = pa[kc]; b[e] = pb[kc];
                    if (k + e >= K) { a[e] = 0.f; b[e] = 0.f; }
                }
                sa[j] = make_float4(a[0], a[1], a[2], a[3]);
                sb[j] = make_float4(b[0], b[1], b[2], b[3]);
            }
        }
    };
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    load_step(0);
    for (int s = 0; s < S; ++s) {
        __syncthreads();    // the previous step's (or the caller's) LDS reads are done
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            *reinterpret_cast<float4 *>(As + (srow + 32 * j) * LDS_LD + spc * 4) = sa[j];
            *reinterpret_cast<float4 *>(Bs + (srow + 32 * j) * LDS_LD + spc * 4) = sb[j];
        }
        __syncthreads();
        if (s + 1 < S) load_step(s + 1);
        const bool seg1 = s >= steps0;
        const int K = seg1 ? d.K1 : d.K0, kb = (seg1 ? s - steps0 : s) * BK;
        const int nblk = min(4, (K - kb + 7) >> 3);
        const float *Ab = As + (wr * 32 + l31) * LDS_LD + half * 4;
        const float *Bb = Bs + (wc * 32 + l31) * LDS_LD + half * 4;
        for (int blk = 0; blk < nblk; ++blk) {
            const float4 af = *reinterpret_cast<const float4 *>(Ab + blk * 8);
            const float4 bf = *reinterpret_cast<const float4 *>(Bb + blk * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, acc, 0, 0, 0);
        }
    }
}

// The body of a statistics kernel (NTHREADS threads; As / Bs: BM x LDS_LD floats each, Ss: BM x G_LD floats of LDS), block
// = (chunk, row panel).  Thread tid serves row prow = tid >> 2 of the panel and, of every tile, its candidates
// 16 pq .. 16 pq + 15 (pq = tid & 3).  The criterion functor `stat` (per-thread state allowed) provides
//   stat.start(row, in_range, col0) -- once, with the chunk's first candidate: what the thread keeps for its row;
//   stat.tile(col0)                 -- for every tile BEFORE score_tile: what it issues retires under the tile's loads;
//   stat.add(s, row, col0, c_lo, cnt) -- the thread's cnt (1..16) candidates c_lo .. of the tile, s = its row of Ss;
//   stat.publish(tid)               -- after the last tile: the thread's sums to the criterion's LDS;
//   stat.write(row, chunk, tid)     -- behind the barrier, thread pq == 0 of a row < B: the four threads' sums
//                                      (LDS slots tid .. tid + 3) reduced, the one partial of (row, chunk) written.
template <bool VEC4, typename P, typename Stat>
__device__ __forceinline__ void stats_walk(const P &p, Stat &stat, float *As, float *Bs, float *Ss)
{
    const kge_lp_desc &d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    const int chunk = blockIdx.x;
    const int64_t row0 = (int64_t)blockIdx.y * BM;
    int t0, t1;
    chunk_tiles(p, chunk, t0, t1);

    const int prow = tid >> 2, pq = tid & 3;      // row-wise pass: candidates 16 pq .. 16 pq + 15 of row prow
    const int64_t row = row0 + prow;
    stat.start(row, row < d.B, (int64_t)t0 * BN);

    for (int t = t0; t < t1; ++t) {
        const int64_t col0 = (int64_t)t * BN;
        stat.tile(col0);
        f32x16 acc;
        score_tile<VEC4>(d, row0, col0, As, Bs, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            Ss[(wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * G_LD + wc * 32 + l31] = acc[r];
        __syncthreads();
        const int nvalid = (int)min((int64_t)BN, d.N - col0), c_lo = pq * 16;
        if (c_lo < nvalid)      // candidates >= N never enter
            stat.add(Ss + prow * G_LD, row, col0, c_lo, min(16, nvalid - c_lo));
        // (the next score_tile synchronises before anything overwrites Ss)
    }
    stat.publish(tid);
    __syncthreads();
    if (pq == 0 && row < d.B) stat.write(row, chunk, tid);
}

// The body of a gradient kernel (NTHREADS threads; As / Bs: BM x LDS_LD floats each, Gs: BM x G_LD floats of LDS).
// The criterion functor `crit` (per-thread state allowed) provides
//   crit.panel(row0, col0)  -- called by every thread when the block meets a new row panel (TR: every iteration; dA:
//                              once), BEFORE the iteration's score_tile, whose barriers publish what it stores to LDS;
//   crit.tile(col0)         -- called by every thread for every tile, after panel() and before score_tile (the
//                              previous epilogue's LDS reads are behind the barrier before its product phase);
//   crit.G(rloc, cloc, col, s) -- G of row rloc of the panel, column cloc of the tile (global candidate col).
template <bool VEC4, bool TR, typename P, typename Crit>
__device__ __forceinline__ void grad_walk(const P &p, Crit &crit, float *As, float *Bs, float *Gs)
{
    const kge_lp_desc &d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    const int Ktot = d.K0 + d.K1;
    const int chunk = TR ? 0 : (int)blockIdx.x;

    // the walk: candidate tiles of the chunk (dA) or all row panels (dT)
    int it0, it1;
    if (TR) { it0 = 0; it1 = p.row_panels; }
    else chunk_tiles(p, chunk, it0, it1);
    const int64_t own0 = TR ? (int64_t)blockIdx.x * BN : (int64_t)blockIdx.y * BM;    // first candidate / row owned
    const int64_t own_n = TR ? d.N : d.B;

    // output columns: tile 4 ct + wid of the slice, column l31 of it.  X = the walked side's operand rows.
    const int j0 = (int)blockIdx.z * KSLICE;
    const float *xp[CT];
    int64_t xld[CT];
    bool xok[CT];
    int nct = 0;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int jt = j0 + (4 * ct + wid) * 32, j = jt + l31;
        if (jt < Ktot) nct = ct + 1;    // wave-uniform
        xok[ct] = j < Ktot;
        const int jc = xok[ct] ? j : 0;
        const bool s1 = jc >= d.K0;
        xp[ct] = s1 ? (TR ? d.A1 : d.T1) + (jc - d.K0) : (TR ? d.A0 : d.T0) + jc;
        xld[ct] = s1 ? (TR ? d.lda1 : d.ldt1) : (TR ? d.lda0 : d.ldt0);
    }

    f32x16 oacc[2][CT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[rt][ct][r] = 0.f;

    for (int it = it0; it < it1; ++it) {
        const int64_t row0 = TR ? (int64_t)it * BM : own0, col0 = TR ? own0 : (int64_t)it * BN;
        if (TR || it == it0) crit.panel(row0, col0);
        crit.tile(col0);
        f32x16 acc;
        score_tile<VEC4>(d, row0, col0, As, Bs, acc);   // (its barriers publish the criterion's panel / tile vectors)
        // The product phase walks the tile's 64 rows of X in groups of XG MFMA steps (2 rows each), and the global
        // loads of group g + 1 are issued before the MFMAs of group g: a lane's XG x CT dwords are in flight under
        // 2 x CT x XG MFMAs.  The first group is issued here, under the epilogue's expf work.
        const int64_t x0 = TR ? row0 : col0, xn = TR ? d.B : d.N;
        auto load_group = [&](int grp, float (&xv)[XG][CT]) {
#pragma unroll
            for (int s = 0; s < XG; ++s) {
                const int64_t xr = min(x0 + 2 * (grp * XG + s) + half, xn - 1);     // clamped duplicate: its G is zero
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const float x = xp[ct][xr * xld[ct]];
                    xv[s][ct] = xok[ct] ? x : 0.f;
                }
            }
        };
        auto mma_group = [&](int grp, const float (&xv)[XG][CT]) {
#pragma unroll
            for (int s = 0; s < XG; ++s) {
                const int kk = 2 * (grp * XG + s) + half;
                float gv[2];
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
                    gv[rt] = TR ? Gs[kk * G_LD + 32 * rt + l31] : Gs[(32 * rt + l31) * G_LD + kk];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    if (ct < nct) {
#pragma unroll
                        for (int rt = 0; rt < 2; ++rt)
                            oacc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[rt], xv[s][ct], oacc[rt][ct], 0, 0, 0);
                    }
            }
        };
        float xa[XG][CT], xb[XG][CT];
        if (nct > 0) load_group(0, xa);
        const int cloc = wc * 32 + l31;
        const int64_t col = col0 + cloc;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rloc = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const float G = crit.G(rloc, cloc, col, acc[r]);
            Gs[rloc * G_LD + cloc] = (row0 + rloc < d.B && col < d.N) ? G : 0.f;    // padded rows / columns: exact zeros
        }
        __syncthreads();
        if (nct > 0) {
#pragma unroll
            for (int grp = 0; grp < 32 / XG; grp += 2) {
                load_group(grp + 1, xb);
                mma_group(grp, xa);
                if (grp + 2 < 32 / XG) load_group(grp + 2, xa);
                mma_group(grp + 1, xb);
            }
        }
        // (the next score_tile synchronises before As / Bs change; Gs changes only after it)
    }

#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        if (!xok[ct]) continue;
        const int j = j0 + (4 * ct + wid) * 32 + l31;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t o = own0 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (o >= own_n) continue;
                if (TR) {
                    if (j < d.K0) p.o0[o * p.ldo0 + j] = oacc[rt][ct][r];
                    else p.o1[o * p.ldo1 + (j - d.K0)] = oacc[rt][ct][r];
                } else {
                    p.ws_da[((int64_t)chunk * d.B + o) * Ktot + j] = oacc[rt][ct][r];
                }
            }
    }
}

// The body of the dA finish kernel (256 threads, grid-stride): the partial panels added in ascending chunk order.
template <typename P>
__device__ __forceinline__ void sum_chunks(const P &p)
{
    const int Ktot = p.d.K0 + p.d.K1;
    const int64_t n = p.d.B * Ktot;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / Ktot;
        const int j = (int)(e - i * Ktot);
        float s = p.ws_da[e];
        for (int c = 1; c < p.chunks; ++c) s += p.ws_da[(int64_t)c * n + e];
        if (j < p.d.K0) p.o0[i * p.ldo0 + j] = s;
        else p.o1[i * p.ldo1 + (j - p.d.K0)] = s;
    }
}

static inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// rows that are 16-byte aligned with K and ld multiples of 4 are fetched in 16-byte pieces (the bits do not depend on it)
static inline bool operands_vec4(const kge_lp_desc *d)
{
    bool vec4 = (d->K0 % 4 == 0) && (d->lda0 % 4 == 0) && (d->ldt0 % 4 == 0) && kge_aligned16(d->A0) && kge_aligned16(d->T0);
    if (d->K1 > 0)
        vec4 = vec4 && (d->K1 % 4 == 0) && (d->lda1 % 4 == 0) && (d->ldt1 % 4 == 0) && kge_aligned16(d->A1) &&
               kge_aligned16(d->T1);
    return vec4;
}

// The checks every entry of a criterion makes, in their order, and the geometry of the problem.  `have_labels`: whether
// the criterion's own label pointers are all present; `ws_need`: its exported workspace-size query.  B == 0 returns
// with p.d alone filled: the launchers launch nothing for it, behind their own checks.
template <typename P>
static inline int setup(const kge_lp_desc *d, bool have_labels, float eps, void *ws, size_t ws_bytes,
                        size_t (*ws_need)(int64_t, int64_t, int, int), P &p)
{
    if (!d) return KGE_EINVAL;
    if (d->mode != KGE_LP_DOT || d->c_base != 0) return KGE_EUNSUPPORTED;
    if (int e = kge_lp_desc_check(d)) return e;
    if ((int64_t)d->K0 + d->K1 > MAX_K) return KGE_EUNSUPPORTED;
    if (d->B >= ((int64_t)1 << 31) || d->N >= ((int64_t)1 << 31) || d->B > (int64_t)65535 * BM) return KGE_EUNSUPPORTED;
    if (!(eps >= 0.f && eps <= 1.f)) return KGE_EINVAL;
    p.d = *d;
    if (d->B == 0) return 0;
    if (d->N <= 0 || !have_labels) return KGE_EINVAL;
    if (d->lda0 < d->K0 && d->B > 1) return KGE_EINVAL;
    const size_t need = ws_need(d->B, d->N, d->K0, d->K1);
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || need == 0 || ws_bytes < need) return KGE_EINVAL;
    p.chunks = chunk_count(d->N);
    p.col_tiles = (int)((d->N + BN - 1) / BN);
    p.row_panels = (int)((d->B + BM - 1) / BM);
    return 0;
}

// a criterion's kernel, as the launchers take it; of a pair, _s fetches by scalars and _v in 16-byte pieces
template <typename P>
using Kernel = void (*)(const P);

// the forward pair: the statistics of every (row panel, chunk), then one finish per row
template <typename P>
static inline int launch_fwd(Kernel<P> stats_s, Kernel<P> stats_v, Kernel<P> finish, const P &p, hipStream_t s)
{
    if (p.d.B == 0) return 0;
    const bool vec4 = operands_vec4(&p.d);
    hipLaunchKernelGGL(vec4 ? stats_v : stats_s, dim3(p.chunks, p.row_panels), dim3(NTHREADS), 0, s, p);
    KGE_CHECK_LAUNCH();
    hipLaunchKernelGGL(finish, dim3(p.row_panels), dim3(BM), 0, s, p);
    KGE_CHECK_LAUNCH();
    return 0;
}

// the backward sequence, behind the checks of its gradient groups: dT per (candidate tile, slice); dA per (chunk, row
// panel, slice) into the workspace and its chunk sum.  A group whose first pointer is null is not wanted: its kernels are
// not launched.
template <typename P>
static inline int launch_bwd(Kernel<P> dt_s, Kernel<P> dt_v, Kernel<P> da_s, Kernel<P> da_v, Kernel<P> sum, P &p, float *dA0,
                             int64_t ldda0, float *dA1, int64_t ldda1, float *dT0, int64_t lddt0, float *dT1, int64_t lddt1,
                             hipStream_t s)
{
    const kge_lp_desc *d = &p.d;
    const bool want_a = dA0 != nullptr, want_t = dT0 != nullptr;
    if ((!want_a && dA1) || (!want_t && dT1)) return KGE_EINVAL;
    if (d->K1 > 0 && ((want_a && !dA1) || (want_t && !dT1))) return KGE_EINVAL;
    if (want_a && ((ldda0 < d->K0 && d->B > 1) || (d->K1 > 0 && ldda1 < d->K1 && d->B > 1))) return KGE_EINVAL;
    if (want_t && ((lddt0 < d->K0 && d->N > 1) || (d->K1 > 0 && lddt1 < d->K1 && d->N > 1))) return KGE_EINVAL;
    if (d->B == 0) return 0;
    const bool vec4 = operands_vec4(d);
    const int slices = (d->K0 + d->K1 + KSLICE - 1) / KSLICE;
    if (want_t) {
        p.o0 = dT0; p.ldo0 = lddt0; p.o1 = dT1; p.ldo1 = lddt1;
        hipLaunchKernelGGL(vec4 ? dt_v : dt_s, dim3(p.col_tiles, 1, slices), dim3(NTHREADS), 0, s, p);
        KGE_CHECK_LAUNCH();
    }
    if (want_a) {
        p.o0 = dA0; p.ldo0 = ldda0; p.o1 = dA1; p.ldo1 = ldda1;
        hipLaunchKernelGGL(vec4 ? da_v : da_s, dim3(p.chunks, p.row_panels, slices), dim3(NTHREADS), 0, s, p);
        KGE_CHECK_LAUNCH();
        const int64_t n = d->B * (int64_t)(d->K0 + d->K1);
        hipLaunchKernelGGL(sum, dim3(grid1d(n, 256)), dim3(256), 0, s, p);
        KGE_CHECK_LAUNCH();
    }
    return 0;
}

} // namespace tile64
#endif /* KGE_LP_TILE64_H */
