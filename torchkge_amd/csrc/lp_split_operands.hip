// Operand preparation of the f16-split prefilter (lp_split_mfma.hip has the error analysis, lp_operand_cells.h the operand
// formats every writer here is written on): split (hi, lo) rows, planar and fragment-major hi tables, the one-pass
// candidate-table preparations, and the maxima the error bands are built from.
#include "lp_split_common.h"

namespace {

struct SplitRowsParams {
    RowSource s;
    int units_p;
    uint4 *out;
    float *cell_ss;           // optional [units_p][rows_p]: sum of squares of the cell's 16 data values (unscaled)
    const int64_t *row_index; // optional: output row r is built from source row row_index[r] of X0 / X1 / aug (gather)
};

// A block converts tiles of 16 rows x 16 k16 cells: 16 consecutive threads read one row's 1-KiB run (float4
// loads where the cell lies inside one K-segment and is 16-byte aligned) and write its 16 cells; the cells' sums of squares
// go through LDS so that the unit-major cell_ss array is written in 64-byte runs as well (a thread-per-cell store there
// touches one cache line per cell: it cost as much as the split table itself).
__global__ __launch_bounds__(256) void split_rows_kernel(const SplitRowsParams p)
{
    __shared__ float ss_s[16][17];
    float scale = (float)(1 << SPLIT_SCALE_LOG2), nmax = 0.f;
    if (p.s.nmax0) {
        nmax = *p.s.nmax0 + (p.s.nmax1 ? *p.s.nmax1 : 0.f);
        scale = split_scale(nmax);
    }
    const int K = p.s.K0 + p.s.K1;
    const int tiles_u = (p.units_p + 15) / 16;
    const int64_t n_tiles = (p.s.rows_p / 16) * tiles_u;          // rows_p is a multiple of the count kernel's tile
    const int tr_ = threadIdx.x >> 4, tu_ = threadIdx.x & 15;
    const bool vec0 = (p.s.ld0 % 4 == 0) && ((size_t)p.s.X0 & 15) == 0;
    const bool vec1 = p.s.X1 && (p.s.ld1 % 4 == 0) && ((size_t)p.s.X1 & 15) == 0 && (p.s.K0 % 4 == 0);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row = (tile / tiles_u) * 16 + tr_;
        const int u = (int)(tile % tiles_u) * 16 + tu_;
        const int64_t srow = (p.row_index && row < p.s.rows) ? p.row_index[row] : row;    // (gathered source row)
        float ss = 0.f;
        if (u < p.units_p) {
            const int k0 = u * 16;
            float xs[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) xs[e] = 0.f;
            if (row < p.s.rows) {
                if (k0 + 16 <= p.s.K0 && vec0) {
                    const float4 *src = reinterpret_cast<const float4 *>(p.s.X0 + srow * p.s.ld0 + k0);
#pragma unroll
                    for (int v = 0; v < 4; ++v) { const float4 t = src[v]; xs[4 * v] = t.x; xs[4 * v + 1] = t.y; xs[4 * v + 2] = t.z; xs[4 * v + 3] = t.w; }
                } else if (k0 >= p.s.K0 && k0 + 16 <= K && vec1) {
                    const float4 *src = reinterpret_cast<const float4 *>(p.s.X1 + srow * p.s.ld1 + (k0 - p.s.K0));
#pragma unroll
                    for (int v = 0; v < 4; ++v) { const float4 t = src[v]; xs[4 * v] = t.x; xs[4 * v + 1] = t.y; xs[4 * v + 2] = t.z; xs[4 * v + 3] = t.w; }
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int k = k0 + e;
                        if (k < p.s.K0) xs[e] = p.s.X0[srow * p.s.ld0 + k];
                        else if (k < K) xs[e] = p.s.X1[srow * p.s.ld1 + (k - p.s.K0)];
                    }
                }
            }
            Cell16 hi, lo;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = k0 + e;
                float x = xs[e];
                if (row < p.s.rows) {
                    if (k < K) ss = fmaf(x, x, ss);
                    else if (k == K && p.s.aug_mode == 1) x = p.s.aug[srow] * p.s.aug_mul;
                    else if (k == K && p.s.aug_mode == 2) x = p.s.aug_mul;
                    else if (k == K && p.s.aug_mode == 3) x = 0.25f * (sqrtf(p.s.aug[srow]) + sqrtf(nmax) * 0.00390625f);
                }
                x *= scale;
                if (row < p.s.rows && k == K && p.s.aug_mode == 3) x = fmaxf(x, 1.0f);
                _Float16 h = (_Float16)x;                   // round to nearest even
                _Float16 l = (_Float16)(x - (float)h);      // x - hi is exact in fp32
                if (row >= p.s.rows && k == K && (p.s.aug_mode == 1 || p.s.aug_mode == 4)) {
                    h = (_Float16)AUG_PAD;                  // (can never count: lp_operand_cells.h)
                    l = (_Float16)AUG_PAD;
                }
                hi.h[e] = h;
                lo.h[e] = l;
            }
            uint4 *o = cell_addr_split(p.out, row, p.units_p, u);
            o[0] = hi.v[0]; o[1] = hi.v[1]; o[2] = lo.v[0]; o[3] = lo.v[1];
        }
        if (p.cell_ss) {        // (block-uniform)
            ss_s[tu_][tr_] = ss;
            __syncthreads();
            const int u2 = (int)(tile % tiles_u) * 16 + tr_;     // this thread now stores unit u2, row tu_ of the tile
            if (u2 < p.units_p) p.cell_ss[(int64_t)u2 * p.s.rows_p + (tile / tiles_u) * 16 + tu_] = ss_s[tr_][tu_];
            __syncthreads();
        }
    }
}

// ---- one-product level: PLANAR hi operands -----------------------------------------------------------------------
// The hi operand of lp_operand_cells.h (units_p a multiple of 4: one 128-byte row segment = one stage of the LV = 1 count
// kernel), with dn2[row] = ||x - hi(x)||^2 (unscaled) and its maximum.
struct HiRowsParams {
    RowSource s;
    int units_p;
    uint4 *out;
    float *dn2;               // optional (rows)
    float *dn2max;            // optional device scalar, max folded in
    const int64_t *row_index;
    const float *nm_bmax;     // optional [2][nm_blocks]: per-block squared-norm maxima of the two segments (dot_table_norm_max_kernel)
    int nm_blocks;            //   -- every block folds them into *nmax0 / *nmax1 on its way in, block 0 stores the two scalars
    float *dn_bmax;           // optional [gridDim.x]: the blocks' residual maxima as plain stores INSTEAD of the dn2max atomic
    const float *prev_nmax;   // hi_rows_frag_kernel<true> (r06, ONE pass over the table): the two squared-norm maxima a PREVIOUS
    float *nm_out;            //   evaluation measured fix the scale; this pass's maxima per block go to nm_out[2][gridDim.x] and
                              //   the consumer (dot_query_pipeline_kernel) raises the overflow flag if they ask for another scale
    int frag;                 // 1: FRAGMENT-MAJOR output (lp_operand_cells.h), one coalesced global_load_dwordx4 per block of the
                              // free-running sweep (lp_hi_stream.hip)
};

// the squared-norm maxima a norm pass left per block -> *nmax0 / *nmax1 (split_fold_block_max2) -> (scale, nmax)
__device__ __forceinline__ float hi_rows_fold_scale(const HiRowsParams &p, float &nmax)
{
    const float2 n = split_fold_block_max2(p.nm_bmax, p.nm_blocks, const_cast<float *>(p.s.nmax0), const_cast<float *>(p.s.nmax1));
    nmax = n.x + n.y;
    return split_scale(nmax);
}

__global__ __launch_bounds__(256) void hi_rows_kernel(const HiRowsParams p)
{
    __shared__ unsigned bmax[4];
    float scale = (float)(1 << SPLIT_SCALE_LOG2), nmax = 0.f;
    if (p.nm_bmax) {        // (as query_pipeline_kernel: block maxima -> the two scalars, folded into what they hold)
        __shared__ unsigned red[8];
        unsigned m0 = 0u, m1 = 0u;
        for (int j = threadIdx.x; j < p.nm_blocks; j += 256) {
            m0 = max(m0, __float_as_uint(p.nm_bmax[j]));
            m1 = max(m1, __float_as_uint(p.nm_bmax[p.nm_blocks + j]));
        }
        for (int off = 32; off > 0; off >>= 1) {
            m0 = max(m0, (unsigned)__shfl_xor((int)m0, off, 64));
            m1 = max(m1, (unsigned)__shfl_xor((int)m1, off, 64));
        }
        if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = m0; red[4 + (threadIdx.x >> 6)] = m1; }
        __syncthreads();
        m0 = max(max(red[0], red[1]), max(red[2], red[3]));
        m1 = max(max(red[4], red[5]), max(red[6], red[7]));
        const float n0 = __uint_as_float(max(m0, __float_as_uint(*p.s.nmax0)));
        const float n1 = p.s.nmax1 ? __uint_as_float(max(m1, __float_as_uint(*p.s.nmax1))) : 0.f;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            *const_cast<float *>(p.s.nmax0) = n0;
            if (p.s.nmax1) *const_cast<float *>(p.s.nmax1) = n1;
        }
        nmax = n0 + n1;
        scale = split_scale(nmax);
    } else if (p.s.nmax0) {
        nmax = *p.s.nmax0 + (p.s.nmax1 ? *p.s.nmax1 : 0.f);
        scale = split_scale(nmax);
    }
    const float inv2 = 1.0f / (scale * scale);
    const int K = p.s.K0 + p.s.K1;
    const int tr_ = threadIdx.x >> 4, tu_ = threadIdx.x & 15;
    const bool vec0 = (p.s.ld0 % 4 == 0) && ((size_t)p.s.X0 & 15) == 0;
    const bool vec1 = p.s.X1 && (p.s.ld1 % 4 == 0) && ((size_t)p.s.X1 & 15) == 0 && (p.s.K0 % 4 == 0);
    float dmax = 0.f;
    for (int64_t r0 = (int64_t)blockIdx.x * 16; r0 < p.s.rows_p; r0 += (int64_t)gridDim.x * 16) {
        const int64_t row = r0 + tr_;
        const bool real = row < p.s.rows;
        const int64_t srow = (p.row_index && real) ? p.row_index[row] : row;
        float dn = 0.f;
        for (int u = tu_; u < p.units_p; u += 16) {
            const int k0 = u * 16;
            float xs[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) xs[e] = 0.f;
            if (real) {
                if (k0 + 16 <= p.s.K0 && vec0) {
                    const float4 *src = reinterpret_cast<const float4 *>(p.s.X0 + srow * p.s.ld0 + k0);
#pragma unroll
                    for (int v = 0; v < 4; ++v) { const float4 t = src[v]; xs[4 * v] = t.x; xs[4 * v + 1] = t.y; xs[4 * v + 2] = t.z; xs[4 * v + 3] = t.w; }
                } else if (k0 >= p.s.K0 && k0 + 16 <= K && vec1) {
                    const float4 *src = reinterpret_cast<const float4 *>(p.s.X1 + srow * p.s.ld1 + (k0 - p.s.K0));
#pragma unroll
                    for (int v = 0; v < 4; ++v) { const float4 t = src[v]; xs[4 * v] = t.x; xs[4 * v + 1] = t.y; xs[4 * v + 2] = t.z; xs[4 * v + 3] = t.w; }
                } else if (k0 < K) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int k = k0 + e;
                        if (k < p.s.K0) xs[e] = p.s.X0[srow * p.s.ld0 + k];
                        else if (k < K) xs[e] = p.s.X1[srow * p.s.ld1 + (k - p.s.K0)];
                    }
                }
            }
            Cell16 hi;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = k0 + e;
                float x = xs[e] * scale;
                _Float16 h = (_Float16)x;                   // round to nearest even
                if (real && k < K) {
                    const float d = x - (float)h;           // exact in fp32
                    dn = fmaf(d, d, dn);
                }
                if (k == K || k == K + 1) {                 // the augmentation columns
                    float a = 0.f;
                    if (real) {
                        if (p.s.aug_mode == 1) {              // L2 candidates: hi (column K) and lo (column K + 1) of -||e||^2/2
                            const float full = p.s.aug[srow] * p.s.aug_mul * scale;
                            const _Float16 fh = (_Float16)full;
                            a = k == K ? (float)fh : (float)(_Float16)(full - (float)fh);
                        } else if (p.s.aug_mode == 2) {       // L2 queries: 1 against both
                            a = p.s.aug_mul * scale;
                        } else if (p.s.aug_mode == 3 && k == K) {   // DOT queries: the guard column (see split_rows_kernel)
                            a = aug_dot_guard(sqrtf(p.s.aug[srow]), sqrtf(nmax), scale);
                        }
                    } else if ((p.s.aug_mode == 1 || (p.s.aug_mode == 4 && k == K))) {
                        a = AUG_PAD;
                    }
                    h = (_Float16)a;
                }
                hi.h[e] = h;
            }
            cell_store_hi(p.out, row, p.units_p, u, p.frag, hi);
        }
        dn += __shfl_xor(dn, 8, 64);    // the 16 lanes of a row sit in one aligned group of the wavefront
        dn += __shfl_xor(dn, 4, 64);
        dn += __shfl_xor(dn, 2, 64);
        dn += __shfl_xor(dn, 1, 64);
        dn *= inv2 * 1.0001f;           // (fp32 summation error: K * 2^-24 relative)
        if (real && tu_ == 0 && p.dn2) p.dn2[row] = dn;
        if (real) dmax = fmaxf(dmax, dn);
    }
    if (p.dn2max || p.dn_bmax) {
        unsigned m = __float_as_uint(dmax);
        for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
        if ((threadIdx.x & 63) == 0) bmax[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned mm = max(max(bmax[0], bmax[1]), max(bmax[2], bmax[3]));
            if (p.dn_bmax) p.dn_bmax[blockIdx.x] = __uint_as_float(mm);
            else kge_atomic_max_u32(reinterpret_cast<unsigned *>(p.dn2max), mm);
        }
    }
}

// ---- the same table for DOT candidates, FRAGMENT-MAJOR, with coalesced traffic on both sides (r06) -----------------------
// hi_rows_kernel reads 64 bytes per lane (a wave's float4 load touches 16 B of 64 different 64-byte pieces) and writes a
// fragment block 64 bytes at a time: at ComplEx d = 512 on 4.59 M entities it moves 28.8 GB in 8.9 ms (3.2 TB/s), the
// address pipes being the limit, not HBM.  Here a block takes a 32-row group and walks the row in spans of 256 columns:
// a wave reads 1 KiB of ONE row per instruction (lane l: columns 4 l .. 4 l + 3), converts, and leaves the f16 values in
// an LDS tile laid out like the output's fragment blocks (lp_operand_cells.h) -- [unit][k-half][row][16 B], a 16-byte pad
// per k-half block: the 16 lanes of a
// write pass hit 16 different 8-byte bank pairs -- from which every wave then copies whole 1-KiB fragment blocks to the
// table, one coalesced store per block.  Two LDS tiles, ONE barrier per span, the next span's loads in flight across it.
// Same hi values as hi_rows_kernel (aug_mode 4); the residual sums are the same exact differences in another order (a
// bound input: any order, cell_resid_finish).
// Needs float4-readable rows (K0, K1, ld % 4 == 0, 16-byte aligned bases).
constexpr int HF_HST = 512 + 16, HF_UST = 2 * HF_HST;     // LDS strides of a k-half block / a unit

// FUSED (r06): no norm pass in front -- the scale comes from the maxima of the PREVIOUS evaluation (p.prev_nmax; any power
// of two under which nothing overflows is a valid scale: the band is built from residuals measured HERE), the rows'
// squared norms are summed on the way (a bound input: any order) and their maxima left per block in p.nm_out for the
// query pipeline, which checks that they still ask for the scale that was used.
template <bool FUSED>
__global__ __launch_bounds__(256) void hi_rows_frag_kernel(const HiRowsParams p)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[2][16 * HF_UST];
    __shared__ unsigned bmax[4], nbmax[8];
    const RowSource &src = p.s;
    float nmax;
    float scale;
    if (FUSED) {
        nmax = p.prev_nmax[0] + p.prev_nmax[1];
        scale = split_scale(nmax);
    } else {       // the block maxima of dot_table_norm_max_kernel -> the two scalars (as hi_rows_kernel)
        scale = hi_rows_fold_scale(p, nmax);
    }
    const int K = src.K0 + src.K1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nspan = (p.units_p + 15) >> 4;
    const int64_t ngroups = src.rows_p >> 5;
    const int wo = (lane >> 2) * HF_UST + ((lane >> 1) & 1) * HF_HST + (lane & 1) * 8;     // this lane's 8 bytes of a tile row
    const int ro = (lane >> 5) * HF_HST + (lane & 31) * 16;                                 // this lane's chunk of a fragment block
    float4 v[8];
    float dn[8], nn0[8], nn1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) dn[j] = nn0[j] = nn1[j] = 0.f;
    float dmax = 0.f, n0max = 0.f, n1max = 0.f;
    auto load = [&](int64_t g, int s) {
        const int col = s * 256 + 4 * lane;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t row = g * 32 + wv * 8 + j;
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < src.rows && col < K)
                v[j] = col < src.K0 ? *reinterpret_cast<const float4 *>(src.X0 + row * src.ld0 + col)
                                  : *reinterpret_cast<const float4 *>(src.X1 + row * src.ld1 + (col - src.K0));
        }
    };
    int64_t g = blockIdx.x;
    int s = 0, it = 0;
    bool have = g < ngroups;
    if (have) load(g, s);
    while (have) {                      // (block-uniform)
        unsigned char *tl = tile[it & 1];
        const int col = s * 256 + 4 * lane;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool real = g * 32 + wv * 8 + j < src.rows;
            const float xs[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            if (FUSED) {        // (padding lanes hold zeros)
                const float ss = fmaf(xs[0], xs[0], fmaf(xs[1], xs[1], fmaf(xs[2], xs[2], xs[3] * xs[3])));
                if (col < src.K0) nn0[j] += ss; else nn1[j] += ss;
            }
            _Float16 h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = cell_hi(xs[e] * scale, dn[j]);   // (padding rows and columns hold zeros)
            if (col == K && !real && aug_pad_column(4, 0)) h[0] = (_Float16)AUG_PAD;   // (K % 4 == 0: column K leads its float4)
            union { _Float16 hh[4]; uint2 u; } pk;
            pk.hh[0] = h[0]; pk.hh[1] = h[1]; pk.hh[2] = h[2]; pk.hh[3] = h[3];
            *reinterpret_cast<uint2 *>(tl + wo + (wv * 8 + j) * 16) = pk.u;
        }
        int64_t g2 = g;
        int s2 = s + 1;
        if (s2 == nspan) { s2 = 0; g2 += gridDim.x; }
        const bool have2 = g2 < ngroups;
        if (have2) load(g2, s2);
        __syncthreads();                // the tile is complete; the other tile's readers of two spans ago are long past
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) {
            const int ul = wv * 4 + uu, u = s * 16 + ul;
            if (u < p.units_p)
                cell_frag_block(p.out, g, p.units_p, u)[lane] = *reinterpret_cast<const uint4 *>(tl + ul * HF_UST + ro);
        }
        if (s == nspan - 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float a = wave_sum(dn[j]);
                a = cell_resid_finish(a, scale, RESID_SAFETY);
                if (g * 32 + wv * 8 + j < src.rows) dmax = fmaxf(dmax, a);
                dn[j] = 0.f;
                if (FUSED) {
                    const float b0 = wave_sum(nn0[j]), b1 = wave_sum(nn1[j]);
                    n0max = fmaxf(n0max, b0 * RESID_SAFETY);     // (summation order: K * 2^-24 relative)
                    n1max = fmaxf(n1max, b1 * RESID_SAFETY);
                    nn0[j] = nn1[j] = 0.f;
                }
            }
        }
        g = g2; s = s2; have = have2; ++it;
    }
    unsigned m = __float_as_uint(dmax);
    if (lane == 0) { bmax[wv] = m; nbmax[wv] = __float_as_uint(n0max); nbmax[4 + wv] = __float_as_uint(n1max); }   // (wave-uniform)
    __syncthreads();
    if (threadIdx.x == 0) {
        p.dn_bmax[blockIdx.x] = __uint_as_float(max(max(bmax[0], bmax[1]), max(bmax[2], bmax[3])));
        if (FUSED) {
            p.nm_out[blockIdx.x] = __uint_as_float(max(max(nbmax[0], nbmax[1]), max(nbmax[2], nbmax[3])));
            p.nm_out[gridDim.x + blockIdx.x] = __uint_as_float(max(max(nbmax[4], nbmax[5]), max(nbmax[6], nbmax[7])));
        }
    }
}

// Squared-norm maxima of the rows of one or two tables ([Re | Im] segments of a DOT candidate table) in ONE sweep, any
// summation order (they fix the operand scale and bound the error band; no score contains them): row_sqnorm_any_kernel
// for both segments without the per-row outputs, the blocks' maxima as plain stores (bmax[2][gridDim.x]) -- the consumer
// (hi_rows_kernel, nm_bmax) reduces them: no same-address atomics, no zero-fill of the scalars.
__global__ __launch_bounds__(256) void dot_table_norm_max_kernel(const float *__restrict__ X0, int64_t ld0, int K0,
                                                                 const float *__restrict__ X1, int64_t ld1, int K1,
                                                                 int64_t rows, float *bmax_out)
{
    __shared__ unsigned wmax[8];
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
    float big0 = 0.f, big1 = 0.f;
    for (int sg = 0; sg < (X1 ? 2 : 1); ++sg) {
        const float *X = sg ? X1 : X0;
        const int64_t ld = sg ? ld1 : ld0;
        const int K = sg ? K1 : K0;
        const bool vec = (K % 4 == 0) && (ld % 4 == 0) && ((size_t)X & 15) == 0;
        float big = 0.f;
        for (int64_t r0 = (int64_t)blockIdx.x * 64; r0 < rows; r0 += (int64_t)gridDim.x * 64) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec) {
                for (int k = sub * 4; k < K; k += 64) {
                    float4 t[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) t[j] = *reinterpret_cast<const float4 *>(X + min(r0 + grp * 4 + j, rows - 1) * ld + k);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[j] = fmaf(t[j].x, t[j].x, acc[j]); acc[j] = fmaf(t[j].y, t[j].y, acc[j]);
                        acc[j] = fmaf(t[j].z, t[j].z, acc[j]); acc[j] = fmaf(t[j].w, t[j].w, acc[j]);
                    }
                }
            } else {
                for (int k = sub; k < K; k += 16)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float x = X[min(r0 + grp * 4 + j, rows - 1) * ld + k];
                        acc[j] = fmaf(x, x, acc[j]);
                    }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = acc[j];
                a += __shfl_xor(a, 8, 64); a += __shfl_xor(a, 4, 64); a += __shfl_xor(a, 2, 64); a += __shfl_xor(a, 1, 64);
                big = __uint_as_float(max(__float_as_uint(big), __float_as_uint(a)));   // (rows past the end repeat the last row)
            }
        }
        if (sg) big1 = big; else big0 = big;
    }
    const unsigned m0 = wave_max_u32(__float_as_uint(big0)), m1 = wave_max_u32(__float_as_uint(big1));
    if ((threadIdx.x & 63) == 0) { wmax[threadIdx.x >> 6] = m0; wmax[4 + (threadIdx.x >> 6)] = m1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        bmax_out[blockIdx.x] = __uint_as_float(max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
        bmax_out[gridDim.x + blockIdx.x] = __uint_as_float(max(max(wmax[4], wmax[5]), max(wmax[6], wmax[7])));
    }
}

// ---- candidate-table preparation of the L2 one-product sweep in ONE pass (r05) -----------------------------------
// What kge_row_sqnorm (en, its maximum) + a zero-fill + kge_lp_hi_rows_frag (hi table, residual maximum) do in three
// launches with the table read twice: a 256-thread block stages 16 rows in LDS; lanes 0..15 run the rows' sequential
// ||e||^2 chains (row_sqnorm_kernel's: acc = fmaf(x_k, x_k, acc), k ascending -- the score contains en, same bits)
// while all threads convert the data units to f16 hi parts (thread = row + 16 * unit: a unit's 16 rows are one 256-byte
// run of the fragment-major table) and sum their residuals; the two augmentation columns follow once en is known.
// The cells are lp_operand_cells.h's: aug_mode 1 on the fixed scale, aug = en, aug_mul = -0.5.
struct TablePrepParams {
    const float *X;
    int64_t ld, rows, rows_p;
    int K, units_p;
    float *en;                // (rows)
    float *en_max;            // device scalar, max folded in
    uint4 *out;               // fragment-major hi table
    float *dn2max;            // device scalar, max folded in
    float *block_max;         // optional [2][gridDim.x]: the blocks' two maxima as plain stores INSTEAD of the atomics -- ~900
                              // same-address device-scope atomics per scalar serialise for ~50 us at the end of the kernel
                              // (measured in situ: 65 against 14 us); the consumer (kge_lp_query_pipeline) reduces them
    int dbg;                  // env KGE_TP_DBG (timing probes, wrong results): 1 no norm chain, 2 no conversions, 4 no table reads
};

__global__ __launch_bounds__(256) void table_prep_l2_kernel(const TablePrepParams p)
{
    extern __shared__ __attribute__((aligned(16))) float tp_smem[];
    const int K = p.K, LDS_LD = ((K + 3) & ~3) + 4;         // (row stride: 16-byte aligned, 4 floats of padding)
    float *xs = tp_smem;                                    // [16][LDS_LD]
    float *dnp = xs + 16 * LDS_LD;                          // [16][17] partial residual sums
    float *ens = dnp + 16 * 17;                             // [16]
    const int tid = threadIdx.x, r = tid & 15, uu = tid >> 4;
    const float scale = (float)(1 << SPLIT_SCALE_LOG2);
    float emax_b = 0.f, dmax_b = 0.f;
    for (int64_t r0 = (int64_t)blockIdx.x * 16; r0 < p.rows_p; r0 += (int64_t)gridDim.x * 16) {
        // stage the 16 rows (rows past the table: zeros)
        const int nv = K >> 2;                              // float4 per row (K % 4 == 0, checked by the host)
        for (int idx = tid; idx < 16 * nv; idx += 256) {
            const int rr = idx / nv, c = idx - rr * nv;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r0 + rr < p.rows && !(p.dbg & 4)) v = *reinterpret_cast<const float4 *>(p.X + (r0 + rr) * p.ld + c * 4);
            *reinterpret_cast<float4 *>(xs + rr * LDS_LD + c * 4) = v;
        }
        __syncthreads();
        const int64_t row = r0 + r;
        const bool real = row < p.rows;
        if (tid < 16 && !(p.dbg & 1)) {                     // the sequential chain of ||e||^2
            const float *x = xs + r * LDS_LD;
            float acc = 0.f;
            for (int k = 0; k < K; k += 4) {
                const float4 t = *reinterpret_cast<const float4 *>(x + k);
                acc = fmaf(t.x, t.x, acc);
                acc = fmaf(t.y, t.y, acc);
                acc = fmaf(t.z, t.z, acc);
                acc = fmaf(t.w, t.w, acc);
            }
            ens[r] = acc;
            if (real) {
                p.en[row] = acc;
                emax_b = __uint_as_float(max(__float_as_uint(emax_b), __float_as_uint(acc)));
            }
        }
        // data units: hi parts + residuals (the units holding an augmentation column are finished below)
        float dn = 0.f;
        for (int u = uu; u < p.units_p; u += 16) {
            const int k0 = u * 16;
            if (k0 + 16 <= K && !(p.dbg & 2)) {
                Cell16 hi;
                const float *x = xs + r * LDS_LD + k0;
#pragma unroll
                for (int e = 0; e < 16; ++e) hi.h[e] = cell_hi(x[e] * scale, dn);
                cell_store_hi(p.out, row, p.units_p, u, true, hi);
            }
        }
        dnp[r * 17 + uu] = dn;
        __syncthreads();
        // units that straddle / follow K: data tail, the two augmentation columns (hi and lo of -||e||^2/2), zeros
        for (int u = (K >> 4) + uu; u < p.units_p; u += 16) {
            const int k0 = u * 16;
            Cell16 hi;
            float dt = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = k0 + e;
                _Float16 h = (_Float16)0.f;
                if (k < K) {
                    h = cell_hi(xs[r * LDS_LD + k] * scale, dt);
                } else if (k == K || k == K + 1) {          // (aug_mode 1)
                    _Float16 lo;
                    const _Float16 fh = cell_hi_lo(aug_l2_candidate(ens[r], -0.5f, scale), lo);
                    h = real ? (k == K ? fh : lo) : (_Float16)AUG_PAD;
                }
                hi.h[e] = h;
            }
            if (u == (K >> 4)) dnp[r * 17 + 16] = dt;           // (the one unit that may hold a data tail; always present)
            cell_store_hi(p.out, row, p.units_p, u, true, hi);
        }
        __syncthreads();
        if (tid < 16 && real) {
            float t = 0.f;
            for (int j = 0; j < 17; ++j) t += dnp[r * 17 + j];
            t = cell_resid_finish(t, scale, 1.0002f);       // (two levels of any-order fp32 sums)
            dmax_b = fmaxf(dmax_b, t);
        }
        __syncthreads();
    }
    // one store or atomic per block for each maximum (lanes 0..15 hold them, the other lanes 0)
    if (tid < 64) {
        const unsigned m0 = wave_max_u32(__float_as_uint(emax_b)), m1 = wave_max_u32(__float_as_uint(dmax_b));
        if (tid == 0) {
            if (p.block_max) {
                p.block_max[blockIdx.x] = __uint_as_float(m0);
                p.block_max[gridDim.x + blockIdx.x] = __uint_as_float(m1);
            } else {
                if (p.en_max) kge_atomic_max_u32(reinterpret_cast<unsigned *>(p.en_max), m0);
                if (p.dn2max) kge_atomic_max_u32(reinterpret_cast<unsigned *>(p.dn2max), m1);
            }
        }
    }
}

// e2pref[u] = max over rows of the squared norm of the row's first (u+1)*16 data columns: with the
// same prefix norms of a query, || q[:k] || * sqrt(e2pref) bounds every partial sum the MFMA
// accumulator holds while it works through unit u (Cauchy-Schwarz on the prefix) -- the error band
// then charges each unit with ITS magnitude instead of the full ||q|| ||e|| (about half of it).
__global__ __launch_bounds__(1024) void prefix_max_kernel(const float *__restrict__ cell_ss, int64_t rows_p, int64_t rows,
                                                          int units_p, float *e2pref)
{
    // block maxima in LDS, ONE global atomic per (block, unit): same-line atomics serialise at ~12 ns each
    __shared__ unsigned smax[128];
    const int lane = threadIdx.x & 63;
    for (int u = threadIdx.x; u < units_p; u += blockDim.x) smax[u] = 0u;
    __syncthreads();
    for (int64_t r0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane; r0 < rows;
         r0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = r0 + lane;
        float prefix = 0.f;
        for (int u = 0; u < units_p; ++u) {
            if (r < rows) prefix += cell_ss[(int64_t)u * rows_p + r];
            const unsigned m = wave_max_u32(__float_as_uint(prefix));       // sums of squares: >= 0, ordered like their bit patterns
            if (lane == 0) atomicMax(&smax[u], m);
        }
    }
    __syncthreads();
    for (int u = threadIdx.x; u < units_p; u += blockDim.x) kge_atomic_max_u32(reinterpret_cast<unsigned *>(e2pref) + u, smax[u]);
}

__global__ __launch_bounds__(256) void absmax_kernel(const float *__restrict__ x, int64_t n, float *max_io)
{
    // The maximum is taken on the BIT PATTERNS of |x| as unsigned integers: for non-negative floats that is the
    // float order, +inf sorts above every finite value and every NaN above +inf -- a NaN element therefore
    // reaches max_io as a NaN (fmaxf would skip it), and the threshold kernels that consume the scalar turn a
    // non-finite maximum into their overflow flag -> exact path (the SAD prefilter quantised a NaN
    // element to a finite value).  One atomic per block (thousands of same-address atomics serialise in the L2:
    // 96 us for 14 MB when every wave issued its own).
    __shared__ unsigned wmax[4];
    unsigned u = 0u;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        const int64_t n4 = n >> 2;
        const uint4 *x4 = reinterpret_cast<const uint4 *>(x);
        for (int64_t i = tid; i < n4; i += nth) {
            const uint4 v = x4[i];
            u = max(max(u, v.x & 0x7fffffffu), max(v.y & 0x7fffffffu, max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
        }
        for (int64_t i = (n4 << 2) + tid; i < n; i += nth) u = max(u, __float_as_uint(x[i]) & 0x7fffffffu);
    } else {
        for (int64_t i = tid; i < n; i += nth) u = max(u, __float_as_uint(x[i]) & 0x7fffffffu);
    }
    u = block_max_u32(u, wmax);
    if (threadIdx.x == 0) kge_atomic_max_u32(reinterpret_cast<unsigned *>(max_io), u);
}

// [X0 | X1] rows are float4-readable: column counts and row strides multiples of 4, 16-byte aligned bases
bool rows_vec4(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1)
{
    return K0 % 4 == 0 && K1 % 4 == 0 && ld0 % 4 == 0 && kge_aligned16(X0) && (K1 == 0 || (ld1 % 4 == 0 && kge_aligned16(X1)));
}

// Argument check of a row operand (kge_lp_split_rows: aug_mode from 0; the hi rows: from 1).  *done: nothing to do.
int row_operand_check(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1, int64_t rows, int is_query,
                      int aug_mode_min, int aug_mode, const float *aug, const void *out, bool *done)
{
    *done = false;
    if (rows < 0 || K0 <= 0 || K1 < 0 || ld0 < K0 || (K1 > 0 && ld1 < K1) || aug_mode < aug_mode_min || aug_mode > 4)
        return KGE_EINVAL;
    if (rows == 0 && is_query) { *done = true; return 0; }
    if ((rows > 0 && !X0) || (rows > 0 && K1 > 0 && !X1) || !out || ((aug_mode == 1 || aug_mode == 3) && rows > 0 && !aug))
        return KGE_EINVAL;
    return 0;
}

// The rows and the role of a table writer's input (both operand formats)
RowSource row_source(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1, int64_t rows, int is_query,
                     int aug_mode, const float *aug, float aug_mul, const float *nmax0, const float *nmax1)
{
    RowSource s;
    s.X0 = X0; s.X1 = X1; s.ld0 = ld0; s.ld1 = ld1; s.K0 = K0; s.K1 = K1;
    s.rows = rows;
    s.rows_p = kge_lp_split_rows_padded(rows, is_query);
    s.aug_mode = aug_mode; s.aug = aug; s.aug_mul = aug_mul;
    s.nmax0 = nmax0; s.nmax1 = nmax1;
    return s;
}

// A hi table of those rows; the optional inputs and outputs start out absent (null).
HiRowsParams hi_rows_params(const RowSource &s, void *out, int frag)
{
    HiRowsParams p = {};
    p.s = s;
    p.units_p = kge_lp_hi_units(s.K0 + s.K1);
    p.out = reinterpret_cast<uint4 *>(out);
    p.frag = frag;
    return p;
}

// The DOT candidate table of kge_lp_dot_table_prep / _fused (aug_mode 4), after their shared argument check
int dot_table_source(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1, int64_t rows,
                     const float *nmax0, const float *nmax1, RowSource *s)
{
    if (rows <= 0 || K0 <= 0 || K1 < 0 || ld0 < K0 || (K1 > 0 && ld1 < K1)) return KGE_EINVAL;
    if (!X0 || (K1 > 0 && !X1)) return KGE_EINVAL;
    *s = row_source(X0, ld0, K0, K1 > 0 ? X1 : nullptr, ld1, K1, rows, 0, 4, nullptr, 0.f, nmax0, K1 > 0 ? nmax1 : nullptr);
    return 0;
}

} // namespace

extern "C" int kge_lp_split_units(int K, int with_aug)
{
    return (int)round_up((K + (with_aug ? 1 : 0) + 15) / 16, 2);
}

extern "C" int64_t kge_lp_split_rows_padded(int64_t rows, int is_query) { return round_up(rows, is_query ? TQ : TC); }

extern "C" int kge_lp_split_rows(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1,
                                 int64_t rows, int is_query, int aug_mode, const float *aug, float aug_mul,
                                 const float *norm2max0, const float *norm2max1, void *out, float *cell_ss,
                                 const int64_t *row_index, kge_stream_t stream)
{
    bool done;
    const int rc = row_operand_check(X0, ld0, K0, X1, ld1, K1, rows, is_query, 0, aug_mode, aug, out, &done);
    if (rc || done) return rc;
    SplitRowsParams p;
    p.s = row_source(X0, ld0, K0, X1, ld1, K1, rows, is_query, aug_mode, aug, aug_mul, norm2max0, norm2max1);
    p.units_p = kge_lp_split_units(K0 + K1, aug_mode != 0);
    p.out = reinterpret_cast<uint4 *>(out);
    p.cell_ss = cell_ss;
    p.row_index = row_index;
    const int64_t total = (p.s.rows_p / 16) * ((p.units_p + 15) / 16);     // tiles of 16 rows x 16 cells
    if (total == 0) return 0;
    const int grid = (int)(total < 65536 ? total : 65536);
    hipLaunchKernelGGL(split_rows_kernel, dim3(grid), dim3(256), 0, kge_s(stream), p);
    KGE_CHECK_LAUNCH();
    return 0;
}

/* units of a PLANAR hi operand (one-product level): k16 units of K + 2 columns, rounded up to 4 (one 128-byte stage) */
extern "C" int kge_lp_hi_units(int K) { return (int)round_up((K + 2 + 15) / 16, 4); }

static int hi_rows_impl(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1, int64_t rows,
                        int is_query, int aug_mode, const float *aug, float aug_mul, const float *norm2max0,
                        const float *norm2max1, void *out, float *dn2, float *dn2max, const int64_t *row_index,
                        int frag, kge_stream_t stream)
{
    bool done;
    const int rc = row_operand_check(X0, ld0, K0, X1, ld1, K1, rows, is_query, 1, aug_mode, aug, out, &done);
    if (rc || done) return rc;
    HiRowsParams p = hi_rows_params(row_source(X0, ld0, K0, X1, ld1, K1, rows, is_query, aug_mode, aug, aug_mul, norm2max0,
                                               norm2max1), out, frag);
    p.dn2 = dn2; p.dn2max = dn2max; p.row_index = row_index;
    const int64_t blocks = p.s.rows_p / 16;
    if (blocks == 0) return 0;
    // every block ends with ONE same-address atomic (dn2max), and those serialise at ~20-30 ns each (measured r05 on the
    // fused table preparation: 1,824 of them cost 50 us): with a maximum to fold, two blocks per CU walk the rows
    const int64_t cap = dn2max ? 2 * (int64_t)split_num_cus() : 65536;
    hipLaunchKernelGGL(hi_rows_kernel, dim3((int)(blocks < cap ? blocks : cap)), dim3(256), 0, kge_s(stream), p);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_lp_hi_rows(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1, int64_t rows,
                              int is_query, int aug_mode, const float *aug, float aug_mul, const float *norm2max0,
                              const float *norm2max1, void *out, float *dn2, float *dn2max, const int64_t *row_index,
                              kge_stream_t stream)
{
    return hi_rows_impl(X0, ld0, K0, X1, ld1, K1, rows, is_query, aug_mode, aug, aug_mul, norm2max0, norm2max1, out, dn2,
                        dn2max, row_index, 0, stream);
}

/* the CANDIDATE operand of the free-running one-product kernel: same values, fragment-major layout (kge_split_args.es_frag) */
extern "C" int kge_lp_hi_rows_frag(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1, int64_t rows,
                                   int aug_mode, const float *aug, float aug_mul, const float *norm2max0,
                                   const float *norm2max1, void *out, float *dn2, float *dn2max, kge_stream_t stream)
{
    return hi_rows_impl(X0, ld0, K0, X1, ld1, K1, rows, 0, aug_mode, aug, aug_mul, norm2max0, norm2max1, out, dn2, dn2max,
                        nullptr, 1, stream);
}

/* blocks of the two launches of kge_lp_dot_table_prep (which = 0: norm maxima, 1: hi table) = lengths of its per-block arrays */
extern "C" int kge_lp_dot_table_prep_blocks(int64_t rows, int which)
{
    if (which == 0) { const int64_t b = (rows + 63) / 64; return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048); }
    const int64_t b = kge_lp_split_rows_padded(rows, 0) / 16;
    return (int)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

/* Candidate side of a DOT problem on the one-product level in TWO launches (r05): the squared-norm maxima of the table's one
 * or two segments in one sweep (block maxima, no atomics, no zero-fill), then the hi table (planar or fragment-major), whose
 * blocks fold those maxima into *norm2max0_io / *norm2max1_io (block 0 stores the scalars) and leave their residual maxima
 * per block in dn_block_max[kge_lp_dot_table_prep_blocks(rows, 1)] for kge_lp_dot_query_pipeline to fold into *de2max.
 * ws: 2 * kge_lp_dot_table_prep_blocks(rows, 0) floats of scratch. */
extern "C" int kge_lp_dot_table_prep(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1, int64_t rows,
                                     int frag, float *norm2max0_io, float *norm2max1_io, void *out, float *dn_block_max,
                                     float *ws, kge_stream_t stream)
{
    RowSource s;
    if (int e = dot_table_source(X0, ld0, K0, X1, ld1, K1, rows, norm2max0_io, norm2max1_io, &s)) return e;
    if ((K1 > 0 && !norm2max1_io) || !norm2max0_io || !out || !dn_block_max || !ws) return KGE_EINVAL;
    const int nb = kge_lp_dot_table_prep_blocks(rows, 0);
    hipLaunchKernelGGL(dot_table_norm_max_kernel, dim3(nb), dim3(256), 0, kge_s(stream), X0, ld0, K0,
                       K1 > 0 ? X1 : nullptr, ld1, K1, rows, ws);
    KGE_CHECK_LAUNCH();
    HiRowsParams p = hi_rows_params(s, out, frag ? 1 : 0);
    p.nm_bmax = ws; p.nm_blocks = nb; p.dn_bmax = dn_block_max;
    // fragment-major tables of float4-readable rows: the coalesced kernel; unaligned or planar ones: the general one
    if (frag && rows_vec4(X0, ld0, K0, X1, ld1, K1))
        hipLaunchKernelGGL(hi_rows_frag_kernel<false>, dim3(kge_lp_dot_table_prep_blocks(rows, 1)), dim3(256), 0, kge_s(stream), p);
    else
        hipLaunchKernelGGL(hi_rows_kernel, dim3(kge_lp_dot_table_prep_blocks(rows, 1)), dim3(256), 0, kge_s(stream), p);
    KGE_CHECK_LAUNCH();
    return 0;
}

/* The same candidate side in ONE launch and ONE pass over the table (r06): the operand scale is the one the squared-norm
 * maxima of a PREVIOUS evaluation ask for (prev_nmax[2], device; kge_lp_dot_query_pipeline keeps them), the fragment-major
 * hi table, its residual maxima per block (dn_block_max) and THIS pass's squared-norm maxima per block
 * (nm_block_max[2][kge_lp_dot_table_prep_blocks(rows, 1)]) come out; hand both arrays and prev_nmax to
 * kge_lp_dot_query_pipeline, which folds them, raises *overflow when the table has outgrown (or fallen below) the scale
 * that was used -- the caller redoes that evaluation on another path -- and stores the new maxima for the next call.
 * KGE_EINVAL unless the rows are float4-readable (K0, K1, ld % 4 == 0, 16-byte aligned): then kge_lp_dot_table_prep. */
extern "C" int kge_lp_dot_table_prep_fused(const float *X0, int64_t ld0, int K0, const float *X1, int64_t ld1, int K1,
                                           int64_t rows, const float *prev_nmax, void *out, float *dn_block_max,
                                           float *nm_block_max, kge_stream_t stream)
{
    RowSource s;
    if (int e = dot_table_source(X0, ld0, K0, X1, ld1, K1, rows, nullptr, nullptr, &s)) return e;
    if (!prev_nmax || !out || !dn_block_max || !nm_block_max) return KGE_EINVAL;
    if (!rows_vec4(X0, ld0, K0, X1, ld1, K1)) return KGE_EINVAL;
    HiRowsParams p = hi_rows_params(s, out, 1);
    p.dn_bmax = dn_block_max; p.prev_nmax = prev_nmax; p.nm_out = nm_block_max;
    hipLaunchKernelGGL(hi_rows_frag_kernel<true>, dim3(kge_lp_dot_table_prep_blocks(rows, 1)), dim3(256), 0, kge_s(stream), p);
    KGE_CHECK_LAUNCH();
    return 0;
}

/* 1 if kge_lp_split_count takes a fragment-major candidate table (es_frag = 1) for K columns on the one-product level */
extern "C" int kge_lp_hi_stream_supported(int K)
{
    const int units = (K + 2 + 15) / 16;
    return (units <= kge_hi_stream_max_units() || kge_hi_chunk_supported(units)) ? 1 : 0;
}

/* blocks of kge_lp_table_prep_l2 = length of each half of its block_max array */
extern "C" int kge_lp_table_prep_blocks(int64_t rows)
{
    const int64_t blocks = kge_lp_split_rows_padded(rows, 0) / 16;
    return (int)(blocks < 65536 ? blocks : 65536);
}

/* Candidate-table preparation of the L2 one-product sweep in one pass: en[row] = ||X[row]||^2 by kge_row_sqnorm's
 * sequential chain (same bits), *en_max_io = max(., max en), the fragment-major hi table of kge_lp_hi_rows_frag(aug_mode 1,
 * aug = en, aug_mul = -0.5) and *dn2max_io = max(., max_row ||x - hi(x)||^2) -- one launch, the table read once.
 * K % 4 == 0, ld % 4 == 0, X 16-byte aligned (else KGE_EUNSUPPORTED: use the separate entry points). */
extern "C" int kge_lp_table_prep_l2(const float *X, int64_t ld, int64_t rows, int K, float *en, float *en_max_io,
                                    void *out, float *dn2max_io, float *block_max, kge_stream_t stream)
{
    if (rows < 0 || K <= 0 || ld < K) return KGE_EINVAL;
    if (rows == 0) return 0;
    if (!X || !en || !out) return KGE_EINVAL;
    if (!rows_vec4(X, ld, K, nullptr, 0, 0) || K > 8192) return KGE_EUNSUPPORTED;
    TablePrepParams p;
    p.X = X; p.ld = ld; p.rows = rows; p.rows_p = kge_lp_split_rows_padded(rows, 0);
    p.K = K; p.units_p = kge_lp_hi_units(K);
    p.en = en; p.en_max = en_max_io; p.out = reinterpret_cast<uint4 *>(out); p.dn2max = dn2max_io;
    p.block_max = block_max;
    p.dbg = kge_env_int("KGE_TP_DBG", 0);
    const int lds_ld = ((K + 3) & ~3) + 4;
    const int smem = (16 * lds_ld + 16 * 17 + 16) * 4;
    const int64_t blocks = p.rows_p / 16;
    auto k = table_prep_l2_kernel;
    static int attr_dev[16];
    if (smem > 48 * 1024)
        if (int e = kge_ensure_dyn_smem(reinterpret_cast<const void *>(k), smem, attr_dev)) return e;
    hipLaunchKernelGGL(k, dim3((int)(blocks < 65536 ? blocks : 65536)), dim3(256), smem, kge_s(stream), p);
    KGE_CHECK_LAUNCH();
    return 0;
}

extern "C" int kge_lp_split_prefix_max(const float *cell_ss, int64_t rows, int is_query, int units_p, float *e2pref,
                                       kge_stream_t stream)
{
    if (rows < 0 || units_p <= 0) return KGE_EINVAL;
    if (rows == 0) return 0;
    if (!cell_ss || !e2pref) return KGE_EINVAL;
    const int64_t rows_p = kge_lp_split_rows_padded(rows, is_query);
    if (units_p > 128) return KGE_EINVAL;       // (K <= 2031)
    const int64_t want = (rows + 1023) / 1024;
    hipLaunchKernelGGL(prefix_max_kernel, dim3((int)(want < 512 ? want : 512)), dim3(1024), 0, kge_s(stream), cell_ss,
                       rows_p, rows, units_p, e2pref);
    KGE_CHECK_LAUNCH();
    return 0;
}

/* *max_io = max(*max_io, max_i |x[i]|)  (device scalar, non-negative; the bound on the projection gather term) */
extern "C" int kge_absmax(const float *x, int64_t n, float *max_io, kge_stream_t stream)
{
    if (n < 0 || !max_io) return KGE_EINVAL;
    if (n == 0) return 0;
    if (!x) return KGE_EINVAL;
    const int64_t want = (n + 1023) / 1024;
    const int grid = (int)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL(absmax_kernel, dim3(grid), dim3(256), 0, kge_s(stream), x, n, max_io);
    KGE_CHECK_LAUNCH();
    return 0;
}
