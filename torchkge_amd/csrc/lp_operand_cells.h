// THE definition of the f16 operands of the certified split prefilter: what every writer stores and every error band of
// lp_split_common.h assumes.  Writers: split_rows_kernel, hi_rows_kernel, hi_rows_frag_kernel, table_prep_l2_kernel
// (lp_split_operands.hip), query_pipeline_kernel, dot_query_pipeline_kernel (lp_split_query.hip) and the hi path of
// lp_prep_kernel (lp_prep.hip, built WITH the SLP vectoriser: this header carries no KGE_BUILD_NO_SLP check).
// split_rows_kernel and hi_rows_kernel keep their own element loops (every other shape of them measured 1 - 10 % slower
// on DOT query rows, profiles/r11/operand_cells_ab.txt): they take the constants, the guard and the addresses from here.
// tests/operand_ref.py restates it in numpy; tests/test_gpu_operand_cells.py holds every writer to that, byte for byte.
//
// A row of K data columns [X0 | X1] is cut into k16 UNITS of 16 values (units_p per row, zero columns behind the data)
// and multiplied by a power-of-two SCALE.  Two formats:
//   SPLIT operand  64 bytes per unit: hi = f16(x * scale), lo = f16(x * scale - hi) -- [rows_p][units_p][hi 32 B | lo 32 B]
//   HI operand     32 bytes per unit: the hi parts alone, PLANAR [rows_p][units_p][32 B] or FRAGMENT-MAJOR
//                  [rows_p / 32][units_p][64 lanes][16 B]: chunk (row % 32) + 32 * k-half of the 1-KiB block of a 32-row
//                  group and a unit -- the A operand of v_mfma_f32_32x32x16_f16 in lane order
// with the measured residual ||x - hi(x)||^2 of a row (the one-product level's band is built from it), and behind the data
// the AUGMENTATION columns of the row's role (aug_mode):
//   0  none
//   1  L2 candidates: -||e||^2 / 2 = aug[row] * aug_mul.  Split operand: column K, as hi + lo like any value.  Hi operand:
//      hi in column K, lo in column K + 1 -- the norm term keeps its 2^-22 precision
//   2  L2 queries: aug_mul = 1 against it (hi operand: in both columns)
//   3  DOT queries: the guard column at K (aug[row] = ||q||^2)
//   4  DOT candidates: 0 at K
// and PADDING rows (rows .. rows_p) all zero, except candidates' (modes 1, 4): -65504 where the queries hold 1 / their guard.
#pragma once
#include "kge_common.h"

namespace {

constexpr int SPLIT_SCALE_LOG2 = 12;            // the L2 modes' fixed scale 2^12 (rows inside the evaluator's norm guard)

// power-of-two scale that puts rows of squared norm <= norm2max just inside f16 range
__device__ __forceinline__ float split_scale(float norm2max)
{
    const float m = sqrtf(norm2max);
    if (!(m > 0.f) || !(m < INFINITY)) return 1.0f;
    float e = floorf(log2f(16384.0f / m)) - 1.0f;      // one binade of slack for the roundings above
    e = fminf(fmaxf(e, -100.0f), 100.0f);
    return ldexpf(1.0f, (int)e);
}

// The rows a table writer reads and the role they play (the leading fields of SplitRowsParams / HiRowsParams).
struct RowSource {
    const float *X0, *X1;     // segment 1 optional (ComplEx: [Re | Im])
    int64_t ld0, ld1;
    int K0, K1;
    int64_t rows, rows_p;
    int aug_mode;             // see above
    const float *aug;
    float aug_mul;
    const float *nmax0, *nmax1;   // device scalars: squared-norm maxima -> scale (NULL: 2^12)
};

union Cell16 { _Float16 h[16]; uint4 v[2]; };   // the 16 f16 values of one cell half (hi or lo) of a unit
union Cell8 { _Float16 h[8]; uint4 v; };        // ... of one k-half of it

// ---- rounding -------------------------------------------------------------------------------------------------------
// hi part of an ALREADY SCALED value: round to nearest even; d = xs - hi is exact in fp32
__device__ __forceinline__ _Float16 cell_round(float xs, float &d)
{
    const _Float16 h = (_Float16)xs;
    d = xs - (float)h;
    return h;
}
// ... with the residual accumulated (zero columns add exactly nothing)
__device__ __forceinline__ _Float16 cell_hi(float xs, float &resid)
{
    float d;
    const _Float16 h = cell_round(xs, d);
    resid = fmaf(d, d, resid);
    return h;
}
// ... with the lo part
__device__ __forceinline__ _Float16 cell_hi_lo(float xs, _Float16 &lo)
{
    float d;
    const _Float16 h = cell_round(xs, d);
    lo = (_Float16)d;
    return h;
}
// ||x - hi(x)||^2 of a row from the sum of its squared scaled differences.  The sum is fp32 in any order (K * 2^-24
// relative): `safety` covers it, 1.0001 (table_prep_l2_kernel, whose sum has one more level: 1.0002).
constexpr float RESID_SAFETY = 1.0001f;
__device__ __forceinline__ float cell_resid_finish(float sum, float scale, float safety)
{
    return sum * (1.0f / (scale * scale)) * safety;
}

// ---- the augmentation columns (scaled fp32 values; cell_hi_lo / a plain conversion rounds them) ------------------------
// L2 candidates: -||e||^2 / 2 * scale
__device__ __forceinline__ float aug_l2_candidate(float aug, float aug_mul, float scale) { return aug * aug_mul * scale; }
// L2 queries: the 1 that meets it
__device__ __forceinline__ float aug_l2_query(float aug_mul, float scale) { return aug_mul * scale; }
// DOT queries' guard column, from sqrt(||q||^2) of the row and of the largest row the scale was taken from (the DOT query
// pipeline scales every row by its own norm: the row's norm twice).  It meets 0 in every real candidate and AUG_PAD in a
// padding one: a quarter of the scaled norm fits f16 beside the data, the share of the maximum and the floor of 1 keep
// the column positive for zero rows.
__device__ __forceinline__ float aug_dot_guard(float row_nrm, float max_nrm, float scale)
{
    return fmaxf(0.25f * (row_nrm + max_nrm * 0.00390625f) * scale, 1.0f);
}
// Padding candidates hold -65504 where the queries hold their 1 / guard (split operand: hi = lo = -65504): that column
// drives the accumulator below every threshold, so a padding candidate can never count (L2: <= -2 * 65504 * 2^12 against
// >= -16 * 2^24 for norm-guarded queries; DOT: <= -32752 * S_q * ||q|| against >= -16384 * S_q * ||q||).
constexpr float AUG_PAD = -65504.f;
// does column K + c of a PADDING row hold AUG_PAD?  (c = 1: the hi operand's second column)
__device__ __forceinline__ bool aug_pad_column(int aug_mode, int c) { return (aug_mode == 1 && (c == 0 || c == 1)) || (aug_mode == 4 && c == 0); }

// ---- where a cell goes ----------------------------------------------------------------------------------------------
// split operand: hi at [k-half], lo at [2 + k-half]
__device__ __forceinline__ uint4 *cell_addr_split(uint4 *out, int64_t row, int units_p, int u) { return out + (row * units_p + u) * 4; }
// planar hi operand: [k-half]; and its f16 element k of a row
__device__ __forceinline__ uint4 *cell_addr_planar(uint4 *out, int64_t row, int units_p, int u) { return out + (row * units_p + u) * 2; }
__device__ __forceinline__ _Float16 *cell_row_planar(_Float16 *out, int64_t row, int units_p) { return out + row * units_p * 16; }
// fragment-major hi operand: the 64 chunks of the block of (32-row group, unit); a row's k-halves at [0] and [32]
__device__ __forceinline__ uint4 *cell_frag_block(uint4 *out, int64_t group, int units_p, int u) { return out + ((group * units_p + u) << 6); }
__device__ __forceinline__ uint4 *cell_addr_frag(uint4 *out, int64_t row, int units_p, int u)
{
    return cell_frag_block(out, row >> 5, units_p, u) + (row & 31);
}
__device__ __forceinline__ void cell_store_hi(uint4 *out, int64_t row, int units_p, int u, bool frag, const Cell16 &hi)
{
    if (frag) {
        uint4 *o = cell_addr_frag(out, row, units_p, u);
        o[0] = hi.v[0]; o[32] = hi.v[1];
    } else {
        uint4 *o = cell_addr_planar(out, row, units_p, u);
        o[0] = hi.v[0]; o[1] = hi.v[1];
    }
}

} // namespace
