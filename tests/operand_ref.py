# -*- coding: utf-8 -*-
"""numpy model of the f16 operands of the split prefilter, as torchkge_amd/csrc/lp_operand_cells.h defines them.

Two formats.  The SPLIT operand holds hi = f16(x * scale) and lo = f16(x * scale - hi) of every value, 64 bytes per k16
unit; the HI operand holds the hi parts alone, 32 bytes per unit, planar or fragment-major.  Three rules: the rounding
with its measured residual ||x - hi(x)||^2, the augmentation columns behind the K data columns (aug modes 0..4 of
kge_lp_split_rows / kge_lp_hi_rows), and the power-of-two operand scale.  Every fp32 step is taken in fp32, in the
kernels' order; tests/test_gpu_operand_cells.py compares every writer with this byte for byte.  TEST INFRASTRUCTURE."""
import numpy as np

F = np.float32
SPLIT_SCALE_LOG2 = 12
FIXED_SCALE = F(2.0 ** SPLIT_SCALE_LOG2)        # the L2 modes' operand scale (rows inside the norm guard)
PAD_VALUE = F(-65504.0)                         # hi (and lo) of a padding candidate in the column that meets the queries' guard
RESID_SAFETY = 1.0001                           # on an any-order fp32 residual sum (kge_lp_table_prep_l2: 1.0002)


def hi_lo(xs):
    """(hi, lo) as float16 of ALREADY SCALED fp32 values: hi rounds to nearest even, xs - hi is exact in fp32."""
    xs = np.asarray(xs, dtype=F)
    with np.errstate(over='ignore'):
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(F)).astype(F).astype(np.float16)
    return hi, lo


def scale_log2_frac(norm2):
    """Fractional part of log2(16384 / sqrt(norm2)): inside [0.05, 0.95] no log2f can land in another binade than numpy's."""
    v = np.log2(16384.0 / np.sqrt(np.asarray(norm2, dtype=np.float64)))
    return v - np.floor(v)


def scale_is_safe(norm2):
    f = scale_log2_frac(norm2)
    return bool(np.all((f >= 0.05) & (f <= 0.95)))


def split_scale(norm2max):
    """Power of two that puts rows of squared norm <= norm2max just inside f16 range, one binade of slack; 1.0 for a zero
    or non-finite maximum.  Scalar or array; fp32."""
    n = np.asarray(norm2max, dtype=F)
    m = np.sqrt(n).astype(np.float64)
    ok = (m > 0) & np.isfinite(m)
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.floor(np.log2(16384.0 / np.where(ok, m, 1.0))) - 1.0
    e = np.clip(e, -100.0, 100.0)
    return np.where(ok, np.ldexp(1.0, e.astype(np.int64)), 1.0).astype(F)


def guard_value(row_norm2, max_norm2, scale):
    """The DOT queries' guard column: max(0.25 * (sqrt(row norm^2) + sqrt(max norm^2) / 256) * scale, 1), fp32."""
    g = F(0.25) * (np.sqrt(np.asarray(row_norm2, dtype=F)) + np.sqrt(np.asarray(max_norm2, dtype=F)) * F(0.00390625))
    return np.maximum((g * np.asarray(scale, dtype=F)).astype(F), F(1.0))


def _scaled(X0, X1, rows_p, units_p, scale):
    """[rows_p][units_p * 16] fp32: the data columns [X0 | X1] times the scale (per row or one for all), zeros elsewhere."""
    X = np.asarray(X0, dtype=F) if X1 is None else np.concatenate([np.asarray(X0, dtype=F), np.asarray(X1, dtype=F)], axis=1)
    rows, K = X.shape
    assert rows <= rows_p and K <= units_p * 16
    xs = np.zeros((rows_p, units_p * 16), F)
    s = np.asarray(scale, dtype=F)
    with np.errstate(over='ignore'):
        xs[:rows, :K] = X * (s[:, None] if s.ndim == 1 else s)
    return xs, rows, K


def _aug_full(mode, rows, aug, aug_mul, scale, nmax):
    """The fp32 value of augmentation column K of the real rows before it is rounded (modes 1..3)."""
    if mode == 1:       # L2 candidates: aug[row] * aug_mul = -||e||^2 / 2
        return ((np.asarray(aug, dtype=F) * F(aug_mul)).astype(F) * scale).astype(F)
    if mode == 2:       # L2 queries: aug_mul = 1
        return np.full(rows, F(aug_mul) * scale, F)
    return guard_value(aug, nmax, scale)        # 3: DOT queries


def split_values(X0, X1, rows_p, units_p, mode, aug=None, aug_mul=0.0, scale=FIXED_SCALE, nmax=0.0):
    """(hi, lo) float16 [rows_p][units_p * 16] of a split operand: the augmentation value sits in column K as hi AND lo
    (mode 0: no such column; 4: zero), a padding row holds -65504 there in both halves (modes 1 and 4), zeros elsewhere."""
    xs, rows, K = _scaled(X0, X1, rows_p, units_p, scale)
    if mode in (1, 2, 3) and K < units_p * 16:
        xs[:rows, K] = _aug_full(mode, rows, aug, aug_mul, F(scale), nmax)
    hi, lo = hi_lo(xs)
    if mode in (1, 4) and K < units_p * 16:
        hi[rows:, K] = lo[rows:, K] = np.float16(PAD_VALUE)
    return hi, lo


def hi_values(X0, X1, rows_p, units_p, mode, aug=None, aug_mul=0.0, scale=FIXED_SCALE, nmax=0.0):
    """float16 [rows_p][units_p * 16] of a hi operand, TWO augmentation columns: L2 candidates (1) hi and lo of
    -||e||^2 / 2 * scale, L2 queries (2) aug_mul * scale in both, DOT queries (3) the guard column at K, DOT candidates
    (4) zero; a padding row -65504 in both (1) or in column K (4).  ``scale`` may be one value per row."""
    xs, rows, K = _scaled(X0, X1, rows_p, units_p, scale)
    assert K + 2 <= units_p * 16
    hi = hi_lo(xs)[0]
    if mode in (1, 2, 3):
        s = np.asarray(scale, dtype=F)
        a, a_lo = hi_lo(_aug_full(mode, rows, aug, aug_mul, s, nmax))
        hi[:rows, K] = a
        hi[:rows, K + 1] = a_lo if mode == 1 else (a if mode == 2 else np.float16(0))
    if mode in (1, 4):
        hi[rows:, K] = np.float16(PAD_VALUE)
    if mode == 1:
        hi[rows:, K + 1] = np.float16(PAD_VALUE)
    return hi


def residuals(X0, X1, scale=FIXED_SCALE, safety=RESID_SAFETY):
    """||x - hi(x)||^2 per row, unscaled: the exact fp32 differences, summed in float64, times 1 / scale^2 and the
    safety factor of an any-order fp32 sum."""
    rows, K = np.shape(X0)[0], np.shape(X0)[1] + (0 if X1 is None else np.shape(X1)[1])
    xs = _scaled(X0, X1, rows, (K + 15) // 16, scale)[0]
    d =(xs - hi_lo(xs)[0].astype(F)).astype(np.float64)
    s = np.asarray(scale, dtype=np.float64)
    return (d * d).sum(axis=1) / (s * s) * safety


def cell_ss(X0, X1, rows_p, units_p):
    """[units_p][rows_p]: sum of squares of the 16 data values of each cell (unscaled), float64."""
    xs, _, _ = _scaled(X0, X1, rows_p, units_p, F(1.0))
    x = xs.astype(np.float64).reshape(rows_p, units_p, 16)
    return (x * x).sum(axis=2).T.copy()


# ---- the three byte layouts -----------------------------------------------------------------------------------------
def split_bytes(hi, lo):
    """[rows_p][units_p][hi 32 B | lo 32 B]"""
    rows_p, kp = hi.shape
    cells = np.stack([hi.reshape(rows_p, kp // 16, 16), lo.reshape(rows_p, kp // 16, 16)], axis=2)
    return np.ascontiguousarray(cells).view(np.uint8).reshape(-1)


def planar_bytes(hi):
    """[rows_p][units_p][32 B]"""
    return np.ascontiguousarray(hi).view(np.uint8).reshape(-1)


def frag_bytes(hi):
    """[rows_p / 32][units_p][k-half][row % 32][16 B]: the 1-KiB block of a 32-row group and a unit holds values 0..7 of
    row l in lane l and values 8..15 in lane 32 + l (include/kge_hip.h)."""
    rows_p, kp = hi.shape
    assert rows_p % 32 == 0
    h = hi.reshape(rows_p // 32, 32, kp // 16, 2, 8).transpose(0, 2, 3, 1, 4)
    return np.ascontiguousarray(h).view(np.uint8).reshape(-1)


def planar_halves(table, rows_p, units_p, frag):
    """A one-product table (torch uint8 tensor) as [rows_p][units_p * 16] fp32 values on the CPU: the decoder of the
    planar and of the fragment-major layout."""
    import torch
    h = table.view(torch.float16)
    if frag:
        h = h.view(rows_p // 32, units_p, 2, 32, 8).permute(0, 3, 1, 2, 4)
    return h.reshape(rows_p, units_p * 16).float().cpu()
