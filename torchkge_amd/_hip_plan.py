# -*- coding: utf-8 -*-
"""ctypes binding of the work-split queries of libkge_hip.so (include/kge_hip_plan.h): which block of the exact
all-candidates kernels (lp_gemm_mfma.hip, lp_direct.hip) walks which tiles.  Pure host arithmetic, shared with the
kernels and their launchers; no tensor, no launch, no GPU needed (``gemm_plan`` with grid 0 asks the current device for
its compute units as the launcher does, and assumes 256 without one).

The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature table of
their own because include/kge_hip.h and its ABI version do not change for them."""
from collections import namedtuple

from . import _hip
from ._hip import _vp, _i64, _int, _check

_SIGNATURES = {
    'kge_lp_gemm_plan': [_i64, _i64, _int, _vp, _vp],
    'kge_lp_gemm_flush_interval': [],
    'kge_lp_direct_plan': [_i64, _i64, _int, _vp, _vp],
}
# the constants of the header
GEMM_BM, GEMM_BN = 128, 128                     # KGE_LP_GEMM_BM, KGE_LP_GEMM_BN
DIRECT_BM_PLAIN, DIRECT_BM_AXPY = 128, 64       # KGE_LP_DIRECT_BM_PLAIN, KGE_LP_DIRECT_BM_AXPY
DIRECT_BN = 128                                 # KGE_LP_DIRECT_BN

GemmPlan = namedtuple('GemmPlan', 'row_panels col_tiles grid blocks')
DirectPlan = namedtuple('DirectPlan', 'row_panels col_tiles tiles_per_block grid blocks')


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip.bind(_SIGNATURES)


def _triples(flat, n):
    return [tuple(int(v) for v in flat[3 * i:3 * i + 3]) for i in range(n)]


def gemm_plan(B, N, grid=0):
    """kge_lp_gemm_plan: GemmPlan(row_panels, col_tiles, grid, blocks) of a (B, N) problem of an MFMA mode;
    blocks[bid] = (lid, item_begin, item_end), item = panel * col_tiles + tile.  grid 0: the launcher's own grid."""
    lib = load_library()
    dims = (_i64 * 2)()
    g = lib.kge_lp_gemm_plan(B, N, grid, dims, None)
    if g < 0:
        _check(g, 'kge_lp_gemm_plan')
    flat = (_i64 * (3 * max(g, 1)))()
    if g > 0 and lib.kge_lp_gemm_plan(B, N, g, dims, flat) != g:
        raise RuntimeError('torchkge_amd: kge_lp_gemm_plan changed its grid between two calls')
    return GemmPlan(int(dims[0]), int(dims[1]), g, _triples(flat, g))


def gemm_flush_interval():
    """kge_lp_gemm_flush_interval: tiles of one row panel between two flushes of the count kernel's 8-bit counters."""
    return int(load_library().kge_lp_gemm_flush_interval())


def direct_plan(B, N, axpy=False):
    """kge_lp_direct_plan: DirectPlan(row_panels, col_tiles, tiles_per_block, grid, blocks) of a (B, N) problem of a
    VALU mode; blocks[bid] = (row panel, tile_begin, tile_end).  Honours KGE_LP_TARGET_BLOCKS as the launchers do."""
    lib = load_library()
    plan = (_i64 * 4)()
    _check(lib.kge_lp_direct_plan(B, N, 1 if axpy else 0, plan, None), 'kge_lp_direct_plan')
    g = int(plan[3])
    flat = (_i64 * (3 * max(g, 1)))()
    again = (_i64 * 4)()
    _check(lib.kge_lp_direct_plan(B, N, 1 if axpy else 0, again, flat), 'kge_lp_direct_plan')
    if list(again) != list(plan):
        raise RuntimeError('torchkge_amd: kge_lp_direct_plan changed between two calls')
    return DirectPlan(int(plan[0]), int(plan[1]), int(plan[2]), g, _triples(flat, g))
