"""CPU-only tests of include/kge_hip_plan.h: the work split of the exact all-candidates kernels (lp_gemm_mfma.hip,
lp_direct.hip) as pure host functions.  The kernels and their launchers call the same helpers, so what holds here holds
for every launch: each (row panel, candidate tile) is walked by exactly one block.  tests/test_gpu_exact_tile_walk.py
asserts its premises (several items per block, a panel change inside a range, a counter flush) through these functions."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.helpers import ROOT
from torchkge_amd import _hip, _hip_plan

HEADER = os.path.join(ROOT, 'include', 'kge_hip_plan.h')
ENTRIES = ['kge_lp_gemm_plan', 'kge_lp_gemm_flush_interval', 'kge_lp_direct_plan']
KNOBS = ('KGE_LP_ROUNDS', 'KGE_LP_WAVES', 'KGE_LP_TARGET_BLOCKS', 'KGE_DIRECT_SCALAR')


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------
# the header and its binding
# ---------------------------------------------------------------------------
def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_plan.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(ENTRIES) == set(_hip_plan._SIGNATURES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    for name in ENTRIES:
        assert hasattr(lib, name)
    from torchkge_amd.csrc import build as hb
    assert any(h.endswith('kge_hip_plan.h') for h in hb.HEADERS)
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    hdr = open(HEADER).read()
    for name, value in (('KGE_LP_GEMM_BM', _hip_plan.GEMM_BM), ('KGE_LP_GEMM_BN', _hip_plan.GEMM_BN),
                        ('KGE_LP_DIRECT_BM_PLAIN', _hip_plan.DIRECT_BM_PLAIN),
                        ('KGE_LP_DIRECT_BM_AXPY', _hip_plan.DIRECT_BM_AXPY), ('KGE_LP_DIRECT_BN', _hip_plan.DIRECT_BN)):
        m = re.search(r'#define %s (\d+)' % name, hdr)
        assert m and int(m.group(1)) == value, name


def test_ctypes_signatures_match_the_header_prototypes():
    protos = dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', header_text(), flags=re.S))
    assert set(protos) == set(ENTRIES)

    def kind(param):
        param = param.strip()
        if '*' in param:
            return ctypes.c_void_p
        t = param.split()
        for word, c in (('int64_t', ctypes.c_int64), ('int', ctypes.c_int)):
            if word in t:
                return c
        raise AssertionError('unparsed parameter: %r' % param)
    lib = _hip_plan.load_library()
    for name, args in _hip_plan._SIGNATURES.items():
        params = [p for p in protos[name].split(',') if p.strip() != 'void']
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            assert a is kind(prm), (name, prm)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int


def test_the_main_header_does_not_know_the_entries():
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    for name in ENTRIES:
        assert name.encode() not in raw
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


# ---------------------------------------------------------------------------
# MFMA kernel: `grid` contiguous, balanced item ranges, neighbouring ranges on one XCD
# ---------------------------------------------------------------------------
def check_gemm_split(plan, n_items, grid):
    assert plan.grid == grid == len(plan.blocks)
    assert plan.row_panels * plan.col_tiles == n_items
    by_lid = sorted(plan.blocks)
    assert [b[0] for b in by_lid] == list(range(grid))              # every range number once
    pos = 0
    for lid, begin, end in by_lid:                                  # contiguous per lid, disjoint, covering
        assert begin == pos and end >= begin, (grid, n_items, lid)
        pos = end
    assert pos == n_items
    lens = [e - b for _, b, e in by_lid]
    assert max(lens) - min(lens) <= 1, (grid, n_items)
    for xcd in range(min(8, grid)):                                 # blocks of one XCD (bid % 8): neighbouring ranges
        lids = [plan.blocks[bid][0] for bid in range(xcd, grid, 8)]
        assert lids == list(range(lids[0], lids[0] + len(lids))), (grid, xcd)


def test_gemm_ranges_partition_the_items_for_every_grid():
    BM, BN = _hip_plan.GEMM_BM, _hip_plan.GEMM_BN
    for grid in range(1, 601):
        # (row panels, column tiles): fewer items than blocks, as many, one more, a few and many times as many
        shapes = {(1, 1), (1, max(grid - 1, 1)), (1, grid), (1, grid + 1), (3, grid + 5), (1, 7 * grid + 3), (2, 501 * grid + 1)}
        for rp, ct in shapes:
            B, N = rp * BM - 58, ct * BN - 5                        # partial last panel, partial last tile
            plan = _hip_plan.gemm_plan(B, N, grid)
            assert (plan.row_panels, plan.col_tiles) == (rp, ct)
            check_gemm_split(plan, rp * ct, grid)


def test_gemm_launcher_grid_and_refusals(monkeypatch):
    lib = _hip_plan.load_library()
    BM, BN = _hip_plan.GEMM_BM, _hip_plan.GEMM_BN
    small = _hip_plan.gemm_plan(257, 1000)                          # 3 x 8 items: one block each
    assert small.grid == 24 and all(e - b == 1 for _, b, e in small.blocks)
    check_gemm_split(small, 24, 24)
    big = _hip_plan.gemm_plan(3 * BM, 4096 * BN)                    # more items than any device has block slots
    slots = big.grid
    assert 0 < slots < 3 * 4096 and slots % 2 == 0                  # 2 resident blocks per compute unit
    check_gemm_split(big, 3 * 4096, slots)
    monkeypatch.setenv('KGE_LP_ROUNDS', '3')
    assert _hip_plan.gemm_plan(3 * BM, 4096 * BN).grid == min(3 * slots, 3 * 4096)
    monkeypatch.delenv('KGE_LP_ROUNDS')
    assert _hip_plan.gemm_plan(0, 1000).grid == 0 and _hip_plan.gemm_plan(5, 0) == (1, 0, 0, [])
    for bad in ((-1, 5, 0), (5, -1, 0), (5, 5, -2), (1 << 40, 1 << 40, 0)):
        assert lib.kge_lp_gemm_plan(bad[0], bad[1], bad[2], None, None) == -1
    # 8-bit counters, at most (32x32 tiles of a wave along N) = BN / 64 increments per tile: both wave layouts
    assert _hip_plan.gemm_flush_interval() == 255 // (BN // 64) == 127
    monkeypatch.setenv('KGE_LP_WAVES', '8')
    assert _hip_plan.gemm_flush_interval() == 127


# ---------------------------------------------------------------------------
# VALU kernels: one row panel x tiles_per_block tiles per block
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('target', [1, 3, 16384])
def test_direct_plan_covers_every_tile_exactly_once(monkeypatch, target):
    monkeypatch.setenv('KGE_LP_TARGET_BLOCKS', str(target))
    BN = _hip_plan.DIRECT_BN
    for axpy in (False, True):
        BM = _hip_plan.DIRECT_BM_AXPY if axpy else _hip_plan.DIRECT_BM_PLAIN
        for B, N in ((1, 1), (70, 300), (70, 1100), (130, 1100), (200, 1100), (1000, 3000), (64, 128), (65, 129),
                     (4, 40000), (300, 2500000), (20000, 900)):
            plan = _hip_plan.direct_plan(B, N, axpy)
            rp, ct = ceil_div(B, BM), ceil_div(N, BN)
            assert (plan.row_panels, plan.col_tiles) == (rp, ct) and plan.grid == len(plan.blocks)
            seen = [[0] * ct for _ in range(rp)]
            for panel, begin, end in plan.blocks:
                assert 0 <= panel < rp and 0 <= begin < end <= ct and end - begin <= plan.tiles_per_block
                for t in range(begin, end):
                    seen[panel][t] += 1
            assert all(v == 1 for row in seen for v in row), (target, axpy, B, N)
            if target == 1:             # one block walks the whole candidate range of its panel
                assert plan.tiles_per_block == ct and plan.grid == rp
            elif rp * ct <= target:     # fewer tiles than wanted blocks: one tile each
                assert plan.tiles_per_block == 1 and plan.grid == rp * ct
            else:
                assert plan.grid <= target + rp and plan.tiles_per_block == ceil_div(ct, ceil_div(target, rp))


def test_direct_plan_empty_and_refusals():
    lib = _hip_plan.load_library()
    assert _hip_plan.direct_plan(0, 50) == (0, 0, 0, 0, []) and _hip_plan.direct_plan(50, 0, True) == (0, 0, 0, 0, [])
    buf = (ctypes.c_int64 * 4)()
    assert lib.kge_lp_direct_plan(-1, 5, 0, buf, None) == -1 and lib.kge_lp_direct_plan(5, -1, 0, buf, None) == -1
    assert lib.kge_lp_direct_plan(5, 5, 0, None, None) == -1
