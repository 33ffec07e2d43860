"""Host half of the criterion-tile matrix (tests/test_gpu_tile64_matrix.py): the buckets of tests/tile64_table.py against
the published constants and the library's chunk arithmetic -- no GPU."""
import ctypes
import os
import re

from torchkge_amd import _hip, _hip_xent, _hip_bce
from torchkge_amd.csrc import build as hb
from tests import tile64_table as tt


def test_tile64_table_buckets_hold_against_the_library():
    tt.verify(_hip_xent, _hip_bce)


def test_the_restated_tile_constants_are_those_of_the_skeleton():
    """The three numbers the table restates (32-column wave tiles, 4 waves, BK = 32) and KSLICE, read from lp_tile64.h."""
    src = open(os.path.join(hb.HERE, 'lp_tile64.h')).read()

    def const(name):
        return int(re.search(r'\b%s = (\d+)\b' % name, src).group(1))

    assert const('KSLICE') == _hip_xent.KSLICE == _hip_bce.KSLICE
    assert const('BK') == tt.BK and const('NTHREADS') == 64 * tt.WAVES
    assert 'SLICE_TILES = KSLICE / %d' % tt.WT in src and 'CT = SLICE_TILES / %d' % tt.WAVES in src
    assert '(%d * ct + wid) * %d' % (tt.WAVES, tt.WT) in src


def test_every_chunk_count_up_to_the_cap_follows_the_formula():
    """kge_lp_xent_chunks / kge_lp_bce_chunks at every tile count up to past the cap, on both sides of each tile edge."""
    x = _hip_xent
    lib_x, lib_b = _hip_xent.load_library(), _hip_bce.load_library()
    assert int(lib_x.kge_lp_xent_chunks(0)) == 0 and int(lib_b.kge_lp_bce_chunks(-5)) == 0
    for T in range(1, x.MIN_TILES_PER_CHUNK * x.MAX_CHUNKS + 2 * x.MIN_TILES_PER_CHUNK + 1):
        for N in ((T - 1) * x.BN + 1, T * x.BN):
            want = min(x.MAX_CHUNKS, -(-T // x.MIN_TILES_PER_CHUNK))
            assert tt.chunks(x, N) == want == int(lib_x.kge_lp_xent_chunks(N)) == int(lib_b.kge_lp_bce_chunks(N)), N
            ct = tt.chunk_tiles(x, N)
            assert [b - a for a, b in ct] == [T * (j + 1) // want - T * j // want for j in range(want)]
            assert all(b > a for a, b in ct)


# ---------------------------------------------------------------------------
# the order of the entries' checks: argument sets with two faults each, every one answered before any launch
# ---------------------------------------------------------------------------
EINVAL, EUNSUPPORTED = -1, _hip.KGE_EUNSUPPORTED
PTR = 0x10000       # a plausible, 16-byte aligned address; no case gets as far as reading through one


def _entry_call(lib, criterion, entry, **over):
    """One raw call of kge_lp_<criterion>_<entry>: a well-formed argument set (5 x 10, K = 8, both gradient groups wanted,
    an ample workspace) with ``over`` laid over it -- descriptor fields by name, the rest by the keys below.  ``out``: the
    forward's outputs, and in the backward what it saved of them (xent: lse; bce saves nothing, so ``g`` stands in)."""
    a = dict(mode=_hip.LP_DOT, K0=8, K1=0, B=5, N=10, c_base=0, A0=PTR, lda0=8, T0=PTR, ldt0=8, A1=None, lda1=0, T1=None,
             ldt1=0, desc=True, labels=PTR, eps=0.0, out=PTR, g=PTR, dA0=PTR, ldda0=8, dA1=None, ldda1=0, dT0=PTR, lddt0=8,
             dT1=None, lddt1=0, ws=PTR, ws_bytes=1 << 40)
    assert set(over) <= set(a), over
    a.update(over)
    d = _hip.LpDesc(**{k: a[k] for k, _ in _hip.LpDesc._fields_ if k in a})
    desc = ctypes.byref(d) if a['desc'] else None
    labels = [a['labels']] * (1 if criterion == 'xent' else 3)
    grads = [a[k] for k in ('dA0', 'ldda0', 'dA1', 'ldda1', 'dT0', 'lddt0', 'dT1', 'lddt1')]
    if entry == 'fwd':
        outs = [a['out']] * (2 if criterion == 'xent' else 1)       # xent: lse, row_loss
        args = [desc] + labels + [a['eps']] + outs
    else:
        ins = [a['out'], a['g']] if criterion == 'xent' else [a['out'] and a['g']]
        args = [desc] + labels + [a['eps']] + ins + grads
    return int(getattr(lib, 'kge_lp_%s_%s' % (criterion, entry))(*(args + [a['ws'], a['ws_bytes'], None])))


# (what is wrong twice, the overrides, the code) -- the codes are those of the entries before they shared one setup
BOTH_ENTRIES = [
    ('a wrong mode with eps = 2', dict(mode=_hip.LP_L2_EXPAND, eps=2.0), EUNSUPPORTED),
    ('a null output with a wrong mode', dict(out=None, mode=_hip.LP_L2_EXPAND), EINVAL),
    ('a null descriptor with a null output', dict(desc=False, out=None), EINVAL),
    ('c_base != 0 with K0 = 0', dict(c_base=3, K0=0), EUNSUPPORTED),
    ('K0 + K1 > 1024 with a null workspace', dict(K0=1024, K1=8, A1=PTR, lda1=8, T1=PTR, ldt1=8, ws=None), EUNSUPPORTED),
    ('K1 > 0 without its operands, K0 + K1 > 1024', dict(K0=1024, K1=8), EINVAL),
    ('eps = 2 with K0 + K1 > 1024', dict(eps=2.0, K0=1025), EUNSUPPORTED),
    ('B >= 2^31 with eps = 2', dict(B=1 << 31, eps=2.0), EUNSUPPORTED),
    ('B beyond the grid with null labels', dict(B=65535 * 64 + 1, labels=None), EUNSUPPORTED),
    ('N = 0 with K0 + K1 > 1024', dict(N=0, K0=1025), EUNSUPPORTED),
    ('eps < 0 with B = 0', dict(eps=-0.5, B=0), EINVAL),
    ('eps is NaN with N = 0', dict(eps=float('nan'), N=0), EINVAL),
    ('B = 0 with null labels and a null workspace', dict(B=0, labels=None, ws=None, ws_bytes=0), 0),
    ('N = 0 with a null workspace', dict(N=0, ws=None), EINVAL),
    ('null labels with a short workspace', dict(labels=None, ws_bytes=16), EINVAL),
    ('lda0 < K0 with a misaligned workspace', dict(lda0=4, ws=PTR + 4), EINVAL),
    ('a misaligned and short workspace', dict(ws=PTR + 8, ws_bytes=16), EINVAL),
]
BWD_ONLY = [
    ('a null g with a wrong mode', dict(g=None, mode=_hip.LP_L2_EXPAND), EINVAL),
    ('a wrong mode with an unwanted group\'s second pointer', dict(mode=_hip.LP_L2_EXPAND, dA0=None, dA1=PTR), EUNSUPPORTED),
    ('a misaligned workspace with ldda0 < K0', dict(ws=PTR + 4, ldda0=4), EINVAL),
    ('a short workspace with lddt0 < K0', dict(ws_bytes=16, lddt0=4), EINVAL),
    ('an unwanted group\'s second pointer with B = 0', dict(dA0=None, dA1=PTR, B=0), EINVAL),
    ('an unwanted group\'s second pointer with B = 0 (tables)', dict(dT0=None, dT1=PTR, B=0, labels=None), EINVAL),
    ('ldda0 < K0 with B = 0', dict(ldda0=4, B=0), 0),
    ('lddt0 < K0 with B = 0', dict(lddt0=4, B=0), EINVAL),
    ('B = 0 with eps = 2 and an unwanted second pointer', dict(B=0, eps=2.0, dT0=None, dT1=PTR), EINVAL),
    ('no group wanted with ldda0 < K0: nothing to launch', dict(dA0=None, dT0=None, ldda0=4), 0),
]


def test_the_entries_answer_two_faults_at_once_in_the_order_they_always_did():
    for criterion, mod in (('xent', _hip_xent), ('bce', _hip_bce)):
        lib = mod.load_library()
        for entry in ('fwd', 'bwd'):
            for what, over, code in BOTH_ENTRIES + (BWD_ONLY if entry == 'bwd' else []):
                assert _entry_call(lib, criterion, entry, **over) == code, (criterion, entry, what)
