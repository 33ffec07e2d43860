"""Host half of the criterion-tile matrix (tests/test_gpu_tile64_matrix.py): the buckets of tests/tile64_table.py against
the published constants and the library's chunk arithmetic -- no GPU."""
import os
import re

from torchkge_amd import _hip_xent, _hip_bce
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
