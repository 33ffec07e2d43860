"""Host half of the width matrix (tests/test_gpu_width_matrix.py): the width table's buckets against the library's pure
functions, and the mode-aware choice of the fragment-major table -- no GPU."""
import torchkge_amd as tk
from torchkge_amd import _hip
from tests import width_table as wt


def test_width_table_buckets_hold_against_the_library():
    wt.verify(_hip)


def test_projection_models_keep_the_planar_table_past_the_resident_panel():
    """What decides es_frag agrees with what kge_lp_split_count accepts per mode: TransH / TransD sweep with a projection
    epilogue, which the chunked-panel kernel of 33 / 65 units does not have (KGE_EUNSUPPORTED) -- at those widths they keep
    the planar one-product kernel, while the plain-threshold models take the chunked one."""
    _hip.load_library()
    for K in wt.WIDTHS:
        if K % 8 or K > 1040:
            continue
        plain = [tk.TransEModel(K, 5, 2, 'L2'), tk.DistMultModel(K, 5, 2)]
        proj = [tk.TransHModel(K, 5, 2), tk.TransDModel(K + 8, K, 5, 2)]
        if K % 16 == 0:
            plain.append(tk.ComplExModel(K // 2, 5, 2))
        for m in plain + proj:
            assert m._lp_width() == K, (type(m).__name__, K)
            assert m._level1_stream() == wt.frag_ok(K, proj=m in proj), (type(m).__name__, K)
        assert not any(m._lp_proj_counts for m in plain) and all(m._lp_proj_counts for m in proj)
