"""CPU-only tests of the data-redundancy analytics (torchkge/utils/data_redundancy.py): the numpy restatement of
tests/redundancy_ref.py against every array the real reference recorded (tests/golden/ref_redundancy.npz), the module
path and the five reference signatures, the export and ctypes signatures of include/kge_hip_redundancy.h, the untouched
include/kge_hip.h, and the two refusals that come before any device work."""
import ctypes
import hashlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import ROOT
from tests import redundancy_ref as rd

HEADER = os.path.join(ROOT, 'include', 'kge_hip_redundancy.h')
NEW = ('kge_relation_overlap', 'kge_relation_stats', 'kge_overlap_select')
WS = ('kge_relation_overlap_ws_bytes', 'kge_relation_stats_ws_bytes', 'kge_overlap_select_ws_bytes')
# sha256 of include/kge_hip.h as the parent commit has it: nothing of it changes for these entry points
KGE_HIP_H_SHA256 = '1d27fe190e8113e167cb0ae9d5108c0a08ab6569765f853cc884e29f00462b4c'

# the reference's five names: parameter names and defaults, written out (torchkge v0.17.7)
REFERENCE_SIGNATURES = {
    'concat_kgs': [('kg_tr', None), ('kg_val', None), ('kg_te', None)],
    'get_pairs': [('kg', None), ('r', None), ('type', 'ht')],
    'count_triplets': [('kg1', None), ('kg2', None), ('duplicates', None), ('rev_duplicates', None)],
    'duplicates': [('kg_tr', None), ('kg_val', None), ('kg_te', None), ('theta1', 0.8), ('theta2', 0.8), ('verbose', False),
                   ('counts', False), ('reverses', None)],
    'cartesian_product_relations': [('kg_tr', None), ('kg_val', None), ('kg_te', None), ('theta', 0.8)],
}
NO_DEFAULT = {('get_pairs', 'type'), ('duplicates', 'theta1'), ('duplicates', 'theta2'), ('duplicates', 'verbose'),
              ('duplicates', 'counts'), ('duplicates', 'reverses'), ('cartesian_product_relations', 'theta')}


def pairs(a):
    return [tuple(p) for p in np.asarray(a).tolist()]


# ---------------------------------------------------------------------------------------------------------------
# the restatement is pinned to the real reference
# ---------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_generator_promises():
    z = rd.fixture()
    tr, val, te = rd.fixture_graphs()
    assert (int(z['n_ent']), int(z['n_rel'])) == (48, 1345) and len(tr) + len(val) + len(te) == 6073
    h, t, r = rd.concat_kgs(tr, val, te)
    assert set(r.tolist()) == set(range(1345))                  # the reference needs every relation to hold a fact
    assert int((h == t).sum()) >= 12                            # self-loops
    assert len(np.unique((h * 48 + t) * 1345 + r)) < len(h)     # facts repeated across the splits
    assert len(z['dup_08_08']) > 0 and len(z['rev_08_08']) > 0 and len(z['rev_08_08_reverses']) < len(z['rev_08_08'])
    assert z['train_heads'].dtype == np.int32 and os.path.getsize(os.path.join(rd.GOLDEN, 'ref_redundancy.npz')) < 200 * 1024
    # a pair whose two ratios equal 0.8 exactly is recorded as NOT selected
    lengths = rd.stats(h, t, r, 48, 1345)[0]
    same, rev = rd.overlap((h, t, r), None, 48, 1345)
    on = [(a, b) for m in (same, rev) for a, b in zip(*np.nonzero(np.triu(m, 1)))
          if m[a, b] / lengths[a] == 0.8 and m[a, b] / lengths[b] == 0.8]
    assert on and not (set(on) & (set(pairs(z['dup_08_08'])) | set(pairs(z['rev_08_08']))))


def test_restatement_reproduces_every_recorded_list():
    z = rd.fixture()
    kgs = rd.fixture_graphs()
    dup, rev = rd.duplicates(*kgs)
    assert dup == pairs(z['dup_08_08']) and rev == pairs(z['rev_08_08'])
    dup2, rev2 = rd.duplicates(*kgs, theta1=0.5, theta2=0.9)
    assert dup2 == pairs(z['dup_05_09']) and rev2 == pairs(z['rev_05_09'])
    dup3, rev3 = rd.duplicates(*kgs, reverses=pairs(z['reverses']))
    assert dup3 == pairs(z['dup_08_08_reverses']) and rev3 == pairs(z['rev_08_08_reverses'])
    assert rd.cartesian_product_relations(*kgs, theta=0.8) == z['cart_08'].tolist()
    assert rd.cartesian_product_relations(*kgs, theta=0.5) == z['cart_05'].tolist()
    for nm, (k1, k2) in (('train_train', (kgs[0], kgs[0])), ('train_test', (kgs[0], kgs[2])), ('test_test', (kgs[2], kgs[2]))):
        assert list(rd.count_triplets(k1, k2, dup, rev)) == z['count_' + nm].tolist(), nm


def test_restatement_matrices_equal_python_sets_on_a_small_graph():
    """same / rev against the definition, by sets: self-loops, (a, b) with (b, a) in one relation, repeats, an empty relation."""
    rng = np.random.RandomState(3)
    n_ent, n_rel = 6, 5
    h, t, r = rng.randint(0, n_ent, 90), rng.randint(0, n_ent, 90), rng.randint(0, n_rel - 1, 90)      # relation 4 is empty
    g = rd.Graph(h, t, r, n_ent, n_rel)
    T = [rd.get_pairs(g, i) for i in range(n_rel)]
    Ti = [rd.get_pairs(g, i, type='th') for i in range(n_rel)]
    same, rev = rd.overlap((h, t, r), None, n_ent, n_rel)
    assert same.tolist() == [[len(T[a] & T[b]) for b in range(n_rel)] for a in range(n_rel)]
    assert rev.tolist() == [[len(T[a] & Ti[b]) for b in range(n_rel)] for a in range(n_rel)]
    assert rev.diagonal().sum() > 0 and np.array_equal(rev, rev.T) and same[4].sum() == 0
    st = rd.stats(h, t, r, n_ent, n_rel)
    assert st[0].tolist() == [int((r == i).sum()) for i in range(n_rel)] and st[0].sum() > same.diagonal().sum()
    assert st[1].tolist() == [len(set(h[r == i].tolist())) for i in range(n_rel)]
    assert st[2].tolist() == [len(set(t[r == i].tolist())) for i in range(n_rel)]
    # rectangular: A = first half, B = second half
    a, b = (h[:45], t[:45], r[:45]), (h[45:], t[45:], r[45:])
    ga, gb = rd.Graph(*a, n_ent, n_rel), rd.Graph(*b, n_ent, n_rel)
    same, rev = rd.overlap(a, b, n_ent, n_rel)
    assert same.tolist() == [[len(rd.get_pairs(ga, x) & rd.get_pairs(gb, y)) for y in range(n_rel)] for x in range(n_rel)]
    assert rev.tolist() == [[len(rd.get_pairs(ga, x) & rd.get_pairs(gb, y, type='th')) for y in range(n_rel)] for x in range(n_rel)]
    assert not np.array_equal(same, same.T)


# ---------------------------------------------------------------------------------------------------------------
# the module and the header
# ---------------------------------------------------------------------------------------------------------------
def test_module_path_and_the_five_reference_signatures():
    import torchkge_amd.utils.data_redundancy as dr
    for name, want in REFERENCE_SIGNATURES.items():
        params = inspect.signature(getattr(dr, name)).parameters
        assert list(params) == [p for p, _ in want], name
        for p, default in want:
            if (name, p) in NO_DEFAULT:
                assert params[p].default == default and type(params[p].default) is type(default), (name, p)
            else:
                assert params[p].default is inspect.Parameter.empty, (name, p)
    assert list(inspect.signature(dr.relation_overlaps).parameters) == ['kg_tr', 'kg_val', 'kg_te', 'rev', 'max_bytes']
    assert inspect.signature(dr.relation_overlaps).parameters['max_bytes'].default == 1 << 30
    # not re-exported, as in the reference
    import torchkge_amd as tk
    assert not hasattr(tk.utils, 'duplicates') and not hasattr(tk, 'duplicates')
    for quirk in ('range(1345)', 'ZeroDivisionError', 'reverses', 'multiplied by 100', 'tqdm'):
        assert quirk in dr.__doc__, quirk


def test_get_pairs_and_concat_kgs_on_the_host():
    import torchkge_amd.utils.data_redundancy as dr
    g = rd.Graph([0, 1, 1, 2], [1, 0, 0, 2], [0, 0, 0, 1], 3, 2)
    for nm in ('head_idx', 'tail_idx', 'relations'):
        setattr(g, nm, torch.from_numpy(getattr(g, nm)))
    assert dr.get_pairs(g, 0) == {(0, 1), (1, 0)} and dr.get_pairs(g, 1, type='th') == {(2, 2)}
    h, t, r = dr.concat_kgs(g, g, g)
    assert h.tolist() == [0, 1, 1, 2] * 3 and t.tolist() == [1, 0, 0, 2] * 3 and r.tolist() == [0, 0, 0, 1] * 3


def test_library_exports_every_symbol_the_header_declares():
    from torchkge_amd import _hip, _hip_redundancy
    _hip_redundancy.load_library()
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(NEW) | set(WS)
    assert set(NEW) == set(_hip_redundancy._SIGNATURES)
    assert set(WS) == set(_hip_redundancy._WS_SIZES) | set(_hip_redundancy._WS_SIZES_2)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    from torchkge_amd.csrc import build as hb
    assert 'redundancy.hip' in hb.SOURCES and 'redundancy.hip' not in hb.EXTRA_FLAGS and 'mask_scan.h' in hb.HEADERS
    assert any(h.endswith('kge_hip_redundancy.h') for h in hb.HEADERS)
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    # integer adds only: no float atomic, no inline assembly
    code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, 'redundancy.hip')).read())
    assert not re.search(r'\basm\b|__asm', code)
    assert not re.search(r'\bfloat\b', code) and set(re.findall(r'\batomic\w+', code)) == {'atomicAdd'}


def test_ctypes_signatures_match_the_header_prototypes():
    from torchkge_amd import _hip_redundancy
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', hdr, flags=re.S))
    sizes = dict(re.findall(r'\bint64_t\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', hdr, flags=re.S))
    assert set(protos) == set(NEW) and set(sizes) == set(WS)

    def kind(param):
        param = param.strip()
        if '*' in param:
            return ctypes.c_void_p
        t = param.split()
        if 'kge_stream_t' in t:
            return ctypes.c_void_p
        if 'int64_t' in t:
            return ctypes.c_int64
        if 'double' in t:
            return ctypes.c_double
        if 'int' in t or 'int32_t' in t:
            return ctypes.c_int
        raise AssertionError('unparsed parameter: %r' % param)
    lib = _hip_redundancy.load_library()
    for name, args in _hip_redundancy._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            assert a is kind(prm), (name, prm)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    for name in WS:
        want = [kind(p) for p in sizes[name].split(',')]
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype is ctypes.c_int64
    assert len(sizes['kge_relation_overlap_ws_bytes'].split(',')) == 2
    # size queries run on the host: nothing for an empty or an oversized problem
    assert [int(lib.kge_relation_overlap_ws_bytes(a, b)) for a, b in ((0, 0), (-1, 5), (1 << 30, 1 << 30))] == [0, 0, 0]
    assert int(lib.kge_relation_overlap_ws_bytes(1000, 24)) >= 2 * 1024 * 8
    assert int(lib.kge_relation_stats_ws_bytes(0)) == 0 and int(lib.kge_relation_stats_ws_bytes(1024)) >= 2 * 1024 * 8
    assert int(lib.kge_overlap_select_ws_bytes(46341)) == 0 and int(lib.kge_overlap_select_ws_bytes(1345)) >= 1345 * 1345


def test_the_main_header_and_its_abi_are_untouched():
    from torchkge_amd import _hip
    assert _hip.ABI_VERSION == 33 and _hip.load_library().kge_abi_version() == 33
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    assert hashlib.sha256(raw).hexdigest() == KGE_HIP_H_SHA256
    for name in NEW + WS:
        assert name.encode() not in raw
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


# ---------------------------------------------------------------------------------------------------------------
# refusals before any device work
# ---------------------------------------------------------------------------------------------------------------
def torch_graph(h, t, r, n_ent, n_rel):
    g = rd.Graph(h, t, r, n_ent, n_rel)
    for nm in ('head_idx', 'tail_idx', 'relations'):
        setattr(g, nm, torch.from_numpy(getattr(g, nm)))
    return g


def test_max_bytes_and_bad_ids_raise_before_any_device_work(monkeypatch):
    import torchkge_amd.utils.data_redundancy as dr
    from torchkge_amd import _hip_redundancy

    def no_device_work(*a, **k):
        raise AssertionError('reached the device layer')
    for fn in ('relation_overlap', 'relation_stats', 'overlap_select', 'load_library'):
        monkeypatch.setattr(_hip_redundancy, fn, no_device_work)
    monkeypatch.setattr(dr, '_device', no_device_work)
    g = torch_graph([0, 1, 2], [1, 2, 0], [0, 1, 2], 3, 1345)
    # 2 * 1345^2 * 4 bytes = 14,472,200
    with pytest.raises(ValueError, match='14472200'):
        dr.relation_overlaps(g, g, g, max_bytes=14472199)
    with pytest.raises(ValueError, match='7236100'):
        dr.relation_overlaps(g, g, g, rev=False, max_bytes=7236099)
    with pytest.raises(ValueError, match='14472200'):
        dr.relation_overlaps(g, g, g, max_bytes=1 << 20)
    for h, t, r, what in (([0, 3], [1, 1], [0, 0], 'entity'), ([0, 1], [1, -1], [0, 0], 'entity'),
                          ([0, 1], [1, 2], [0, 4], 'relation'), ([0, 1], [1, 2], [-1, 0], 'relation')):
        bad = torch_graph(h, t, r, 3, 4)
        ok = torch_graph([0], [1], [0], 3, 4)
        with pytest.raises(ValueError, match=what):
            dr.duplicates(ok, bad, ok)
        with pytest.raises(ValueError, match=what):
            dr.relation_overlaps(ok, ok, bad)
        with pytest.raises(ValueError, match=what):
            dr.cartesian_product_relations(bad, ok, ok)
        with pytest.raises(ValueError, match=what):
            dr.count_triplets(ok, bad, [], [])
    with pytest.raises(ValueError, match='outside'):
        dr.count_triplets(ok, ok, [(0, 4)], [])


def test_without_a_gpu_the_functions_raise_the_engines_device_error(monkeypatch):
    import torchkge_amd.utils.data_redundancy as dr
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    g = torch_graph([0, 1, 2], [1, 2, 0], [0, 1, 2], 3, 3)
    for call in (lambda: dr.duplicates(g, g, g), lambda: dr.cartesian_product_relations(g, g, g),
                 lambda: dr.count_triplets(g, g, [(0, 1)], []), lambda: dr.relation_overlaps(g, g, g)):
        with pytest.raises(RuntimeError, match='runs only on MI355X .* no CPU fallback'):
            call()
