"""CPU-only tests of triplet classification (torchkge/sampling.py:330-504, :556-592, evaluation.py:428-580): the exports
and ctypes signatures of include/kge_hip_triplet.h, the untouched include/kge_hip.h, the import paths, the possibility
index against the reference fixture, and the numpy restatement the GPU tests compare with (it reproduces the fixture's
reference outputs bit for bit)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import ROOT
from tests import triplet_ref as tr

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_triplet

HEADER = os.path.join(ROOT, 'include', 'kge_hip_triplet.h')
NEW = ('kge_positional_corrupt', 'kge_relation_max', 'kge_threshold_count')
WS = ('kge_positional_ws_elems', 'kge_relation_max_ws_elems')
# sha256 of include/kge_hip.h as the parent commit has it: nothing of it changes for these entry points
KGE_HIP_H_SHA256 = '1d27fe190e8113e167cb0ae9d5108c0a08ab6569765f853cc884e29f00462b4c'


def prototypes():
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', hdr, flags=re.S))


def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_triplet.load_library()
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(NEW) | set(WS)
    assert set(NEW) == set(_hip_triplet._SIGNATURES) == set(prototypes()) and set(WS) == set(_hip_triplet._WS_SIZES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    for name in declared:
        assert hasattr(lib, name), name
    from torchkge_amd.csrc import build as hb
    assert 'triplet.hip' in hb.SOURCES and 'mask_scan.h' in hb.HEADERS
    assert any(h.endswith('kge_hip_triplet.h') for h in hb.HEADERS)
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    # workspace sizes: one int32 per 1024 positions + 1; one per relation + 1
    assert [int(lib.kge_positional_ws_elems(b)) for b in (-1, 0, 1, 1024, 1025)] == [0, 0, 2, 2, 3]
    assert [int(lib.kge_relation_max_ws_elems(n)) for n in (-1, 0, 1, 237)] == [0, 0, 2, 238]


def test_ctypes_signatures_match_the_header_prototypes():
    """Same number of parameters, pointers as void*, int64_t as c_int64 (the checker of tests/test_convkb_host.py)."""
    protos = prototypes()

    def kind(param):
        param = param.strip()
        if '*' in param:
            return ctypes.c_void_p
        t = param.split()
        if 'kge_stream_t' in t:
            return ctypes.c_void_p
        if 'int64_t' in t:
            return ctypes.c_int64
        if 'float' in t:
            return ctypes.c_float
        if 'int' in t or 'int32_t' in t:
            return ctypes.c_int
        raise AssertionError('unparsed parameter: %r' % param)
    for name, args in _hip_triplet._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            k = kind(prm)
            if k is ctypes.c_int:
                assert a in (ctypes.c_int, ctypes.c_int32), (name, prm)
            else:
                assert a is k, (name, prm)
    lib = _hip_triplet.load_library()
    for name, args in _hip_triplet._SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    for name in WS:
        assert getattr(lib, name).argtypes == [ctypes.c_int64] and getattr(lib, name).restype is ctypes.c_int64
        assert re.search(r'\bint64_t\s+%s\s*\(\s*int64_t \w+\s*\)\s*;' % name, open(HEADER).read())


def test_the_main_header_and_its_abi_are_untouched():
    assert _hip.ABI_VERSION == 33 and _hip.load_library().kge_abi_version() == 33
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    assert hashlib.sha256(raw).hexdigest() == KGE_HIP_H_SHA256
    for name in NEW + WS:
        assert name.encode() not in raw
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


def test_the_submodules_provide_the_two_classes_and_the_helper():
    from torchkge_amd.sampling import PositionalNegativeSampler, get_possible_heads_tails
    from torchkge_amd.evaluation import TripletClassificationEvaluator
    from torchkge_amd.sampling import BernoulliNegativeSampler
    assert issubclass(PositionalNegativeSampler, BernoulliNegativeSampler) and callable(get_possible_heads_tails)
    for name in ('get_scores', 'evaluate', 'accuracy'):
        assert callable(getattr(TripletClassificationEvaluator, name))
    for name in ('corrupt_batch', 'corrupt_kg', 'find_possibilities'):
        assert callable(getattr(PositionalNegativeSampler, name))


def test_the_top_level_names_still_say_not_provided_and_name_the_submodule():
    for name, sub in (('TripletClassificationEvaluator', 'torchkge_amd.evaluation'),
                      ('PositionalNegativeSampler', 'torchkge_amd.sampling')):
        assert not hasattr(tk, name)
        with pytest.raises(AttributeError, match='does not provide') as e:
            getattr(tk, name)
        assert sub in str(e.value)


def test_cpu_built_index_reproduces_the_fixture():
    from torchkge_amd.sampling import PositionalNegativeSampler
    z = tr.fixture()
    kg_val, kg_test = tr.fixture_kgs(tk)
    n_rel, empty = int(z['n_rel']), int(z['empty_rel'])
    assert (kg_val.n_facts, kg_test.n_facts, int((kg_test.relations == empty).sum())) == (351, 300, 45)
    s = PositionalNegativeSampler(kg_val, kg_test=kg_test)          # the evaluator's construction: test facts add nothing
    ih, it = s._indices(torch.device('cpu'))
    for idx, side in ((ih, 'heads'), (it, 'tails')):
        assert idx.offsets.dtype == torch.int64 and idx.values.dtype == torch.int32
        assert np.array_equal(idx.offsets.numpy(), z['poss_%s_offsets' % side])
        assert np.array_equal(idx.values.numpy(), z['poss_%s_values' % side])
    assert s.n_poss_heads.dtype == torch.int64 and tuple(s.n_poss_heads.shape) == (n_rel,)
    assert np.array_equal(s.n_poss_heads.numpy(), z['n_poss_heads'])
    assert np.array_equal(s.n_poss_tails.numpy(), z['n_poss_tails'])
    assert int(s.n_poss_heads[empty]) == 0 and int(s.n_poss_tails[empty]) == 0 and s._has_empty
    assert np.array_equal(s.bern_probs.numpy(), z['bern_probs']) and float(s.bern_probs[empty]) == 0.5
    ph, pt, nh, nt = s.find_possibilities()
    assert ph is s.possible_heads and nh is s.n_poss_heads
    for lists, side in ((ph, 'heads'), (pt, 'tails')):
        assert sorted(lists) == list(range(n_rel)) and lists[empty] == []
        off, val = z['poss_%s_offsets' % side], z['poss_%s_values' % side]
        for r in range(n_rel):
            assert lists[r] == val[off[r]:off[r + 1]].tolist() == sorted(set(lists[r]))
    # kg + kg_val are indexed, kg_test never: a sampler of (val-part, rest-of-val) equals the one above
    a = tk.KnowledgeGraph(kg={'heads': kg_val.head_idx[:100], 'tails': kg_val.tail_idx[:100], 'relations': kg_val.relations[:100]},
                          ent2ix=kg_val.ent2ix, rel2ix=kg_val.rel2ix)
    b = tk.KnowledgeGraph(kg={'heads': kg_val.head_idx[100:], 'tails': kg_val.tail_idx[100:], 'relations': kg_val.relations[100:]},
                          ent2ix=kg_val.ent2ix, rel2ix=kg_val.rel2ix)
    s2 = PositionalNegativeSampler(a, kg_val=b, kg_test=kg_test)
    assert s2.possible_heads == ph and s2.possible_tails == pt and torch.equal(s2.n_poss_tails, nt)


def test_get_possible_heads_tails_chains_over_a_second_graph():
    from torchkge_amd.sampling import get_possible_heads_tails
    z = tr.fixture()
    kg_val, _ = tr.fixture_kgs(tk)
    n_rel, empty = int(z['n_rel']), int(z['empty_rel'])
    want = {}
    for side in ('heads', 'tails'):
        off, val = z['poss_%s_offsets' % side], z['poss_%s_values' % side]
        want[side] = {r: set(val[off[r]:off[r + 1]].tolist()) for r in range(n_rel) if off[r + 1] > off[r]}
    ph, pt = get_possible_heads_tails(kg_val)
    assert type(ph) == dict and ph == want['heads'] and pt == want['tails'] and empty not in ph
    assert all(type(v) == set for v in ph.values())
    mk = lambda sl: tk.KnowledgeGraph(kg={'heads': kg_val.head_idx[sl], 'tails': kg_val.tail_idx[sl],      # noqa: E731
                                          'relations': kg_val.relations[sl]}, ent2ix=kg_val.ent2ix, rel2ix=kg_val.rel2ix)
    ph1, pt1 = get_possible_heads_tails(mk(slice(0, 120)))
    assert ph1 != want['heads']
    ph2, pt2 = get_possible_heads_tails(mk(slice(120, None)), ph1, pt1)
    assert ph2 == want['heads'] and pt2 == want['tails']


def test_restatement_reproduces_the_reference_negatives_from_its_draws():
    z = tr.fixture()
    n_fb = 0
    for which, n_batches, last in (('main', 6, 31), ('test', 5, 44)):
        batches = tr.fixture_batches(which)
        assert len(batches) == n_batches and len(batches[-1]['heads']) == last
        for d in batches:
            nh, nt = tr.positional_corrupt(d['heads'], d['tails'], d['rels'], d['mask'], d['u_h'], d['u_t'], d['fb_h'], d['fb_t'],
                                           z['poss_heads_offsets'], z['poss_heads_values'], z['poss_tails_offsets'],
                                           z['poss_tails_values'])
            assert np.array_equal(nh, d['neg_heads']) and np.array_equal(nt, d['neg_tails'])
            n_fb += int((d['fb_h'] >= 0).sum() + (d['fb_t'] >= 0).sum())
            assert float(d['u_h'].max(initial=0)) < 1.0 and d['u_h'].dtype == np.float32
    assert n_fb == 45           # every test fact of the empty relation took the uniform fallback


@pytest.mark.parametrize('kind,p', tr.CASES)
def test_restatement_reproduces_the_reference_thresholds_and_count(kind, p):
    z, t = tr.fixture(), tr.tag(kind, p)
    n_rel = int(z['n_rel'])
    thr = tr.relation_max(z[t + '_val_neg_scores'], z['val_rels'], n_rel)
    assert thr.dtype == np.float32 and np.array_equal(thr.view(np.uint32), z[t + '_thresholds'].view(np.uint32))
    assert thr[int(z['empty_rel'])] == z[t + '_val_neg_scores'].max()       # absent relation: the overall maximum
    n_pos, n_neg = tr.threshold_count(z[t + '_pos_scores'], z[t + '_neg_scores'], z['test_rels'], thr)
    assert n_pos + n_neg == int(z[t + '_correct'])
    assert int(z[t + '_near']) <= 12 and float(z['near']) == 2e-5


def test_restatement_edge_cases():
    nan, inf = float('nan'), float('inf')
    thr = tr.relation_max(np.array([-3, -1, nan, -inf], np.float32), np.array([0, 0, 2, 3]), 5)
    assert tr.same_values(thr, [-1, nan, nan, -inf, nan])
    thr = tr.relation_max(np.array([-3, -1, -2], np.float32), np.array([0, 0, 2]), 4)
    assert tr.same_values(thr, [-1, -1, -2, -1])
    assert tr.threshold_count([1, 2, nan, 3], [1, 2, 0, nan], [0, 0, 0, 1], np.array([2, nan], np.float32)) == (0, 2)
    off, val = np.array([0, 0, 3, 4]), np.array([5, 6, 7, 9], np.int32)
    one = np.float32(1.0)
    nh, nt = tr.positional_corrupt([1, 2, 3, 4], [1, 2, 3, 4], [1, 1, 0, 2], [1, 1, 1, 0], np.array([one, 0, 0.5], np.float32),
                                   np.array([np.nextafter(one, np.float32(0))]), np.array([-1, -1, 8]), None, off, val, off, val)
    assert nh.tolist() == [7, 5, 8, 4] and nt.tolist() == [1, 2, 3, 9]     # u = 1.0 clamps to the segment's last entry


def test_corrupt_batch_on_cpu_tensors_raises_the_engines_device_error():
    from torchkge_amd.sampling import PositionalNegativeSampler
    kg_val, kg_test = tr.fixture_kgs(tk)
    s = PositionalNegativeSampler(kg_val, kg_test=kg_test)
    with pytest.raises(RuntimeError, match='runs only on MI355X .* no CPU fallback'):
        s.corrupt_batch(kg_val.head_idx[:8], kg_val.tail_idx[:8], kg_val.relations[:8])
    s.sync_free = True
    with pytest.raises(RuntimeError, match='runs only on MI355X'):
        s.corrupt_batch(kg_val.head_idx[:8], kg_val.tail_idx[:8], kg_val.relations[:8])
