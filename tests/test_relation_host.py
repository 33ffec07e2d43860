"""CPU-only tests of the relation side (torchkge/sampling.py:507-553, inference.py:78-154): the export and ctypes
signature of include/kge_hip_relation.h, the untouched include/kge_hip.h, the import paths, the sampler's probabilities
against the reference fixture, and the plain-Python restatement the GPU tests compare with (it reproduces the fixture's
reference outputs exactly from the arrays the reference consumed)."""
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
from tests import relation_ref as rr

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_relation

HEADER = os.path.join(ROOT, 'include', 'kge_hip_relation.h')
NEW = ('kge_relation_corrupt',)
WS = ('kge_relation_corrupt_ws_elems',)
# sha256 of include/kge_hip.h as the parent commit has it: nothing of it changes for this entry point
KGE_HIP_H_SHA256 = '1d27fe190e8113e167cb0ae9d5108c0a08ab6569765f853cc884e29f00462b4c'


def prototypes():
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', hdr, flags=re.S))


def test_the_submodules_provide_the_two_classes():
    from torchkge_amd.sampling import BernoulliRelationNegativeSampler, NegativeSampler
    from torchkge_amd.inference import RelationInference
    assert issubclass(BernoulliRelationNegativeSampler, NegativeSampler)
    for name in ('corrupt_batch', 'corrupt_kg', 'evaluate_probabilities'):
        assert callable(getattr(BernoulliRelationNegativeSampler, name))
    assert callable(RelationInference.evaluate)


def test_the_top_level_name_still_says_not_provided_and_names_the_module():
    assert not hasattr(tk, 'RelationInference')
    with pytest.raises(AttributeError, match='does not provide') as e:
        tk.RelationInference
    assert 'torchkge_amd.inference' in str(e.value)
    with pytest.raises(ImportError):
        from torchkge_amd import RelationInference  # noqa: F401
    assert not hasattr(tk, 'BernoulliRelationNegativeSampler')      # (never was a top-level name of the reference either)


def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_relation.load_library()
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(NEW) | set(WS)
    assert set(NEW) == set(_hip_relation._SIGNATURES) == set(prototypes()) and set(WS) == set(_hip_relation._WS_SIZES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    from torchkge_amd.csrc import build as hb
    assert 'relation_corrupt.hip' in hb.SOURCES and 'mask_scan.h' in hb.HEADERS
    assert any(h.endswith('kge_hip_relation.h') for h in hb.HEADERS)
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    # workspace: two arrays of (one int32 per 1024 positions, + 1) and one byte per position
    assert [int(lib.kge_relation_corrupt_ws_elems(n)) for n in (-1, 0, 1, 4, 5, 1024, 1025)] == [0, 0, 5, 5, 6, 260, 263]
    # every store an ordinary store: the source of the entry point takes no atomic
    code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, 'relation_corrupt.hip')).read())
    assert not re.search(r'atomic', code, flags=re.I)


def test_ctypes_signatures_match_the_header_prototypes():
    """Same number of parameters, pointers as void*, int64_t as c_int64 (the checker of tests/test_triplet_host.py)."""
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
        if 'int' in t or 'int32_t' in t:
            return ctypes.c_int
        raise AssertionError('unparsed parameter: %r' % param)
    for name, args in _hip_relation._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args) == 15, (name, len(params), len(args))
        for prm, a in zip(params, args):
            assert a is kind(prm), (name, prm)
    lib = _hip_relation.load_library()
    for name, args in _hip_relation._SIGNATURES.items():
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


def test_sampler_probabilities_equal_the_fixture_and_the_names_are_the_references():
    from torchkge_amd.sampling import BernoulliRelationNegativeSampler
    z = rr.fixture()
    kg = rr.fixture_kg(tk)
    assert (kg.n_facts, kg.n_ent, kg.n_rel) == (1385, int(z['n_ent']), int(z['n_rel']))
    s = BernoulliRelationNegativeSampler(kg)
    assert s.bern_probs.dtype == torch.float32
    assert np.array_equal(s.bern_probs.numpy().view(np.uint32), z['bern_probs'].view(np.uint32))
    assert s.rel_share == .33 == float(z['rel_share']) and s.n_neg == 1 and s.sync_free is False
    s = BernoulliRelationNegativeSampler(kg, kg_val=None, kg_test=None, n_neg=3, rel_share=.5)
    assert s.rel_share == .5 and s.n_neg == 3 and s.n_ent == kg.n_ent and s.n_facts == kg.n_facts
    assert list(inspect.signature(BernoulliRelationNegativeSampler.__init__).parameters) == \
        ['self', 'kg', 'kg_val', 'kg_test', 'n_neg', 'rel_share']
    assert list(inspect.signature(BernoulliRelationNegativeSampler.corrupt_batch).parameters) == \
        ['self', 'heads', 'tails', 'relations', 'n_neg']
    doc = BernoulliRelationNegativeSampler.__doc__
    for quirk in ('ENTITY', 'randint(1, .)', 'may equal the true one', 'n_neg`` is honoured', 'three vectors'):
        assert quirk in doc, quirk


@pytest.mark.parametrize('which', [64, 'all'])
def test_restatement_reproduces_the_reference_negatives_from_its_arrays(which):
    d = rr.fixture_batch(which)
    B = len(d['heads'])
    k, q = int(d['mask_ent'].sum()), int(d['mask_head'].sum())
    assert B == (1385 if which == 'all' else 64) and 0 < q < k < B          # all three branches are taken
    if which == 64:
        assert (k, q, B - k) == (20, 4, 44)
    assert (len(d['mask_ent']), len(d['mask_head']), len(d['draws_r']), len(d['draws_h']), len(d['draws_t'])) == (B, k, B - k, q, k - q)
    got = rr.relation_corrupt(d['heads'], d['tails'], d['rels'], d['mask_ent'], d['mask_head'], d['draws_r'], d['draws_h'], d['draws_t'])
    for g, nm in zip(got, ('neg_heads', 'neg_tails', 'neg_rels')):
        assert g.dtype == np.int64 and np.array_equal(g, d[nm]), nm
    # the reference's quirk: no draw is id 0
    assert min(d['draws_r'].min(), d['draws_h'].min(), d['draws_t'].min()) >= 1
    # padded arrays (a caller that does not know the split) give the same negatives
    got = rr.relation_corrupt(d['heads'], d['tails'], d['rels'], d['mask_ent'], rr.pad_to(d['mask_head'], B, 1, np.uint8),
                              rr.pad_to(d['draws_r'], B, -7, np.int64), rr.pad_to(d['draws_h'], B, -8, np.int64),
                              rr.pad_to(d['draws_t'], B, -9, np.int64))
    for g, nm in zip(got, ('neg_heads', 'neg_tails', 'neg_rels')):
        assert np.array_equal(g, d[nm]), nm


def test_restatement_edge_cases():
    h, t, r = np.array([10, 11, 12]), np.array([20, 21, 22]), np.array([1, 2, 3])
    # n_neg = 2: position j reads fact j % 3; entity positions 1, 2, 4 take head, tail, head
    got = rr.relation_corrupt(h, t, r, [0, 1, 1, 0, 1, 0], [1, 0, 1], [5, 6, 7], [90, 91], [80], n_neg=2)
    assert got[0].tolist() == [10, 90, 12, 10, 91, 12]
    assert got[1].tolist() == [20, 21, 80, 20, 21, 22]
    assert got[2].tolist() == [5, 2, 3, 6, 2, 7]
    # all-zero / all-one masks never reach the arrays of the other branches
    got = rr.relation_corrupt(h, t, r, [0, 0, 0], None, [4, 5, 6], None, None)
    assert got[0].tolist() == h.tolist() and got[1].tolist() == t.tolist() and got[2].tolist() == [4, 5, 6]
    got = rr.relation_corrupt(h, t, r, [1, 1, 1], [1, 1, 1], None, [7, 8, 9], None)
    assert got[0].tolist() == [7, 8, 9] and got[1].tolist() == t.tolist() and got[2].tolist() == r.tolist()
    got = rr.relation_corrupt(h, t, r, [1, 1, 1], [0, 0, 0], None, None, [7, 8, 9])
    assert got[0].tolist() == h.tolist() and got[1].tolist() == [7, 8, 9] and got[2].tolist() == r.tolist()


def test_fixture_inference_part_is_what_the_generator_promises():
    z = rr.fixture()
    n, n_rel, k = int(z['n_pairs']), int(z['n_rel']), int(z['top_k'])
    assert (n, n_rel, k, int(z['b_size']), float(z['near'])) == (64, 7, 3, 16, 2e-5)
    for kind in rr.KINDS:
        for variant in ('raw', 'filt'):
            tag = '%s_%s_' % (kind, variant)
            mat = torch.from_numpy(z[tag + 'scores'].copy())
            assert tuple(mat.shape) == (n, n_rel) and int(z[tag + 'near']) <= 1
            vals, ids = mat.sort(descending=True, stable=True)
            assert np.array_equal(vals[:, :k].numpy(), z[tag + 'top_vals'])
            finite = np.isfinite(z[tag + 'top_vals'])
            assert np.array_equal(ids[:, :k].numpy()[finite], z[tag + 'top_ids'][finite])
            assert finite.all() if variant == 'raw' else (finite[:, :2].all() and not finite.all())


def test_relation_inference_attributes_and_the_cpu_model_error():
    from torchkge_amd.inference import RelationInference
    assert list(inspect.signature(RelationInference.__init__).parameters) == \
        ['self', 'model', 'entities1', 'entities2', 'top_k', 'dictionary']
    assert list(inspect.signature(RelationInference.evaluate).parameters) == ['self', 'b_size', 'verbose']
    m = tk.TransEModel(8, 20, 4, 'L2')
    e1, e2 = torch.arange(5), torch.arange(5) + 1
    d = {(0, 1): [2]}
    inf = RelationInference(m, e1, e2, top_k=3, dictionary=d)
    assert inf.model is m and inf.entities1 is e1 and inf.entities2 is e2 and inf.dictionary is d
    assert inf.topk == 3 and inf.top_k == 3
    assert tuple(inf.predictions.shape) == (5, 3) and inf.predictions.dtype == torch.int64 and not inf.predictions.is_cuda
    assert tuple(inf.scores.shape) == (5, 3) and inf.scores.dtype == torch.float32
    assert RelationInference(m, e1, e2).topk == 1 and RelationInference(m, e1, e2).dictionary is None
    with pytest.raises(RuntimeError, match='runs on MI355X .* move the model to `cuda`'):
        inf.evaluate(b_size=4, verbose=False)


def test_corrupt_batch_on_cpu_tensors_raises_the_engines_device_error():
    from torchkge_amd.sampling import BernoulliRelationNegativeSampler
    kg = rr.fixture_kg(tk)
    s = BernoulliRelationNegativeSampler(kg)
    for sync_free in (False, True):
        s.sync_free = sync_free
        with pytest.raises(RuntimeError, match='runs only on MI355X .* no CPU fallback'):
            s.corrupt_batch(kg.head_idx[:8], kg.tail_idx[:8], kg.relations[:8])
