"""CPU-only tests of ConvKB (torchkge/models/deep.py:13-154): the exports and ctypes signatures of
include/kge_hip_convkb.h, the untouched include/kge_hip.h, the class surface against the reference fixture, and the
float64 restatement the GPU tests compare with (it reproduces the fixture's scores; the fixture's ranks lie inside its
tie intervals)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.helpers import ROOT
from tests import convkb_ref as cr

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_convkb

TIE = 2e-5
HEADER = os.path.join(ROOT, 'include', 'kge_hip_convkb.h')
NEW = ('kge_convkb_prepare', 'kge_convkb_scores', 'kge_convkb_pair_scores', 'kge_convkb_count_ge', 'kge_convkb_filter_sub',
       'kge_convkb_score_triples', 'kge_convkb_score_triples_bwd')
# sha256 of include/kge_hip.h as the parent commit has it: kge_lp_desc and ABI 33 do not change for this model
KGE_HIP_H_SHA256 = '1d27fe190e8113e167cb0ae9d5108c0a08ab6569765f853cc884e29f00462b4c'


def prototypes():
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', hdr, flags=re.S))


def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_convkb.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(NEW) == set(_hip_convkb._SIGNATURES) == set(prototypes())
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    for name in declared:
        assert hasattr(lib, name), name
    from torchkge_amd.csrc import build as hb
    assert 'convkb.hip' in hb.SOURCES and '-fno-slp-vectorize' in hb.EXTRA_FLAGS['convkb.hip']
    assert any(h.endswith('kge_hip_convkb.h') for h in hb.HEADERS)
    hdr = open(HEADER).read()
    m = re.search(r'#define KGE_CONVKB_SLOT_BOTH (\d+)', hdr)
    assert m and int(m.group(1)) == _hip_convkb.SLOT_BOTH
    m = re.search(r'#define KGE_CONVKB_MAX_DIM (\d+)', hdr)
    assert m and int(m.group(1)) == _hip_convkb.MAX_DIM >= 512
    src = open(os.path.join(ROOT, 'torchkge_amd', 'csrc', 'convkb.hip')).read()
    tq, tc, th = (int(re.search(r'constexpr int %s = (\d+);' % n, src).group(1)) for n in ('CKB_TQ', 'CKB_TC', 'CKB_THREADS'))
    assert (tq, tc * th) == (_hip_convkb.TILE_Q, _hip_convkb.TILE_C)       # the tile sizes the GPU tests straddle


def test_ctypes_signatures_match_the_header_prototypes():
    """The checker of test_host_logic.py::test_ctypes_signatures_match_the_header_prototypes on the new header and
    table: same number of parameters, pointers as void*, int as c_int, int64_t as c_int64, float as c_float."""
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
    for name, args in _hip_convkb._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            k = kind(prm)
            if k is ctypes.c_int:
                assert a in (ctypes.c_int, ctypes.c_int32), (name, prm)
            else:
                assert a is k, (name, prm)
    lib = _hip_convkb.load_library()
    for name, args in _hip_convkb._SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int


def test_descriptor_layout_matches_the_header():
    """ConvKBDesc field by field against the struct of the header: names, order, and C types."""
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct kge_convkb_desc \{(.*?)\} kge_convkb_desc;', hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ptr = '*' in decl
        ctype = ctypes.c_void_p if ptr else (ctypes.c_int64 if decl.startswith('int64_t') else ctypes.c_int32)
        assert ptr or decl.startswith(('int64_t', 'int32_t')), decl
        for nm in re.sub(r'^(const\s+)?\w+\s*', '', decl).split(','):
            fields.append((nm.replace('*', '').strip(), ctype))
    assert fields == [(n, t) for n, t in _hip_convkb.ConvKBDesc._fields_]
    assert ctypes.sizeof(_hip_convkb.ConvKBDesc) == 16 + 4 * 8 + 8 * 8 + 4 * 8


def test_the_main_header_and_its_abi_are_untouched():
    assert _hip.ABI_VERSION == 33 and _hip.load_library().kge_abi_version() == 33
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    assert hashlib.sha256(raw).hexdigest() == KGE_HIP_H_SHA256
    assert b'kge_convkb' not in raw
    for name in NEW:
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


def test_class_surface_matches_the_reference_fixture():
    z = cr.fixture()
    n_ent, n_rel, d, F = int(z['n_ent']), int(z['n_rel']), int(z['dim']), int(z['n_filters'])
    m = tk.ConvKBModel(d, F, n_ent, n_rel)
    assert isinstance(m, tk.models.Model) and tk.models.ConvKBModel is tk.ConvKBModel
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in z['state_keys']] == cr.PARAMS
    want = [row[:n].tolist() for row, n in zip(z['state_shapes'], z['state_ndim'])]
    assert [list(v.shape) for v in sd.values()] == want
    assert want[2] == [F, 3, 1] and want[4] == [2, F * d]
    params = cr.fixture_params(z)
    m.load_state_dict({n: t.clone() for n, t in zip(cr.PARAMS, params)})     # a reference checkpoint loads
    for got, ref in zip(m.get_embeddings(), params[:2]):
        assert torch.equal(got, ref)
    m.normalize_parameters()                                # a no-op (deep.py:79-85)
    for got, ref in zip(m._tables(), params):
        assert torch.equal(got.data, ref)
    assert m.split_filter is False and m.lp_dedupe_queries is False and not m._uses_guard()
    assert m.lp_guard_begin(torch.device('cpu')) is None
    for name in ('forward', 'lp_scoring_function', 'lp_prep_cands'):        # inherited
        assert getattr(tk.ConvKBModel, name) is getattr(tk.models.Model, name)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.scoring_function(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long),
                           torch.zeros(2, dtype=torch.long))
    surface = ('scores', 'scores_chunk', 'scores_rows', 'pair_scores', 'count_ge', 'filter_sub')
    assert all(callable(getattr(_hip_convkb.ConvKBProblem, n)) for n in surface)


def test_same_initialisation_as_the_reference_module_tree():
    """Same constructor calls in the same order: the same seed gives torch's own Conv1d / Linear initialisation."""
    torch.manual_seed(3)
    m = tk.ConvKBModel(6, 4, 11, 3)
    torch.manual_seed(3)
    from torchkge_amd.utils.modeling import init_embedding
    ent, rel = init_embedding(11, 6), init_embedding(3, 6)
    conv, lin = torch.nn.Conv1d(3, 4, 1, stride=1), torch.nn.Linear(24, 2)
    for got, ref in zip(m._tables(), (ent.weight, rel.weight, conv.weight, conv.bias, lin.weight, lin.bias)):
        assert torch.equal(got, ref)


def test_sizes_beyond_the_kernels_limits_and_sharding_are_refused():
    with pytest.raises(RuntimeError, match='emb_dim <= 512'):
        tk.ConvKBModel(513, 4, 11, 3)
    with pytest.raises(RuntimeError, match='n_filters <= 512'):
        tk.ConvKBModel(8, 513, 11, 3)
    m = tk.ConvKBModel(8, 2, 11, 3)
    with pytest.raises(RuntimeError, match='row-sharded entity tables are out of scope for ConvKBModel'):
        m.shard_entities_(0, 5)
    with pytest.raises(RuntimeError, match='row-sharded entity tables are out of scope for ConvKBModel'):
        m.as_entity_shard_(22, 0, 11)


def test_float64_restatement_reproduces_the_fixture():
    z = cr.fixture()
    B = int(z['b_size'])
    params = cr.fixture_params(z)
    h, t, r = (x[:B] for x in cr.fixture_test_triples(z))
    assert np.abs(cr.sf64(params, h, t, r).numpy() - z['sf']).max() < 1e-5
    assert np.abs(cr.scores64(params, 'tail', h=h, r=r).numpy() - z['s_tail']).max() < 1e-5
    assert np.abs(cr.scores64(params, 'head', t=t, r=r).numpy() - z['s_head']).max() < 1e-5
    assert np.abs(cr.scores64(params, 'rel', h=h, t=t).numpy() - z['s_rel']).max() < 1e-5
    assert z['s_tail'].shape == (B, int(z['n_ent'])) and z['s_rel'].shape == (B, int(z['n_rel']))
    nh, nt = torch.from_numpy(z['neg_heads']), torch.from_numpy(z['neg_tails'])
    assert np.abs(cr.sf64(params, nh, nt, r.repeat(2)).numpy() - z['fwd_neg']).max() < 1e-5
    assert np.abs(cr.sf64(params, h, t, r).repeat(2).numpy() - z['fwd_pos']).max() < 1e-5
    # scoring_function is the tail-side score at column t
    assert torch.equal(cr.scores64(params, 'tail', h=h, r=r).gather(1, t.view(-1, 1)).view(-1), cr.sf64(params, h, t, r))
    assert float(z['s_tail'].max() - z['s_tail'].min()) > 0.5          # the x32 head spreads the scores


def test_reference_ranks_lie_in_the_restatements_tie_intervals():
    z = cr.fixture()
    params = cr.fixture_params(z)
    heads, tails, rels = (torch.from_numpy(z[k]) for k in ('heads', 'tails', 'rels'))
    h, t, r = cr.fixture_test_triples(z)
    dh, dt, _ = orc.build_filter_dicts(heads, tails, rels)
    st, sh = cr.scores64(params, 'tail', h=h, r=r), cr.scores64(params, 'head', t=t, r=r)
    bounds = {'rank_true_tails': orc._tie_interval(st, t, TIE), 'rank_true_heads': orc._tie_interval(sh, h, TIE),
              'filt_rank_true_tails': orc._tie_interval(orc.filter_scores_vec(st, dt, h, r, t), t, TIE),
              'filt_rank_true_heads': orc._tie_interval(orc.filter_scores_vec(sh, dh, t, r, h), h, TIE)}
    for nm, (lo, hi) in bounds.items():
        ref = torch.from_numpy(z[nm])
        assert bool(((ref >= lo) & (ref <= hi)).all()), nm          # every row
    assert 0.01 < float(z['mrr'][0]) < 0.1                          # ranks are spread, not degenerate
