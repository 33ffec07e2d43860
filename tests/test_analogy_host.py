"""CPU-only tests of ANALOGY (torchkge/models/bilinear.py:559-763): the exports and ctypes signatures of
include/kge_hip_analogy.h, the untouched ABI of include/kge_hip.h, the class surface against the reference fixture, and
the float64 restatement the GPU tests compare with (it reproduces the fixture's scores; the fixture's ranks lie inside
its tie intervals)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.helpers import ROOT
from tests import analogy_ref as ar

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_analogy

TIE = 2e-5
HEADER = os.path.join(ROOT, 'include', 'kge_hip_analogy.h')
NEW = ('kge_analogy_pack_rows', 'kge_analogy_query', 'kge_analogy_score_triples', 'kge_analogy_score_triples_bwd')


def prototypes():
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', hdr, flags=re.S))


def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_analogy.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(NEW) == set(_hip_analogy._SIGNATURES) == set(prototypes())
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    for name in declared:
        assert hasattr(lib, name), name
    # compiled into libkge_hip.so without the SLP vectoriser, as bilinear_xform.hip is
    from torchkge_amd.csrc import build as hb
    assert 'analogy.hip' in hb.SOURCES and '-fno-slp-vectorize' in hb.EXTRA_FLAGS['analogy.hip']
    assert any(h.endswith('kge_hip_analogy.h') for h in hb.HEADERS)
    m = re.search(r'#define KGE_ANALOGY_SIDE_REL (\d+)', open(HEADER).read())
    assert m and int(m.group(1)) == _hip_analogy.SIDE_REL and _hip_analogy.SIDE_REL not in range(5)


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
    for name, args in _hip_analogy._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            k = kind(prm)
            if k is ctypes.c_int:
                assert a in (ctypes.c_int, ctypes.c_int32), (name, prm)
            else:
                assert a is k, (name, prm)
    lib = _hip_analogy.load_library()
    for name, args in _hip_analogy._SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int


def test_the_main_header_and_its_abi_are_untouched():
    assert _hip.ABI_VERSION == 33 and _hip.load_library().kge_abi_version() == 33
    hdr = open(os.path.join(ROOT, 'include', 'kge_hip.h')).read()
    assert 'kge_analogy' not in hdr
    for name in NEW:
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


@pytest.mark.parametrize('dim,share,want', [(32, .5, (16, 16)), (33, .5, (16, 17)), (33, .3, (9, 24)), (4, 0., (0, 4)),
                                            (4, 1., (4, 0))])
def test_scalar_and_complex_dims(dim, share, want):
    m = tk.AnalogyModel(dim, 11, 3, scalar_share=share)
    assert (m.scalar_dim, m.complex_dim) == want and m.emb_dim == dim
    assert m._lp_width() == want[0] + 2 * want[1]
    assert tuple(m.sc_ent_emb.weight.shape) == (11, want[0]) and tuple(m.im_rel_emb.weight.shape) == (3, want[1])
    assert [tuple(x.shape) for x in m.get_embeddings()] == [(11, want[0]), (11, want[1]), (11, want[1]),
                                                            (3, want[0]), (3, want[1]), (3, want[1])]


def test_class_surface_matches_the_reference_fixture():
    z = ar.fixture()
    n_ent, n_rel, d = int(z['n_ent']), int(z['n_rel']), int(z['dim'])
    m = tk.AnalogyModel(d, n_ent, n_rel)                    # scalar_share defaults to 0.5
    assert isinstance(m, tk.models.BilinearModel) and hasattr(tk.models, 'AnalogyModel')
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in z['state_keys']] == [n + '.weight' for n in ar.NAMES]
    assert [list(v.shape) for v in sd.values()] == z['state_shapes'].tolist()
    tabs = ar.fixture_tables(z)
    m.load_state_dict({n + '.weight': t.clone() for n, t in zip(ar.NAMES, tabs)})
    for got, want in zip(m.get_embeddings(), tabs):
        assert torch.equal(got, want)
    m.normalize_parameters()                                # a no-op (bilinear.py:652-656)
    for got, want in zip(m.get_embeddings(), tabs):
        assert torch.equal(got, want)
    m2 = tk.AnalogyModel(d, n_ent, n_rel)
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(m2.get_embeddings(), tabs))
    assert m._ENT_TABLES == ('sc_ent_emb', 're_ent_emb', 'im_ent_emb') and m._ENT_POS == (0, 1, 2)
    assert m.entity_table_bytes() == 4 * n_ent * (m.scalar_dim + 2 * m.complex_dim)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.scoring_function(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long),
                           torch.zeros(2, dtype=torch.long))


def test_float64_restatement_reproduces_the_fixture():
    z = ar.fixture()
    B = int(z['b_size'])
    tabs = ar.fixture_tables(z)
    h, t, r = (x[:B] for x in ar.fixture_test_triples(z))
    assert np.abs(ar.sf64(tabs, h, t, r).numpy() - z['sf']).max() < 1e-6
    assert np.abs(ar.scores64(tabs, 'tail', h=h, r=r).numpy() - z['s_tail']).max() < 1e-6
    assert np.abs(ar.scores64(tabs, 'head', t=t, r=r).numpy() - z['s_head']).max() < 1e-6
    assert np.abs(ar.scores64(tabs, 'rel', h=h, t=t).numpy() - z['s_rel']).max() < 1e-6
    assert z['s_tail'].shape == (B, int(z['n_ent'])) and z['s_rel'].shape == (B, int(z['n_rel']))
    # the uneven split (9 | 24 | 24), which the reference can only score triple by triple
    u = ar.fixture_tables(z, 'u_')
    assert [x.shape[1] for x in u] == [9, 24, 24, 9, 24, 24]
    assert np.abs(ar.sf64(u, h, t, r).numpy() - z['u_sf']).max() < 1e-6
    nh, nt = torch.from_numpy(z['u_neg_heads']), torch.from_numpy(z['u_neg_tails'])
    assert np.abs(ar.sf64(u, nh, nt, r.repeat(2)).numpy() - z['u_fwd_neg']).max() < 1e-6
    assert np.abs(ar.sf64(u, h, t, r).repeat(2).numpy() - z['u_fwd_pos']).max() < 1e-6


def test_reference_ranks_lie_in_the_restatements_tie_intervals():
    z = ar.fixture()
    tabs = ar.fixture_tables(z)
    heads, tails, rels = (torch.from_numpy(z[k]) for k in ('heads', 'tails', 'rels'))
    h, t, r = ar.fixture_test_triples(z)
    dh, dt, _ = orc.build_filter_dicts(heads, tails, rels)
    st, sh = ar.scores64(tabs, 'tail', h=h, r=r), ar.scores64(tabs, 'head', t=t, r=r)
    bounds = {'rank_true_tails': orc._tie_interval(st, t, TIE), 'rank_true_heads': orc._tie_interval(sh, h, TIE),
              'filt_rank_true_tails': orc._tie_interval(orc.filter_scores_vec(st, dt, h, r, t), t, TIE),
              'filt_rank_true_heads': orc._tie_interval(orc.filter_scores_vec(sh, dh, t, r, h), h, TIE)}
    for nm, (lo, hi) in bounds.items():
        ref = torch.from_numpy(z[nm])
        assert bool(((ref >= lo) & (ref <= hi)).all()), nm          # every row
    assert 0.01 < float(z['mrr'][0]) < 0.1                          # ranks are spread, not degenerate
