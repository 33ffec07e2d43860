"""CPU-only tests of RotatE: the numbers and the prototype of include/kge_hip_rotate.h against the binding, the untouched
include/kge_hip.h, the build list, the class surface, the constructor's refusals, the refusal of host tensors before any
launch, the all-candidates criteria that stay unimplemented, and the float64 restatement (tests/rotate_ref.py) against
itself on the identity the head-side query rests on."""
import math
import os
import re

import pytest
import torch

from tests.helpers import ROOT
from tests import rotate_ref as ref

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_rotate

HEADER = os.path.join(ROOT, 'include', 'kge_hip_rotate.h')


def test_header_numbers_prototype_and_binding():
    hdr = open(HEADER).read()
    assert re.search(r'#define KGE_LP_CMOD 9\b', hdr) and re.search(r'#define KGE_ROTATE 13\b', hdr)
    assert (_hip.LP_CMOD, _hip.ROTATE, _hip.ABI_VERSION) == (9, 13, 33)
    assert _hip.LP_CMOD not in _hip.LP_MFMA_MODES
    # they continue the enums of kge_hip.h without a gap and without a clash
    main = open(os.path.join(ROOT, 'include', 'kge_hip.h')).read()
    modes = [int(v) for v in re.findall(r'\bKGE_LP_[A-Z0-9_]+ = (\d+)', main)]
    kinds = [int(v) for v in re.findall(r'\bKGE_(?:TRANS|DIST|COMPLEX|RESCAL|HOLE|TORUSE)[A-Z0-9_]* = (\d+)', main)]
    assert max(modes) + 1 == _hip.LP_CMOD and max(kinds) + 1 == _hip.ROTATE
    assert b'kge_rotate_query' not in open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    assert 'kge_rotate_query' not in _hip.EXPORTED_SYMBOLS and 'kge_rotate_query' not in _hip._SIGNATURES
    # KGE_LP_IS_MFMA of the main header is false for the new mode
    body = re.search(r'#define KGE_LP_IS_MFMA\(mode\)(.*?)\n(?!\s)', main.replace('\\\n', ' '), re.S).group(1)
    enums = dict(re.findall(r'\b(KGE_LP_[A-Z0-9_]+) = (\d+)', main))
    expr = body.replace('||', ' or ').replace('&&', ' and ')
    for n in sorted(enums, key=len, reverse=True):
        expr = expr.replace(n, enums[n])
    assert not eval(expr.replace('(mode)', '(9)').replace('mode', '9'))
    # the prototype against the ctypes signature: one argtype per parameter, pointers as void *, sizes as int64
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    protos = dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', code, flags=re.S))
    assert sorted(protos) == _hip_rotate.EXPORTED_SYMBOLS == ['kge_rotate_query']
    params = [p.strip() for p in protos['kge_rotate_query'].split(',')]
    sig = _hip_rotate._SIGNATURES['kge_rotate_query']
    assert len(params) == len(sig) == 15
    for p, a in zip(params, sig):
        want = _hip._vp if ('*' in p or p.startswith('kge_stream_t')) else (_hip._i64 if p.startswith('int64_t') else _hip._int)
        assert a is want, p


def test_build_list():
    from torchkge_amd.csrc import build as hb
    assert 'rotate.hip' in hb.SOURCES and 'rotate.hip' not in hb.EXTRA_FLAGS and '-ffp-contract=off' in hb.FLAGS
    assert any(h.endswith('kge_hip_rotate.h') for h in hb.HEADERS)
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h


@pytest.mark.parametrize('d', [1, 3, 16, 17, 512])
def test_class_surface_and_parameter_shapes(d):
    torch.manual_seed(0)
    m = tk.RotatEModel(d, 50, 5)
    assert tk.models.RotatEModel is tk.RotatEModel and isinstance(m, tk.models.Model)
    from torchkge_amd import RotatEModel as top
    from torchkge_amd.models import RotatEModel as sub
    assert top is sub is type(m)
    assert not isinstance(m, tk.models.TranslationModel)        # no dissimilarity_type, no margin inside the score
    assert m.emb_dim == d and (m.n_ent, m.n_rel) == (50, 5)
    assert tuple(m.ent_emb.weight.shape) == (50, 2 * d) and tuple(m.rel_emb.weight.shape) == (5, d)
    assert sorted(m.state_dict().keys()) == ['ent_emb.weight', 'rel_emb.weight']
    P = m.rel_emb.weight.detach()
    assert float(P.min()) >= -math.pi and float(P.max()) <= math.pi and (d < 16 or float(P.abs().max()) > 2.0)
    # init_embedding's Xavier bound of a (50, 2d) table
    assert float(m.ent_emb.weight.detach().abs().max()) <= math.sqrt(6.0 / (50 + 2 * d)) + 1e-7
    for name in ('scoring_function', 'forward', 'forward_grouped', 'normalize_parameters', 'get_embeddings', 'lp_problem',
                 'inference_prepare_candidates', 'inference_scoring_function', 'lp_problem_both'):
        assert callable(getattr(m, name))
    assert m._hip_kind() == m._triple_kind() == _hip.ROTATE and (m._d_ent, m._d_rel) == (2 * d, d)
    assert m.split_filter is False and not m._uses_guard()
    before = [x.detach().clone() for x in m._tables()]
    assert m.normalize_parameters() is None
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, m._tables()))
    # the grouped scorer has no RotatE kind: forward_grouped falls back to forward
    from torchkge_amd import _hip_factgroup
    assert _hip.ROTATE not in _hip_factgroup.KINDS
    # both tables are row-gradient tables
    from torchkge_amd import optim
    row, dense = optim.split_parameters(m)
    assert {id(p) for p in row} == {id(m.ent_emb.weight), id(m.rel_emb.weight)} and dense == []


def test_get_embeddings_is_the_complex_view():
    m = tk.RotatEModel(7, 11, 3)
    ent, rel = m.get_embeddings()
    assert ent.dtype == torch.complex64 and tuple(ent.shape) == (11, 7) and tuple(rel.shape) == (3, 7)
    E = m.ent_emb.weight.detach()
    assert torch.equal(ent.real, E[:, 0::2]) and torch.equal(ent.imag, E[:, 1::2])
    assert ent.data_ptr() == E.data_ptr() and rel.data_ptr() == m.rel_emb.weight.data_ptr()
    assert torch.equal(ref.as_complex(E).real.float(), ent.real)


@pytest.mark.parametrize('bad', [0, -1, 513, 2.5])
def test_constructor_refusals(bad):
    with pytest.raises(ValueError, match='emb_dim'):
        tk.RotatEModel(bad, 10, 2)


def test_host_tensors_are_refused_before_any_launch():
    m = tk.RotatEModel(4, 10, 2)
    h, t, r = torch.tensor([0, 1]), torch.tensor([2, 3]), torch.tensor([0, 1])
    for call in (lambda: m.scoring_function(h, t, r), lambda: m(h, t, r, t, h),
                 lambda: m.lp_problem(h, t, r, 'tail'), lambda: m.lp_problem(h, t, r, 'both'),
                 lambda: m.inference_prepare_candidates(h, t, r),
                 lambda: m.inference_scoring_function(torch.zeros(2, 8), torch.zeros(2, 10, 8), torch.zeros(2, 4)),
                 lambda: m.inference_scoring_function(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2, 2, 4))):
        with pytest.raises(RuntimeError, match='no CPU fallback|MI355X'):
            call()


def test_all_candidates_criteria_stay_unimplemented():
    m = tk.RotatEModel(4, 10, 2)
    idx = torch.tensor([0, 1])
    with pytest.raises(NotImplementedError, match='DistMultModel and ComplExModel'):
        m.one_vs_all_loss(idx, idx, idx)
    with pytest.raises(NotImplementedError, match='DistMultModel and ComplExModel'):
        m.k_vs_all_loss(idx, idx, torch.zeros(2, 10), 'tail')


def test_reference_tail_head_identity_and_layout():
    """|h o r - t| = |h - t o conj(r)| for |r| = 1: the restatement's head-side query rows give the head-side scores of the
    definition, its tail-side ones the tail-side scores, and both agree with scoring_function's formula on the true
    entity."""
    g = torch.Generator().manual_seed(1)
    n_ent, n_rel, d, b = 23, 4, 5, 9
    E = torch.rand(n_ent, 2 * d, generator=g) * 2 - 1
    P = (torch.rand(n_rel, d, generator=g) * 2 - 1) * math.pi
    h, t, r = (torch.randint(0, n, (b,), generator=g) for n in (n_ent, n_ent, n_rel))
    Ec = ref.as_complex(E)
    assert torch.equal(Ec.real, E[:, 0::2].double()) and torch.equal(Ec.imag, E[:, 1::2].double())
    assert float((ref.rotation(P).abs() - 1).abs().max()) < 1e-15
    for side in ('tail', 'head'):
        q = ref.queries64(E, P, h, t, r, side)
        via_rows = -(q.unsqueeze(1) - Ec.unsqueeze(0)).abs().sum(-1)
        assert float((via_rows - ref.scores64(E, P, h, t, r, side)).abs().max()) < 1e-13
        true = t if side == 'tail' else h
        assert float((via_rows.gather(1, true.view(-1, 1)).view(-1) - ref.sf64(E, P, h, t, r)).abs().max()) < 1e-13
    # the interleaved float view of the rows is what cmod_scores64 takes
    q = ref.queries64(E, P, h, t, r, 'tail')
    Q = torch.view_as_real(q).reshape(b, 2 * d)
    assert float((ref.cmod_scores64(Q, E.double()) - ref.scores64(E, P, h, t, r, 'tail')).abs().max()) < 1e-13
    assert float((ref.relation_scores64(E, P, h, t)[torch.arange(b), r] - ref.sf64(E, P, h, t, r)).abs().max()) < 1e-13


@pytest.mark.parametrize('d', [3, 16, 17])
def test_reference_has_no_near_ties(d):
    """The seeds of tests/test_gpu_rotate.py: in float64 no candidate but the true one lies within the tie band of
    tests/test_gpu_toruse.py around a true score, so a rank inside the tie interval IS the reference's rank and the GPU
    comparisons excuse no fact."""
    from tests.test_gpu_rotate import reference_ranks, DIMS
    assert d in DIMS
    for nm, (rank, lo, hi) in reference_ranks(d).items():
        assert bool((hi == lo + 1).all()) and bool((rank == hi).all()), nm
