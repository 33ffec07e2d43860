"""CPU-only tests of TorusE (torchkge/models/translation.py:655-767, utils/dissimilarities.py:28-54): the class, its
tables and state_dict against the reference fixtures, the constructor's frac, the ABI enums and the MFMA / VALU
classification of every all-candidates mode, a float64 restatement of the three torus formulas against the fixtures'
scores (which pins the reference's literal, wrap-around-free application: positive scores), TranslationModel with the
torus types and the utils exports."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, GOLDEN

import torchkge_amd as tk
from torchkge_amd import _hip

TYPES = {'L1': 'l1', 'torus_L1': 'tl1', 'torus_L2': 'tl2', 'torus_eL2': 'tel2'}


def fixture(diss):
    return np.load(os.path.join(GOLDEN, 'ref_toruse_%s.npz' % TYPES[diss]))


def diss64(diss, x):
    """The reference's dissimilarity of x = a - b in float64, applied literally (no wrap-around)."""
    if diss == 'L1':
        return x.abs().sum(-1)
    if diss == 'torus_L1':
        return 2 * torch.minimum(x.abs(), 1 - x.abs()).sum(-1)
    if diss == 'torus_L2':
        return 4 * torch.minimum(x ** 2, 1 - x ** 2).sum(-1)
    u = torch.minimum(x, 1 - x)
    return (2 * (1 - torch.cos(2 * math.pi * u))).sum(-1) / 4


def frac64(x):
    x = torch.as_tensor(x, dtype=torch.float64)
    return x - torch.trunc(x)


def test_abi_kinds_modes_and_exports():
    assert (_hip.TORUSE_L1, _hip.TORUSE_TORUS_L1, _hip.TORUSE_TORUS_L2, _hip.TORUSE_TORUS_EL2) == (8, 9, 10, 11)
    assert (_hip.LP_TORUS_L1, _hip.LP_TORUS_L2, _hip.LP_TORUS_EL2) == (6, 7, 8) and _hip.ABI_VERSION == 33
    hdr = open(os.path.join(ROOT, 'include', 'kge_hip.h')).read()
    for name, v in (('KGE_TORUSE_L1', 8), ('KGE_TORUSE_TORUS_L1', 9), ('KGE_TORUSE_TORUS_L2', 10),
                    ('KGE_TORUSE_TORUS_EL2', 11), ('KGE_LP_TORUS_L1', 6), ('KGE_LP_TORUS_L2', 7), ('KGE_LP_TORUS_EL2', 8)):
        assert re.search(r'\b%s = %d\b' % (name, v), hdr), name
    assert 'kge_frac_rows' in _hip.EXPORTED_SYMBOLS and 'kge_frac_rows(' in hdr


def test_is_mfma_classifies_every_mode():
    """KGE_LP_IS_MFMA of the header, evaluated for every mode: the four GEMM modes of ABI <= 32 stay MFMA, the two
    DIRECT ones and the three torus ones do not."""
    hdr = open(os.path.join(ROOT, 'include', 'kge_hip.h')).read()
    body = re.search(r'#define KGE_LP_IS_MFMA\(mode\)(.*?)\n(?!\s)', hdr.replace('\\\n', ' '), re.S).group(1)
    enums = dict((n, int(v)) for n, v in re.findall(r'\b(KGE_LP_[A-Z0-9_]+) = (\d+)', hdr))
    expr = body.replace('||', ' or ').replace('&&', ' and ')
    for n in sorted(enums, key=len, reverse=True):
        expr = expr.replace(n, str(enums[n]))
    want = {0: True, 1: True, 2: False, 3: False, 4: True, 5: True, 6: False, 7: False, 8: False}
    assert max(enums.values()) == 8
    for mode, mfma in want.items():
        assert bool(eval(expr.replace('(mode)', '(%d)' % mode).replace('mode', str(mode)))) == mfma, mode
        assert (mode in _hip.LP_MFMA_MODES) == mfma


@pytest.mark.parametrize('diss', list(TYPES))
def test_class_surface_constructor_frac_and_state_dict(diss):
    z = fixture(diss)
    n_ent, n_rel, d = int(z['n_ent']), int(z['n_rel']), int(z['dim'])
    torch.manual_seed(0)
    m = tk.TorusEModel(d, n_ent, n_rel, diss)
    assert isinstance(m, tk.models.TranslationModel) and tk.models.TorusEModel is tk.TorusEModel
    assert m.emb_dim == d and m.dissimilarity_type == diss and m.normalized is True
    assert sorted(m.state_dict().keys()) == list(z['state_dict_keys']) == ['ent_emb.weight', 'rel_emb.weight']
    # the reference's constructor under the same seed: init_embedding, then frac_ of both tables
    assert np.array_equal(m.ent_emb.weight.detach().numpy(), z['ctor_table0'])
    assert np.array_equal(m.rel_emb.weight.detach().numpy(), z['ctor_table1'])
    for name in ('scoring_function', 'normalize_parameters', 'get_embeddings', 'inference_prepare_candidates',
                 'inference_scoring_function', 'lp_problem', 'lp_eval_prepare', 'forward'):
        assert callable(getattr(m, name))
    m.load_state_dict({'ent_emb.weight': torch.from_numpy(z['table0']), 'rel_emb.weight': torch.from_numpy(z['table1'])})
    assert np.array_equal(m.ent_emb.weight.detach().numpy(), z['table0'])
    # the fixture's tables after the evaluation = frac of the raw ones (x - trunc(x): sign kept, in (-1, 1))
    for k in (0, 1):
        assert np.array_equal(frac64(z['table%d' % k]).float().numpy(), z['after_table%d' % k])
        assert np.abs(z['after_table%d' % k]).max() < 1 and (z['after_table%d' % k] < 0).any()
        assert np.abs(z['table%d' % k]).max() > 1


def test_constructor_rejects_l2():
    with pytest.raises(AssertionError):
        tk.TorusEModel(4, 5, 2, 'L2')


@pytest.mark.parametrize('diss', list(TYPES))
def test_float64_restatement_reproduces_fixture_scores(diss):
    z = fixture(diss)
    n_test, B = int(z['n_test']), int(z['b_size'])
    h = torch.from_numpy(z['heads'][-n_test:][:B])
    t = torch.from_numpy(z['tails'][-n_test:][:B])
    r = torch.from_numpy(z['rels'][-n_test:][:B])
    # x = a - b rounded to fp32 as the reference forms it, every term and the sum in float64; scores reach ~100 here
    # (fp32 ulp 7.6e-6), so the bound is 1e-5 relative to max(1, |s|)
    E, R = frac64(z['table0']).float(), frac64(z['table1']).float()
    sf = -diss64(diss, ((E[h] + R[r]) - E[t]).double())

    def close(a, ref):
        return (np.abs(a.numpy() - ref) / np.maximum(1.0, np.abs(ref))).max() < 1e-5
    assert close(sf, z['sf'])
    Ea, Ra = (torch.from_numpy(z['after_table%d' % k]) for k in (0, 1))
    s_tail = -diss64(diss, ((Ea[h] + Ra[r]).unsqueeze(1) - Ea.unsqueeze(0)).double())
    s_head = -diss64(diss, ((Ea.unsqueeze(0) + Ra[r].unsqueeze(1)) - Ea[t].unsqueeze(1)).double())
    assert close(s_tail, z['s_tail']) and close(s_head, z['s_head'])
    # the quirk the engine must keep: |x| > 1 makes torus terms negative, and most scores of torus_L1 / _L2 are positive
    if diss in ('torus_L1', 'torus_L2'):
        assert (z['s_tail'] > 0).mean() > 0.5 and (z['sf'] > 0).any()


@pytest.mark.parametrize('diss', ['torus_L1', 'torus_L2', 'torus_eL2'])
def test_translation_model_accepts_torus_types(diss):
    from torchkge_amd.models import TranslationModel
    from torchkge_amd.utils import dissimilarities as D

    class UserTorus(TranslationModel):
        def __init__(self):
            super().__init__(5, 2, diss)
    m = UserTorus()
    assert m.dissimilarity_type == diss
    assert m._direct_mode() == {'torus_L1': _hip.LP_TORUS_L1, 'torus_L2': _hip.LP_TORUS_L2,
                                'torus_eL2': _hip.LP_TORUS_EL2}[diss]
    assert m.dissimilarity is {'torus_L1': D.l1_torus_dissimilarity, 'torus_L2': D.l2_torus_dissimilarity,
                               'torus_eL2': D.el2_torus_dissimilarity}[diss]
    assert not m._uses_guard()


def test_utils_exports():
    from torchkge_amd.utils import l1_torus_dissimilarity, l2_torus_dissimilarity, el2_torus_dissimilarity
    from torchkge_amd.models import TorusEModel
    assert TorusEModel is tk.TorusEModel
    for fn in (l1_torus_dissimilarity, l2_torus_dissimilarity, el2_torus_dissimilarity):
        assert callable(fn) and fn.__module__ == 'torchkge_amd.utils.dissimilarities'
