"""CPU-only tests of TransR (torchkge/models/translation.py:287-458): the ABI additions, the class and its state_dict
against the reference fixture, a float64 restatement of the fixture's scores, gradients and ranks written from the
formulas (it is the yardstick of tests/test_gpu_transr.py), and the built ISA of transr_xform.hip."""
import inspect
import os
import re
import subprocess

import numpy as np
import torch

from tests.helpers import ROOT, GOLDEN

import torchkge_amd as tk
from torchkge_amd import _hip
from oracle import kge_oracle as orc

NEW_SYMBOLS = ('kge_transr_proj_sqnorm', 'kge_transr_query', 'kge_transr_rel_grad')


def fixture():
    return np.load(os.path.join(GOLDEN, 'ref_transr.npz'))


def tables64(z):
    E, R, P = (torch.from_numpy(z['table%d' % k]).double() for k in range(3))
    return E, R, P.view(R.shape[0], R.shape[1], E.shape[1])


def scoring64(E, R, M, h, t, r):
    """-|| M_r h^ + r - M_r t^ ||^2 with x^ = x / max(||x||, 1e-12)."""
    hn = E[h] / E[h].norm(dim=1, keepdim=True).clamp_min(1e-12)
    tn = E[t] / E[t].norm(dim=1, keepdim=True).clamp_min(1e-12)
    p = torch.einsum('bck,bk->bc', M[r], hn) + R[r] - torch.einsum('bck,bk->bc', M[r], tn)
    return -(p * p).sum(1)


def side_scores64(E, R, M, h, t, r):
    """(tail side, head side) all-candidates scores on the RAW entity rows."""
    proj = torch.einsum('bck,nk->bnc', M[r], E)                         # (b, N, d_r): M_r e_c
    qt = torch.einsum('bck,bk->bc', M[r], E[h]) + R[r]
    qh = torch.einsum('bck,bk->bc', M[r], E[t]) - R[r]
    return -((qt.unsqueeze(1) - proj) ** 2).sum(2), -((proj - qh.unsqueeze(1)) ** 2).sum(2)


def relation_scores64(E, R, M, h, t):
    """s[i, r'] = -|| M_r' h_i + R[r'] - M_r' t_i ||^2 for every relation r'."""
    p = torch.einsum('rck,bk->brc', M, E[h] - E[t]) + R.unsqueeze(0)
    return -(p * p).sum(2)


def test_abi_kind_symbols_and_no_new_lp_mode():
    hdr = open(os.path.join(ROOT, 'include', 'kge_hip.h')).read()
    assert re.search(r'\bKGE_TRANSR\s*=\s*12\b', hdr) and _hip.TRANSR == 12
    assert _hip.ABI_VERSION == 33
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and s in _hip.EXPORTED_SYMBOLS and s in _hip._SIGNATURES, s
    modes = {n: int(v) for n, v in re.findall(r'\b(KGE_LP_[A-Z0-9_]+)\s*=\s*(\d+)', hdr)}
    assert max(modes.values()) == 8 and len(modes) == 9
    # the declared parameter counts match the binding's
    for s in NEW_SYMBOLS:
        m = re.search(r'int %s\((.*?)\);' % s, hdr, re.S)
        assert m and len(m.group(1).split(',')) == len(_hip._SIGNATURES[s]), s


def test_class_surface_constructor_and_state_dict():
    z = fixture()
    n_ent, n_rel, de, dr = int(z['n_ent']), int(z['n_rel']), int(z['dim']), int(z['dim_rel'])
    assert list(inspect.signature(tk.TransRModel.__init__).parameters)[1:] == ['ent_emb_dim', 'rel_emb_dim', 'n_entities',
                                                                               'n_relations']
    torch.manual_seed(0)
    m = tk.TransRModel(de, dr, n_ent, n_rel)
    assert isinstance(m, tk.models.TranslationModel) and tk.models.TransRModel is tk.TransRModel
    assert (m.ent_emb_dim, m.rel_emb_dim, m.n_ent, m.n_rel, m.dissimilarity_type) == (de, dr, n_ent, n_rel, 'L2')
    assert m.evaluated_projections is False
    assert tuple(m.ent_emb.weight.shape) == (n_ent, de) and tuple(m.rel_emb.weight.shape) == (n_rel, dr)
    assert tuple(m.proj_mat.weight.shape) == (n_rel, dr * de)
    for k, name in enumerate(('ent_emb', 'rel_emb', 'proj_mat')):     # the reference's constructor under the same seed
        assert np.array_equal(getattr(m, name).weight.detach().numpy(), z['ctor_table%d' % k]), name
    ref_keys = [k for k in z['state_dict_keys'] if k != 'projected_entities']
    assert 'projected_entities' in list(z['state_dict_keys'])
    assert sorted(m.state_dict().keys()) == ref_keys == ['ent_emb.weight', 'proj_mat.weight', 'rel_emb.weight']
    for name in ('scoring_function', 'project', 'normalize_parameters', 'get_embeddings', 'inference_prepare_candidates',
                 'inference_scoring_function', 'evaluate_projectionss', 'lp_problem', 'forward'):
        assert callable(getattr(m, name)), name
    m.evaluate_projectionss()
    assert m.evaluated_projections is True
    # a reference state_dict carries the (n_rel, n_ent, d_r) cache: it loads, and the cache is dropped
    sd = {'ent_emb.weight': torch.from_numpy(z['table0']), 'rel_emb.weight': torch.from_numpy(z['table1']),
          'proj_mat.weight': torch.from_numpy(z['table2']), 'projected_entities': torch.zeros(n_rel, n_ent, dr)}
    m.load_state_dict(sd)
    assert np.array_equal(m.proj_mat.weight.detach().numpy(), z['table2'])
    assert 'projected_entities' not in m.state_dict() and not hasattr(m, 'projected_entities')
    assert m._ENT_TABLES == ('ent_emb',) and m.lp_sort_queries_by_relation is True
    # project(): M e on host tensors, the reference's helper
    e = torch.from_numpy(z['table0'][:3])
    M = torch.from_numpy(z['table2'][:3]).view(3, dr, de)
    assert torch.allclose(m.project(e, M), torch.einsum('bck,bk->bc', M, e), atol=1e-6)
    assert 'projected_entities' not in z.files


def test_float64_restatement_reproduces_fixture():
    z = fixture()
    E, R, M = tables64(z)
    n_test, B = int(z['n_test']), int(z['b_size'])
    H, T, Rl = (torch.from_numpy(z[k][-n_test:]) for k in ('heads', 'tails', 'rels'))
    h, t, r = H[:B], T[:B], Rl[:B]

    def close(a, ref, tol=1e-5):
        ref = np.asarray(ref, dtype=np.float64)
        return np.abs(a.numpy() - ref).max() <= tol * max(1.0, np.abs(ref).max())
    assert close(scoring64(E, R, M, h, t, r), z['sf'])
    nh, nt = torch.from_numpy(z['neg_heads']), torch.from_numpy(z['neg_tails'])
    assert close(scoring64(E, R, M, h, t, r).repeat(2), z['fwd_pos'])
    assert close(scoring64(E, R, M, nh, nt, r.repeat(2)), z['fwd_neg'])
    st, sh = side_scores64(E, R, M, h, t, r)
    assert close(st, z['s_tail']) and close(sh, z['s_head'])
    assert close(relation_scores64(E, R, M, h, t), z['s_rel'])
    # gradients of (scoring_function * g).sum() by float64 autograd
    Eg, Rg, Pg = (torch.from_numpy(z['table%d' % k]).double().requires_grad_(True) for k in range(3))
    (scoring64(Eg, Rg, Pg.view(M.shape), h, t, r) * torch.from_numpy(z['grad_out']).double()).sum().backward()
    for g, name in ((Eg, 'grad_ent'), (Rg, 'grad_rel'), (Pg, 'grad_proj')):
        assert close(g.grad, z[name], 1e-4), name
    # ranks of the whole test split, raw and filtered, from the float64 scores
    dh, dt, dr_ = orc.build_filter_dicts(z['heads'], z['tails'], z['rels'])
    st, sh = side_scores64(E, R, M, H, T, Rl)
    for s, true, d, k1, raw, filt in ((st, T, dt, H, 'rank_true_tails', 'filt_rank_true_tails'),
                                      (sh, H, dh, T, 'rank_true_heads', 'filt_rank_true_heads')):
        s_true = s.gather(1, true.view(-1, 1))
        assert np.array_equal(((s >= s_true).sum(1)).numpy(), z[raw]), raw
        rows, cols = orc.filter_pairs(d, k1, Rl, true)
        f = s.clone()
        f[torch.as_tensor(rows), torch.as_tensor(cols)] = float('-inf')
        assert np.array_equal(((f >= s_true).sum(1)).numpy(), z[filt]), filt
    sr = relation_scores64(E, R, M, H, T)
    s_true = sr.gather(1, Rl.view(-1, 1))
    assert np.array_equal((sr >= s_true).sum(1).numpy(), z['rel_dir_rank'])


def test_transr_kernels_isa():
    """transr_xform.hip is built without the SLP vectoriser (no packed f32 instruction with an op_sel bit set: the form
    test_host_logic.py explains); the projected-norm kernel runs on the fp32 MFMA and spills nothing."""
    from torchkge_amd.csrc import build as hb
    src = 'transr_xform.hip'
    assert src in hb.SOURCES and '-fno-slp-vectorize' in hb.EXTRA_FLAGS[src]
    cmd = [hb._hipcc()] + hb.FLAGS + hb.EXTRA_FLAGS[src] + ['-S', '--cuda-device-only', os.path.join(hb.HERE, src),
                                                           '-o', '-']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout
    for k in ('proj_sqnorm_kernel', 'rel_query_kernelINS_8TransROpELb0EEE', 'transr_score_fwd_kernel',
              'transr_score_bwd_kernel', 'rel_outer_grad_kernel'):
        assert k in text, k
    bad = [l.strip() for l in text.split('\n')
           if re.search(r'\bv_pk_(fma|mul|add)_f32\b', l) and re.search(r'op_sel:\[[01,]*1[01,]*\]', l)]
    assert not bad, bad[:4]
    assert re.search(r'\bv_mfma_f32_(32x32x2|16x16x4)_?f32\b', text)
    spills = re.findall(r'\.name:\s*(\S*proj_sqnorm_kernel\S*).*?\.private_segment_fixed_size:\s*(\d+).*?'
                        r'\.vgpr_spill_count:\s*(\d+)', text, re.S)
    assert len(spills) == 2, spills
    for name, scratch, spilled in spills:
        assert int(scratch) == 0 and int(spilled) == 0, (name, scratch, spilled)
