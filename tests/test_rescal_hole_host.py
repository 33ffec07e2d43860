"""CPU-only tests of RESCAL / HolE (torchkge/models/bilinear.py:14-143, :270-411): the classes, their tables and
state_dict keys against the reference fixtures, the rolling matrix, a float64 restatement of the fixtures' scores, the
ABI enums, and the built ISA of the new kernels (no lane-crossing packed f32 operand)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, GOLDEN

import torchkge_amd as tk
from torchkge_amd import _hip

KINDS = {'rescal': ('ref_rescal.npz', 'rel_mat'), 'hole': ('ref_hole.npz', 'rel_emb')}


def fixture(kind):
    return np.load(os.path.join(GOLDEN, KINDS[kind][0]))


def make_model(kind, d, n_ent, n_rel):
    return tk.RESCALModel(d, n_ent, n_rel) if kind == 'rescal' else tk.HolEModel(d, n_ent, n_rel)


def operators64(kind, rel, d):
    """(n, d, d) float64 relation operators, written from the formulas: RESCAL M[i, j] = row[i*d + j],
    HolE B[i, j] = r[(j - i) mod d]."""
    rel = torch.as_tensor(rel, dtype=torch.float64)
    if kind == 'rescal':
        return rel.view(-1, d, d)
    i = torch.arange(d).view(d, 1)
    j = torch.arange(d).view(1, d)
    return rel[:, (j - i) % d]


def scores64(kind, E, rel, d, h, t, r):
    E = torch.as_tensor(E, dtype=torch.float64)
    B = operators64(kind, rel, d)
    hn = E[h] / E[h].norm(dim=1, keepdim=True).clamp_min(1e-12)
    tn = E[t] / E[t].norm(dim=1, keepdim=True).clamp_min(1e-12)
    sf = torch.einsum('bi,bij,bj->b', hn, B[r], tn)
    s_tail = torch.einsum('bi,bij->bj', E[h], B[r]) @ E.T       # raw tables at inference
    s_head = torch.einsum('bij,bj->bi', B[r], E[t]) @ E.T
    return sf, s_tail, s_head


def test_abi_kinds_and_exports():
    assert (_hip.RESCAL, _hip.HOLE) == (6, 7) and _hip.ABI_VERSION == 33
    hdr = open(os.path.join(ROOT, 'include', 'kge_hip.h')).read()
    assert re.search(r'KGE_RESCAL = 6', hdr) and re.search(r'KGE_HOLE = 7', hdr)
    for name in ('kge_bilinear_query', 'kge_bilinear_relation_rows', 'kge_rescal_rel_grad'):
        assert name in _hip.EXPORTED_SYMBOLS and name + '(' in hdr


@pytest.mark.parametrize('kind', ['rescal', 'hole'])
def test_classes_shapes_and_state_dict_load(kind):
    z = fixture(kind)
    n_ent, n_rel, d = int(z['n_ent']), int(z['n_rel']), int(z['dim'])
    m = make_model(kind, d, n_ent, n_rel)
    sd = m.state_dict()
    rel_key = KINDS[kind][1] + '.weight'
    assert set(sd) == {'ent_emb.weight', rel_key}
    assert tuple(sd['ent_emb.weight'].shape) == z['table0'].shape == (n_ent, d)
    assert tuple(sd[rel_key].shape) == z['table1'].shape == ((n_rel, d * d) if kind == 'rescal' else (n_rel, d))
    # Xavier initialisation followed by normalised entity rows (bilinear.py:50-58, :303-309)
    assert torch.allclose(m.ent_emb.weight.norm(dim=1), torch.ones(n_ent), atol=1e-5)
    m.load_state_dict({'ent_emb.weight': torch.from_numpy(z['table0']), rel_key: torch.from_numpy(z['table1'])})
    assert torch.equal(m.ent_emb.weight.data, torch.from_numpy(z['table0']))
    assert m._lp_width() == d and m._ENT_TABLES == ('ent_emb',) and m.lp_dedupe_queries
    assert hasattr(tk.models, 'RESCALModel') and hasattr(tk.models, 'HolEModel')


def test_rolling_matrix_is_the_index_formula():
    x = torch.randn(3, 7, dtype=torch.float64)
    mat = tk.HolEModel.get_rolling_matrix(x)
    assert mat.shape == (3, 7, 7) and mat.device.type == 'cpu'
    for b in range(3):
        for i in range(7):
            for j in range(7):
                assert mat[b, i, j] == x[b, (j - i) % 7]


@pytest.mark.parametrize('kind', ['rescal', 'hole'])
def test_float64_restatement_reproduces_the_fixture(kind):
    z = fixture(kind)
    d, B, nt = int(z['dim']), int(z['b_size']), int(z['n_test'])
    heads, tails, rels = (torch.from_numpy(z[k]) for k in ('heads', 'tails', 'rels'))
    h, t, r = heads[-nt:][:B], tails[-nt:][:B], rels[-nt:][:B]
    sf, s_tail, s_head = scores64(kind, z['table0'], z['table1'], d, h, t, r)
    assert np.abs(sf.numpy() - z['sf']).max() < 1e-5
    assert np.abs(s_tail.numpy() - z['s_tail']).max() < 1e-5
    assert np.abs(s_head.numpy() - z['s_head']).max() < 1e-5


def test_operator_kernels_hold_no_lane_crossing_packed_f32_operand():
    """bilinear_xform.hip (its instantiations of rel_operator.h's query transform, relation rows, K1 forward / backward;
    the d rel_mat reduction is transr_xform.hip's kernel) is built without the SLP vectoriser like the MFMA count kernels;
    its gfx950 assembly, compiled with the build's own flags, holds no packed f32 instruction with an op_sel bit set (the
    form test_host_logic.py explains)."""
    from torchkge_amd.csrc import build as hb
    src = 'bilinear_xform.hip'
    assert src in hb.SOURCES and '-fno-slp-vectorize' in hb.EXTRA_FLAGS[src]
    cmd = [hb._hipcc()] + hb.FLAGS + hb.EXTRA_FLAGS[src] + ['-S', '--cuda-device-only', os.path.join(hb.HERE, src),
                                                           '-o', '-']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout
    full, general = ('rel_query_kernelINS_10BilinearOpELb%dEEE' % f for f in (1, 0))
    for k in (full, general, 'relation_rows_kernel', 'bilinear_score_fwd_kernel', 'bilinear_score_bwd_kernel'):
        assert k in text, k
    bad = [l.strip() for l in text.split('\n')
           if re.search(r'\bv_pk_(fma|mul|add)_f32\b', l) and re.search(r'op_sel:\[[01,]*1[01,]*\]', l)]
    assert not bad, bad[:4]
    # no scratch spills in the query transform (its 16 accumulators stay in registers)
    m = re.search(r'\.name:\s*\S*' + full + r'\S*\n.*?\.private_segment_fixed_size:\s*(\d+)', text, re.S)
    assert m is not None and int(m.group(1)) == 0, m
