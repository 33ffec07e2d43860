"""float64 restatement of ANALOGY (torchkge/models/bilinear.py:559-763), written from the three formulas of
include/kge_hip_analogy.h, and the fixture loader shared by tests/test_analogy_host.py and tests/test_gpu_analogy.py.
Test-only."""
import os

import numpy as np
import torch

from tests.helpers import GOLDEN

NAMES = ['sc_ent_emb', 're_ent_emb', 'im_ent_emb', 'sc_rel_emb', 're_rel_emb', 'im_rel_emb']


def fixture():
    return np.load(os.path.join(GOLDEN, 'ref_analogy.npz'))


def fixture_tables(z, prefix=''):
    return [torch.from_numpy(z['%stable%d' % (prefix, i)]) for i in range(6)]


def fixture_test_triples(z):
    nt = int(z['n_test'])
    return tuple(torch.from_numpy(z[k])[-nt:] for k in ('heads', 'tails', 'rels'))


def packed64(sc, re, im):
    return torch.cat([sc.double(), re.double(), im.double()], dim=1)


def queries64(tabs, side, h=None, t=None, r=None):
    """float64 query rows [sc | re | im] of the side 'tail' (h, r), 'head' (t, r) or 'rel' (h, t)."""
    sc_e, re_e, im_e, sc_r, re_r, im_r = [x.double() for x in tabs]
    if side == 'tail':
        a, b, c, d, e, f = sc_e[h], re_e[h], im_e[h], sc_r[r], re_r[r], im_r[r]
        return torch.cat([a * d, b * e - c * f, b * f + c * e], dim=1)
    if side == 'head':
        a, b, c, d, e, f = sc_e[t], re_e[t], im_e[t], sc_r[r], re_r[r], im_r[r]
        return torch.cat([d * a, e * b + f * c, e * c - f * b], dim=1)
    a, b, c, d, e, f = sc_e[h], re_e[h], im_e[h], sc_e[t], re_e[t], im_e[t]
    return torch.cat([a * d, b * e + c * f, b * f - c * e], dim=1)


def scores64(tabs, side, h=None, t=None, r=None):
    """(b, N) float64 scores of every entity ('tail' / 'head') or every relation ('rel')."""
    cand = packed64(*tabs[3:]) if side == 'rel' else packed64(*tabs[:3])
    return queries64(tabs, side, h, t, r) @ cand.T


def sf64(tabs, h, t, r):
    """scoring_function: the tail-side query row against the tail's packed row."""
    return (queries64(tabs, 'tail', h=h, r=r) * packed64(*tabs[:3])[t]).sum(dim=1)
