"""float64 restatement of ConvKB (torchkge/models/deep.py:13-154), written from the closed form of
include/kge_hip_convkb.h, and the fixture loaders shared by tests/test_convkb_host.py and tests/test_gpu_convkb.py.
Test-only.

    v[f][j] = w[f][0] x0[j] + w[f][1] x1[j] + w[f][2] x2[j] + cb[f]
    z       = sum_{f,j} (L[1] - L[0])[f d + j] relu(v[f][j]) + (lb[1] - lb[0]),   score = 1 / (1 + exp(-z))
"""
import os

import numpy as np
import torch

from tests.helpers import GOLDEN

PARAMS = ['ent_emb.weight', 'rel_emb.weight', 'convlayer.0.weight', 'convlayer.0.bias', 'output.0.weight', 'output.0.bias']
CHUNK = 256     # candidates per step of scores64 (the (b, chunk, F, d) activation stays small)


def fixture():
    return np.load(os.path.join(GOLDEN, 'ref_convkb.npz'))


def fixture_params(z):
    """[ent, rel, conv weight (F, 3, 1), conv bias (F), linear weight (2, F d), linear bias (2)]"""
    return [torch.from_numpy(z['table%d' % i]) for i in range(6)]


def fixture_test_triples(z):
    nt = int(z['n_test'])
    return tuple(torch.from_numpy(z[k])[-nt:] for k in ('heads', 'tails', 'rels'))


def _layer64(params):
    conv_w, conv_b, lin_w, lin_b = [x.double() for x in params[2:]]
    F = conv_w.shape[0]
    w = conv_w.reshape(F, 3)
    D = (lin_w[1] - lin_w[0]).reshape(F, -1)        # (F, d): flattening index f d + j
    return w, conv_b, D, lin_b[1] - lin_b[0]


def z64(params, x0, x1, x2):
    """Logit difference of rows that broadcast against each other, (..., d) each."""
    w, cb, D, db = _layer64(params)
    v = (w[:, 0, None] * x0.double().unsqueeze(-2) + w[:, 1, None] * x1.double().unsqueeze(-2)
         + w[:, 2, None] * x2.double().unsqueeze(-2) + cb[:, None])        # (..., F, d)
    return (D * torch.relu(v)).sum(dim=(-2, -1)) + db


def sf64(params, h, t, r):
    """scoring_function of index vectors, float64; differentiable in the six parameters."""
    ent, rel = params[0], params[1]
    return torch.sigmoid(z64(params, ent[h], rel[r], ent[t]))


def scores64(params, side, h=None, t=None, r=None, cand=None):
    """(b, N) float64 scores of every entity ('tail' / 'head') or every relation ('rel'), chunked over the candidates.
    ``cand``: another candidate table than the model's own."""
    ent, rel = params[0].double(), params[1].double()
    table = cand.double() if cand is not None else (rel if side == 'rel' else ent)
    out = []
    for c0 in range(0, table.shape[0], CHUNK):
        c = table[c0:c0 + CHUNK].unsqueeze(0)           # (1, chunk, d)
        if side == 'tail':
            zz = z64(params, ent[h].unsqueeze(1), rel[r].unsqueeze(1), c)
        elif side == 'head':
            zz = z64(params, c, rel[r].unsqueeze(1), ent[t].unsqueeze(1))
        else:
            zz = z64(params, ent[h].unsqueeze(1), c, ent[t].unsqueeze(1))
        out.append(torch.sigmoid(zz))
    return torch.cat(out, dim=1)
