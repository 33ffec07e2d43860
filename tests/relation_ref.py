"""Plain-Python restatement of the contract of include/kge_hip_relation.h and the loader of tests/golden/ref_relation.npz
(tests/golden/make_golden_relation.py), shared by tests/test_relation_host.py and tests/test_gpu_relation.py.  Test-only."""
import os

import numpy as np
import torch

from tests.helpers import GOLDEN

KINDS = ('transe', 'distmult', 'complex', 'transh', 'transd')
N_TABLES = {'transe': 2, 'distmult': 2, 'complex': 4, 'transh': 3, 'transd': 4}
_CACHE = {}


def fixture():
    """The fixture as a dict of arrays: loaded once, shared, left unchanged."""
    if 'z' not in _CACHE:
        with np.load(os.path.join(GOLDEN, 'ref_relation.npz')) as z:
            _CACHE['z'] = {k: z[k] for k in z.files}
        for v in _CACHE['z'].values():
            v.setflags(write=False)
    return _CACHE['z']


def fixture_tables(kind):
    """The model tables of the kind, from ref_relpred.npz (ref_relation.npz does not repeat them)."""
    z = np.load(os.path.join(GOLDEN, 'ref_relpred.npz'))
    return [torch.from_numpy(z['%s_table%d' % (kind, i)]) for i in range(N_TABLES[kind])]


def fixture_batch(which):
    """One recorded corrupt_batch call (``which``: 64 or 'all'): the facts, the five arrays the reference consumed (compact)
    and its three outputs."""
    z = fixture()
    B = len(z['heads']) if which == 'all' else int(which)
    tag = 'b%s_' % which
    d = dict(heads=z['heads'][:B], tails=z['tails'][:B], rels=z['rels'][:B])
    for nm in ('mask_ent', 'mask_head', 'draws_r', 'draws_h', 'draws_t', 'neg_heads', 'neg_tails', 'neg_rels'):
        d[nm] = z[tag + nm]
    return d


def fixture_kg(tk):
    z = fixture()
    n_ent, n_rel = int(z['n_ent']), int(z['n_rel'])
    h, t, r = (torch.from_numpy(z[nm].copy()) for nm in ('heads', 'tails', 'rels'))
    return tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                             rel2ix={i: i for i in range(n_rel)})


def relation_corrupt(heads, tails, rels, mask_ent, mask_head, draws_r, draws_h, draws_t, n_neg=1):
    """The rule of kge_relation_corrupt, one position after the other: (neg_heads, neg_tails, neg_rels) int64 (B * n_neg).
    An array that is None must not be reached."""
    heads, tails, rels, mask_ent, mask_head, draws_r, draws_h, draws_t = (
        None if x is None else np.asarray(x).tolist() for x in (heads, tails, rels, mask_ent, mask_head, draws_r, draws_h, draws_t))
    B = len(heads)
    n = B * n_neg
    nh, nt, nr = [0] * n, [0] * n, [0] * n
    p = q = 0                                   # entity positions so far; those of them that took the head
    for j in range(n):
        b = j % B
        nh[j], nt[j], nr[j] = heads[b], tails[b], rels[b]
        if mask_ent[j] == 0:
            nr[j] = draws_r[j - p]
        else:
            if mask_head[p] != 0:
                nh[j] = draws_h[q]
                q += 1
            else:
                nt[j] = draws_t[p - q]
            p += 1
    return tuple(np.array(x, dtype=np.int64) for x in (nh, nt, nr))


def pad_to(a, n, fill, dtype):
    """``a`` followed by ``fill`` up to n entries: the array of a caller that does not know the split."""
    out = np.full(n, fill, dtype=dtype)
    out[:len(a)] = a
    return out
