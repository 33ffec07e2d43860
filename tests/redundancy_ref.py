"""Plain-numpy restatement of torchkge/utils/data_redundancy.py (parameterised on n_rel where the reference hard-codes
1345) and of the contract of include/kge_hip_redundancy.h, plus the loader of tests/golden/ref_redundancy.npz
(tests/golden/make_golden_redundancy.py).  Shared by tests/test_redundancy_host.py, tests/test_gpu_redundancy.py and
tools/redundancy_time.py.  Test-only.

The formulation is a set join, not the engine's sorted-run walk: distinct (h, t, r) triples by np.unique on packed keys,
then for every distinct triple of A the matching triples of B by binary search on B's (h, t) keys."""
import os

import numpy as np

from tests.helpers import GOLDEN

_CACHE = {}


class Graph(object):
    """The attributes of a KnowledgeGraph the five functions read."""

    def __init__(self, h, t, r, n_ent, n_rel):
        self.head_idx, self.tail_idx, self.relations = (np.asarray(x, dtype=np.int64) for x in (h, t, r))
        self.n_ent, self.n_rel, self.n_facts = int(n_ent), int(n_rel), len(self.head_idx)

    def __len__(self):
        return self.n_facts


def fixture():
    """The fixture as a dict of arrays: loaded once, shared, left unchanged."""
    if 'z' not in _CACHE:
        with np.load(os.path.join(GOLDEN, 'ref_redundancy.npz')) as z:
            _CACHE['z'] = {k: z[k] for k in z.files}
        for v in _CACHE['z'].values():
            v.setflags(write=False)
    return _CACHE['z']


def fixture_graphs():
    """(train, valid, test) of the fixture as Graph objects."""
    z = fixture()
    return tuple(Graph(z[s + '_heads'], z[s + '_tails'], z[s + '_rels'], int(z['n_ent']), int(z['n_rel']))
                 for s in ('train', 'valid', 'test'))


def concat_kgs(kg_tr, kg_val, kg_te):
    return tuple(np.concatenate([getattr(k, nm) for k in (kg_tr, kg_val, kg_te)]) for nm in ('head_idx', 'tail_idx', 'relations'))


def get_pairs(kg, r, type='ht'):
    m = kg.relations == r
    hs, ts = kg.head_idx[m].tolist(), kg.tail_idx[m].tolist()
    assert type in ('ht', 'th')
    return set(zip(hs, ts)) if type == 'ht' else set(zip(ts, hs))


def _distinct(h, t, r, n_ent, n_rel):
    """Distinct triples as (pair key h * n_ent + t, relation), sorted by pair key then relation."""
    h, t, r = (np.asarray(x, dtype=np.int64) for x in (h, t, r))
    assert n_ent * n_ent * n_rel < 2 ** 63
    k = np.unique((h * n_ent + t) * n_rel + r)
    return k // n_rel, k % n_rel


def _join_counts(pa, ra, pb, rb, n_rel):
    """out[x][y] = number of pair keys p with (p, x) in A and (p, y) in B; A and B distinct, B sorted by pair key."""
    lo, hi = np.searchsorted(pb, pa, 'left'), np.searchsorted(pb, pa, 'right')
    cnt = hi - lo
    total = int(cnt.sum())
    src = np.repeat(np.arange(len(pa)), cnt)
    within = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    cells = ra[src] * n_rel + rb[lo[src] + within]
    return np.bincount(cells, minlength=n_rel * n_rel).reshape(n_rel, n_rel).astype(np.int64)


def overlap(a, b, n_ent, n_rel):
    """(same, rev) int64 (n_rel, n_rel) of the fact lists a = (h, t, r) and b (None: b = a)."""
    b = a if b is None else b
    pa, ra = _distinct(a[0], a[1], a[2], n_ent, n_rel)
    pb, rb = _distinct(b[0], b[1], b[2], n_ent, n_rel)
    pbi, rbi = _distinct(b[1], b[0], b[2], n_ent, n_rel)            # T_inv of B
    return _join_counts(pa, ra, pb, rb, n_rel), _join_counts(pa, ra, pbi, rbi, n_rel)


def stats(h, t, r, n_ent, n_rel):
    """int64 (3, n_rel): facts with repeats, distinct heads, distinct tails per relation."""
    h, t, r = (np.asarray(x, dtype=np.int64) for x in (h, t, r))
    out = np.zeros((3, n_rel), dtype=np.int64)
    out[0] = np.bincount(r, minlength=n_rel)
    out[1] = np.bincount(np.unique(r * n_ent + h) // n_ent, minlength=n_rel)
    out[2] = np.bincount(np.unique(r * n_ent + t) // n_ent, minlength=n_rel)
    return out


def select(counts, lengths, theta1, theta2):
    """The pairs r1 < r2 in the order of itertools.combinations with c / len[r1] > theta1 and c / len[r2] > theta2 (Python
    float division of two ints); a zero length never qualifies."""
    counts, lengths = np.asarray(counts), np.asarray(lengths)
    out = []
    r1s, r2s = np.nonzero(np.triu(counts, 1))          # a zero count never passes a threshold >= 0 ... unless theta < 0:
    if theta1 < 0 or theta2 < 0:
        r1s, r2s = np.triu_indices(counts.shape[0], 1)
    for r1, r2 in zip(r1s.tolist(), r2s.tolist()):
        c, l1, l2 = int(counts[r1, r2]), int(lengths[r1]), int(lengths[r2])
        if l1 > 0 and l2 > 0 and c / l1 > theta1 and c / l2 > theta2:
            out.append((r1, r2))
    return out


def duplicates(kg_tr, kg_val, kg_te, theta1=0.8, theta2=0.8, reverses=None):
    reverses = [] if reverses is None else reverses
    n_ent, n_rel = kg_tr.n_ent, kg_tr.n_rel
    h, t, r = concat_kgs(kg_tr, kg_val, kg_te)
    lengths = stats(h, t, r, n_ent, n_rel)[0]
    same, rev = overlap((h, t, r), None, n_ent, n_rel)
    return select(same, lengths, theta1, theta2), [p for p in select(rev, lengths, theta1, theta2) if p not in reverses]


def count_triplets(kg1, kg2, duplicates, rev_duplicates):
    n_ent, n_rel = kg1.n_ent, kg1.n_rel
    same, rev = overlap((kg2.head_idx, kg2.tail_idx, kg2.relations), (kg1.head_idx, kg1.tail_idx, kg1.relations), n_ent, n_rel)
    return (sum(int(same[r1, r2]) + int(same[r2, r1]) for r1, r2 in duplicates),
            sum(int(rev[r1, r2]) + int(rev[r2, r1]) for r1, r2 in rev_duplicates))


def cartesian_product_relations(kg_tr, kg_val, kg_te, theta=0.8):
    h, t, r = concat_kgs(kg_tr, kg_val, kg_te)
    ln, s, o = stats(h, t, r, kg_tr.n_ent, kg_tr.n_rel).tolist()
    return [i for i in range(kg_tr.n_rel) if ln[i] > 0 and ln[i] / (s[i] * o[i]) > theta]
