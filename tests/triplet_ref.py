"""numpy restatement of the three contracts of include/kge_hip_triplet.h and the loader of tests/golden/ref_triplet.npz
(tests/golden/make_golden_triplet.py), shared by tests/test_triplet_host.py and tests/test_gpu_triplet.py.  Test-only."""
import os

import numpy as np
import torch

from tests.helpers import GOLDEN, KIND_FILES, N_TABLES

CASES = [('transe', 2), ('transe', 1), ('transh', 2), ('transd', 2), ('distmult', 2), ('complex', 2)]
_CACHE = {}


def tag(kind, p):
    return kind + ('_l1' if p == 1 else '')


def fixture():
    """The fixture as a dict of arrays: loaded once, shared, left unchanged."""
    if 'z' not in _CACHE:
        with np.load(os.path.join(GOLDEN, 'ref_triplet.npz')) as z:
            _CACHE['z'] = {k: z[k] for k in z.files}
        for v in _CACHE['z'].values():
            v.setflags(write=False)
    return _CACHE['z']


def fixture_tables(kind, p):
    """The model tables of the kind, from its own committed fixture (ref_triplet.npz does not repeat them)."""
    z = np.load(os.path.join(GOLDEN, KIND_FILES[(kind, p)]))
    return [torch.from_numpy(z['table%d' % i]) for i in range(N_TABLES[kind])]


def fixture_kgs(tk, device=None):
    """(kg_val, kg_test) of the fixture as torchkge_amd KnowledgeGraphs."""
    z = fixture()
    n_ent, n_rel = int(z['n_ent']), int(z['n_rel'])
    out = []
    for part in ('val', 'test'):
        h, t, r = (torch.from_numpy(z['%s_%s' % (part, nm)].copy()) for nm in ('heads', 'tails', 'rels'))
        if device is not None:
            h, t, r = h.to(device), t.to(device), r.to(device)
        out.append(tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                                     rel2ix={i: i for i in range(n_rel)}))
    return out


def fixture_batches(which):
    """Per recorded batch of corrupt_kg(b_size = 64, which): a dict of heads, tails, rels, mask, u_h, u_t, fb_h, fb_t and
    the reference's neg_heads / neg_tails."""
    z = fixture()
    part = 'val' if which == 'main' else 'test'
    b, n = int(z['b_size']), len(z[part + '_heads'])
    out, ph, pt = [], 0, 0
    for i, lo in enumerate(range(0, n, b)):
        hi = min(lo + b, n)
        k = int(z[which + '_k'][i])
        kt = hi - lo - k
        d = dict(heads=z[part + '_heads'][lo:hi], tails=z[part + '_tails'][lo:hi], rels=z[part + '_rels'][lo:hi],
                 mask=z[which + '_mask'][lo:hi], neg_heads=z[which + '_neg_heads'][lo:hi],
                 neg_tails=z[which + '_neg_tails'][lo:hi])
        for nm in ('u_h', 'fb_h'):
            d[nm] = z['%s_%s' % (which, nm)][ph:ph + k]
        for nm in ('u_t', 'fb_t'):
            d[nm] = z['%s_%s' % (which, nm)][pt:pt + kt]
        ph, pt = ph + k, pt + kt
        out.append(d)
    assert ph == len(z[which + '_u_h']) and pt == len(z[which + '_u_t'])
    return out


# ---- the three contracts ------------------------------------------------------------------------------------------
def _replace(keep, rels, u, fb, offsets, values, n_rel):
    rels = np.asarray(rels, dtype=np.int64)
    inside = (rels >= 0) & (rels < n_rel)
    rc = np.where(inside, rels, 0)
    lo = offsets[rc]
    n = np.where(inside, offsets[rc + 1] - lo, 0)
    x = np.floor(n.astype(np.float32) * np.asarray(u, dtype=np.float32))        # one fp32 multiply
    assert x.dtype == np.float32
    with np.errstate(invalid='ignore'):
        c = np.where(x > 0, np.minimum(x, np.float32(9.0e18)), np.float32(0)).astype(np.int64)
    c = np.minimum(c, np.maximum(n - 1, 0))
    vals = np.concatenate([np.asarray(values, dtype=np.int64), [0]])            # (an empty index still indexes)
    picked = vals[np.where(n > 0, lo + c, len(vals) - 1)]
    empty = np.asarray(fb, dtype=np.int64) if fb is not None else np.asarray(keep, dtype=np.int64)
    return np.where(n > 0, picked, empty)


def positional_corrupt(heads, tails, rels, mask, u_h, u_t, fb_h, fb_t, offsets_h, values_h, offsets_t, values_t):
    """kge_positional_corrupt.  u_* / fb_* may be longer than the number of positions that consume them."""
    heads, tails, rels = (np.asarray(x, dtype=np.int64) for x in (heads, tails, rels))
    m = np.asarray(mask) != 0
    n_rel = len(offsets_h) - 1
    k, kt = int(m.sum()), int((~m).sum())
    nh, nt = heads.copy(), tails.copy()
    nh[m] = _replace(heads[m], rels[m], u_h[:k], None if fb_h is None else fb_h[:k], offsets_h, values_h, n_rel)
    nt[~m] = _replace(tails[~m], rels[~m], u_t[:kt], None if fb_t is None else fb_t[:kt], offsets_t, values_t, n_rel)
    return nh, nt


def relation_max(scores, rels, n_rel):
    """kge_relation_max: NaN-propagating per-relation maximum from -inf, absent relations take the overall maximum."""
    scores, rels = np.asarray(scores, dtype=np.float32), np.asarray(rels, dtype=np.int64)
    thr = np.full(n_rel, -np.inf, dtype=np.float32)
    inside = (rels >= 0) & (rels < n_rel)
    with np.errstate(invalid='ignore'):
        np.maximum.at(thr, rels[inside], scores[inside])    # np.maximum propagates NaN
    present = np.bincount(rels[inside], minlength=n_rel) > 0
    thr[~present] = np.max(scores)                          # np.max propagates NaN
    return thr


def threshold_count(pos, neg, rels, thr):
    """kge_threshold_count: (#{pos > thr[rels]}, #{neg < thr[rels]}), strict fp32 compares."""
    pos, neg, thr = (np.asarray(x, dtype=np.float32) for x in (pos, neg, thr))
    rels = np.asarray(rels, dtype=np.int64)
    inside = (rels >= 0) & (rels < len(thr))
    t = thr[np.where(inside, rels, 0)]
    with np.errstate(invalid='ignore'):
        return int(((pos > t) & inside).sum()), int(((neg < t) & inside).sum())


def same_values(a, b):
    """Equal by value, NaN = NaN (and +0.0 = -0.0)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
