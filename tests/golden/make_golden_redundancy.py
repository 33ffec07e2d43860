# -*- coding: utf-8 -*-
"""Generate the data-redundancy golden fixture in this directory by RUNNING THE REAL REFERENCE
(torchkge v0.17.7 imported from /root/reference, CPU).  Run in the build container only (the
reference does not exist on the GPU box):

    python tests/golden/make_golden_redundancy.py

Output (committed): tests/golden/ref_redundancy.npz, written with fixed archive timestamps so that
a second run gives the same bytes.

The graph is made so that the reference runs at all: n_rel = 1345 exactly (data_redundancy.py:147
hard-codes range(1345)) and every relation holds at least one fact (an empty one divides by zero).
48 entities, about 6,000 facts:

  * 1-6 random facts for every relation that is not planted;
  * 40 planted relation pairs (ra, rb), relation ids drawn at random: ra holds 20 pairs (h, t), rb
    holds 14 / 16 / 18 / 20 of them (70 / 80 / 90 / 100 %) -- as (t, h) in every second group of four
    -- and, in every second group of eight, other pairs up to 20 facts (so both lengths are 20 and
    the ratios are 0.7 / 0.8 / 0.9 / 1.0 exactly); in the other groups rb holds the shared pairs only
    (lengths 20 and k: the two ratios differ, which tells theta1 from theta2);
  * one 5 x 7 cartesian relation, and one that holds 25 of its 5 x 7 pairs (ratio 0.71: in at 0.5,
    out at 0.8);
  * self-loops (a, a) shared by two relations, three times;
  * after the shuffle and the 80 / 10 / 10 split, 12 train facts of unplanted relations repeated in
    the validation and the test split (lengths count them, the pair sets do not).

Recorded: the three splits (int32), duplicates / rev_duplicates at (0.8, 0.8) and (0.5, 0.9), the
same at (0.8, 0.8) with a non-empty ``reverses``, cartesian_product_relations at 0.8 and 0.5, and
count_triplets of the (0.8, 0.8) lists for (train, train), (train, test), (test, test).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchkge  # noqa: E402
from torchkge.data_structures import KnowledgeGraph  # noqa: E402
from torchkge.utils import data_redundancy as ref  # noqa: E402
from make_golden_triplet import save_npz  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
assert torchkge.__version__ == '0.17.7'
N_ENT, N_REL, N_PLANTED, PAIRS, SEED = 48, 1345, 40, 20, 1909


def make_facts():
    rng = np.random.RandomState(SEED)
    rel_ids = rng.permutation(N_REL)
    planted_rels = rel_ids[:2 * N_PLANTED].reshape(N_PLANTED, 2)
    cart_rel, part_rel = int(rel_ids[2 * N_PLANTED]), int(rel_ids[2 * N_PLANTED + 1])
    loop_rels = rel_ids[2 * N_PLANTED + 2:2 * N_PLANTED + 8].reshape(3, 2)
    special = set(planted_rels.ravel().tolist()) | {cart_rel, part_rel}
    facts, planted = [], []
    for i, (ra, rb) in enumerate(planted_rels.tolist()):
        share, reverse, extras = (14, 16, 18, 20)[i % 4], (i // 4) % 2 == 1, (i // 8) % 2 == 0
        # 2 * PAIRS - share distinct unordered pairs {a, b}, a != b, each with a random orientation
        un = rng.permutation(N_ENT * N_ENT)
        un = [(int(u // N_ENT), int(u % N_ENT)) for u in un if u // N_ENT < u % N_ENT][:2 * PAIRS - share]
        pairs = [(a, b) if rng.randint(2) else (b, a) for a, b in un]
        facts += [(h, t, ra) for h, t in pairs[:PAIRS]]
        facts += [((t, h, rb) if reverse else (h, t, rb)) for h, t in pairs[:share]]
        if extras:
            facts += [(h, t, rb) for h, t in pairs[PAIRS:]]
        planted.append((min(ra, rb), max(ra, rb), share, PAIRS, PAIRS if extras else share, reverse))
    facts += [(h, t, cart_rel) for h in range(3, 8) for t in range(20, 27)]
    facts += [(h, t, part_rel) for h in range(10, 15) for t in range(30, 37) if (h + t) % 7 > 1]      # 25 of 5 x 7
    for r in range(N_REL):
        if r in special:
            continue
        for _ in range(rng.randint(1, 7)):
            facts.append((int(rng.randint(N_ENT)), int(rng.randint(N_ENT)), r))
    for k, (r1, r2) in enumerate(loop_rels.tolist()):
        for a in (5 + k, 30 + k):
            facts += [(a, a, r1), (a, a, r2)]
    facts = np.array(facts, dtype=np.int64)
    facts = facts[rng.permutation(len(facts))]
    n = len(facts)
    n_tr, n_val = int(0.8 * n), int(0.1 * n)
    tr, val, te = facts[:n_tr], facts[n_tr:n_tr + n_val], facts[n_tr + n_val:]
    plain = np.array([f for f in tr.tolist() if f[2] not in special][:12], dtype=np.int64)
    val, te = np.concatenate([val, plain]), np.concatenate([te, plain])
    return tr, val, te, planted


def graph(f):
    return KnowledgeGraph(kg={'heads': torch.from_numpy(f[:, 0].copy()), 'tails': torch.from_numpy(f[:, 1].copy()),
                              'relations': torch.from_numpy(f[:, 2].copy())},
                          ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})


def pair_array(lst):
    return np.array(lst, dtype=np.int32).reshape(-1, 2)


def main():
    tr, val, te, planted = make_facts()
    allf = np.concatenate([tr, val, te])
    assert set(allf[:, 2].tolist()) == set(range(N_REL)), 'every relation needs a fact'
    assert allf[:, :2].max() == N_ENT - 1 and allf[:, 2].max() == N_REL - 1
    kgs = [graph(f) for f in (tr, val, te)]
    assert all(k.n_rel == N_REL and k.n_ent == N_ENT for k in kgs)
    print('facts', len(allf), 'train / valid / test', len(tr), len(val), len(te))
    out = dict(n_ent=N_ENT, n_rel=N_REL)
    for nm, f in (('train', tr), ('valid', val), ('test', te)):
        out[nm + '_heads'], out[nm + '_tails'], out[nm + '_rels'] = (f[:, i].astype(np.int32) for i in range(3))

    # a planted pair whose two ratios equal a threshold exactly: '>' must leave it out
    lengths = np.bincount(allf[:, 2], minlength=N_REL)
    at_threshold = [p for p in planted if p[2] / lengths[p[0]] == 0.8 and p[2] / lengths[p[1]] == 0.8]
    assert at_threshold, 'no planted pair sits exactly on the threshold'

    dup, rev = ref.duplicates(*kgs, theta1=0.8, theta2=0.8)
    assert dup and rev, 'both lists must be non-empty'
    for p in at_threshold:
        assert (p[0], p[1]) not in dup and (p[0], p[1]) not in rev
    dup2, rev2 = ref.duplicates(*kgs, theta1=0.5, theta2=0.9)
    assert dup2 and rev2 and (dup2 != dup or rev2 != rev)
    reverses = rev[::3] + [(0, 1)]
    dup3, rev3 = ref.duplicates(*kgs, theta1=0.8, theta2=0.8, reverses=reverses)
    assert dup3 == dup and len(rev3) < len(rev)
    out.update(dup_08_08=pair_array(dup), rev_08_08=pair_array(rev), dup_05_09=pair_array(dup2), rev_05_09=pair_array(rev2),
               reverses=pair_array(reverses), dup_08_08_reverses=pair_array(dup3), rev_08_08_reverses=pair_array(rev3))
    cart8, cart5 = ref.cartesian_product_relations(*kgs, theta=0.8), ref.cartesian_product_relations(*kgs, theta=0.5)
    assert cart8 and len(cart5) > len(cart8)
    out.update(cart_08=np.array(cart8, dtype=np.int32), cart_05=np.array(cart5, dtype=np.int32))
    for nm, (k1, k2) in (('train_train', (kgs[0], kgs[0])), ('train_test', (kgs[0], kgs[2])), ('test_test', (kgs[2], kgs[2]))):
        out['count_' + nm] = np.array(ref.count_triplets(k1, k2, dup, rev), dtype=np.int64)
        print('count_triplets', nm, out['count_' + nm].tolist())
    print('duplicates %d, reverse %d at (0.8, 0.8); %d, %d at (0.5, 0.9); %d reverse with `reverses`; cartesian %d / %d; '
          '%d planted pairs exactly on 0.8' % (len(dup), len(rev), len(dup2), len(rev2), len(rev3), len(cart8), len(cart5),
                                               len(at_threshold)))
    path = os.path.join(HERE, 'ref_redundancy.npz')
    save_npz(path, out)
    print('ref_redundancy.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 200 * 1024


if __name__ == '__main__':
    main()
