# -*- coding: utf-8 -*-
"""Generate the relation-side golden fixture in this directory by RUNNING THE REAL REFERENCE
(torchkge v0.17.7 imported from /root/reference, CPU).  Run in the build container only (the
reference does not exist on the GPU box):

    python tests/golden/make_golden_relation.py

Output (committed): tests/golden/ref_relation.npz, written with fixed archive timestamps so that
a second run gives the same bytes.  Graph: make_golden.make_kg(0).

Sampler part.  For B = 64 (the first 64 facts) and B = all facts, the outputs of the reference's
BernoulliRelationNegativeSampler.corrupt_batch (sampling.py:526-553) under a fixed seed, and the
five arrays it consumed, recorded by replaying the same torch RNG calls under the same seed:
bernoulli(rel_share * ones(B)) -> mask_ent, randint(1, n_rel, (B - k,)) -> draws_r,
bernoulli(bern_probs[relations[mask_ent == 1]]) -> mask_head (COMPACT: one entry per entity
position), randint(1, n_ent, (q,)) -> draws_h, randint(1, n_ent, (k - q,)) -> draws_t.  Asserted
here: the replay reproduces the reference's outputs exactly, and all three branches occur.

Inference part, for the five model kinds whose tables ref_relpred.npz holds (make_golden.build_model;
the tables must equal the committed ones, they are not stored twice): the pairs are the last 64
facts, top_k = 3, b_size = 16, dictionary = kg.dict_of_rels.  The reference's
RelationInference.evaluate cannot run (it stores scores with a tuple index and raises IndexError
on the first batch), so its own pieces are called in its order: inference_prepare_candidates(
entities=False), inference_scoring_function, filter_scores(..., None), sort(descending=True), slice.
Recorded, raw and filtered: the (64, n_rel) score matrix, the top-3 ids and values, and the number
of rows where two ADJACENT finite scores among the top 4 lie within NEAR = 2e-5 -- twice the
project's score tolerance 1e-5: only there can an engine whose scores lie within 1e-5 of the
reference's order two relations differently.  Asserted: at most 2 % of the 64 rows per model and
variant, and every filtered row keeps at least 2 finite scores (so filtered top-3 rows do hold -inf).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchkge  # noqa: E402
from torchkge.sampling import BernoulliRelationNegativeSampler  # noqa: E402
from torchkge.utils import filter_scores  # noqa: E402
from make_golden import make_kg, build_model, tables_of, N_ENT, N_REL  # noqa: E402
from make_golden_triplet import save_npz  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
assert torchkge.__version__ == '0.17.7'
SEEDS = {64: 21, 'all': 22}
N_PAIRS, TOP_K, B_SIZE, NEAR = 64, 3, 16, 2e-5
KINDS = ('transe', 'distmult', 'complex', 'transh', 'transd')


def replay(samp, h, t, r, seed):
    """The five arrays corrupt_batch(h, t, r) consumes under ``seed`` and the negatives they give, restated."""
    torch.manual_seed(seed)
    B = h.shape[0]
    mask_ent = torch.bernoulli(samp.rel_share * torch.ones(B))
    k = int(mask_ent.sum().item())
    draws_r = torch.randint(1, samp.kg.n_rel, (B - k,))
    mask_head = torch.bernoulli(samp.bern_probs[r[mask_ent == 1]])
    q = int(mask_head.sum().item())
    draws_h = torch.randint(1, samp.n_ent, (q,))
    draws_t = torch.randint(1, samp.n_ent, (k - q,))
    nh, nt, nr = h.clone(), t.clone(), r.clone()
    nr[mask_ent == 0] = draws_r
    ent = torch.nonzero(mask_ent == 1).flatten()
    nh[ent[mask_head == 1]] = draws_h
    nt[ent[mask_head == 0]] = draws_t
    arrays = dict(mask_ent=mask_ent.numpy().astype(np.uint8), mask_head=mask_head.numpy().astype(np.uint8),
                  draws_r=draws_r.numpy(), draws_h=draws_h.numpy(), draws_t=draws_t.numpy())
    return arrays, nh, nt, nr


def near_rows(values):
    """Rows of the descending (n, >= 4) matrix where two adjacent finite scores among the first 4 lie within NEAR."""
    top = values[:, :4].double()
    gap = top[:, :-1] - top[:, 1:]
    both = torch.isfinite(top[:, :-1]) & torch.isfinite(top[:, 1:])
    return int(((gap <= NEAR) & both).any(dim=1).sum())


def main():
    kg = make_kg(0)
    assert (kg.n_facts, kg.n_ent, kg.n_rel) == (1385, N_ENT, N_REL)
    out = dict(n_ent=N_ENT, n_rel=N_REL, near=NEAR, top_k=TOP_K, b_size=B_SIZE, n_pairs=N_PAIRS,
               heads=kg.head_idx.numpy(), tails=kg.tail_idx.numpy(), rels=kg.relations.numpy())

    # ---- sampler ---------------------------------------------------------------------------------------------
    samp = BernoulliRelationNegativeSampler(kg)
    assert samp.rel_share == .33
    out.update(bern_probs=samp.bern_probs.numpy(), rel_share=samp.rel_share)
    for which, seed in SEEDS.items():
        B = kg.n_facts if which == 'all' else which
        h, t, r = kg.head_idx[:B], kg.tail_idx[:B], kg.relations[:B]
        torch.manual_seed(seed)
        ref_h, ref_t, ref_r = samp.corrupt_batch(h, t, r)                      # the reference as it is
        arrays, nh, nt, nr = replay(samp, h, t, r, seed)
        assert torch.equal(ref_h, nh) and torch.equal(ref_t, nt) and torch.equal(ref_r, nr), 'the order of draws is not the replayed one'
        n_ent_pos, n_head = int(arrays['mask_ent'].sum()), int(arrays['mask_head'].sum())
        assert 0 < n_head < n_ent_pos < B, 'a branch is not taken'
        assert len(arrays['mask_head']) == n_ent_pos and len(arrays['draws_r']) == B - n_ent_pos
        assert len(arrays['draws_h']) == n_head and len(arrays['draws_t']) == n_ent_pos - n_head
        if B == 64:
            assert (n_ent_pos, n_head, B - n_ent_pos) == (20, 4, 44)
        print('B %4d: entity positions %d (heads %d), relation positions %d' % (B, n_ent_pos, n_head, B - n_ent_pos))
        tag = 'b%s_' % which
        out[tag + 'seed'] = seed
        for nm, a in arrays.items():
            out[tag + nm] = a
        out[tag + 'neg_heads'], out[tag + 'neg_tails'], out[tag + 'neg_rels'] = ref_h.numpy(), ref_t.numpy(), ref_r.numpy()

    # ---- inference, five model kinds ---------------------------------------------------------------------------
    e1, e2, true_r = kg.head_idx[-N_PAIRS:], kg.tail_idx[-N_PAIRS:], kg.relations[-N_PAIRS:]
    z = np.load(os.path.join(HERE, 'ref_relpred.npz'))
    for kind in KINDS:
        m = build_model(kind, 2)
        for i, tb in enumerate(tables_of(kind, m)):
            assert np.array_equal(tb, z['%s_table%d' % (kind, i)]), (kind, i)
        raw, filt = [], []
        with torch.no_grad():
            for lo in range(0, N_PAIRS, B_SIZE):
                a, b = e1[lo:lo + B_SIZE], e2[lo:lo + B_SIZE]
                h_emb, t_emb, _, cand = m.inference_prepare_candidates(a, b, torch.tensor([]).long(), entities=False)
                s = m.inference_scoring_function(h_emb, t_emb, cand)
                raw.append(s)
                filt.append(filter_scores(s, kg.dict_of_rels, a, b, None))
        for variant, mat in (('raw', torch.cat(raw)), ('filt', torch.cat(filt))):
            vals, ids = mat.sort(descending=True)
            n_near = near_rows(vals)
            n_finite = torch.isfinite(mat).sum(dim=1)
            print('%-9s %-4s near-tie rows %d / %d, fewest finite scores in a row %d'
                  % (kind, variant, n_near, N_PAIRS, int(n_finite.min())))
            assert n_near <= 0.02 * N_PAIRS, (kind, variant, n_near)
            assert int(n_finite.min()) >= 2
            if variant == 'filt':
                assert int(n_finite.min()) < TOP_K          # filtered top-3 rows do hold -inf
                # every pair is a fact of the graph: its own relation is among the masked ones
                assert bool(torch.isinf(mat[torch.arange(N_PAIRS), true_r]).all())
            tag = '%s_%s_' % (kind, variant)
            out[tag + 'scores'] = mat.numpy()
            out[tag + 'top_ids'], out[tag + 'top_vals'] = ids[:, :TOP_K].numpy(), vals[:, :TOP_K].numpy()
            out[tag + 'near'] = n_near
    path = os.path.join(HERE, 'ref_relation.npz')
    save_npz(path, out)
    print('ref_relation.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
