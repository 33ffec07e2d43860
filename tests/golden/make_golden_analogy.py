# -*- coding: utf-8 -*-
"""Generate the ANALOGY golden fixture in this directory by RUNNING THE REAL
REFERENCE (torchkge v0.17.7 imported from /root/reference, CPU).  Run in the
build container only (the reference does not exist on the GPU box):

    python tests/golden/make_golden_analogy.py

Output (committed): tests/golden/ref_analogy.npz.  Same knowledge graph, sizes,
b_size and table perturbation as make_golden.py, seed 0.  It holds, for
AnalogyModel(32, scalar_share=0.5): the six tables, the reference's
scoring_function, forward (n_neg = 2, with the negatives), inference_scoring_function
on both sides and on the relations, the LinkPredictionEvaluator ranks + metrics,
the RelationPredictionEvaluator ranks + metrics (directed and undirected) and the
state_dict's keys and shapes; and, under the prefix ``u_``, a second model with an
UNEVEN split, AnalogyModel(33, scalar_share=0.3) = 9 | 24 | 24: tables,
scoring_function and forward only -- the reference's inference_scoring_function
adds (b, N, scalar_dim) to (b, N, complex_dim) tensors and raises unless the two
are equal, so the reference cannot evaluate that model.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchkge  # noqa: E402
from torchkge.evaluation import LinkPredictionEvaluator, RelationPredictionEvaluator  # noqa: E402
from torchkge.models import AnalogyModel  # noqa: E402
from make_golden import make_kg, sub_kg, N_ENT, N_REL, DIM, N_TEST, B  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
assert torchkge.__version__ == '0.17.7'
NAMES = ['sc_ent_emb', 're_ent_emb', 'im_ent_emb', 'sc_rel_emb', 're_rel_emb', 'im_rel_emb']


def build_model(dim, share):
    torch.manual_seed(0)
    m = AnalogyModel(dim, N_ENT, N_REL, scalar_share=share)
    with torch.no_grad():       # the perturbation of make_golden.py
        for prm in m.parameters():
            if prm.requires_grad:
                prm.mul_(1.0 + 0.05 * torch.sin(torch.arange(prm.numel()).float()).view_as(prm))
    return m


def training_outputs(m, kg_test, prefix):
    h, t, r = kg_test.head_idx[:B], kg_test.tail_idx[:B], kg_test.relations[:B]
    out = {}
    for i, n in enumerate(NAMES):
        out['%stable%d' % (prefix, i)] = getattr(m, n).weight.detach().clone().numpy()
    with torch.no_grad():
        g = torch.Generator().manual_seed(7)
        nh = torch.randint(0, N_ENT, (2 * B,), generator=g)
        nt = torch.randint(0, N_ENT, (2 * B,), generator=g)
        pos, neg = m(h, t, r, nh, nt)
        out.update({prefix + 'sf': m.scoring_function(h, t, r).numpy(), prefix + 'fwd_pos': pos.numpy(),
                    prefix + 'fwd_neg': neg.numpy(), prefix + 'neg_heads': nh.numpy(), prefix + 'neg_tails': nt.numpy()})
    return out


def main():
    kg = make_kg(1234)
    kg_test = sub_kg(kg, N_TEST)
    out = dict(heads=kg.head_idx.numpy(), tails=kg.tail_idx.numpy(), rels=kg.relations.numpy(),
               n_test=N_TEST, n_ent=N_ENT, n_rel=N_REL, b_size=B, dim=DIM, share=0.5, u_dim=33, u_share=0.3)
    m = build_model(DIM, 0.5)
    out.update(training_outputs(m, kg_test, ''))
    sd = m.state_dict()
    out['state_keys'] = np.array(list(sd))
    out['state_shapes'] = np.array([list(v.shape) for v in sd.values()], dtype=np.int64)
    h, t, r = kg_test.head_idx[:B], kg_test.tail_idx[:B], kg_test.relations[:B]
    with torch.no_grad():
        h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=True)
        out['s_tail'] = m.inference_scoring_function(h_e, cand, r_e).numpy()
        out['s_head'] = m.inference_scoring_function(cand, t_e, r_e).numpy()
        h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=False)
        out['s_rel'] = m.inference_scoring_function(h_e, t_e, cand).numpy()
        ev = LinkPredictionEvaluator(m, kg_test)
        ev.evaluate(b_size=B, verbose=False)
        out.update(rank_true_heads=ev.rank_true_heads.numpy(), rank_true_tails=ev.rank_true_tails.numpy(),
                   filt_rank_true_heads=ev.filt_rank_true_heads.numpy(),
                   filt_rank_true_tails=ev.filt_rank_true_tails.numpy(),
                   hit10=np.array(ev.hit_at_k(10)), mrr=np.array(ev.mrr()), mean_rank=np.array(ev.mean_rank()))
        print('link prediction: hit10', ev.hit_at_k(10), 'mrr', ev.mrr())
        for directed in (True, False):
            rv = RelationPredictionEvaluator(m, kg_test, directed=directed)
            rv.evaluate(b_size=B, verbose=False)
            tag = 'dir' if directed else 'undir'
            out[tag + '_rank'] = rv.rank_true_rels.numpy()
            out[tag + '_frank'] = rv.filt_rank_true_rels.numpy()
            out[tag + '_mrr'] = np.array(rv.mrr())
            out[tag + '_hit3'] = np.array(rv.hit_at_k(3))
    u = build_model(33, 0.3)
    assert (u.scalar_dim, u.complex_dim) == (9, 24)
    out.update(training_outputs(u, kg_test, 'u_'))
    path = os.path.join(HERE, 'ref_analogy.npz')
    np.savez_compressed(path, **out)
    print('ref_analogy.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
