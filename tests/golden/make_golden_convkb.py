# -*- coding: utf-8 -*-
"""Generate the ConvKB golden fixture in this directory by RUNNING THE REAL
REFERENCE (torchkge v0.17.7 imported from /root/reference, CPU).  Run in the
build container only (the reference does not exist on the GPU box):

    python tests/golden/make_golden_convkb.py

Output (committed): tests/golden/ref_convkb.npz.  Same knowledge graph, sizes,
b_size and parameter perturbation as make_golden.py / make_golden_analogy.py, seed 0.
The model is ConvKBModel(32, 5, N_ENT, N_REL) with ``output.0.weight`` multiplied by
HEAD_GAIN = 32 after the perturbation: with the default head every score lies in
0.509-0.533 and about two candidates per query fall inside the 2e-5 tie interval of
the true score; with the x32 head the scores span 0.17-0.83 and the tie intervals are
almost always a single rank.  It holds the six parameters, the reference's
scoring_function, forward (n_neg = 2, with the negatives), inference_scoring_function
on both sides and on the relations, the LinkPredictionEvaluator ranks + metrics, the
RelationPredictionEvaluator ranks + metrics (directed and undirected) and the
state_dict's keys and shapes.

Asserted here: the reference's fp32 scores lie within 2.5e-6 of its own float64 run,
and the number of OTHER candidates inside the 2e-5 tie interval of the true score
is <= 0.25 on average and <= 2 at most over the checked queries.
"""
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchkge  # noqa: E402
from torchkge.evaluation import LinkPredictionEvaluator, RelationPredictionEvaluator  # noqa: E402
from torchkge.models import ConvKBModel  # noqa: E402
from make_golden import make_kg, sub_kg, N_ENT, N_REL, DIM, N_TEST, B  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
assert torchkge.__version__ == '0.17.7'
N_FILTERS = 5
HEAD_GAIN = 32.0
TIE = 2e-5
PARAMS = ['ent_emb.weight', 'rel_emb.weight', 'convlayer.0.weight', 'convlayer.0.bias', 'output.0.weight', 'output.0.bias']


def build_model():
    torch.manual_seed(0)
    m = ConvKBModel(DIM, N_FILTERS, N_ENT, N_REL)
    with torch.no_grad():       # the perturbation of make_golden.py
        for prm in m.parameters():
            if prm.requires_grad:
                prm.mul_(1.0 + 0.05 * torch.sin(torch.arange(prm.numel()).float()).view_as(prm))
        m.output[0].weight.mul_(HEAD_GAIN)
    return m


def all_scores(m, h, t, r):
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=True)
    s_tail = m.inference_scoring_function(h_e, cand, r_e)
    s_head = m.inference_scoring_function(cand, t_e, r_e)
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=False)
    return s_tail, s_head, m.inference_scoring_function(h_e, t_e, cand)


def main():
    kg = make_kg(1234)
    kg_test = sub_kg(kg, N_TEST)
    out = dict(heads=kg.head_idx.numpy(), tails=kg.tail_idx.numpy(), rels=kg.relations.numpy(),
               n_test=N_TEST, n_ent=N_ENT, n_rel=N_REL, b_size=B, dim=DIM, n_filters=N_FILTERS, head_gain=HEAD_GAIN)
    m = build_model()
    sd = m.state_dict()
    assert list(sd) == PARAMS
    out['state_keys'] = np.array(list(sd))
    out['state_shapes'] = np.array([list(v.shape) + [0] * (3 - v.dim()) for v in sd.values()], dtype=np.int64)
    out['state_ndim'] = np.array([v.dim() for v in sd.values()], dtype=np.int64)
    for i, n in enumerate(PARAMS):
        out['table%d' % i] = sd[n].detach().clone().numpy()
    h, t, r = kg_test.head_idx[:B], kg_test.tail_idx[:B], kg_test.relations[:B]
    with torch.no_grad():
        g = torch.Generator().manual_seed(7)
        nh = torch.randint(0, N_ENT, (2 * B,), generator=g)
        nt = torch.randint(0, N_ENT, (2 * B,), generator=g)
        pos, neg = m(h, t, r, nh, nt)
        out.update(sf=m.scoring_function(h, t, r).numpy(), fwd_pos=pos.numpy(), fwd_neg=neg.numpy(),
                   neg_heads=nh.numpy(), neg_tails=nt.numpy())
        s_tail, s_head, s_rel = all_scores(m, h, t, r)
        out.update(s_tail=s_tail.numpy(), s_head=s_head.numpy(), s_rel=s_rel.numpy())
        # the reference against its own float64 run, and the population of the tie intervals of the true scores
        m64 = copy.deepcopy(m).double()
        d_tail, d_head, d_rel = all_scores(m64, h, t, r)
        err = max(float((a.double() - b).abs().max()) for a, b in ((s_tail, d_tail), (s_head, d_head), (s_rel, d_rel)))
        print('fp32 vs float64 reference: max |diff| = %.3g' % err)
        assert err <= 2.5e-6, err
        near = []
        for s, true in ((d_tail, t), (d_head, h)):
            st = s.gather(1, true.view(-1, 1))
            near.append(((s - st).abs() <= TIE).sum(dim=1) - 1)
        near = torch.cat(near).double()
        print('scores span %.3f .. %.3f; other candidates inside the tie interval: mean %.3f, max %d'
              % (float(d_tail.min()), float(d_tail.max()), float(near.mean()), int(near.max())))
        assert float(near.mean()) <= 0.25 and int(near.max()) <= 2
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
    path = os.path.join(HERE, 'ref_convkb.npz')
    np.savez_compressed(path, **out)
    print('ref_convkb.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
