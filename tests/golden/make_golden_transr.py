# -*- coding: utf-8 -*-
"""Generate the TransR golden fixture in this directory by RUNNING THE REAL
REFERENCE (torchkge v0.17.7 imported from /root/reference, CPU).  Run in the
build container only (the reference does not exist on the GPU box):

    python tests/golden/make_golden_transr.py

Output (committed): tests/golden/ref_transr.npz.  Same knowledge graph, sizes
and b_size as make_golden.py; TransRModel(DIM, DIM_REL, ...) = (32, 24).  The
tables are set from torch.Generator().manual_seed(17): ent_emb = randn * 0.25,
rel_emb = randn * 0.2, proj_mat = randn * 0.15, drawn in that order, so that
||q||^2 + max ||M_r e||^2 stays inside the engine's expansion limit and no
candidate's score lies within 2e-5 of a true score (ranks are then unique).
The file holds the constructor's tables (seed 0), the set tables, the
reference's scoring_function, forward (n_neg = 2), the gradients of
(scoring_function * g).sum() wrt the three tables, inference_scoring_function
on both sides, the relation-candidate scores, LinkPredictionEvaluator and
RelationPredictionEvaluator (directed and undirected) ranks + metrics, and the
sorted state_dict keys.  The reference's (n_rel, n_ent, d_r) projected_entities
cache is NOT stored.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchkge  # noqa: E402
from torchkge.evaluation import LinkPredictionEvaluator, RelationPredictionEvaluator  # noqa: E402
from torchkge.models import TransRModel  # noqa: E402
from make_golden import make_kg, sub_kg, N_ENT, N_REL, DIM, DIM_REL, N_TEST, B  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
assert torchkge.__version__ == '0.17.7'


def main():
    kg = make_kg(1234)
    kg_test = sub_kg(kg, N_TEST)
    out = dict(heads=kg.head_idx.numpy(), tails=kg.tail_idx.numpy(), rels=kg.relations.numpy(),
               n_test=N_TEST, n_ent=N_ENT, n_rel=N_REL, b_size=B, dim=DIM, dim_rel=DIM_REL)
    torch.manual_seed(0)
    m = TransRModel(DIM, DIM_REL, N_ENT, N_REL)
    names = ('ent_emb', 'rel_emb', 'proj_mat')
    for i, n in enumerate(names):
        out['ctor_table%d' % i] = getattr(m, n).weight.detach().clone().numpy()
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        m.ent_emb.weight.copy_(torch.randn(N_ENT, DIM, generator=g) * 0.25)
        m.rel_emb.weight.copy_(torch.randn(N_REL, DIM_REL, generator=g) * 0.2)
        m.proj_mat.weight.copy_(torch.randn(N_REL, DIM_REL * DIM, generator=g) * 0.15)
    for i, n in enumerate(names):
        out['table%d' % i] = getattr(m, n).weight.detach().clone().numpy()
    h, t, r = kg_test.head_idx[:B], kg_test.tail_idx[:B], kg_test.relations[:B]
    with torch.no_grad():
        out['sf'] = m.scoring_function(h, t, r).numpy()
        gn = torch.Generator().manual_seed(7)
        nh = torch.randint(0, N_ENT, (2 * B,), generator=gn)
        nt = torch.randint(0, N_ENT, (2 * B,), generator=gn)
        pos, neg = m(h, t, r, nh, nt)
    gvec = torch.randn(B, generator=gn)
    m.zero_grad()
    (m.scoring_function(h, t, r) * gvec).sum().backward()
    out.update(fwd_pos=pos.numpy(), fwd_neg=neg.numpy(), neg_heads=nh.numpy(), neg_tails=nt.numpy(), grad_out=gvec.numpy(),
               grad_ent=m.ent_emb.weight.grad.clone().numpy(), grad_rel=m.rel_emb.weight.grad.clone().numpy(),
               grad_proj=m.proj_mat.weight.grad.clone().numpy())
    with torch.no_grad():
        m.evaluated_projections = False
        ev = LinkPredictionEvaluator(m, kg_test)
        ev.evaluate(b_size=B, verbose=False)
        h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=True)
        out['s_tail'] = m.inference_scoring_function(h_e, cand, r_e).numpy()
        out['s_head'] = m.inference_scoring_function(cand, t_e, r_e).numpy()
        out.update(rank_true_heads=ev.rank_true_heads.numpy(), rank_true_tails=ev.rank_true_tails.numpy(),
                   filt_rank_true_heads=ev.filt_rank_true_heads.numpy(),
                   filt_rank_true_tails=ev.filt_rank_true_tails.numpy(),
                   hit10=np.array(ev.hit_at_k(10)), mrr=np.array(ev.mrr()), mean_rank=np.array(ev.mean_rank()))
        h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=False)
        out['s_rel'] = m.inference_scoring_function(h_e, t_e, cand).numpy()
        for directed in (True, False):
            rv = RelationPredictionEvaluator(m, kg_test, directed=directed)
            rv.evaluate(b_size=B, verbose=False)
            tag = 'rel_dir' if directed else 'rel_undir'
            out[tag + '_rank'] = rv.rank_true_rels.numpy()
            out[tag + '_frank'] = rv.filt_rank_true_rels.numpy()
            out[tag + '_mrr'] = np.array(rv.mrr())
            out[tag + '_hit3'] = np.array(rv.hit_at_k(3))
    keys = sorted(m.state_dict().keys())
    assert 'projected_entities' in keys
    out['state_dict_keys'] = np.array(keys)
    assert 'projected_entities' not in out
    np.savez_compressed(os.path.join(HERE, 'ref_transr.npz'), **out)
    smax = max(np.abs(out['s_tail']).max(), np.abs(out['s_head']).max())
    print('ref_transr.npz', 'hit10', ev.hit_at_k(10), 'mrr', ev.mrr(), 'max |score|', smax)
    print('done')


if __name__ == '__main__':
    main()
