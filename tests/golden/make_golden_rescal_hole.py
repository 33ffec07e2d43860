# -*- coding: utf-8 -*-
"""Generate the RESCAL / HolE golden fixtures in this directory by RUNNING THE
REAL REFERENCE (torchkge v0.17.7 imported from /root/reference, CPU).  Run in
the build container only (the reference does not exist on the GPU box):

    python tests/golden/make_golden_rescal_hole.py

Outputs (committed): tests/golden/ref_rescal.npz, ref_hole.npz,
ref_relpred_rescal_hole.npz.  Same knowledge graph, sizes, b_size and table
perturbation as make_golden.py.  Each model file holds the tables, the
reference's scoring_function, forward (n_neg = 2), inference_scoring_function
on both sides, the LinkPredictionEvaluator ranks + metrics; the relation file
the relation-candidate scores and RelationPredictionEvaluator ranks + metrics,
directed and undirected.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchkge  # noqa: E402
from torchkge.evaluation import LinkPredictionEvaluator, RelationPredictionEvaluator  # noqa: E402
from torchkge.models import RESCALModel, HolEModel  # noqa: E402
from make_golden import make_kg, sub_kg, N_ENT, N_REL, DIM, N_TEST, B  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
assert torchkge.__version__ == '0.17.7'


def build_model(kind):
    torch.manual_seed(0)
    if kind == 'rescal':
        return RESCALModel(DIM, N_ENT, N_REL)
    if kind == 'hole':
        return HolEModel(DIM, N_ENT, N_REL)
    raise ValueError(kind)


def tables_of(kind, m):
    t = [m.ent_emb.weight, m.rel_mat.weight if kind == 'rescal' else m.rel_emb.weight]
    return [x.detach().clone().numpy() for x in t]


def main():
    kg = make_kg(1234)
    kg_test = sub_kg(kg, N_TEST)
    common = dict(heads=kg.head_idx.numpy(), tails=kg.tail_idx.numpy(), rels=kg.relations.numpy(),
                  n_test=N_TEST, n_ent=N_ENT, n_rel=N_REL, b_size=B, dim=DIM)
    rp = dict(common)
    for kind in ('rescal', 'hole'):
        m = build_model(kind)
        # perturb tables a little so they are NOT exactly normalised (as make_golden.py): pins "normalise in
        # scoring_function, raw tables at inference"
        with torch.no_grad():
            for prm in m.parameters():
                if prm.requires_grad:
                    prm.mul_(1.0 + 0.05 * torch.sin(torch.arange(prm.numel()).float()).view_as(prm))
        tabs = tables_of(kind, m)
        h, t, r = kg_test.head_idx[:B], kg_test.tail_idx[:B], kg_test.relations[:B]
        with torch.no_grad():
            sf = m.scoring_function(h, t, r).numpy()
            g = torch.Generator().manual_seed(7)
            nh = torch.randint(0, N_ENT, (2 * B,), generator=g)
            nt = torch.randint(0, N_ENT, (2 * B,), generator=g)
            pos, neg = m(h, t, r, nh, nt)
            h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=True)
            s_tail = m.inference_scoring_function(h_e, cand, r_e).numpy()
            s_head = m.inference_scoring_function(cand, t_e, r_e).numpy()
            ev = LinkPredictionEvaluator(m, kg_test)
            ev.evaluate(b_size=B, verbose=False)
        out = dict(common)
        for i, tb in enumerate(tabs):
            out['table%d' % i] = tb
        out.update(sf=sf, fwd_pos=pos.numpy(), fwd_neg=neg.numpy(), neg_heads=nh.numpy(), neg_tails=nt.numpy(),
                   s_tail=s_tail, s_head=s_head,
                   rank_true_heads=ev.rank_true_heads.numpy(),
                   rank_true_tails=ev.rank_true_tails.numpy(),
                   filt_rank_true_heads=ev.filt_rank_true_heads.numpy(),
                   filt_rank_true_tails=ev.filt_rank_true_tails.numpy(),
                   hit10=np.array(ev.hit_at_k(10)), mrr=np.array(ev.mrr()),
                   mean_rank=np.array(ev.mean_rank()))
        np.savez_compressed(os.path.join(HERE, 'ref_%s.npz' % kind), **out)
        print('ref_%s.npz' % kind, 'hit10', ev.hit_at_k(10), 'mrr', ev.mrr())

        # ---- relation prediction (evaluation.py:16-204), on the same perturbed tables ----
        for i, tb in enumerate(tabs):
            rp['%s_table%d' % (kind, i)] = tb
        with torch.no_grad():
            h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=False)
            rp['%s_s_rel' % kind] = m.inference_scoring_function(h_e, t_e, cand).numpy()
            for directed in (True, False):
                ev = RelationPredictionEvaluator(m, kg_test, directed=directed)
                ev.evaluate(b_size=B, verbose=False)
                tag = '%s_%s' % (kind, 'dir' if directed else 'undir')
                rp[tag + '_rank'] = ev.rank_true_rels.numpy()
                rp[tag + '_frank'] = ev.filt_rank_true_rels.numpy()
                rp[tag + '_mrr'] = np.array(ev.mrr())
                rp[tag + '_hit3'] = np.array(ev.hit_at_k(3))
    np.savez_compressed(os.path.join(HERE, 'ref_relpred_rescal_hole.npz'), **rp)
    print('done')


if __name__ == '__main__':
    main()
