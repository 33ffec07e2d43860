# -*- coding: utf-8 -*-
"""Generate the TorusE golden fixtures in this directory by RUNNING THE REAL
REFERENCE (torchkge v0.17.7 imported from /root/reference, CPU).  Run in the
build container only (the reference does not exist on the GPU box):

    python tests/golden/make_golden_toruse.py

Outputs (committed): tests/golden/ref_toruse_<type>.npz for the four
dissimilarity types ('L1', 'torus_L1', 'torus_L2', 'torus_eL2').  Same knowledge
graph, sizes and b_size as make_golden.py.  The tables are loaded with RAW values
in (-3, 3) -- frac() in scoring_function matters, and after the in-place frac of
the evaluation they are spread over (-1, 1), so |(h + r) - c| > 1 (negative
terms, positive scores) is common.  Each file holds the raw tables, the
reference's scoring_function, forward (n_neg = 2), the gradients of
(scoring_function * g).sum() wrt both tables, LinkPredictionEvaluator ranks +
metrics, the tables after that evaluation (the in-place frac), and
inference_scoring_function on both sides on those tables.  The reference's
relation-prediction branch raises AttributeError (translation.py:765): no
fixture for it.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchkge  # noqa: E402
from torchkge.evaluation import LinkPredictionEvaluator  # noqa: E402
from torchkge.models import TorusEModel  # noqa: E402
from make_golden import make_kg, sub_kg, N_ENT, N_REL, DIM, N_TEST, B  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
assert torchkge.__version__ == '0.17.7'
TYPES = ('L1', 'torus_L1', 'torus_L2', 'torus_eL2')


def tag(diss):
    return diss.replace('torus_', 't').lower()


def main():
    kg = make_kg(1234)
    kg_test = sub_kg(kg, N_TEST)
    common = dict(heads=kg.head_idx.numpy(), tails=kg.tail_idx.numpy(), rels=kg.relations.numpy(),
                  n_test=N_TEST, n_ent=N_ENT, n_rel=N_REL, b_size=B, dim=DIM)
    for diss in TYPES:
        torch.manual_seed(0)
        m = TorusEModel(DIM, N_ENT, N_REL, diss)
        ctor = [m.ent_emb.weight.detach().clone().numpy(), m.rel_emb.weight.detach().clone().numpy()]
        g = torch.Generator().manual_seed(17)
        with torch.no_grad():
            m.ent_emb.weight.copy_(torch.rand(N_ENT, DIM, generator=g) * 6.0 - 3.0)
            m.rel_emb.weight.copy_(torch.rand(N_REL, DIM, generator=g) * 6.0 - 3.0)
        raw = [m.ent_emb.weight.detach().clone().numpy(), m.rel_emb.weight.detach().clone().numpy()]
        h, t, r = kg_test.head_idx[:B], kg_test.tail_idx[:B], kg_test.relations[:B]
        with torch.no_grad():
            sf = m.scoring_function(h, t, r).numpy()
            gn = torch.Generator().manual_seed(7)
            nh = torch.randint(0, N_ENT, (2 * B,), generator=gn)
            nt = torch.randint(0, N_ENT, (2 * B,), generator=gn)
            pos, neg = m(h, t, r, nh, nt)
        gvec = torch.randn(B, generator=gn)
        m.zero_grad()
        (m.scoring_function(h, t, r) * gvec).sum().backward()
        g_ent, g_rel = m.ent_emb.weight.grad.clone().numpy(), m.rel_emb.weight.grad.clone().numpy()
        assert not m.normalized
        with torch.no_grad():
            ev = LinkPredictionEvaluator(m, kg_test)
            ev.evaluate(b_size=B, verbose=False)
            assert m.normalized
            after = [m.ent_emb.weight.detach().clone().numpy(), m.rel_emb.weight.detach().clone().numpy()]
            h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=True)
            s_tail = m.inference_scoring_function(h_e, cand, r_e).numpy()
            s_head = m.inference_scoring_function(cand, t_e, r_e).numpy()
        out = dict(common)
        out.update(diss=np.array(diss), ctor_table0=ctor[0], ctor_table1=ctor[1], table0=raw[0], table1=raw[1],
                   sf=sf, fwd_pos=pos.numpy(), fwd_neg=neg.numpy(), neg_heads=nh.numpy(), neg_tails=nt.numpy(),
                   grad_out=gvec.numpy(), grad_ent=g_ent, grad_rel=g_rel,
                   after_table0=after[0], after_table1=after[1], s_tail=s_tail, s_head=s_head,
                   rank_true_heads=ev.rank_true_heads.numpy(),
                   rank_true_tails=ev.rank_true_tails.numpy(),
                   filt_rank_true_heads=ev.filt_rank_true_heads.numpy(),
                   filt_rank_true_tails=ev.filt_rank_true_tails.numpy(),
                   hit10=np.array(ev.hit_at_k(10)), mrr=np.array(ev.mrr()),
                   mean_rank=np.array(ev.mean_rank()),
                   state_dict_keys=np.array(sorted(m.state_dict().keys())))
        name = 'ref_toruse_%s.npz' % tag(diss)
        np.savez_compressed(os.path.join(HERE, name), **out)
        print(name, 'hit10', ev.hit_at_k(10), 'mrr', ev.mrr(), 'positive scores', int((s_tail > 0).sum()), '/',
              s_tail.size)
    print('done')


if __name__ == '__main__':
    main()
