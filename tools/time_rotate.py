# -*- coding: utf-8 -*-
"""RotatE at FB15k-237 shape (14,541 entities, 237 relations, emb_dim = 100 so that entity rows are 200 floats -- the width
of DESIGN.md 3.8's table -- and 20,466 test facts of a Zipf graph): one JSON line with, each as the median / min / max of
--reps device-event timings after warm-up,

  evaluate_ms   one LinkPredictionEvaluator.evaluate (the evaluator replays its captured hipGraph),
  count_ms      the rank-count launch of one evaluate's 2 x 20,466 both-sides queries on its own (kge_lp_count_ge of
                KGE_LP_CMOD on the broadcast-subtract kernel),
  step_ms       one training step with n_neg = 256 on a batch of --batch facts: forward of B (1 + 256) triples, the
                self-adversarial criterion, backward, Adagrad.

Tables: entities uniform in (-1, 1), phases uniform in (-pi, pi).  Run it in several processes for a spread between
processes; kernel times come from a separate profiler run.

    python tools/time_rotate.py [--reps 20] [--batch 512] [--neg 256]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchkge_amd as tk  # noqa: E402
from oracle import kge_oracle as orc  # noqa: E402
from torchkge_amd.utils.group_losses import SelfAdversarialLoss  # noqa: E402

N_ENT, N_REL, D, N_TEST = 14541, 237, 100, 20466


def events_ms(fn, reps):
    """(median, min, max) of `reps` device-event timings of fn()."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return [round(out[len(out) // 2], 4), round(out[0], 4), round(out[-1], 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--neg', type=int, default=256)
    args = ap.parse_args()
    heads, tails, rels = orc.synthetic_triples_zipf(N_ENT, N_REL, 310116, seed=237)
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})
    _, kg_test = kg.split_kg(sizes=(len(heads) - N_TEST, N_TEST))
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    torch.manual_seed(0)
    m = tk.RotatEModel(D, N_ENT, N_REL)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        m.ent_emb.weight.copy_(torch.rand(N_ENT, 2 * D, generator=g) * 2 - 1)
        m.rel_emb.weight.copy_((torch.rand(N_REL, D, generator=g) * 2 - 1) * math.pi)
    m = m.cuda()
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    for _ in range(3):
        ev.evaluate(b_size=2048, verbose=False)
    t_eval = events_ms(lambda: ev.evaluate(b_size=2048, verbose=False), args.reps)
    mrr = [round(x, 6) for x in ev.mrr()]
    with m.lp_session():
        prob = m.lp_problem(h, t, r, 'both')
        s_true = prob.pair_scores(torch.cat([t, h]))
        raw = torch.zeros(prob.B, dtype=torch.int32, device='cuda')
        count = lambda: prob.count_ge(s_true, raw)      # noqa: E731
        for _ in range(2):
            count()
        t_count = events_ms(count, args.reps)
    # one training step: K negatives per fact in tile order, each replacing the head or the tail
    B, K = args.batch, args.neg
    hb, tb, rb = h[:B], t[:B], r[:B]
    side = torch.rand(K * B, generator=g) < 0.5
    draw = torch.randint(0, N_ENT, (K * B,), generator=g)
    nh = torch.where(side.cuda(), draw.cuda(), hb.repeat(K))
    nt = torch.where(side.cuda(), tb.repeat(K), draw.cuda())
    crit = SelfAdversarialLoss(margin=6.0, n_neg=K)
    opt = torch.optim.Adagrad(m.parameters(), lr=0.01)

    def step():
        opt.zero_grad()
        pos, neg = m(hb, tb, rb, nh, nt)
        crit(pos, neg).backward()
        opt.step()
    for _ in range(3):
        step()
    t_step = events_ms(step, args.reps)
    pairs = 2 * N_TEST * N_ENT * D      # complex coordinates scored by the count launch
    print(json.dumps({'model': 'RotatE', 'n_ent': N_ENT, 'n_rel': N_REL, 'emb_dim': D, 'row_floats': 2 * D, 'n_test': N_TEST,
                      'reps': args.reps, 'evaluate_ms': t_eval, 'count_ms': t_count, 'step_ms': t_step, 'step_batch': B,
                      'step_n_neg': K, 'complex_coordinates': pairs,
                      'coordinates_per_s': round(pairs / (t_count[0] * 1e-3), 1), 'mrr': mrr}), flush=True)


if __name__ == '__main__':
    main()
