# -*- coding: utf-8 -*-
"""TorusE at FB15k-237 shape (14,541 entities, 237 relations, d = 200, 20,466 test facts of a Zipf graph): one JSON
line per dissimilarity type with the ms per LinkPredictionEvaluator.evaluate (median of --reps calls, device events
around each call, after warm-up; the evaluator replays its captured hipGraph) and the ms of the rank-count launch of
one evaluate's 2 x 20,466 both-sides queries on its own (kge_lp_count_ge on the broadcast-subtract kernel, device
events).  Tables are uniform in (-1, 1), as normalize_parameters leaves them.  Kernel times come from a separate
profiler run, e.g.  rocprofv3 --kernel-trace --stats -- python tools/time_toruse.py

    python tools/time_toruse.py [--reps 20] [--types torus_L1,torus_L2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchkge_amd as tk  # noqa: E402
from oracle import kge_oracle as orc  # noqa: E402

N_ENT, N_REL, D, N_TEST = 14541, 237, 200, 20466
TYPES = ('L1', 'torus_L1', 'torus_L2', 'torus_eL2')


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--types', default=','.join(TYPES))
    args = ap.parse_args()
    heads, tails, rels = orc.synthetic_triples_zipf(N_ENT, N_REL, 310116, seed=237)
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})
    _, kg_test = kg.split_kg(sizes=(len(heads) - N_TEST, N_TEST))
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    for diss in args.types.split(','):
        torch.manual_seed(0)
        m = tk.TorusEModel(D, N_ENT, N_REL, diss)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            m.ent_emb.weight.copy_(torch.rand(N_ENT, D, generator=g) * 2 - 1)
            m.rel_emb.weight.copy_(torch.rand(N_REL, D, generator=g) * 2 - 1)
        m = m.cuda()
        ev = tk.LinkPredictionEvaluator(m, kg_test)
        for _ in range(3):
            ev.evaluate(b_size=2048, verbose=False)
        t_eval = events_ms(lambda: ev.evaluate(b_size=2048, verbose=False), args.reps)
        with m.lp_session():
            prob = m.lp_problem(h, t, r, 'both')
            s_true = prob.pair_scores(torch.cat([t, h]))
            raw = torch.zeros(prob.B, dtype=torch.int32, device='cuda')
            count = lambda: prob.count_ge(s_true, raw)      # noqa: E731
            for _ in range(2):
                count()
            t_count = events_ms(count, args.reps)
        pairs_k = 2 * N_TEST * N_ENT * D
        print(json.dumps({'model': 'TorusE', 'dissimilarity': diss, 'n_ent': N_ENT, 'n_rel': N_REL, 'd': D,
                          'n_test': N_TEST, 'evaluate_ms': round(t_eval, 4), 'count_ms': round(t_count, 4),
                          'pair_k_elements': pairs_k, 'elements_per_s': round(pairs_k / (t_count * 1e-3), 1),
                          'mrr': [round(x, 6) for x in ev.mrr()]}), flush=True)


if __name__ == '__main__':
    main()
