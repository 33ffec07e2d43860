# -*- coding: utf-8 -*-
"""RESCAL / HolE at FB15k-237 shape (14,541 entities, 237 relations, d = 200, 20,466 test facts of a Zipf graph):
one JSON line per model with the ms per LinkPredictionEvaluator.evaluate (device events around each call, after
warm-up; the evaluator replays its captured hipGraph) and the ms of the relation-grouped query transform of one
evaluate's both-sides rows (kge_key_sort + kge_bilinear_query on 2 x 20,466 rows, device events).  Kernel times come
from a separate profiler run, e.g.  rocprofv3 --kernel-trace --stats -- python tools/time_rescal_hole.py

    python tools/time_rescal_hole.py [--reps 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchkge_amd as tk  # noqa: E402
from torchkge_amd import _hip  # noqa: E402
from oracle import kge_oracle as orc  # noqa: E402

N_ENT, N_REL, D, N_TEST = 14541, 237, 200, 20466


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
    args = ap.parse_args()
    heads, tails, rels = orc.synthetic_triples_zipf(N_ENT, N_REL, 310116, seed=237)
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})
    _, kg_test = kg.split_kg(sizes=(len(heads) - N_TEST, N_TEST))
    for name, cls in (('rescal', tk.RESCALModel), ('hole', tk.HolEModel)):
        torch.manual_seed(0)
        m = cls(D, N_ENT, N_REL).cuda()
        ev = tk.LinkPredictionEvaluator(m, kg_test)
        for _ in range(3):
            ev.evaluate(b_size=2048, verbose=False)
        t_eval = events_ms(lambda: ev.evaluate(b_size=2048, verbose=False), args.reps)
        E, Rt = m.ent_emb.weight.data, m._rel_param().weight.data
        h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
        q = lambda: _hip.bilinear_query(m._kind, _hip.SIDE_BOTH, E, Rt, h, t, r)   # noqa: E731
        for _ in range(3):
            q()
        t_q = events_ms(q, args.reps)
        print(json.dumps({'model': name, 'n_ent': N_ENT, 'n_rel': N_REL, 'd': D, 'n_test': N_TEST,
                          'evaluate_ms': round(t_eval, 4), 'query_transform_ms': round(t_q, 4),
                          'mrr': [round(x, 6) for x in ev.mrr()]}), flush=True)


if __name__ == '__main__':
    main()
