# -*- coding: utf-8 -*-
"""ConvKB at FB15k-237 shape (14,541 entities, 237 relations, 20,466 test facts of a Zipf graph) with the paper's
d = 100, F = 50, and at WN18RR shape (40,943 entities, 11 relations, 3,134 test facts) with d = 50, F = 500.

Per shape: ms per LinkPredictionEvaluator.evaluate (device events around each call, after warm-ups, median of --reps;
the evaluator replays its captured hipGraph), and the score / count kernel alone on one both-sides batch of
2 x --batch queries against every entity (kge_convkb_scores, kge_convkb_count_ge).  Each time is also printed as the
fraction of the plain-VALU rate the work would need at the contract's operation count: 3 d F operations per pair (fma,
max, fma) over 63e12 lane-ops/s (tools/probe/valu_rate_probe.hip, quoted in csrc/build.py).  One JSON line per shape.
Kernel times come from a separate profiler run, e.g.  rocprofv3 --kernel-trace --stats -- python tools/time_convkb.py

    python tools/time_convkb.py [--reps 5] [--batch 256] [--shape fb15k237|wn18rr|all]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchkge_amd as tk  # noqa: E402
from oracle import kge_oracle as orc  # noqa: E402

VALU_RATE = 63e12       # plain (unpacked) f32 VALU lane-operations per second, measured
SHAPES = {'fb15k237': dict(n_ent=14541, n_rel=237, n_facts=310116, n_test=20466, d=100, F=50),
          'wn18rr': dict(n_ent=40943, n_rel=11, n_facts=93003, n_test=3134, d=50, F=500)}


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


def fraction(pairs, d, F, ms):
    return round(3.0 * d * F * pairs / VALU_RATE / (ms * 1e-3), 4)


def run(name, s, reps, batch):
    heads, tails, rels = orc.synthetic_triples_zipf(s['n_ent'], s['n_rel'], s['n_facts'], seed=237)
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(s['n_ent'])}, rel2ix={i: i for i in range(s['n_rel'])})
    _, kg_test = kg.split_kg(sizes=(len(heads) - s['n_test'], s['n_test']))
    torch.manual_seed(0)
    m = tk.ConvKBModel(s['d'], s['F'], s['n_ent'], s['n_rel'])
    with torch.no_grad():
        m.output[0].weight.mul_(32.0)       # spread scores (the default head keeps every score within 0.51-0.53)
    m = m.cuda()
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    for _ in range(2):                      # eager, then the capture
        ev.evaluate(b_size=2048, verbose=False)
    eval_ms = events_ms(lambda: ev.evaluate(b_size=2048, verbose=False), reps)
    h, t, r = (x[:batch].cuda() for x in (kg_test.head_idx, kg_test.tail_idx, kg_test.relations))
    prob = m.lp_problem(h, t, r, 'both')
    out = torch.empty(prob.B, prob.N, dtype=torch.float32, device='cuda')
    s_true = prob.pair_scores(torch.cat([t, h]))
    raw = torch.zeros(prob.B, dtype=torch.int32, device='cuda')
    for f in (lambda: prob.scores(out), lambda: prob.count_ge(s_true, raw)):
        f()
    scores_ms = events_ms(lambda: prob.scores(out), reps)
    count_ms = events_ms(lambda: prob.count_ge(s_true, raw), reps)
    pairs_eval, pairs_batch = 2.0 * s['n_test'] * s['n_ent'], float(prob.B) * prob.N
    print(json.dumps(dict(shape=name, n_ent=s['n_ent'], n_rel=s['n_rel'], n_test=s['n_test'], emb_dim=s['d'], n_filters=s['F'],
                          reps=reps, evaluate_ms=round(eval_ms, 3), evaluate_valu_fraction=fraction(pairs_eval, s['d'], s['F'], eval_ms),
                          batch_queries=prob.B, scores_ms=round(scores_ms, 4),
                          scores_valu_fraction=fraction(pairs_batch, s['d'], s['F'], scores_ms), count_ms=round(count_ms, 4),
                          count_valu_fraction=fraction(pairs_batch, s['d'], s['F'], count_ms),
                          mrr=[round(x, 6) for x in ev.mrr()])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--shape', default='all', choices=['all'] + sorted(SHAPES))
    args = ap.parse_args()
    for name in sorted(SHAPES):
        if args.shape in ('all', name):
            run(name, SHAPES[name], args.reps, args.batch)


if __name__ == '__main__':
    main()
