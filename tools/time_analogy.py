# -*- coding: utf-8 -*-
"""ANALOGY at FB15k-237 shape (14,541 entities, 237 relations, emb_dim = 200 so K = 100 + 2 * 100 = 300, 20,466 test
facts of a Zipf graph), with HolE at d = 300 in the same process as the yardstick: HolE solves the identical KGE_LP_DOT
problem (same B, N, K) behind a strictly more expensive query transform.

First asserts that ANALOGY's ranks through the split prefilter equal those with split_filter = False on this workload.
Then, per round, the two models ALTERNATE: ms per LinkPredictionEvaluator.evaluate (device events around each call,
after 3 warm-ups, median of --reps; the evaluator replays its captured hipGraph).  One JSON line per model with the
per-round medians (their spread is the run-to-run noise the two are compared within), and for ANALOGY the ms and the
bytes moved of the pack of the candidate table (kge_analogy_pack_rows) and of the query rows of one evaluate's
both-sides batch rows (kge_analogy_query on 2 x 20,466 rows).  Kernel times come from a separate profiler run, e.g.
rocprofv3 --kernel-trace --stats -- python tools/time_analogy.py

    python tools/time_analogy.py [--reps 20] [--rounds 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchkge_amd as tk  # noqa: E402
from torchkge_amd import _hip, _hip_analogy  # noqa: E402
from oracle import kge_oracle as orc  # noqa: E402

N_ENT, N_REL, D, N_TEST = 14541, 237, 200, 20466
NAMES = ['rank_true_heads', 'rank_true_tails', 'filt_rank_true_heads', 'filt_rank_true_tails']


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
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    heads, tails, rels = orc.synthetic_triples_zipf(N_ENT, N_REL, 310116, seed=237)
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})
    _, kg_test = kg.split_kg(sizes=(len(heads) - N_TEST, N_TEST))
    torch.manual_seed(0)
    ana = tk.AnalogyModel(D, N_ENT, N_REL).cuda()
    K = ana._lp_width()
    torch.manual_seed(0)
    hole = tk.HolEModel(K, N_ENT, N_REL).cuda()

    # the split prefilter's ranks are the exact fp32 counts' on this workload
    ev = tk.LinkPredictionEvaluator(ana, kg_test)
    ev.evaluate(b_size=2048, verbose=False)
    ana.split_filter = False
    ex = tk.LinkPredictionEvaluator(ana, kg_test)
    ex.evaluate(b_size=2048, verbose=False)
    ana.split_filter = True
    for nm in NAMES:
        assert torch.equal(getattr(ev, nm), getattr(ex, nm)), nm

    evs = {'analogy': ev, 'hole': tk.LinkPredictionEvaluator(hole, kg_test)}
    times = {k: [] for k in evs}
    for e in evs.values():
        for _ in range(3):
            e.evaluate(b_size=2048, verbose=False)
    for _ in range(args.rounds):
        for name, e in evs.items():
            times[name].append(events_ms(lambda: e.evaluate(b_size=2048, verbose=False), args.reps))

    tabs = [x.data for x in ana._tables()]
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    pack = lambda: _hip_analogy.pack_rows(tabs[:3])     # noqa: E731
    query = lambda: _hip_analogy.query(_hip.SIDE_BOTH, tabs[:3], tabs[3:], h, t, r)     # noqa: E731
    hq = lambda: _hip.bilinear_query(_hip.HOLE, _hip.SIDE_BOTH, hole.ent_emb.weight.data, hole.rel_emb.weight.data, h, t, r)   # noqa: E731
    for f in (pack, query, hq):
        for _ in range(3):
            f()
    common = {'n_ent': N_ENT, 'n_rel': N_REL, 'K': K, 'n_test': N_TEST, 'reps': args.reps}
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    print(json.dumps(dict(common, model='analogy', emb_dim=D, evaluate_ms=round(med(times['analogy']), 4),
                          evaluate_ms_rounds=[round(x, 4) for x in times['analogy']],
                          pack_ms=round(events_ms(pack, args.reps), 4), pack_bytes=2 * 4 * N_ENT * K,
                          query_transform_ms=round(events_ms(query, args.reps), 4),
                          query_bytes=2 * N_TEST * (2 * 4 * K + 4 * K + 16),
                          split_equals_fp32=True, mrr=[round(x, 6) for x in ev.mrr()])), flush=True)
    print(json.dumps(dict(common, model='hole', emb_dim=K, evaluate_ms=round(med(times['hole']), 4),
                          evaluate_ms_rounds=[round(x, 4) for x in times['hole']],
                          query_transform_ms=round(events_ms(hq, args.reps), 4),
                          mrr=[round(x, 6) for x in evs['hole'].mrr()])), flush=True)


if __name__ == '__main__':
    main()
