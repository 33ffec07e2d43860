# -*- coding: utf-8 -*-
"""Triplet classification at FB15k-237 shape (14,541 entities, 237 relations, 17,535 validation and 20,466 test facts of a
Zipf graph), TransE d = 200, b_size 32,768.

Two ways to run evaluate() + accuracy() on the same GPU, the same model and the same scoring_function:
  engine      torchkge_amd.evaluation.TripletClassificationEvaluator: negatives, scores, thresholds and the two counts
              on the device (kge_positional_corrupt, kge_relation_max, kge_threshold_count), one host read;
  torch ops   the same steps composed in the reference's formulation (torchkge/evaluation.py:513-580): the negatives come
              back through host memory (corrupt_kg's .cpu(), then one copy per batch up again), one boolean mask over all
              facts and one ``mask.sum() > 0`` per relation, ``thresholds[r_idx]`` gathers and two ``.sum().item()``.
              Its negatives are drawn by the engine's sampler too (the reference's own sampler is a Python loop over the
              batch with two .item() per element; it is not what is compared here).

Per way: ms per evaluate + accuracy (wall clock around a device synchronise, median of --reps after a warm-up), device
operations (kernels, memsets, copies as torch.profiler sees them) and host synchronisations (torch's sync debug mode)
of one call.  One JSON line.

    python tools/time_triplet.py [--reps 7]
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchkge_amd as tk  # noqa: E402
from torchkge_amd.evaluation import TripletClassificationEvaluator  # noqa: E402
from oracle import kge_oracle as orc  # noqa: E402

SHAPE = dict(n_ent=14541, n_rel=237, n_facts=310116, n_val=17535, n_test=20466, d=200, b_size=32768)


class TorchOpsEvaluator(TripletClassificationEvaluator):
    """evaluate / accuracy of the reference, line by line, on torch ops (evaluation.py:513-580)."""

    def __init__(self, model, kg_val, kg_test):
        super().__init__(model, kg_val, kg_test)
        self.sampler.sync_free = False

    def get_scores(self, heads, tails, relations, batch_size):
        scores = []
        with torch.no_grad():
            for lo in range(0, heads.shape[0], batch_size):         # DataLoader(use_cuda='batch')
                sl = slice(lo, lo + batch_size)
                scores.append(self.model.scoring_function(heads[sl].cuda(), tails[sl].cuda(), relations[sl].cuda()))
        return torch.cat(scores, dim=0)

    def evaluate(self, b_size):
        r_idx = self.kg_val.relations
        neg_heads, neg_tails = self.sampler.corrupt_kg(b_size, True, which='main')      # host tensors
        neg_scores = self.get_scores(neg_heads, neg_tails, r_idx, b_size)
        r_dev = r_idx.cuda()
        self.thresholds = torch.zeros(self.kg_val.n_rel)
        for i in range(self.kg_val.n_rel):
            mask = (r_dev == i).bool()
            if mask.sum() > 0:
                self.thresholds[i] = neg_scores[mask].max()
            else:
                self.thresholds[i] = neg_scores.max()
        self.evaluated = True

    def accuracy(self, b_size):
        if not self.evaluated:
            self.evaluate(b_size)
        r_idx = self.kg_test.relations
        neg_heads, neg_tails = self.sampler.corrupt_kg(b_size, True, which='test')
        scores = self.get_scores(self.kg_test.head_idx, self.kg_test.tail_idx, r_idx, b_size)
        neg_scores = self.get_scores(neg_heads, neg_tails, r_idx, b_size)
        thr = self.thresholds.cuda()[r_idx.cuda()]
        return ((scores > thr).sum().item() + (neg_scores < thr).sum().item()) / (2 * self.kg_test.n_facts)


def one_call(ev, b):
    ev.evaluate(b)
    return ev.accuracy(b)


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2]


def device_ops(fn):
    """Device-side operations of one call as torch.profiler records them, or None where it is not available."""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_type = torch.autograd.DeviceType.CUDA
        return sum(1 for e in prof.events() if e.device_type == dev_type)
    except Exception as exc:       # noqa: BLE001 -- a missing profiler backend must not cost the timings
        print('device operations not counted: %r' % (exc,), file=sys.stderr)
        return None


def host_syncs(fn):
    """Synchronising calls torch itself reports (.item(), .cpu(), .tolist(), nonzero / boolean-mask indexing)."""
    try:
        torch.cuda.set_sync_debug_mode('warn')
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn()
        return sum(1 for x in w if 'synchroniz' in str(x.message))
    except Exception as exc:       # noqa: BLE001
        print('host synchronisations not counted: %r' % (exc,), file=sys.stderr)
        return None
    finally:
        torch.cuda.set_sync_debug_mode('default')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    s = SHAPE
    heads, tails, rels = orc.synthetic_triples_zipf(s['n_ent'], s['n_rel'], s['n_facts'], seed=237)
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(s['n_ent'])}, rel2ix={i: i for i in range(s['n_rel'])})
    _, kg_val, kg_test = kg.split_kg(sizes=(len(heads) - s['n_val'] - s['n_test'], s['n_val'], s['n_test']))
    torch.manual_seed(0)
    m = tk.TransEModel(s['d'], s['n_ent'], s['n_rel'], 'L2').cuda()
    b = s['b_size']
    out = dict(shape='fb15k237', model='TransE', emb_dim=s['d'], b_size=b, n_val=s['n_val'], n_test=s['n_test'], reps=args.reps)
    for name, cls in (('engine', TripletClassificationEvaluator), ('torch_ops', TorchOpsEvaluator)):
        ev = cls(m, kg_val, kg_test)
        torch.manual_seed(1)
        acc = one_call(ev, b)               # warm-up: kernel loading, index copies, allocator
        one_call(ev, b)
        out[name + '_ms'] = round(wall_ms(lambda: one_call(ev, b), args.reps), 3)
        out[name + '_device_ops'] = device_ops(lambda: one_call(ev, b))
        out[name + '_host_syncs'] = host_syncs(lambda: one_call(ev, b))
        out[name + '_accuracy'] = round(acc, 4)
    out['speedup'] = round(out['torch_ops_ms'] / out['engine_ms'], 2)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
