# -*- coding: utf-8 -*-
"""Filtered negative sampling (``FilteredNegativeSampler``, include/kge_hip_filtered.h) against the unfiltered
``BernoulliNegativeSampler`` with ``sync_free=True`` in the same build: the yardstick.

    python tools/filtered_sampler_step.py --out FILE [--shapes 1024x256,512x1024]

The graph has FB15k-237's shape (14,541 entities, 237 relations, 272,115 drawn facts) and is Zipf-skewed: heads, tails
and relations are drawn independently with probability proportional to 1 / rank, so a few (entity, relation) keys are
hubs with hundreds of known answers -- the keys at which an unfiltered sampler hands out true facts as negatives.

Three figures per shape (B facts, K negatives each):

    (a) one ``corrupt_batch(n_neg=K)`` of each sampler on a fixed batch of B facts of the graph;
    (b) a whole step with each sampler: sample, TransE (L2) d = 200 ``forward_grouped``, ``SelfAdversarialLoss``, backward,
        torch.optim.Adagrad;
    (c) the share of each sampler's negatives that ``known()`` flags as facts of the graph, over 8 batches of B facts.

Each timing runs in 3 fresh processes; a process measures every (shape, sampler), the two samplers of a shape taking
turns sample by sample.  After a warm-up a sample is the host clock around ``--reps`` calls that end in a device
synchronise, divided by the calls; a process reports the median of its samples.  The report gives the median of the three
medians with min .. max.  The first process also traces one ``corrupt_batch`` of each sampler with torch.profiler and
reports the device time of its kernels by name (one trace, not repeated: a breakdown, not a measurement of its own)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN, ALPHA, LR = 6.0, 1.0, 0.1
N_ENT, N_REL, N_FACTS, DIM = 14541, 237, 272115, 200
SAMPLERS = ('bernoulli', 'filtered')
SHARE_BATCHES = 8


def timed(fns, reps, samples, warmup):
    """The median sample of every function of ``fns``; the functions take turns sample by sample, so a drift of the
    machine meets all of them alike."""
    import torch
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(samples):
        for fn, ts in zip(fns, times):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / reps)
    return [statistics.median(ts) for ts in times]


def trace(fn):
    """[(kernel name, device us)] of one call of ``fn``, largest first; None without a profiler."""
    import torch
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        by_name = {}
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA:
                by_name[e.name] = by_name.get(e.name, 0.0) + float(e.time_range.elapsed_us())
        return sorted(((k[:70], v) for k, v in by_name.items()), key=lambda kv: -kv[1]) or None
    except Exception:       # noqa: BLE001 -- a trace that cannot be taken is reported as not measured
        return None


def zipf_graph(seed=1):
    """(heads, tails, relations) of the distinct facts among N_FACTS draws, shuffled; every id drawn with probability
    proportional to 1 / (rank + 1), the rank a fixed permutation of the ids."""
    import torch
    g = torch.Generator().manual_seed(seed)

    def draw(n):
        p = 1.0 / torch.arange(1, n + 1, dtype=torch.float64)
        ids = torch.multinomial(p, N_FACTS, replacement=True, generator=g)
        return torch.randperm(n, generator=g)[ids]
    trip = torch.unique(torch.stack([draw(N_ENT), draw(N_ENT), draw(N_REL)], 1), dim=0)
    trip = trip[torch.randperm(trip.shape[0], generator=g)]
    return trip[:, 0].contiguous(), trip[:, 1].contiguous(), trip[:, 2].contiguous()


def worker(shapes, reps, samples, want_trace):
    import torch
    import torchkge_amd as tk
    from torchkge_amd.sampling import FilteredNegativeSampler
    from torchkge_amd.utils import group_losses
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    h, t, r = zipf_graph()
    kg = tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(N_ENT)},
                           rel2ix={i: i for i in range(N_REL)})
    filtered = FilteredNegativeSampler(kg)
    tail_ix, head_ix = filtered.indexes('cuda')
    longest = [int((ix.offsets[1:] - ix.offsets[:-1]).max()) for ix in (tail_ix, head_ix)]
    graph = dict(facts=int(h.shape[0]), tail_keys=tail_ix.n_keys, head_keys=head_ix.n_keys, longest_tail_list=longest[0],
                 longest_head_list=longest[1], exhaustible=filtered.exhaustible)
    hd, td, rd = h.cuda(), t.cuda(), r.cuda()
    out = []
    for B, K in shapes:
        crit = group_losses.SelfAdversarialLoss(MARGIN, ALPHA, n_neg=K)
        hb, tb, rb = hd[:B], td[:B], rd[:B]
        bern = tk.BernoulliNegativeSampler(kg, n_neg=K)
        bern.sync_free = True
        samplers = dict(bernoulli=bern, filtered=filtered)

        def draw_of(sampler):
            return lambda: sampler.corrupt_batch(hb, tb, rb, n_neg=K)

        def step_of(sampler):
            torch.manual_seed(0)
            model = tk.TransEModel(DIM, N_ENT, N_REL, 'L2').cuda()
            opt = torch.optim.Adagrad(model.parameters(), lr=LR)

            def step():
                nh, nt = sampler.corrupt_batch(hb, tb, rb, n_neg=K)
                opt.zero_grad()
                p, n = model.forward_grouped(hb, tb, rb, nh, nt, check=False)
                loss = crit(p, n)
                loss.backward()
                opt.step()
                return loss.detach()
            return step
        draws = [draw_of(samplers[name]) for name in SAMPLERS]
        steps = [step_of(samplers[name]) for name in SAMPLERS]
        torch.manual_seed(5)
        t_sample = timed(draws, reps, samples, 3)
        firsts = []
        for st in steps:
            torch.manual_seed(5)
            firsts.append(float(st()))
        t_step = timed(steps, reps, samples, 3)
        for q, name in enumerate(SAMPLERS):
            # (c): the share of known facts among the negatives of SHARE_BATCHES different batches
            flagged = total = 0
            for b in range(SHARE_BATCHES):
                sl = slice(b * B, (b + 1) * B)
                nh, nt = samplers[name].corrupt_batch(hd[sl], td[sl], rd[sl], n_neg=K)
                flagged += int(filtered.known(nh, nt, rd[sl].repeat(K)).sum())
                total += nh.shape[0]
            out.append(dict(B=B, K=K, sampler=name, t_sample=t_sample[q], t_step=t_step[q], loss=firsts[q], flagged=flagged,
                            total=total, trace=trace(draws[q]) if want_trace else None))
        del steps
    print(json.dumps(dict(graph=graph, rows=out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--shapes', default='1024x256,512x1024')
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--samples', type=int, default=15)
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split('x')) for s in a.shapes.split(',')]
    if a.worker:
        return worker(shapes, a.reps, a.samples, a.trace)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    runs = []
    for i in range(a.procs):        # one fresh process at a time
        cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--shapes', a.shapes, '--reps', str(a.reps), '--samples',
               str(a.samples)] + (['--trace'] if i == 0 else [])
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=500, check=True).stdout
        runs.append(json.loads(res.strip().splitlines()[-1]))
        print('process %d of %d done' % (i + 1, a.procs), file=sys.stderr, flush=True)
    g = runs[0]['graph']
    say('Filtered negative sampling, FilteredNegativeSampler (kge_filtered_corrupt) against BernoulliNegativeSampler with '
        'sync_free=True (tools/filtered_sampler_step.py): median of %d fresh processes\' medians, min .. max; a sample is %d calls '
        'between two synchronisations' % (a.procs, a.reps))
    say('graph: %d entities, %d relations, %d distinct facts of %d Zipf draws (probability 1 / rank on heads, tails and relations); '
        '%d (h, r) keys, longest list %d tails; %d (t, r) keys, longest list %d heads; exhaustible keys %d'
        % (N_ENT, N_REL, g['facts'], N_FACTS, g['tail_keys'], g['longest_tail_list'], g['head_keys'], g['longest_head_list'],
           g['exhaustible']))
    say('sample: one corrupt_batch(n_neg = K) on a fixed batch of B facts; step: sample, TransE L2 d = %d forward_grouped, '
        'self-adversarial criterion (margin %g temperature %g), backward, torch.optim.Adagrad; known: the share of the negatives '
        'of %d batches that FilteredNegativeSampler.known() flags as facts of the graph' % (DIM, MARGIN, ALPHA, SHARE_BATCHES))
    for i, first in enumerate(runs[0]['rows']):
        ts = [r['rows'][i]['t_sample'] for r in runs]
        tp = [r['rows'][i]['t_step'] for r in runs]
        if first['sampler'] == SAMPLERS[0]:
            say('')
            say('B = %d facts, K = %d negatives each' % (first['B'], first['K']))
            base = statistics.median(ts), statistics.median(tp)
        say('  %-10s sample %9.1f us (%.1f .. %.1f)   step %9.1f us (%.1f .. %.1f)   known %d of %d = %.4f %%   loss %.4f'
            % (first['sampler'], 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts), 1e6 * statistics.median(tp),
               1e6 * min(tp), 1e6 * max(tp), first['flagged'], first['total'], 100.0 * first['flagged'] / first['total'],
               first['loss']))
        if first['trace'] is None:
            say('    kernel trace of one corrupt_batch: not measured')
        else:
            say('    one traced corrupt_batch: %d kernel names, %.1f us of device time; the largest:'
                % (len(first['trace']), sum(v for _, v in first['trace'])))
            for k, v in first['trace'][:4]:
                say('      %7.1f us  %s' % (v, k))
        if first['sampler'] == SAMPLERS[1]:
            say('  filtered / bernoulli: sample time %.2f, step time %.2f'
                % (statistics.median(ts) / base[0], statistics.median(tp) / base[1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
