# -*- coding: utf-8 -*-
"""Training with an N3 regularizer: the engine's penalty (torchkge_amd.utils.regularizers, include/kge_hip_penalty.h --
one gather of the penalised rows, gradient ROWS) against the same penalty written out in torch on ``emb(ids)`` (a dense
``embedding_dense_backward`` per table), in the same build.  The torch-written step is the yardstick.

    python tools/regularizer_step.py --out FILE [--models transe,complex]

A step is: sample (UniformNegativeSampler.corrupt_batch on a fixed batch of B facts, one negative each), forward, the fused
pair criterion (one kge_pair_loss), the penalty of the batch's facts, backward, optimizer.  Two shapes:

    transe    TransE (L2) d = 200 at FB15k-237's shape (14,541 entities, 237 relations), B = 1,024, torch.optim.Adagrad on
              dense gradients on both sides;
    complex   ComplEx d = 512 on 10^6 entities, B = 32,768.  Engine: RowAdagrad inside row_gradients().  Torch: the penalty
              hands the tables a dense gradient, which the row optimizers refuse, so the whole step runs on dense
              gradients with torch.optim.Adagrad -- that is the point of the feature.

Three variants per shape: ``none`` (no penalty, the engine side's optimizer), ``engine``, ``torch``.  Each measurement runs
in 3 fresh processes.  After a warm-up a sample is the host clock around ``--reps`` steps that end in a device
synchronise, divided by the steps; a process reports the median of its samples.  The report gives the median of the three
medians with min .. max.

``--trace-worker`` runs a few engine steps of ``--models`` and nothing else: the program to put behind
``rocprofv3 --kernel-trace --stats --``; ``--stats-csv transe=FILE,complex=FILE`` adds the kernel times of those runs
(penalty forward and backward next to kge_score_triples forward and backward) to the report."""
import argparse
import contextlib
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHT, LR, N_FACTS = 0.05, 0.1, 272115
MODELS = {'transe': dict(n_ent=14541, n_rel=237, d=200, B=1024, row=False),
          'complex': dict(n_ent=1000000, n_rel=237, d=512, B=32768, row=True)}
VARIANTS = ('none', 'engine', 'torch')
KERNELS = ('penalty_terms_kernel', 'penalty_sum_kernel', 'st_final_kernel', 'penalty_bwd_kernel', 'score_fwd_kernel',
           'score_bwd_kernel')


def timed(fn, reps, samples, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / reps)
    return statistics.median(times)


def torch_n3(name, model, h, t, r):
    """The penalty written out: what a user writes today."""
    B = h.shape[0]
    if name == 'transe':
        return WEIGHT / B * ((model.ent_emb(h).abs() ** 3).sum() + (model.ent_emb(t).abs() ** 3).sum()
                             + (model.rel_emb(r).abs() ** 3).sum())

    def mod3(re, im, ids):
        return ((re(ids) ** 2 + im(ids) ** 2).sqrt() ** 3).sum()
    return WEIGHT / B * (mod3(model.re_ent_emb, model.im_ent_emb, h) + mod3(model.re_ent_emb, model.im_ent_emb, t)
                         + mod3(model.re_rel_emb, model.im_rel_emb, r))


def make_step(name, variant):
    import torch
    import torchkge_amd as tk
    from torchkge_amd import optim
    from torchkge_amd.rowgrad import row_gradients
    from torchkge_amd.utils.fused_losses import fused_for
    from torchkge_amd.utils.regularizers import N3Regularizer
    m = MODELS[name]
    g = torch.Generator().manual_seed(1)
    facts = [torch.randint(0, n, (N_FACTS,), generator=g) for n in (m['n_ent'], m['n_ent'], m['n_rel'])]
    kg = tk.KnowledgeGraph(kg={'heads': facts[0], 'tails': facts[1], 'relations': facts[2]},
                           ent2ix={i: i for i in range(m['n_ent'])}, rel2ix={i: i for i in range(m['n_rel'])})
    torch.manual_seed(0)
    model = (tk.TransEModel(m['d'], m['n_ent'], m['n_rel'], 'L2') if name == 'transe'
             else tk.ComplExModel(m['d'], m['n_ent'], m['n_rel'])).cuda()
    row = m['row'] and variant != 'torch'
    opt = optim.RowAdagrad(model.parameters(), lr=LR) if row else torch.optim.Adagrad(model.parameters(), lr=LR)
    crit = fused_for(tk.MarginLoss(1.0) if name == 'transe' else tk.LogisticLoss())
    sampler = tk.UniformNegativeSampler(kg)
    reg = N3Regularizer(WEIGHT)
    h, t_, r = (x[:m['B']].cuda() for x in facts)

    def step():
        with row_gradients() if row else contextlib.nullcontext():
            nh, nt = sampler.corrupt_batch(h, t_, r, n_neg=1)
            opt.zero_grad()
            p, n = model(h, t_, r, nh, nt)
            loss = crit(p, n)
            if variant == 'engine':
                loss = loss + reg(model, (h, t_), (r,))
            elif variant == 'torch':
                loss = loss + torch_n3(name, model, h, t_, r)
            loss.backward()
            opt.step()
        return loss.detach()
    return step


def worker(models, reps, samples):
    import torch
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    out = []
    for name in models:
        for variant in VARIANTS:
            step = make_step(name, variant)
            torch.manual_seed(5)
            first = float(step())
            out.append(dict(model=name, variant=variant, t=timed(step, reps, samples, 3), loss=first))
            del step
            torch.cuda.empty_cache()
    print(json.dumps(out))


def trace_worker(models, steps):
    import torch
    for name in models:
        step = make_step(name, 'engine')
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        del step
        torch.cuda.empty_cache()


def kernel_stats(path):
    """{kernel of KERNELS: (calls, average ns)} from a rocprofv3 kernel-stats CSV."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row['Name']:        # (the template instances of a kernel count together)
                    calls, total = out.get(k, (0, 0.0))
                    out[k] = (calls + int(row['Calls']), total + float(row['TotalDurationNs']))
    return {k: (c, tot / c) for k, (c, tot) in out.items() if c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--trace-worker', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--models', default='transe,complex')
    ap.add_argument('--stats-csv', default='')
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=9)
    ap.add_argument('--steps', type=int, default=20)
    a = ap.parse_args()
    models = a.models.split(',')
    if a.worker:
        return worker(models, a.reps, a.samples)
    if a.trace_worker:
        return trace_worker(models, a.steps)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    runs = []
    for i in range(a.procs):        # one fresh process at a time
        cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--models', a.models, '--reps', str(a.reps), '--samples',
               str(a.samples)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900, check=True).stdout
        runs.append(json.loads(res.strip().splitlines()[-1]))
        print('process %d of %d done' % (i + 1, a.procs), file=sys.stderr, flush=True)
    say('One training step with an N3 penalty (weight %g) of the batch\'s facts, the engine\'s regularizer (kge_row_penalty) '
        'against the penalty written out in torch (tools/regularizer_step.py): median of %d fresh processes\' medians, '
        'min .. max; a sample is %d steps between two synchronisations' % (WEIGHT, a.procs, a.reps))
    say('step: sample (uniform, one negative per fact), forward, fused pair criterion, penalty, backward, optimizer')
    say('transe: TransE L2 d = 200, 14,541 entities, 237 relations, B = 1,024, torch.optim.Adagrad on dense gradients on both '
        'sides; complex: ComplEx d = 512, 10^6 entities, B = 32,768, engine: RowAdagrad inside row_gradients(), torch: dense '
        'gradients and torch.optim.Adagrad (a torch penalty makes the tables\' gradients dense)')
    for i, first in enumerate(runs[0]):
        med = [r[i]['t'] for r in runs]
        if first['variant'] == VARIANTS[0]:
            say('')
            say('%s' % first['model'])
        if first['variant'] == 'engine':
            engine = statistics.median(med)
        say('  %-8s step %10.1f us (%.1f .. %.1f)   loss %.4f'
            % (first['variant'], 1e6 * statistics.median(med), 1e6 * min(med), 1e6 * max(med), first['loss']))
        if first['variant'] == 'torch':
            say('  torch / engine step time %.2f' % (statistics.median(med) / engine))
    for item in [x for x in a.stats_csv.split(',') if x]:
        name, path = item.split('=', 1)
        say('')
        say('%s, engine steps under rocprofv3 --kernel-trace --stats (a run of its own): calls, average kernel time' % name)
        try:
            stats = kernel_stats(path)
        except (OSError, KeyError, ValueError) as e:    # a trace that cannot be read is reported as not measured
            say('  not measured: %s: %r' % (type(e).__name__, e))
            continue
        for k in KERNELS:
            if k in stats:
                say('  %-22s %5d calls  %9.1f us' % (k, stats[k][0], stats[k][1] / 1e3))
        say('  (st_final_kernel is the second stage of the fp64 sum: the criterion\'s and the penalty\'s launches share the name)')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
