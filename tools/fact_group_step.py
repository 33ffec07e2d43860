# -*- coding: utf-8 -*-
"""Training with K negatives per fact: the grouped scorer (``Model.forward_grouped``, include/kge_hip_factgroup.h -- a
fact's rows gathered once for its K negatives) against ``Model.forward`` (kge_score_triples over the B (K + 1)
concatenated triples), in the same build.  The second is the code of the commit before the grouped scorer: the
yardstick.

    python tools/fact_group_step.py --out FILE [--shapes 1024x256,512x1024]

A step is: sample (UniformNegativeSampler.corrupt_batch(n_neg=K) on a fixed batch of B facts), forward, the
self-adversarial criterion (one kge_group_loss), backward, optimizer.  Two models:

    transe    TransE (L2) d = 200 at FB15k-237's shape (14,541 entities, 237 relations), torch.optim.Adagrad on the dense
              gradients (the rows go through the sort and the row reduction);
    complex   ComplEx d = 512 on 10^6 entities, inside row_gradients() with RowAdagrad (the rows go through the row
              optimizer's coalesce).

Each measurement runs in 3 fresh processes; a process measures every (model, shape, path), the two paths of a shape one
after the other.  After a warm-up a sample is the host clock around ``--reps`` steps that end in a device synchronise,
divided by the steps; a process reports the median of its samples.  The report gives the median of the three medians
with min .. max.  The first process also traces one step of every configuration with torch.profiler and reports the
device time of the scorer's forward and backward kernels and of everything else by kernel name (one trace, not
repeated: a breakdown, not a measurement of its own)."""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN, ALPHA, LR, N_FACTS = 6.0, 1.0, 0.1, 272115
MODELS = {'transe': dict(n_ent=14541, n_rel=237, d=200, row=False), 'complex': dict(n_ent=1000000, n_rel=237, d=512, row=True)}
PATHS = ('forward', 'forward_grouped')
SCORER = {'forward': ('score_fwd_kernel', 'score_bwd_kernel'), 'forward_grouped': ('fact_fwd_kernel', 'fact_bwd_kernel')}


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


def trace(fn, path):
    """{'fwd': us, 'bwd': us, 'rest': [(kernel name, us)], 'total': us} of one call of ``fn``; None without a profiler."""
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
                us = e.time_range.elapsed_us()      # a device event's own range
                by_name[e.name] = by_name.get(e.name, 0.0) + float(us)
        if not by_name:
            return None
        fwd = sum(v for k, v in by_name.items() if SCORER[path][0] in k)
        bwd = sum(v for k, v in by_name.items() if SCORER[path][1] in k)
        rest = sorted(((k, v) for k, v in by_name.items() if not any(s in k for s in SCORER[path])), key=lambda kv: -kv[1])
        return dict(fwd=fwd, bwd=bwd, total=sum(by_name.values()), rest=[(k[:60], v) for k, v in rest[:6]])
    except Exception:       # noqa: BLE001 -- a trace that cannot be taken is reported as not measured
        return None


def worker(shapes, reps, samples, models, want_trace):
    import torch
    import torchkge_amd as tk
    from torchkge_amd import optim
    from torchkge_amd.rowgrad import row_gradients
    from torchkge_amd.utils import group_losses
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    out = []
    for name in models:
        m = MODELS[name]
        g = torch.Generator().manual_seed(1)
        facts = [torch.randint(0, n, (N_FACTS,), generator=g) for n in (m['n_ent'], m['n_ent'], m['n_rel'])]
        kg = tk.KnowledgeGraph(kg={'heads': facts[0], 'tails': facts[1], 'relations': facts[2]},
                               ent2ix={i: i for i in range(m['n_ent'])}, rel2ix={i: i for i in range(m['n_rel'])})
        for B, K in shapes:
            crit = group_losses.SelfAdversarialLoss(MARGIN, ALPHA, n_neg=K)
            for path in PATHS:
                torch.manual_seed(0)
                model = (tk.TransEModel(m['d'], m['n_ent'], m['n_rel'], 'L2') if name == 'transe'
                         else tk.ComplExModel(m['d'], m['n_ent'], m['n_rel'])).cuda()
                opt = (optim.RowAdagrad(model.parameters(), lr=LR) if m['row'] else torch.optim.Adagrad(model.parameters(), lr=LR))
                sampler = tk.UniformNegativeSampler(kg, n_neg=K)
                h, t_, r = (x[:B].cuda() for x in facts)

                def step():
                    with row_gradients() if m['row'] else contextlib.nullcontext():
                        nh, nt = sampler.corrupt_batch(h, t_, r, n_neg=K)
                        opt.zero_grad()
                        if path == 'forward':
                            p, n = model(h, t_, r, nh, nt)
                        else:
                            p, n = model.forward_grouped(h, t_, r, nh, nt, check=False)
                        loss = crit(p, n)
                        loss.backward()
                        opt.step()
                    return loss.detach()
                torch.manual_seed(5)
                first = float(step())
                t = timed(step, reps, samples, 3)
                out.append(dict(model=name, B=B, K=K, path=path, t=t, loss=first, trace=trace(step, path) if want_trace else None))
                del model, opt
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--shapes', default='1024x256,512x1024')
    ap.add_argument('--models', default='transe,complex')
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--samples', type=int, default=15)
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split('x')) for s in a.shapes.split(',')]
    models = a.models.split(',')
    if a.worker:
        return worker(shapes, a.reps, a.samples, models, a.trace)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    runs = []
    for i in range(a.procs):        # one fresh process at a time
        cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--shapes', a.shapes, '--models', a.models, '--reps',
               str(a.reps), '--samples', str(a.samples)] + (['--trace'] if i == 0 else [])
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=1100, check=True).stdout
        runs.append(json.loads(res.strip().splitlines()[-1]))
        print('process %d of %d done' % (i + 1, a.procs), file=sys.stderr, flush=True)
    say('K negatives per fact, Model.forward_grouped (kge_score_fact_groups) against Model.forward (kge_score_triples over the '
        'B (K + 1) concatenated triples) (tools/fact_group_step.py): median of %d fresh processes\' medians, min .. max; a sample '
        'is %d steps between two synchronisations' % (a.procs, a.reps))
    say('step: sample (uniform, n_neg = K), forward, self-adversarial criterion (margin %g temperature %g), backward, optimizer'
        % (MARGIN, ALPHA))
    say('transe: TransE L2 d = 200, 14,541 entities, 237 relations, torch.optim.Adagrad on dense gradients; complex: ComplEx '
        'd = 512, 10^6 entities, RowAdagrad inside row_gradients()')
    for i, first in enumerate(runs[0]):
        med = [r[i]['t'] for r in runs]
        if first['path'] == PATHS[0]:
            say('')
            say('%s, B = %d facts, K = %d negatives each' % (first['model'], first['B'], first['K']))
            base = statistics.median(med)
        say('  %-16s step %9.1f us (%.1f .. %.1f)   loss %.4f'
            % (first['path'], 1e6 * statistics.median(med), 1e6 * min(med), 1e6 * max(med), first['loss']))
        tr = first['trace']
        if tr is None:
            say('    kernel trace: not measured')
        else:
            say('    one traced step: scorer forward %.1f us, scorer backward %.1f us, all kernels %.1f us; the largest others:'
                % (tr['fwd'], tr['bwd'], tr['total']))
            for k, v in tr['rest']:
                say('      %9.1f us  %s' % (v, k))
        if first['path'] == PATHS[1]:
            say('  forward_grouped / forward step time %.2f' % (statistics.median(med) / base))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
