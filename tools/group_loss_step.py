# -*- coding: utf-8 -*-
"""Training with K negatives per fact: the grouped criteria of torchkge_amd.utils.group_losses (one kge_group_loss)
against the same criteria written out in torch -- ``F.softmax(a * n, 0).detach()`` with ``F.logsigmoid`` for the
self-adversarial loss, ``F.cross_entropy`` on the concatenated (B, K + 1) scores for the sampled softmax: the only
alternative a user has without them.

    python tools/group_loss_step.py --out FILE [--shapes 1024x256,512x1024]

Two measurements per (B, K) and kind:

    criterion   the criterion alone on fixed (B) / (K, B) score vectors that require a gradient: forward plus backward;
    step        one whole training step of TransE (L2) d = 200 at FB15k-237's shape (14,541 entities, 237 relations):
                UniformNegativeSampler.corrupt_batch(n_neg=K) on a fixed batch of B facts, Model.forward, the
                criterion, backward, torch.optim.Adagrad.

Each measurement runs in 3 fresh processes; a process measures every (shape, kind, path), the two paths of a shape one
after the other.  After a warm-up a sample is the host clock around ``--reps`` repetitions that end in a device
synchronise, divided by the repetitions; a process reports the median of its samples, its peak
``torch.cuda.max_memory_allocated`` over the timed samples, and the number of device kernels of one repetition counted by
torch.profiler in a run of its own (not timed).  The report gives the median of the three medians with min .. max."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ENT, N_REL, DIM, N_FACTS = 14541, 237, 200, 272115       # FB15k-237
MARGIN, ALPHA, LR = 6.0, 1.0, 0.1
KINDS = ('nssa', 'softmax')
PATHS = ('fused', 'written out')


def written_out(kind, p, n, K):
    """The criterion in stock torch on what Model.forward returns (p repeated K times, n in tile order)."""
    import torch
    import torch.nn.functional as F
    B = n.shape[0] // K
    p, n = p[:B], n.view(K, B)
    if kind == 'nssa':
        w = F.softmax(ALPHA * n, dim=0).detach()
        return (-F.logsigmoid(MARGIN + p) - (w * F.logsigmoid(-(MARGIN + n))).sum(dim=0)).sum()
    scores = torch.cat([p.view(-1, 1), n.t()], dim=1)
    return F.cross_entropy(scores, torch.zeros(B, dtype=torch.long, device=p.device), reduction='sum')


def count_kernels(fn):
    """Device kernels of one call of ``fn``, by torch.profiler; None where the profiler gives none."""
    import torch
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
                and 'memset' not in e.name.lower())
        return n or None
    except Exception:       # noqa: BLE001 -- a count that cannot be taken is reported as not measured
        return None


def timed(fn, reps, samples, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / reps)
    return statistics.median(times), int(torch.cuda.max_memory_allocated())


def worker(shapes, reps, samples):
    import torch
    import torchkge_amd as tk
    from torchkge_amd.utils import group_losses
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    g = torch.Generator().manual_seed(1)
    facts = [torch.randint(0, m, (N_FACTS,), generator=g) for m in (N_ENT, N_ENT, N_REL)]
    kg = tk.KnowledgeGraph(kg={'heads': facts[0], 'tails': facts[1], 'relations': facts[2]},
                           ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})
    out = []
    for B, K in shapes:
        for kind in KINDS:
            fused = (group_losses.SelfAdversarialLoss(MARGIN, ALPHA, n_neg=K) if kind == 'nssa'
                     else group_losses.SampledSoftmaxLoss(n_neg=K))
            crit = {'fused': fused, 'written out': lambda p, n: written_out(kind, p, n, K)}
            # the criterion alone
            pos = (torch.randn(B, generator=g) * 2 - 4).cuda().requires_grad_()
            neg = (torch.randn(K * B, generator=g) * 2 - 6).cuda().requires_grad_()
            for path in PATHS:
                def alone():
                    pos.grad = neg.grad = None
                    loss = crit[path](pos, neg)
                    loss.backward()
                    return loss
                first = float(alone())
                t, peak = timed(alone, reps, samples, 3)
                out.append(dict(what='criterion', B=B, K=K, kind=kind, path=path, t=t, peak=peak, loss=first,
                                kernels=count_kernels(alone)))
            # the whole step
            for path in PATHS:
                torch.manual_seed(0)
                model = tk.TransEModel(DIM, N_ENT, N_REL, 'L2').cuda()
                opt = torch.optim.Adagrad(model.parameters(), lr=LR)
                sampler = tk.UniformNegativeSampler(kg, n_neg=K)
                h, t_, r = (x[:B].cuda() for x in facts)

                def step():
                    nh, nt = sampler.corrupt_batch(h, t_, r, n_neg=K)
                    opt.zero_grad()
                    p, n = model(h, t_, r, nh, nt)
                    loss = crit[path](p, n)
                    loss.backward()
                    opt.step()
                    return loss.detach()
                torch.manual_seed(5)
                first = float(step())
                t, peak = timed(step, max(reps // 10, 1), samples, 3)
                out.append(dict(what='step', B=B, K=K, kind=kind, path=path, t=t, peak=peak, loss=first,
                                kernels=count_kernels(step)))
                del model, opt
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--out')
    ap.add_argument('--shapes', default='1024x256,512x1024')
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--samples', type=int, default=15)
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split('x')) for s in a.shapes.split(',')]
    if a.worker:
        return worker(shapes, a.reps, a.samples)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    runs = []
    for _ in range(a.procs):        # one fresh process at a time
        res = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', '--shapes', a.shapes, '--reps', str(a.reps),
                              '--samples', str(a.samples)], stdout=subprocess.PIPE, text=True, timeout=1100, check=True).stdout
        runs.append(json.loads(res.strip().splitlines()[-1]))
    say('K negatives per fact, the grouped criteria (kge_group_loss) against the criteria written out in torch '
        '(tools/group_loss_step.py): median of %d fresh processes\' medians, min .. max; a sample is %d repetitions '
        '(criterion) / %d (step) between two synchronisations' % (a.procs, a.reps, max(a.reps // 10, 1)))
    say('step: sample (uniform, n_neg = K), forward, criterion, backward, Adagrad; TransE L2 d = %d, %d entities, %d relations; '
        'self-adversarial margin %g temperature %g' % (DIM, N_ENT, N_REL, MARGIN, ALPHA))
    for i, first in enumerate(runs[0]):
        med = [r[i]['t'] for r in runs]
        if first['path'] == PATHS[0]:
            say('')
            say('%s, %s, B = %d facts, K = %d negatives each' % (first['what'], first['kind'], first['B'], first['K']))
            base = statistics.median(med)
        kernels = first['kernels']
        say('  %-12s %9.1f us (%.1f .. %.1f)   %s device kernels   peak allocation %8.2f MB   loss %.4f'
            % (first['path'], 1e6 * statistics.median(med), 1e6 * min(med), 1e6 * max(med),
               'not measured:' if kernels is None else '%4d' % kernels, max(r[i]['peak'] for r in runs) / 1e6, first['loss']))
        if first['path'] == PATHS[1]:
            say('  fused / written out time %.2f' % (base / statistics.median(med)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
