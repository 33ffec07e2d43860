# -*- coding: utf-8 -*-
"""One 1-vs-all training step, fused against materialised, at two shapes:

    fb15k     DistMult d = 200, N = 14,951 entities, 1,345 relations, B = 1,024 facts, both sides (2,048 query rows)
    million   ComplEx  d = 512, N = 1,000,000 entities, 1,000 relations, B = 1,024 facts, both sides

    python tools/one_vs_all_step.py --out FILE [--shapes fb15k,million]

A step is zero_grad, loss, backward, SGD step on one fixed batch.  ``fused``: ``model.one_vs_all_loss(h, t, r)`` (kge_lp_prep,
kge_lp_xent_fwd / _bwd: no (2B, N) tensor).  ``materialised``: the same model's tables, query rows written out in torch,
``F.cross_entropy(Q @ E.T, target)`` (ComplEx: one product over the concatenated [Re | Im] columns) and autograd.

Each (shape, path) runs in 3 fresh processes.  A process warms up, then times --steps steps one by one (host clock around a
device synchronise), reports their median and ``torch.cuda.max_memory_allocated`` over the timed steps.  The report gives
the median of the three medians with min .. max, the peak allocation, the first step's loss on both paths, and
2 K (2B) N (GEMM passes) / time as a fraction of the 157 TFLOP/s fp32 matrix peak: an end-to-end rate of the whole step,
not a kernel's share of peak.  GEMM passes: materialised 3 (S, dQ, dE); fused 1 + 2 (slices + 1) -- the forward sweep, and
per backward product one recomputation of S per column slice of 512 plus the product itself."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    'fb15k': dict(model='distmult', d=200, n_ent=14951, n_rel=1345, B=1024, steps=20, warmup=3),
    'million': dict(model='complex', d=512, n_ent=1000000, n_rel=1000, B=1024, steps=3, warmup=1),
}
PEAK = 157e12       # fp32 matrix peak of the MI355X, FLOP/s
LR = 0.1


def gemm_passes(path, K):
    if path == 'materialised':
        return 3
    slices = -(-K // 512)
    return 1 + 2 * (slices + 1)


def worker(shape, path):
    import torch
    import torch.nn.functional as F
    import torchkge_amd as tk
    cfg = SHAPES[shape]
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    torch.manual_seed(0)
    cls = {'distmult': tk.DistMultModel, 'complex': tk.ComplExModel}[cfg['model']]
    model = cls(cfg['d'], cfg['n_ent'], cfg['n_rel']).cuda()
    g = torch.Generator().manual_seed(1)
    h, t = (torch.randint(0, cfg['n_ent'], (cfg['B'],), generator=g).cuda() for _ in range(2))
    r = torch.randint(0, cfg['n_rel'], (cfg['B'],), generator=g).cuda()
    opt = torch.optim.SGD(model.parameters(), lr=LR)
    target = torch.cat([t, h])

    def materialised():
        if cfg['model'] == 'distmult':
            E, R = model.ent_emb.weight, model.rel_emb.weight
            Q = torch.cat([E[h] * R[r], R[r] * E[t]])
        else:
            Ere, Eim, Rre, Rim = (x.weight for x in (model.re_ent_emb, model.im_ent_emb, model.re_rel_emb, model.im_rel_emb))
            tail = torch.cat([Ere[h] * Rre[r] - Eim[h] * Rim[r], Ere[h] * Rim[r] + Eim[h] * Rre[r]], dim=1)
            head = torch.cat([Rre[r] * Ere[t] + Rim[r] * Eim[t], Rre[r] * Eim[t] - Rim[r] * Ere[t]], dim=1)
            Q, E = torch.cat([tail, head]), torch.cat([Ere, Eim], dim=1)
        return F.cross_entropy(Q @ E.t(), target)

    def step():
        opt.zero_grad()
        loss = model.one_vs_all_loss(h, t, r) if path == 'fused' else materialised()
        loss.backward()
        opt.step()
        return loss.detach()

    first = float(step())
    for _ in range(cfg['warmup'] - 1):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(cfg['steps']):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print(json.dumps({'shape': shape, 'path': path, 'median_s': statistics.median(times), 'min_s': min(times),
                      'max_s': max(times), 'peak_bytes': int(torch.cuda.max_memory_allocated()), 'first_loss': first}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', nargs=2, metavar=('SHAPE', 'PATH'))
    ap.add_argument('--out')
    ap.add_argument('--shapes', default='fb15k,million')
    ap.add_argument('--procs', type=int, default=3)
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('one 1-vs-all training step, fused against materialised (tools/one_vs_all_step.py): median of %d fresh processes\' '
        'medians, min .. max' % a.procs)
    for shape in a.shapes.split(','):
        cfg = SHAPES[shape]
        K = cfg['d'] * (2 if cfg['model'] == 'complex' else 1)
        say('')
        say('%s: %s d = %d (K = %d), N = %d, B = %d facts, both sides (%d query rows), %d timed steps per process'
            % (shape, cfg['model'], cfg['d'], K, cfg['n_ent'], cfg['B'], 2 * cfg['B'], cfg['steps']))
        res = {}
        for path in ('fused', 'materialised'):
            runs = []
            for _ in range(a.procs):      # one fresh process at a time
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', shape, path],
                                     stdout=subprocess.PIPE, text=True, timeout=900, check=True).stdout
                runs.append(json.loads(out.strip().splitlines()[-1]))
            med = [x['median_s'] for x in runs]
            res[path] = dict(t=statistics.median(med), lo=min(med), hi=max(med), peak=max(x['peak_bytes'] for x in runs),
                             loss=runs[0]['first_loss'])
            flops = 2.0 * K * (2 * cfg['B']) * cfg['n_ent'] * gemm_passes(path, K)
            say('  %-13s %9.3f ms (%.3f .. %.3f)   peak allocation %8.3f GB   first loss %.6f   %d GEMM passes: %.1f TFLOP/s = '
                '%.1f %% of the fp32 matrix peak' % (path, 1e3 * res[path]['t'], 1e3 * res[path]['lo'], 1e3 * res[path]['hi'],
                                                     res[path]['peak'] / 1e9, res[path]['loss'], gemm_passes(path, K),
                                                     flops / res[path]['t'] / 1e12, 100 * flops / res[path]['t'] / PEAK))
        one = 4.0 * 2 * cfg['B'] * cfg['n_ent']
        saved = res['materialised']['peak'] - res['fused']['peak']
        say('  fused / materialised time %.2f; the fused step\'s peak allocation is lower by %.3f GB = %.2f (2B, N) fp32 '
            'matrices of %.3f GB' % (res['fused']['t'] / res['materialised']['t'], saved / 1e9, saved / one, one / 1e9))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
