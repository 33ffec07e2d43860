# -*- coding: utf-8 -*-
"""One K-vs-all training step, fused against materialised, at two shapes:

    fb15k     DistMult d = 200, N = 14,951 entities, 1,345 relations, B = 1,024 keys (h, r), tail side
    million   ComplEx  d = 512, N = 1,000,000 entities, 1,000 relations, B = 1,024 keys (h, r), tail side

    python tools/k_vs_all_step.py --out FILE [--shapes fb15k,million]

Every key has a sorted answer set of 1 .. 8 entities, key 0 a hub of 5,000; the sets lie in one CSR on the device, as a
FilterIndex keeps them.  A step is zero_grad, loss, backward, SGD step on one fixed batch.  ``fused``:
``model.k_vs_all_loss(h, r, labels, 'tail')`` (kge_lp_prep, kge_lp_bce_fwd / _bwd: no (B, N) tensor).  ``materialised``:
the same model's tables, query rows written out in torch, a dense (B, N) label matrix built by scatter from the CSR,
``F.binary_cross_entropy_with_logits(Q @ E.T, Y)`` (ComplEx: one product over the concatenated [Re | Im] columns) and
autograd.

Each (shape, path) runs in 3 fresh processes.  A process warms up, then times --steps steps one by one (host clock around a
device synchronise), reports their median and ``torch.cuda.max_memory_allocated`` over the timed steps.  The report gives
the median of the three medians with min .. max, the peak allocation, the first step's loss on both paths, and
2 K B N (GEMM passes) / time as a fraction of the 157 TFLOP/s fp32 matrix peak: an end-to-end rate of the whole step,
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
HUB = 5000


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
    B, N = cfg['B'], cfg['n_ent']
    h = torch.randint(0, N, (B,), generator=g).cuda()
    r = torch.randint(0, cfg['n_rel'], (B,), generator=g).cuda()
    lens = torch.randint(1, 9, (B,), generator=g)
    lens[0] = HUB
    sets = [torch.unique(torch.randint(0, N, (int(n),), generator=g)) for n in lens]     # sorted, duplicate-free
    lens = torch.tensor([s.shape[0] for s in sets])
    seg_hi = torch.cumsum(lens, 0)
    labels = ((seg_hi - lens).cuda(), seg_hi.cuda(), torch.cat(sets).to(torch.int32).cuda())
    row_of = torch.repeat_interleave(torch.arange(B), lens).cuda()      # the row of every CSR entry, for the scatter
    col_of = labels[2].long()
    opt = torch.optim.SGD(model.parameters(), lr=LR)

    def materialised():
        if cfg['model'] == 'distmult':
            E, R = model.ent_emb.weight, model.rel_emb.weight
            Q = E[h] * R[r]
        else:
            Ere, Eim, Rre, Rim = (x.weight for x in (model.re_ent_emb, model.im_ent_emb, model.re_rel_emb, model.im_rel_emb))
            Q = torch.cat([Ere[h] * Rre[r] - Eim[h] * Rim[r], Ere[h] * Rim[r] + Eim[h] * Rre[r]], dim=1)
            E = torch.cat([Ere, Eim], dim=1)
        Y = torch.zeros(B, N, dtype=torch.float32, device=h.device)
        Y[row_of, col_of] = 1.0
        return F.binary_cross_entropy_with_logits(Q @ E.t(), Y)

    def step():
        opt.zero_grad()
        loss = model.k_vs_all_loss(h, r, labels, 'tail') if path == 'fused' else materialised()
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
    say('one K-vs-all training step, fused against materialised (tools/k_vs_all_step.py): median of %d fresh processes\' '
        'medians, min .. max' % a.procs)
    for shape in a.shapes.split(','):
        cfg = SHAPES[shape]
        K = cfg['d'] * (2 if cfg['model'] == 'complex' else 1)
        say('')
        say('%s: %s d = %d (K = %d), N = %d, B = %d keys, tail side, answer sets of 1 .. 8 and one hub of %d, %d timed steps '
            'per process' % (shape, cfg['model'], cfg['d'], K, cfg['n_ent'], cfg['B'], HUB, cfg['steps']))
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
            flops = 2.0 * K * cfg['B'] * cfg['n_ent'] * gemm_passes(path, K)
            say('  %-13s %9.3f ms (%.3f .. %.3f)   peak allocation %8.3f GB   first loss %.6f   %d GEMM passes: %.1f TFLOP/s = '
                '%.1f %% of the fp32 matrix peak' % (path, 1e3 * res[path]['t'], 1e3 * res[path]['lo'], 1e3 * res[path]['hi'],
                                                     res[path]['peak'] / 1e9, res[path]['loss'], gemm_passes(path, K),
                                                     flops / res[path]['t'] / 1e12, 100 * flops / res[path]['t'] / PEAK))
        one = 4.0 * cfg['B'] * cfg['n_ent']
        saved = res['materialised']['peak'] - res['fused']['peak']
        say('  fused / materialised time %.2f; the fused step\'s peak allocation is lower by %.3f GB = %.2f (B, N) fp32 '
            'matrices of %.3f GB' % (res['fused']['t'] / res['materialised']['t'], saved / 1e9, saved / one, one / 1e9))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
