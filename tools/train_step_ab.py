"""Time one training step -- corrupt_batch, forward, MarginLoss, backward, optimizer step -- on the two gradient paths:

    python tools/train_step_ab.py [--shapes fb15k237,large] [--procs 3] [--blocks 5] [--window 0.5] [--out FILE]

  dense   the row-gradient switch off and torch.optim.Adagrad: the backward reduces its rows into zeros_like(table) and
          the optimizer walks every table (with the switch off this is the code of the commit before the switch existed)
  rows    torchkge_amd.row_gradients() and torchkge_amd.optim.RowAdagrad: uncoalesced row gradients, kge_rows_coalesce,
          kge_row_adagrad on the touched rows

Shapes: fb15k237 = TransE d = 200, N = 14,541, R = 237, B = 32,768; large = ComplEx d = 512, N = 10^6, R = 822, B = 32,768.
Facts are Zipf(1) draws over permuted ids; one uniform negative per fact.

Method: every process is a fresh child of this driver (the driver never opens the GPU).  A child holds one model and one
optimizer per path, warms both up, probes each path to size REPS so that a window lasts about --window seconds,
then times BLOCKS windows per path with device events around REPS back-to-back steps inside a synchronised window, the
paths ALTERNATING window by window, and reports the median window per path.  The driver runs PROCS children per shape
and prints the median over the children with their min .. max as the run-to-run spread."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    'fb15k237': ('transe', 200, 14541, 237, 32768),
    'large': ('complex', 512, 1000000, 822, 32768),
}
PATHS = ('dense', 'rows')


def child(args):
    sys.path.insert(0, HERE)
    import torch
    import torchkge_amd as tk
    from torchkge_amd import optim
    from oracle import kge_oracle as orc
    kind, d, N, R, B = SHAPES[args.shape]
    g = torch.Generator().manual_seed(3)
    n_facts = 4 * B
    heads = orc._zipf_draw(N, n_facts, 1.0, g, torch.randperm(N, generator=g))
    tails = orc._zipf_draw(N, n_facts, 1.0, g, torch.randperm(N, generator=g))
    rels = orc._zipf_draw(R, n_facts, 1.0, g, torch.randperm(R, generator=g))
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(N)}, rel2ix={i: i for i in range(R)})
    sampler = tk.UniformNegativeSampler(kg)
    loss_fn = tk.MarginLoss(0.5)
    H, T, Rl = heads.cuda(), tails.cuda(), rels.cuda()
    runs = {}
    for path in PATHS:
        torch.manual_seed(0)
        with torch.device('cuda'):      # the tables are drawn on the device (10^6 x 512 on the host takes longer than the run)
            m = tk.TransEModel(d, N, R, 'L2') if kind == 'transe' else tk.ComplExModel(d, N, R)
        opt = optim.RowAdagrad(m.parameters(), lr=0.05) if path == 'rows' else torch.optim.Adagrad(m.parameters(), lr=0.05)
        runs[path] = (m, opt, [0])

    def step(path):
        m, opt, n = runs[path]
        lo = (n[0] * B) % n_facts
        n[0] += 1
        h, t, r = H[lo:lo + B], T[lo:lo + B], Rl[lo:lo + B]
        with tk.row_gradients(path == 'rows'):
            nh, nt = sampler.corrupt_batch(h, t, r)
            loss = loss_fn(*m(h, t, r, nh, nt))
            opt.zero_grad()
            loss.backward()
            opt.step()

    def window(path, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            step(path)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per step

    for path in PATHS:
        for _ in range(5):
            step(path)
    torch.cuda.synchronize()
    # (the faster of two probes: the first window after the warm-up still pays for the allocator's growth)
    reps = {p: max(3, min(5000, int(math.ceil(args.window * 1e6 / min(window(p, 3), window(p, 3)))))) for p in PATHS}
    wins = {p: [] for p in PATHS}
    for _ in range(args.blocks):
        for p in PATHS:
            wins[p].append(window(p, reps[p]))
    assert runs['rows'][0].parameters().__next__().grad.is_sparse and not runs['dense'][0].parameters().__next__().grad.is_sparse
    res = {'shape': args.shape, 'reps': reps, 'step_us': {p: statistics.median(v) for p, v in wins.items()},
           'window_s': {p: statistics.median(v) * reps[p] * 1e-6 for p, v in wins.items()},
           'peak_GB': round(torch.cuda.max_memory_allocated() / 1e9, 2)}
    print('RESULT ' + json.dumps(res), flush=True)


def driver(args):
    out = []
    for shape in args.shapes.split(','):
        rs = []
        for i in range(args.procs):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--shape', shape, '--blocks', str(args.blocks),
                   '--window', str(args.window)]
            txt = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout, check=True).stdout
            line = [x for x in txt.splitlines() if x.startswith('RESULT ')][-1]
            print('# shape %s process %d: %s' % (shape, i, line[7:]), file=sys.stderr, flush=True)
            rs.append(json.loads(line[7:]))
        kind, d, N, R, B = SHAPES[shape]
        out.append('shape %s: %s d = %d, N = %d, R = %d, B = %d (+ %d negatives); Adagrad; %d processes, median of %d windows '
                   'per path, windows of %s steps (%.2f .. %.2f s)'
                   % (shape, kind, d, N, R, B, B, args.procs, args.blocks,
                      ' / '.join('%d' % rs[0]['reps'][p] for p in PATHS),
                      min(x['window_s'][p] for x in rs for p in PATHS), max(x['window_s'][p] for x in rs for p in PATHS)))
        out.append('  one training step (us, device events around a synchronised window)')
        med = {}
        for p in PATHS:
            v = [x['step_us'][p] for x in rs]
            med[p] = statistics.median(v)
            out.append('    %-8s median %10.1f   spread %10.1f .. %10.1f' % (p, med[p], min(v), max(v)))
        ratios = [x['step_us']['dense'] / x['step_us']['rows'] for x in rs]
        out.append('    dense / rows: %.2f x   (per process %.2f .. %.2f)' % (med['dense'] / med['rows'], min(ratios), max(ratios)))
        out.append('    peak device memory of a process holding both paths: %.2f GB' % max(x['peak_GB'] for x in rs))
    text = '\n'.join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--shape', default='fb15k237')
    ap.add_argument('--shapes', default='fb15k237,large')
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--timeout', type=int, default=400)
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.child:
        child(a)
    else:
        driver(a)
