"""Time training epochs -- a fresh corruption, the steps, normalize_parameters -- on four paths:

    python tools/train_epoch_ab.py [--shapes fb15k237,large] [--procs 3] [--blocks 5] [--window 0.5] [--out FILE]

  tutorial   the hand-written loop exactly as tools/train_step_ab.py's ``step`` has it (corrupt_batch per step, forward,
             MarginLoss, zero_grad, backward, step: the code that existed before torchkge_amd.utils.training), with
             normalize_parameters after every epoch
  generic    Trainer(fused=False): corrupt_kg per epoch, utils/losses.py's MarginLoss, one loss.item() per step
  fused      Trainer(fused=True): the criterion through kge_pair_loss, one loss.item() per step
  syncfree   Trainer(fused=True, sync_free=True): no host read in run()

All four train with torchkge_amd.row_gradients() and optim.RowAdagrad (``--optimizer dense``: the switch off and
torch.optim.Adagrad).  Shapes and facts are those of tools/train_step_ab.py: an epoch is 4 batches of 32,768 facts.

Method: that tool's.  Every process is a fresh child of this driver (the driver never opens the GPU).  A child holds
one model and one optimizer per path, warms every path up, probes each to size its window (a whole number of epochs
lasting about --window seconds), then times BLOCKS windows per path with device events around a synchronised window,
the paths ALTERNATING window by window, and reports the median window per path as microseconds per step.  The driver
runs PROCS children per shape and prints the median over the children with their min .. max as the run-to-run spread."""
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
PATHS = ('tutorial', 'generic', 'fused', 'syncfree')
EPOCH_BATCHES = 4


def child(args):
    sys.path.insert(0, HERE)
    import torch
    import torchkge_amd as tk
    from torchkge_amd import optim
    from torchkge_amd.utils.training import Trainer
    from oracle import kge_oracle as orc
    kind, d, N, R, B = SHAPES[args.shape]
    rows = args.optimizer == 'rows'
    g = torch.Generator().manual_seed(3)
    n_facts = EPOCH_BATCHES * B
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
        opt = optim.RowAdagrad(m.parameters(), lr=0.05) if rows else torch.optim.Adagrad(m.parameters(), lr=0.05)
        trainer = None
        if path != 'tutorial':
            trainer = Trainer(m, loss_fn, kg, 1, B, opt, sampling_type='unif', use_cuda='all', fused=path != 'generic',
                              sync_free=path == 'syncfree', verbose=False)
        runs[path] = (m, opt, trainer)

    def tutorial_epochs(m, opt, epochs):
        for _ in range(epochs):
            for lo in range(0, n_facts, B):
                h, t, r = H[lo:lo + B], T[lo:lo + B], Rl[lo:lo + B]
                with tk.row_gradients(rows):
                    nh, nt = sampler.corrupt_batch(h, t, r)
                    loss = loss_fn(*m(h, t, r, nh, nt))
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
            m.normalize_parameters()

    def window(path, epochs):
        m, opt, trainer = runs[path]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        if trainer is None:
            tutorial_epochs(m, opt, epochs)
        else:
            with tk.row_gradients(rows):        # (the Trainer turns the switch on by itself for a row optimizer)
                trainer.n_epochs = epochs
                trainer.run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (epochs * EPOCH_BATCHES) * 1e3         # us per step

    for path in PATHS:
        window(path, 2)
    # (the faster of two probes: the first window after the warm-up still pays for the allocator's growth)
    reps = {p: max(1, min(1500, int(math.ceil(args.window * 1e6 / (EPOCH_BATCHES * min(window(p, 1), window(p, 1)))))))
            for p in PATHS}
    wins = {p: [] for p in PATHS}
    for _ in range(args.blocks):
        for p in PATHS:
            wins[p].append(window(p, reps[p]))
    assert runs['fused'][2]._fused_criterion is not None and runs['generic'][2]._fused_criterion is None
    assert next(runs['fused'][0].parameters()).grad.is_sparse == rows
    res = {'shape': args.shape, 'epochs': reps, 'step_us': {p: statistics.median(v) for p, v in wins.items()},
           'window_s': {p: statistics.median(v) * reps[p] * EPOCH_BATCHES * 1e-6 for p, v in wins.items()},
           'peak_GB': round(torch.cuda.max_memory_allocated() / 1e9, 2)}
    print('RESULT ' + json.dumps(res), flush=True)


def driver(args):
    out = []
    for shape in args.shapes.split(','):
        rs = []
        for i in range(args.procs):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--shape', shape, '--blocks', str(args.blocks),
                   '--window', str(args.window), '--optimizer', args.optimizer]
            txt = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout, check=True).stdout
            line = [x for x in txt.splitlines() if x.startswith('RESULT ')][-1]
            print('# shape %s process %d: %s' % (shape, i, line[7:]), file=sys.stderr, flush=True)
            rs.append(json.loads(line[7:]))
        kind, d, N, R, B = SHAPES[shape]
        out.append('shape %s: %s d = %d, N = %d, R = %d, B = %d (+ %d negatives), %d steps per epoch; %s; %d processes, '
                   'median of %d windows per path, windows of %s epochs (%.2f .. %.2f s)'
                   % (shape, kind, d, N, R, B, B, EPOCH_BATCHES,
                      'row gradients + RowAdagrad' if args.optimizer == 'rows' else 'dense gradients + torch Adagrad',
                      args.procs, args.blocks, ' / '.join('%d' % rs[0]['epochs'][p] for p in PATHS),
                      min(x['window_s'][p] for x in rs for p in PATHS), max(x['window_s'][p] for x in rs for p in PATHS)))
        out.append('  one training step, epoch overheads included (us, device events around a synchronised window)')
        med = {}
        for p in PATHS:
            v = [x['step_us'][p] for x in rs]
            med[p] = statistics.median(v)
            out.append('    %-9s median %10.1f   spread %10.1f .. %10.1f' % (p, med[p], min(v), max(v)))
        for a, b in (('tutorial', 'generic'), ('tutorial', 'fused'), ('generic', 'fused'), ('tutorial', 'syncfree')):
            ratios = [x['step_us'][a] / x['step_us'][b] for x in rs]
            out.append('    %s / %s: %.3f x   (per process %.3f .. %.3f)' % (a, b, med[a] / med[b], min(ratios), max(ratios)))
        out.append('    peak device memory of a process holding the four paths: %.2f GB' % max(x['peak_GB'] for x in rs))
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
    ap.add_argument('--optimizer', default='rows', choices=['rows', 'dense'])
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
