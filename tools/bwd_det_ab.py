"""Time one full backward of scoring_function -- kge_score_triples_bwd + key sort + row reduction, as
_hip.score_triples_bwd runs it -- with the deterministic mode off and on:

    python tools/bwd_det_ab.py [--shapes a,b,c] [--procs 3] [--reps 50] [--blocks 7] [--root DIR --label NAME] [--out FILE]

Shapes: (a) TransE d = 200, N = 14,541, R = 237, B = 32,768 (the benchmark's training batch); (b) the same with R = 11
(long relation runs); (c) ComplEx d = 512, N = 200,000, R = 822, B = 2^18.  Ids are Zipf(1) draws over permuted ids.

Method: every process is a fresh child of this driver (the driver never opens the GPU).  A child warms every mode up,
then times BLOCKS windows per mode with device events around REPS back-to-back calls, the modes ALTERNATING window by
window, and reports the median window per mode.  For the shapes whose launches are shorter than the host's enqueue (a, b)
it also captures REPS calls into a graph and times its replays: device time without the host.  The driver runs PROCS
children per tree and prints the median over the children with their min .. max as the run-to-run spread.  This tree
is run twice: both modes alternating in one process, and the default mode alone (the process to hold against the parent).

--root DIR: time the package of another checkout (the parent commit built in a scratch copy) with this same tool; a tree
without torchkge_amd.determinism has no mode column and is reported under --label.  Several --root / --label pairs may
be given; their children alternate with this tree's.

The parts (row kernel, the two sorts, the row sums) are timed one by one in the same child, eagerly."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    'a': ('transe', 200, 14541, 237, 32768),
    'b': ('transe', 200, 14541, 11, 32768),
    'c': ('complex', 512, 200000, 822, 1 << 18),
}


def child(args):
    sys.path.insert(0, args.root)
    import torch
    import torchkge_amd as tk
    from torchkge_amd import _hip
    from oracle import kge_oracle as orc
    assert os.path.realpath(os.path.dirname(os.path.dirname(tk.__file__))) == os.path.realpath(args.root)
    has_mode = hasattr(tk, 'deterministic')
    modes = args.modes.split(',') if has_mode else [args.label]
    kind, d, N, R, B = SHAPES[args.shape]
    g = torch.Generator().manual_seed(3)
    h = orc._zipf_draw(N, B, 1.0, g, torch.randperm(N, generator=g)).cuda()
    t = orc._zipf_draw(N, B, 1.0, g, torch.randperm(N, generator=g)).cuda()
    r = orc._zipf_draw(R, B, 1.0, g, torch.randperm(R, generator=g)).cuda()
    n_tab = 2 if kind == 'transe' else 4
    tabs = [(torch.randn(N if (i < 2 if n_tab == 4 else i < 1) else R, d, generator=g) * 0.1).cuda() for i in range(n_tab)]
    code = _hip.TRANSE_L2 if kind == 'transe' else _hip.COMPLEX
    go = torch.randn(B, generator=g).cuda()
    needs = (True,) * n_tab

    class mode_ctx(object):
        def __init__(self, m):
            self.c = tk.deterministic(m == 'on') if has_mode else None

        def __enter__(self):
            if self.c is not None:
                self.c.__enter__()

        def __exit__(self, *e):
            if self.c is not None:
                self.c.__exit__(*e)

    def bwd():
        return _hip.score_triples_bwd(code, tabs, d, d, h, t, r, go, needs)

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3        # us per call

    res = {'shape': args.shape, 'label': args.label, 'modes': modes, 'eager_us': {}, 'graph_us': {}, 'parts_us': {}}
    for m in modes:
        with mode_ctx(m):
            for _ in range(10):
                bwd()
    torch.cuda.synchronize()
    eager = {m: [] for m in modes}
    for _ in range(args.blocks):
        for m in modes:
            with mode_ctx(m):
                eager[m].append(window(bwd, args.reps))
    res['eager_us'] = {m: statistics.median(v) for m, v in eager.items()}
    rows_bytes = (3 if kind == 'transe' else 6) * B * d * 4
    if rows_bytes < (1 << 30):          # device time of REPS calls replayed from a graph
        graphs = {}
        for m in modes:
            with mode_ctx(m):
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for _ in range(args.reps):
                        bwd()
                gr.replay()
                graphs[m] = gr
        torch.cuda.synchronize()
        rep = {m: [] for m in modes}
        for _ in range(args.blocks):
            for m in modes:
                rep[m].append(window(graphs[m].replay, 1) / args.reps)
        res['graph_us'] = {m: statistics.median(v) for m, v in rep.items()}
        del graphs
    # the parts, one by one (eager windows)
    lib = _hip.load_library()
    p, st = _hip._p, _hip._stream
    n_streams = 3 if kind == 'transe' else 6
    rows = torch.empty(n_streams * B * d, dtype=torch.float32, device='cuda')
    t4 = [p(x) for x in tabs] + [None] * (4 - n_tab)

    def rows_kernel():
        _hip._check(lib.kge_score_triples_bwd(code, t4[0], t4[1], t4[2], t4[3], d, d, p(h), p(t), p(r), B, p(go), None, None,
                                              None, None, p(rows), d, st()), 'kge_score_triples_bwd')
    parts = {'rows_kernel': window(rows_kernel, args.reps),
             'sort_ht': window(lambda: _hip._key_perm(h, t, N), args.reps),
             'sort_r': window(lambda: _hip._key_perm(r, None, R), args.reps)}
    perm_ht, perm_r = _hip._key_perm(h, t, N), _hip._key_perm(r, None, R)
    gE, gR = torch.zeros(N, d, device='cuda'), torch.zeros(R, d, device='cuda')
    r_off = (n_streams - 1) * B * d * 4     # one entity stream and one relation stream (ComplEx has two of each per table pair)
    if has_mode:
        from torchkge_amd import _hip_det
        for m in modes:
            with mode_ctx(m):
                for _ in range(3):
                    _hip_det.segment_sum(rows, d, d, h, B, t, B, perm_ht, gE, d)
                    _hip_det.segment_sum(rows.data_ptr() + r_off, d, d, r, B, None, 0, perm_r, gR, d)
                parts['sum_ht_' + m] = window(lambda: _hip_det.segment_sum(rows, d, d, h, B, t, B, perm_ht, gE, d), args.reps)
                parts['sum_r_' + m] = window(lambda: _hip_det.segment_sum(rows.data_ptr() + r_off, d, d, r, B, None, 0, perm_r, gR, d),
                                             args.reps)
    else:
        def seg(k0, n0, k1, n1, perm, out, off):
            _hip._check(lib.kge_segment_sum_rows(rows.data_ptr() + off, d, d, p(k0), n0, p(k1), n1, p(perm), p(out), d, st()),
                        'kge_segment_sum_rows')
        parts['sum_ht_' + args.label] = window(lambda: seg(h, B, t, B, perm_ht, gE, 0), args.reps)
        parts['sum_r_' + args.label] = window(lambda: seg(r, B, None, 0, perm_r, gR, r_off), args.reps)
    res['parts_us'] = parts
    print('RESULT ' + json.dumps(res), flush=True)


def driver(args):
    # this tree twice: both modes alternating in one process, and the default mode ALONE -- the process whose allocations
    # and launches are the parent's, which is the one to hold against the parent
    trees = [(HERE, 'branch', 'off,on'), (HERE, 'branch, off alone', 'off')] + [(r, l, 'off') for r, l in zip(args.root or [], args.label or [])]
    out = []
    for shape in args.shapes.split(','):
        runs = {}
        for i in range(args.procs):
            for root, label, modes in trees:    # the trees alternate, process by process
                cmd = [sys.executable, os.path.abspath(__file__), '--child', '--shape', shape, '--root', os.path.abspath(root),
                       '--label', label, '--modes', modes, '--reps', str(args.reps), '--blocks', str(args.blocks)]
                txt = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout, check=True).stdout
                line = [x for x in txt.splitlines() if x.startswith('RESULT ')][-1]
                print('# shape %s process %d %s: %s' % (shape, i, label, line[7:]), file=sys.stderr, flush=True)
                runs.setdefault(label, []).append(json.loads(line[7:]))
        kind, d, N, R, B = SHAPES[shape]
        out.append('shape (%s): %s d = %d, N = %d, R = %d, B = %d; %d processes per tree, median window of %d x %d calls'
                   % (shape, kind, d, N, R, B, args.procs, args.blocks, args.reps))
        for key, title in (('eager_us', 'full backward, eager (us per call, events)'),
                           ('graph_us', 'full backward, graph replay (us per call, device only)'),
                           ('parts_us', 'parts, eager (us per call)')):
            out.append('  ' + title)
            for label, rs in runs.items():
                for col in rs[0][key]:
                    v = [x[key][col] for x in rs]
                    name = col if key == 'parts_us' or col == label else 'mode ' + col
                    out.append('    %-28s median %9.1f   spread %9.1f .. %9.1f   (%s)'
                               % (name, statistics.median(v), min(v), max(v), label))
    text = '\n'.join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--shape', default='a')
    ap.add_argument('--shapes', default='a,b,c')
    ap.add_argument('--modes', default='off,on')
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--root', action='append')
    ap.add_argument('--label', action='append')
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.child:
        a.root, a.label = a.root[0], a.label[0]
        child(a)
    else:
        driver(a)
