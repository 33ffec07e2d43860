# -*- coding: utf-8 -*-
"""Data-redundancy analytics at FB15k's shape: 14,951 entities, 1,345 relations, 592,213 facts of the project's Zipf
generator (oracle.kge_oracle.synthetic_triples_zipf) in which 300 rare relations are replaced by copies (every second one:
reversed copies) of 300 others, split 80 / 10 / 10.

    python tools/redundancy_time.py --out FILE           the engine, in 3 fresh processes, beside the numpy restatement
    python tools/redundancy_time.py --reference DIR      the reference itself (torchkge imported from DIR) on this CPU

Engine: ``duplicates(kg_tr, kg_val, kg_te, counts=True)`` of torchkge_amd.utils.data_redundancy, ids starting on the
host, wall clock around a device synchronise.  Each process reports its first call (code-object load included) and the
median of --reps further calls; the report gives the median of the three processes' medians with min .. max.  One more
call per process runs under torch.profiler for the per-launch times of the sort and the pair-count kernel.  The lists are
compared with the restatement's (tests/redundancy_ref.py, timed on the host CPU beside it): equal, or the run fails.

The pair-count kernel has one add form, the plain one (one int32 atomicAdd per partner).  A wave-aggregated form was
measured against it once, lost and was deleted; profiles/r09/redundancy.txt keeps that A/B below this tool's report.
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import kge_oracle as orc  # noqa: E402
from tests import redundancy_ref as rd  # noqa: E402

N_ENT, N_REL, N_FACTS, N_PLANTED, SEED = 14951, 1345, 592213, 300, 15


def make_graphs():
    """(train, valid, test) as light graph objects with CPU id tensors, and the (h, t, r) numpy arrays of the union."""
    h, t, r = (x.numpy() for x in orc.synthetic_triples_zipf(N_ENT, N_REL, N_FACTS + 10000, seed=SEED))
    cnt = np.bincount(r, minlength=N_REL)
    rare = [int(i) for i in np.argsort(cnt, kind='stable') if cnt[i] >= 5][:2 * N_PLANTED]
    src, dst = rare[:N_PLANTED], rare[N_PLANTED:]
    keep = ~np.isin(r, dst)
    hs, ts, rs = [h[keep]], [t[keep]], [r[keep]]
    for i, (p, q) in enumerate(zip(src, dst)):
        m = r == p
        hs.append(t[m] if i % 2 else h[m])
        ts.append(h[m] if i % 2 else t[m])
        rs.append(np.full(int(m.sum()), q))
    h, t, r = np.concatenate(hs), np.concatenate(ts), np.concatenate(rs)
    perm = np.random.RandomState(SEED).permutation(len(h))
    h, t, r = h[perm][:N_FACTS], t[perm][:N_FACTS], r[perm][:N_FACTS]     # (planting removes a few thousand facts: cut to size)
    n = len(h)
    cut = (0, int(0.8 * n), int(0.9 * n), n)
    kgs = []
    for lo, hi in zip(cut[:-1], cut[1:]):
        g = rd.Graph(h[lo:hi], t[lo:hi], r[lo:hi], N_ENT, N_REL)
        for nm in ('head_idx', 'tail_idx', 'relations'):
            setattr(g, nm, torch.from_numpy(getattr(g, nm)))
        kgs.append(g)
    return kgs, (h, t, r)


def numpy_graphs(kgs):
    return [rd.Graph(g.head_idx.numpy(), g.tail_idx.numpy(), g.relations.numpy(), N_ENT, N_REL) for g in kgs]


def restatement(kgs):
    """What duplicates(..., counts=True) computes, by tests/redundancy_ref.py: the two lists and the three count pairs."""
    ng = numpy_graphs(kgs)
    dup, rev = rd.duplicates(*ng)
    cnts = [rd.count_triplets(k1, k2, dup, rev) for k1, k2 in ((ng[0], ng[0]), (ng[0], ng[2]), (ng[2], ng[2]))]
    return dup, rev, cnts


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        out = fn()
    return out, buf.getvalue()


def child(reps):
    from torchkge_amd.utils import data_redundancy as dr
    assert torch.cuda.is_available(), 'the engine is timed on an MI355X; there is no fallback'
    kgs, _ = make_graphs()
    torch.cuda.init()
    torch.cuda.synchronize()

    def call():
        return dr.duplicates(*kgs, counts=True)
    t0 = time.perf_counter()
    (dup, rev), text = quiet(call)
    torch.cuda.synchronize()
    first = (time.perf_counter() - t0) * 1e3
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        quiet(call)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    out = dict(first_ms=first, warm_ms=times[len(times) // 2], warm_min_ms=times[0], warm_max_ms=times[-1], n_dup=len(dup), n_rev=len(rev),
               device=torch.cuda.get_device_name(0), dup=dup, rev=rev, printed=[ln for ln in text.split('\n') if ln], kernels=None)
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            quiet(call)
            torch.cuda.synchronize()
        rows = {}
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA:
                c = rows.setdefault(e.name, [0, 0.0])
                c[0] += 1
                c[1] += e.device_time if hasattr(e, 'device_time') else e.cuda_time
        out['kernels'] = sorted(([k, v[0], v[1]] for k, v in rows.items()), key=lambda x: -x[2])
    except Exception as exc:       # noqa: BLE001 -- a missing profiler backend must not cost the timings
        out['kernels_error'] = repr(exc)
    print('RESULT ' + json.dumps(out), flush=True)


def parent(out_path, reps, processes):
    kgs, _ = make_graphs()
    n = [len(g) for g in kgs]
    t0 = time.perf_counter()
    want_dup, want_rev, want_counts = restatement(kgs)
    numpy_s = time.perf_counter() - t0
    runs = []
    for _ in range(processes):      # one after the other: fresh processes, never two on the device at once
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--reps', str(reps)], stdout=subprocess.PIPE,
                           text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit('a timing process ended with status %d' % r.returncode)
        runs.append(json.loads([ln for ln in r.stdout.split('\n') if ln.startswith('RESULT ')][-1][7:]))
    for run in runs:
        assert [tuple(p) for p in run['dup']] == want_dup and [tuple(p) for p in run['rev']] == want_rev, 'lists differ from the restatement'
        got = [int(ln.split()[0]) for ln in run['printed']]
        assert got == [c for pair in want_counts for c in pair], 'counts differ from the restatement'

    def mid(key):
        v = sorted(run[key] for run in runs)
        return '%.1f ms (min %.1f .. max %.1f)' % (v[len(v) // 2], v[0], v[-1])
    lines = ['Data-redundancy analytics at FB15k shape: %d entities, %d relations, %d facts (%d / %d / %d), %d planted pairs'
             % (N_ENT, N_REL, sum(n), n[0], n[1], n[2], N_PLANTED),
             'device: %s' % runs[0].get('device', 'MI355X'),
             'duplicates(kg_tr, kg_val, kg_te, counts=True): %d duplicate pairs, %d reverse pairs; lists and counts equal the numpy restatement'
             % (len(want_dup), len(want_rev)),
             '',
             'engine, %d fresh processes, ids start on the host, wall clock around a device synchronise:' % processes,
             '  first call of a process (code objects loaded)   median %s' % mid('first_ms'),
             '  later calls (median of %d per process)           median %s' % (reps, mid('warm_ms')),
             'numpy restatement (tests/redundancy_ref.py) on the host CPU of the same machine, one run: %.2f s' % numpy_s,
             '',
             'device operations of one call (torch.profiler, a run of its own; count, total us), first process:']
    if runs[0]['kernels'] is None:
        lines.append('  not measured: %s' % runs[0].get('kernels_error'))
    else:
        for name, count, us in runs[0]['kernels']:
            lines.append('  %8.1f us  x%-3d %s' % (us, count, name[:110]))
        sort_us = sum(k[2] for k in runs[0]['kernels'] if 'radix' in k[0].lower() or 'sort' in k[0].lower() or 'onesweep' in k[0].lower())
        n_sorts = 1 + 2 + 3        # relation_overlaps: one overlap sort, two stats sorts; three count_triplets overlaps
        count = [k for k in runs[0]['kernels'] if 'ro_count_kernel' in k[0]]
        lines.append('  rocPRIM sort kernels in total: %.1f us over %d sorts' % (sort_us, n_sorts))
        for k in count:
            lines.append('  pair-count kernel (plain int32 atomicAdd form): %.1f us over %d launches (the first is the union of the '
                         'three graphs, the others the count_triplets lists)' % (k[2], k[1]))
    lines += ['', 'the lines printed with counts=True:'] + ['  ' + ln for ln in runs[0]['printed']]
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)
    print(text)


def reference(path):
    """The reference's own duplicates(..., counts=True) on this machine's CPU, at the same shape."""
    sys.path.insert(0, path)
    from torchkge.utils import data_redundancy as ref
    kgs, _ = make_graphs()
    t0 = time.perf_counter()
    (dup, rev), text = quiet(lambda: ref.duplicates(*kgs, counts=True))
    s = time.perf_counter() - t0
    want_dup, want_rev, _ = restatement(kgs)
    print('reference duplicates(..., counts=True) at FB15k shape on this CPU (%d cores): %.1f s; %d duplicate pairs, %d reverse pairs; '
          'lists equal the restatement: %s' % (os.cpu_count(), s, len(dup), len(rev), dup == want_dup and rev == want_rev))
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r09', 'redundancy.txt'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--processes', type=int, default=3)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--reference', default=None, metavar='DIR')
    args = ap.parse_args()
    if args.reference:
        reference(args.reference)
    elif args.child:
        child(args.reps)
    else:
        parent(args.out, args.reps, args.processes)


if __name__ == '__main__':
    main()
