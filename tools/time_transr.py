# -*- coding: utf-8 -*-
"""TransR at FB15k-237 shape (14,541 entities, 237 relations, 20,466 test facts of a Zipf graph), d_e = d_r = 200 and
(200, 100): one JSON line per (shape, step), each step in a fresh child process under its own time limit; a step that
fails or runs out of time ends the run.

  fused   ms per LinkPredictionEvaluator.evaluate (median of --reps calls, device events around each call, after
          warm-up; the evaluator replays its captured hipGraph): the expanded KGE_LP_L2_PROJH problem
  exact   the same evaluation forced onto the exact relation-grouped path (l2_mode = 'direct', graph=False: per relation
          one KGE_LP_DOT problem for E M_r^T and one KGE_LP_L2_DIRECT problem), wall clock around synchronised calls
  kernel  kge_transr_proj_sqnorm alone on the whole entity table (the Z table of one evaluation): ms, and
          2 n_rel N d_e d_r / time as a fraction of the 155 TF fp32 MFMA peak

Tables have the norms of the golden fixture (standard deviations scaled by the square root of the dimension ratio), so
that the expansion is taken.

    python tools/time_transr.py [--reps 20] [--shapes 200x200,200x100] [--steps fused,exact,kernel]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ENT, N_REL, N_TEST = 14541, 237, 20466
PEAK_F32_MFMA = 155e12
LIMITS = {'fused': 300, 'exact': 420, 'kernel': 120}     # seconds per child


def events_ms(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2]


def child(step, de, dr, reps):
    import torch
    import torchkge_amd as tk
    from torchkge_amd import _hip
    from oracle import kge_oracle as orc
    g = torch.Generator().manual_seed(17)
    m = tk.TransRModel(de, dr, N_ENT, N_REL)
    with torch.no_grad():
        m.ent_emb.weight.copy_(torch.randn(N_ENT, de, generator=g) * (0.25 * (32.0 / de) ** 0.5))
        m.rel_emb.weight.copy_(torch.randn(N_REL, dr, generator=g) * (0.2 * (24.0 / dr) ** 0.5))
        m.proj_mat.weight.copy_(torch.randn(N_REL, dr * de, generator=g) * (0.15 * (24.0 / dr) ** 0.5))
    m = m.cuda()
    res = {'model': 'TransR', 'step': step, 'n_ent': N_ENT, 'n_rel': N_REL, 'd_e': de, 'd_r': dr, 'n_test': N_TEST}
    if step == 'kernel':
        E, M = m.ent_emb.weight.data, m.proj_mat.weight.data
        out = torch.empty(N_REL, _hip.padded_cols(N_ENT), dtype=torch.float32, device='cuda')
        run = lambda: _hip.transr_proj_sqnorm(M, E, de, dr, out=out)     # noqa: E731
        for _ in range(3):
            run()
        ms = events_ms(run, reps)
        flop = 2.0 * N_REL * N_ENT * de * dr
        res.update(kernel_ms=round(ms, 4), flop=flop, tflops=round(flop / (ms * 1e-3) / 1e12, 2),
                   fraction_of_peak=round(flop / (ms * 1e-3) / PEAK_F32_MFMA, 4))
    else:
        heads, tails, rels = orc.synthetic_triples_zipf(N_ENT, N_REL, 310116, seed=237)
        kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                               ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})
        _, kg_test = kg.split_kg(sizes=(len(heads) - N_TEST, N_TEST))
        if step == 'fused':
            ev = tk.LinkPredictionEvaluator(m, kg_test)
            for _ in range(3):
                ev.evaluate(b_size=2048, verbose=False)
            ms = events_ms(lambda: ev.evaluate(b_size=2048, verbose=False), reps)
        else:
            m.l2_mode = 'direct'
            ev = tk.LinkPredictionEvaluator(m, kg_test, graph=False)
            ev.evaluate(b_size=2048, verbose=False)
            times = []
            for _ in range(max(1, min(reps, 3))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev.evaluate(b_size=2048, verbose=False)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            ms = sorted(times)[len(times) // 2]
        res.update(evaluate_ms=round(ms, 4), path=m.lp_last_path, redo=bool(ev._last_redo),
                   mrr=[round(x, 6) for x in ev.mrr()])
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--shapes', default='200x200,200x100')
    ap.add_argument('--steps', default='fused,exact,kernel')
    ap.add_argument('--child', default=None)
    args = ap.parse_args()
    if args.child:
        step, de, dr = args.child.split(':')
        return child(step, int(de), int(dr), args.reps)
    for shape in args.shapes.split(','):
        de, dr = shape.split('x')
        for step in args.steps.split(','):
            cmd = [sys.executable, os.path.abspath(__file__), '--reps', str(args.reps), '--child', '%s:%s:%s' % (step, de, dr)]
            try:
                rc = subprocess.run(cmd, cwd=ROOT, timeout=LIMITS[step]).returncode
            except subprocess.TimeoutExpired:
                print(json.dumps({'step': step, 'd_e': int(de), 'd_r': int(dr), 'error': 'time limit'}), flush=True)
                return 124
            if rc != 0:     # nothing more is started on the GPU after a failed step
                print(json.dumps({'step': step, 'd_e': int(de), 'd_r': int(dr), 'error': 'exit %d' % rc}), flush=True)
                return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
