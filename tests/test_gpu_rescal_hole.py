"""GPU tests of RESCAL / HolE on the HIP engine (run with -m gpu on an MI355X): scoring_function forward / backward,
the relation-grouped query transform (kge_bilinear_query), the inference API, LinkPredictionEvaluator and
RelationPredictionEvaluator against the reference's fixtures, an FB15k-237-shaped graph, top-k inference and
row-sharded entity tables on two ranks.  float64 restatements are written from the models' formulas."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.helpers import ROOT, GOLDEN

pytestmark = pytest.mark.gpu

TOL = 1e-5
TIE = 2e-5
KINDS = ('rescal', 'hole')
NAMES = ['rank_true_heads', 'rank_true_tails', 'filt_rank_true_heads', 'filt_rank_true_tails']


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


def build(kind, E, rel, n_ent, n_rel, d, dev='cuda'):
    import torchkge_amd as tk
    m = tk.RESCALModel(d, n_ent, n_rel) if kind == 'rescal' else tk.HolEModel(d, n_ent, n_rel)
    key = 'rel_mat.weight' if kind == 'rescal' else 'rel_emb.weight'
    m.load_state_dict({'ent_emb.weight': torch.as_tensor(E).float().clone(), key: torch.as_tensor(rel).float().clone()})
    return m.to(dev)


def operators64(kind, rel, d):
    rel = rel.double()
    if kind == 'rescal':
        return rel.view(-1, d, d)
    i = torch.arange(d, device=rel.device).view(d, 1)
    j = torch.arange(d, device=rel.device).view(1, d)
    return rel[:, (j - i) % d]


def queries64(kind, E, rel, d, e, r, side):
    """float64 query rows: tail side x . B_r, head side B_r . x."""
    B = operators64(kind, rel, d)[r]
    x = E.double()[e]
    return torch.einsum('bi,bij->bj', x, B) if side == 'tail' else torch.einsum('bij,bj->bi', B, x)


def sf64(kind, E, rel, d, h, t, r):
    E = E.double()
    hn = E[h] / E[h].norm(dim=1, keepdim=True).clamp_min(1e-12)
    tn = E[t] / E[t].norm(dim=1, keepdim=True).clamp_min(1e-12)
    return torch.einsum('bi,bij,bj->b', hn, operators64(kind, rel, d)[r], tn)


def load(kind):
    import torchkge_amd as tk
    z = np.load(os.path.join(GOLDEN, 'ref_%s.npz' % kind))
    n_ent, n_rel, d = int(z['n_ent']), int(z['n_rel']), int(z['dim'])
    m = build(kind, z['table0'], z['table1'], n_ent, n_rel, d)
    heads, tails, rels = (torch.from_numpy(z[k]) for k in ('heads', 'tails', 'rels'))
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    nt = int(z['n_test'])
    _, kg_test = kg.split_kg(sizes=(len(heads) - nt, nt))
    return z, m, kg, kg_test


@pytest.mark.parametrize('kind', KINDS)
def test_scoring_function_and_forward_vs_reference(hip, kind):
    z, m, kg, kg_test = load(kind)
    B = int(z['b_size'])
    h, t, r = kg_test.head_idx[:B].cuda(), kg_test.tail_idx[:B].cuda(), kg_test.relations[:B].cuda()
    s = m.scoring_function(h, t, r)
    assert np.abs(s.detach().cpu().numpy() - z['sf']).max() < TOL
    pos, neg = m(h, t, r, torch.from_numpy(z['neg_heads']).cuda(), torch.from_numpy(z['neg_tails']).cuda())
    assert np.abs(pos.detach().cpu().numpy() - z['fwd_pos']).max() < TOL
    assert np.abs(neg.detach().cpu().numpy() - z['fwd_neg']).max() < TOL


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('B', [300, 5000])
def test_backward_vs_float64_autograd_and_repeatable(hip, kind, B):
    from torchkge_amd import _hip
    assert (B < _hip.BWD_SORTED_MIN_BATCH) == (B == 300)
    n_ent, n_rel, d = 700, 9, 24
    g = torch.Generator().manual_seed(11)
    E = torch.randn(n_ent, d, generator=g) * 0.3
    rel = torch.randn(n_rel, d * d if kind == 'rescal' else d, generator=g) * 0.3
    h = torch.randint(0, n_ent, (B,), generator=g)
    t = torch.randint(0, n_ent, (B,), generator=g)
    r = torch.randint(0, n_rel, (B,), generator=g)
    r[: (3 * B) // 4] = 4                                    # one relation holds most of the triples
    go = torch.randn(B, generator=g)
    E64, R64 = E.double().requires_grad_(), rel.double().requires_grad_()
    (sf64(kind, E64, R64, d, h, t, r) * go.double()).sum().backward()
    grads = []
    for _ in range(2):
        m = build(kind, E, rel, n_ent, n_rel, d)
        s = m.scoring_function(h.cuda(), t.cuda(), r.cuda())
        assert (s.detach().cpu().double() - sf64(kind, E, rel, d, h, t, r)).abs().max().item() < TOL
        (s * go.cuda()).sum().backward()
        gE, gR = m.ent_emb.weight.grad.cpu(), m._rel_param().weight.grad.cpu()
        scale = 1e-5 * max(1.0, float(E64.grad.abs().max()))
        assert (gE.double() - E64.grad).abs().max().item() < scale * 10
        assert (gR.double() - R64.grad).abs().max().item() < 1e-5 * max(1.0, float(R64.grad.abs().max())) * 10
        grads.append(gR)
    if kind == 'rescal':
        # d rel_mat is reduced per relation in sorted order (kge_rescal_rel_grad): no atomics, the same bits every run
        assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', [1, 8, 17, 32, 100, 200, 256, 512])
def test_query_transform_vs_float64_and_bit_identical(hip, kind, d):
    from torchkge_amd import _hip
    n_ent, n_rel = 400, 6
    g = torch.Generator().manual_seed(d)
    E = (torch.randn(n_ent, d, generator=g) * 0.2).cuda()
    rel = (torch.randn(n_rel, d * d if kind == 'rescal' else d, generator=g) * 0.2).cuda()
    B = 700
    h = torch.randint(0, n_ent, (B,), generator=g).cuda()
    t = torch.randint(0, n_ent, (B,), generator=g).cuda()
    r = torch.randint(0, n_rel, (B,), generator=g)
    r[5] = 5
    r[r == 5] = 4
    r[5] = 5                                                 # relation 5 has exactly one row
    r = r.cuda()
    code = _hip.RESCAL if kind == 'rescal' else _hip.HOLE
    Q = _hip.bilinear_query(code, _hip.SIDE_BOTH, E, rel, h, t, r)
    want = torch.cat([queries64(kind, E, rel, d, h, r, 'tail'), queries64(kind, E, rel, d, t, r, 'head')])
    assert (Q.double() - want).abs().max().item() < 4e-7 * d * max(1.0, float(want.abs().max()))
    # (e, r, side) alone fixes the row: other batch, other positions, one side at a time, unsorted
    perm = torch.randperm(B, generator=g).cuda()[:333]
    Qt = _hip.bilinear_query(code, _hip.SIDE_TAIL, E, rel, h[perm], t[perm], r[perm])
    Qh = _hip.bilinear_query(code, _hip.SIDE_HEAD, E, rel, h[perm], t[perm], r[perm], sort=False)
    assert torch.equal(Qt, Q[:B][perm]) and torch.equal(Qh, Q[B:][perm])
    # the same rows through the row-sharded contract: owners write them, everyone else zeros
    lo, hi = 100, 250
    Qs = _hip.bilinear_query(code, _hip.SIDE_BOTH, E[lo:hi].contiguous(), rel, h, t, r, ent_lo=lo, ent_n=hi - lo)
    own = torch.cat([(h >= lo) & (h < hi), (t >= lo) & (t < hi)])
    assert torch.equal(Qs[own], Q[own]) and bool((Qs[~own] == 0).all())


@pytest.mark.parametrize('kind', KINDS)
def test_query_transform_relation_with_many_rows(hip, kind):
    from torchkge_amd import _hip
    n_ent, n_rel, d = 3000, 4, 64
    g = torch.Generator().manual_seed(3)
    E = (torch.randn(n_ent, d, generator=g) * 0.2).cuda()
    rel = (torch.randn(n_rel, d * d if kind == 'rescal' else d, generator=g) * 0.2).cuda()
    B = 12000
    h = torch.randint(0, n_ent, (B,), generator=g).cuda()
    t = torch.randint(0, n_ent, (B,), generator=g).cuda()
    r = torch.full((B,), 2, dtype=torch.int64).cuda()
    r[:7] = 1
    code = _hip.RESCAL if kind == 'rescal' else _hip.HOLE
    Q = _hip.bilinear_query(code, _hip.SIDE_BOTH, E, rel, h, t, r)
    want = torch.cat([queries64(kind, E, rel, d, h, r, 'tail'), queries64(kind, E, rel, d, t, r, 'head')])
    assert (Q.double() - want).abs().max().item() < 4e-7 * d * max(1.0, float(want.abs().max()))
    Q1 = _hip.bilinear_query(code, _hip.SIDE_BOTH, E, rel, h[-50:], t[-50:], r[-50:])
    assert torch.equal(Q1[:50], Q[B - 50:B]) and torch.equal(Q1[50:], Q[2 * B - 50:])


@pytest.mark.parametrize('kind', KINDS)
def test_inference_api_vs_reference(hip, kind):
    z, m, kg, kg_test = load(kind)
    B = int(z['b_size'])
    h, t, r = kg_test.head_idx[:B].cuda(), kg_test.tail_idx[:B].cuda(), kg_test.relations[:B].cuda()
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=True)
    assert r_e.dim() == 3 and tuple(r_e.shape) == (B, m.emb_dim, m.emb_dim) and cand.stride(0) == 0
    for fn in (m.inference_scoring_function, m.lp_scoring_function):
        assert np.abs(fn(h_e, cand, r_e).cpu().numpy() - z['s_tail']).max() < TOL
        assert np.abs(fn(cand, t_e, r_e).cpu().numpy() - z['s_head']).max() < TOL
    # real materialised tensors, as a user may pass them
    R = r_e.materialize()
    C = cand.contiguous()
    assert np.abs(m.inference_scoring_function(h_e, C, R).cpu().numpy() - z['s_tail']).max() < TOL
    assert np.abs(m.inference_scoring_function(C, t_e, R).cpu().numpy() - z['s_head']).max() < TOL
    h2, t2, r2, c2 = m.lp_prep_cands(h, t, r)
    assert torch.equal(h2, h_e) and torch.equal(c2, cand)
    if kind == 'hole':
        import torchkge_amd as tk
        rr = m.rel_emb.weight.data[r]
        assert torch.equal(R, tk.HolEModel.get_rolling_matrix(rr))


@pytest.mark.parametrize('kind', KINDS)
def test_link_prediction_evaluator_vs_reference(hip, kind):
    import torchkge_amd as tk
    z, m, kg, kg_test = load(kind)
    B, d = int(z['b_size']), int(z['dim'])
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=B, verbose=False)
    # the reference's ranks, or inside the tie interval of the float64 restatement's scores
    E, rel = torch.from_numpy(z['table0']), torch.from_numpy(z['table1'])
    h, t, r = kg_test.head_idx, kg_test.tail_idx, kg_test.relations
    dh, dt, _ = orc.build_filter_dicts(kg.head_idx, kg.tail_idx, kg.relations)
    st = queries64(kind, E, rel, d, h, r, 'tail') @ E.double().T
    sh = queries64(kind, E, rel, d, t, r, 'head') @ E.double().T
    bounds = {'rank_true_tails': orc._tie_interval(st, t, TIE), 'rank_true_heads': orc._tie_interval(sh, h, TIE),
              'filt_rank_true_tails': orc._tie_interval(orc.filter_scores_vec(st, dt, h, r, t), t, TIE),
              'filt_rank_true_heads': orc._tie_interval(orc.filter_scores_vec(sh, dh, t, r, h), h, TIE)}
    for nm in NAMES:
        got, ref = getattr(ev, nm), torch.from_numpy(z[nm])
        lo, hi = bounds[nm]
        assert bool(((got == ref) | ((got >= lo) & (got <= hi))).all()), nm
    assert np.abs(np.array(ev.mrr()) - z['mrr']).max() < TOL
    assert np.abs(np.array(ev.hit_at_k(10)) - z['hit10']).max() < TOL
    assert np.abs(np.array(ev.mean_rank()) - z['mean_rank']).max() < 1e-3
    want = [getattr(ev, nm).clone() for nm in NAMES]

    def same(e, b_size=B, n=1):
        for _ in range(n):
            e.evaluate(b_size=b_size, verbose=False)
            for nm, w in zip(NAMES, want):
                assert torch.equal(getattr(e, nm), w), nm
    same(tk.LinkPredictionEvaluator(m, kg_test, fused=False), b_size=7)
    same(tk.LinkPredictionEvaluator(m, kg_test, both_sides=False), b_size=5)
    same(tk.LinkPredictionEvaluator(m, kg_test, coalesce=32768), b_size=3)
    same(tk.LinkPredictionEvaluator(m, kg_test, graph=True), n=3)
    m.split_filter = False
    same(tk.LinkPredictionEvaluator(m, kg_test))
    m.split_filter = True
    m.split_level = 1
    same(tk.LinkPredictionEvaluator(m, kg_test), n=2)
    m.split_level = 'auto'


@pytest.mark.parametrize('kind', KINDS)
def test_relation_prediction_vs_reference(hip, kind):
    import torchkge_amd as tk
    z0, m, kg, kg_test = load(kind)
    z = np.load(os.path.join(GOLDEN, 'ref_relpred_rescal_hole.npz'))
    n_ent, n_rel, d = int(z['n_ent']), int(z['n_rel']), int(z['dim'])
    m = build(kind, z['%s_table0' % kind], z['%s_table1' % kind], n_ent, n_rel, d)
    B = int(z['b_size'])
    h, t, r = kg_test.head_idx[:B].cuda(), kg_test.tail_idx[:B].cuda(), kg_test.relations[:B].cuda()
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=False)
    assert cand.dim() == 4 and tuple(cand.shape) == (B, n_rel, d, d)
    s = m.inference_scoring_function(h_e, t_e, cand)
    assert np.abs(s.cpu().numpy() - z['%s_s_rel' % kind]).max() < TOL
    s2 = m.inference_scoring_function(h_e, t_e, cand.materialize())             # stride-0 (b, n_rel, d, d) tensor
    s3 = m.inference_scoring_function(h_e, t_e, cand.materialize().contiguous())  # a real one
    assert (s2 - s).abs().max().item() < TOL and (s3 - s).abs().max().item() < TOL
    for directed, tag in ((True, 'dir'), (False, 'undir')):
        ev = tk.RelationPredictionEvaluator(m, kg_test, directed=directed)
        ev.evaluate(b_size=B, verbose=False)
        assert np.array_equal(ev.rank_true_rels.numpy(), z['%s_%s_rank' % (kind, tag)])
        assert np.array_equal(ev.filt_rank_true_rels.numpy(), z['%s_%s_frank' % (kind, tag)])
        assert abs(ev.mrr()[1] - z['%s_%s_mrr' % (kind, tag)][1]) < TOL
        assert abs(ev.hit_at_k(3)[1] - z['%s_%s_hit3' % (kind, tag)][1]) < TOL


@pytest.mark.parametrize('kind', KINDS)
def test_entity_inference_topk_equals_materialised(hip, kind):
    import torchkge_amd as tk
    z, m, kg, kg_test = load(kind)
    e, r = kg.head_idx[:200], kg.relations[:200]
    for missing, side in (('tails', 'tail'), ('heads', 'head')):
        a = tk.EntityInference(m, e, r, top_k=9, missing=missing, dictionary=None)
        a.evaluate(b_size=64, verbose=False)
        S = m.lp_problem(e.cuda(), e.cuda(), r.cuda(), side).scores().cpu()
        v, i = S.sort(dim=1, descending=True)
        assert torch.equal(a.scores.cpu(), v[:, :9])
        assert bool((S.gather(1, a.predictions.cpu()) == a.scores.cpu()).all())


@pytest.mark.parametrize('kind', KINDS)
def test_fb15k237_shape_ranks_vs_float64_and_split_equals_fp32(hip, kind):
    import torchkge_amd as tk
    n_ent, n_rel, d, n_test = 14541, 237, 200, 20466
    heads, tails, rels = orc.synthetic_triples_zipf(n_ent, n_rel, 310116, seed=237)
    g = torch.Generator().manual_seed(5)
    E = torch.nn.functional.normalize(torch.randn(n_ent, d, generator=g), dim=1)
    rel = torch.randn(n_rel, d * d if kind == 'rescal' else d, generator=g) * (0.07 if kind == 'rescal' else 1.0)
    m = build(kind, E, rel, n_ent, n_rel, d)
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    _, kg_test = kg.split_kg(sizes=(len(heads) - n_test, n_test))
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=2048, verbose=False)
    ev.evaluate(b_size=2048, verbose=False)
    m.split_filter = False
    ev2 = tk.LinkPredictionEvaluator(m, kg_test)
    ev2.evaluate(b_size=2048, verbose=False)
    m.split_filter = True
    for nm in NAMES:
        assert torch.equal(getattr(ev, nm), getattr(ev2, nm)), nm
    # raw ranks inside the tie interval of a float64 ATen restatement on the GPU
    Ed, Rd = E.cuda().double(), rel.cuda()
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    for side, nm, e, tr in (('tail', 'rank_true_tails', h, t), ('head', 'rank_true_heads', t, h)):
        got = getattr(ev, nm).cuda()
        for c0 in range(0, n_test, 2048):
            sl = slice(c0, c0 + 2048)
            S = queries64(kind, Ed, Rd, d, e[sl], r[sl], side) @ Ed.T
            lo, hi = orc._tie_interval(S, tr[sl], TIE)
            assert bool(((got[sl] >= lo) & (got[sl] <= hi)).all()), (nm, c0)


WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
rank, world, port, kind, out_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = port
torch.cuda.set_device(0)
dist.init_process_group('gloo', rank=rank, world_size=world)
import torchkge_amd as tk
from torchkge_amd import distributed as kd
from oracle import kge_oracle as orc
n_ent, n_rel, d = 3001, 11, 48
g = torch.Generator().manual_seed(3)
E = torch.nn.functional.normalize(torch.randn(n_ent, d, generator=g), dim=1)
rel = torch.randn(n_rel, d * d if kind == 'rescal' else d, generator=g) * 0.2
m = tk.RESCALModel(d, n_ent, n_rel) if kind == 'rescal' else tk.HolEModel(d, n_ent, n_rel)
m.load_state_dict({'ent_emb.weight': E, ('rel_mat.weight' if kind == 'rescal' else 'rel_emb.weight'): rel})
m = m.cuda()
h, t, r = orc.synthetic_triples_zipf(n_ent, n_rel, 20000, 9, hubs=((900, 'head'), (300, 'tail')))
kg = tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                       rel2ix={i: i for i in range(n_rel)})
_, kg_test = kg.split_kg(sizes=(19000, 1000))
ref = tk.LinkPredictionEvaluator(m, kg_test, graph=False)
ref.evaluate(b_size=256, verbose=False)
want = [ref.rank_true_heads, ref.rank_true_tails, ref.filt_rank_true_heads, ref.filt_rank_true_tails]
kd.shard_model_(m)
ok = True
for exchange, graph, qx in (('counts', False, 'evaluate'), ('counts', True, 'evaluate'), ('counts', False, 'batch')):
    ev = tk.LinkPredictionEvaluator(m, kg_test, shard='entities', exchange=exchange, graph=graph, query_exchange=qx)
    for _ in range(2):
        ev.evaluate(b_size=256, verbose=False)
    got = [ev.rank_true_heads, ev.rank_true_tails, ev.filt_rank_true_heads, ev.filt_rank_true_tails]
    for a, b in zip(want, got):
        if not torch.equal(a, b):
            ok = False
            print('MISMATCH', rank, kind, exchange, graph, qx, int((a != b).sum()), flush=True)
dist.barrier()
dist.destroy_process_group()
open(out_path, 'w').write('ok' if ok else 'bad')
sys.exit(0 if ok else 1)
'''


@pytest.mark.parametrize('kind', KINDS)
def test_row_sharded_two_ranks_on_one_gpu(kind, tmp_path):
    """Two ranks (gloo) sharing the one GPU, each holding half of ent_emb: the owner builds the query row
    (kge_bilinear_query on the shard, zeros elsewhere) or every rank builds it from the replicas; ranks equal the
    unsharded ones."""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'root': ROOT})
    port = str(31700 + (os.getpid() % 50) * 7 + KINDS.index(kind))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('KGE_FORCE_COLLECTIVES', None)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', port, kind, str(tmp_path / ('r%d' % r))],
                              env=env, cwd=ROOT) for r in range(2)]
    codes = [p.wait(timeout=600) for p in procs]
    assert codes == [0, 0]
