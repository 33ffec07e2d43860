"""GPU tests of RotatEModel (run with -m gpu on an MI355X): scoring_function forward / backward against the float64
complex formula and float64 autograd, the zero-modulus gradient, row gradients, LinkPredictionEvaluator (filtered, with
its graph replay), EntityInference top-k, relation prediction, training with K negatives per fact and the
self-adversarial criterion, the grouped scorer's fallback and row-sharded entity tables on two ranks.  The yardstick is
tests/rotate_ref.py, float64 on the fp32 tables the engine holds."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.helpers import ROOT
from tests import rotate_ref as ref
from tests.test_gpu_toruse import TOL, TIE, close, NAMES
from tests.test_gpu_layout_contract import GRAD_TOL, grad_close

pytestmark = pytest.mark.gpu

N_ENT, N_REL, N_FACTS = 50, 5, 300
DIMS = (3, 16, 17)
BATCHES = (0, 7, 300)
# per emb_dim the seed of tables(): chosen on the CPU so that the float64 reference has no other candidate within TIE of a
# true score, raw or filtered, entity or relation side (tests/test_rotate_host.py checks it, without a GPU)
SEEDS = {3: 1, 16: 1, 17: 1}


def tables(d):
    g = torch.Generator().manual_seed(SEEDS[d] * 100 + d)
    E = torch.rand(N_ENT, 2 * d, generator=g) * 2 - 1
    P = (torch.rand(N_REL, d, generator=g) * 2 - 1) * math.pi
    h, t, r = (torch.randint(0, n, (N_FACTS,), generator=g) for n in (N_ENT, N_ENT, N_REL))
    return E, P, h, t, r


def bits(x):
    return x.contiguous().view(torch.int32)


def build(d, E, P, n_ent=N_ENT, n_rel=N_REL):
    import torchkge_amd as tk
    m = tk.RotatEModel(d, n_ent, n_rel)
    m.load_state_dict({'ent_emb.weight': E.clone(), 'rel_emb.weight': P.clone()})
    return m.cuda()


def graph(h, t, r, n_ent=N_ENT, n_rel=N_REL):
    import torchkge_amd as tk
    return tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                             rel2ix={i: i for i in range(n_rel)})


def reference_ranks(d):
    """float64 ranks of the 300 facts from the fp32 tables, raw and filtered, with their tie intervals; and the relation
    side."""
    E, P, h, t, r = tables(d)
    dh, dt, dr = orc.build_filter_dicts(h, t, r)
    st, sh = ref.scores64(E, P, h, t, r, 'tail'), ref.scores64(E, P, h, t, r, 'head')
    sr = ref.relation_scores64(E, P, h, t)
    mats = {'rank_true_tails': (st, t), 'rank_true_heads': (sh, h),
            'filt_rank_true_tails': (orc.filter_scores_vec(st, dt, h, r, t), t),
            'filt_rank_true_heads': (orc.filter_scores_vec(sh, dh, t, r, h), h),
            'rank_true_rels': (sr, r), 'filt_rank_true_rels': (orc.filter_scores_vec(sr, dr, h, t, r), r)}
    out = {}
    for nm, (S, true) in mats.items():
        rank = (S >= S.gather(1, true.view(-1, 1))).sum(1)
        out[nm] = (rank,) + tuple(orc._tie_interval(S, true, TIE))
    return out


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


# ---- score and backward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('d', DIMS)
def test_scoring_function_vs_float64(hip, d, B):
    E, P, h, t, r = tables(d)
    m = build(d, E, P)
    s = m.scoring_function(h[:B].cuda(), t[:B].cuda(), r[:B].cuda())
    assert tuple(s.shape) == (B,) and s.requires_grad
    assert B == 0 or close(s.detach().cpu(), ref.sf64(E, P, h[:B], t[:B], r[:B]))
    # forward: positives and negatives in one launch, the same bits
    if B:
        pos, neg = m(h[:B].cuda(), t[:B].cuda(), r[:B].cuda(), t[:B].cuda(), h[:B].cuda())
        assert torch.equal(bits(pos), bits(s)) and close(neg.detach().cpu(), ref.sf64(E, P, t[:B], h[:B], r[:B]))


def backward(d, E, P, h, t, r, go):
    m = build(d, E, P)
    (m.scoring_function(h.cuda(), t.cuda(), r.cuda()) * go.cuda()).sum().backward()
    return m.ent_emb.weight.grad, m.rel_emb.weight.grad


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('d', DIMS)
def test_backward_vs_float64_autograd_and_deterministic_twice(hip, d, B):
    import torchkge_amd as tk
    E, P, h, t, r = tables(d)
    keep = h != t       # (a random fact with h == t has y != 0 unless theta == 0: kept out only to keep the reference smooth)
    h, t, r = h[keep][:B], t[keep][:B], r[keep][:B]
    go = torch.randn(h.shape[0], generator=torch.Generator().manual_seed(B))
    wE, wP = ref.grads64(E, P, h, t, r, go)
    gE, gP = backward(d, E, P, h, t, r, go)
    assert not gE.is_sparse and grad_close(gE.cpu().double(), wE) and grad_close(gP.cpu().double(), wP)
    with tk.deterministic():
        a = backward(d, E, P, h, t, r, go)
        b = backward(d, E, P, h, t, r, go)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    assert grad_close(a[0].cpu().double(), wE) and grad_close(a[1].cpu().double(), wP)


@pytest.mark.parametrize('d', DIMS)
def test_zero_modulus_coordinates_have_zero_gradient(hip, d):
    """Triples with h == t under a relation whose phases are 0: y = 0 in every coordinate, where the written-out
    sqrt(re^2 + im^2) differentiates to NaN.  Alone they leave every gradient exactly zero; mixed into a batch they change
    nothing beyond the rounding of a reordered sum."""
    import torchkge_amd as tk
    E, P, h, t, r = tables(d)
    P[0] = 0.0
    keep = h != t
    h, t, r = h[keep][:64], t[keep][:64], r[keep][:64]
    zh = torch.arange(0, 20)
    go = torch.randn(84, generator=torch.Generator().manual_seed(3))
    gE, gP = backward(d, E, P, zh, zh, torch.zeros(20, dtype=torch.int64), go[:20])
    assert not bool(gE.any()) and not bool(gP.any())
    s = build(d, E, P).scoring_function(zh.cuda(), zh.cuda(), torch.zeros(20, dtype=torch.int64).cuda())
    assert not bool(s.any())
    wE, wP = ref.grads64(E, P, h, t, r, go[20:])
    for det in (False, True):
        with tk.deterministic(det):
            gE, gP = backward(d, E, P, torch.cat([zh, h]), torch.cat([zh, t]), torch.cat([torch.zeros(20, dtype=torch.int64), r]), go)
        assert bool(torch.isfinite(gE).all()) and bool(torch.isfinite(gP).all())
        assert grad_close(gE.cpu().double(), wE) and grad_close(gP.cpu().double(), wP)
    # a single coordinate at zero inside an otherwise ordinary triple
    E2 = E.clone()
    E2[1, 0:2] = E2[0, 0:2]
    gE, gP = backward(d, E2, P, torch.tensor([0]), torch.tensor([1]), torch.tensor([0]), torch.ones(1))
    assert bool(torch.isfinite(gE).all()) and not bool(gE[:2, 0:2].any()) and float(gP[0, 0]) == 0.0
    assert d == 1 or bool(gE[:2, 2:].any())


@pytest.mark.parametrize('d', DIMS)
def test_row_gradients_equal_the_dense_deterministic_ones_and_rowadagrad_steps(hip, d):
    import torchkge_amd as tk
    from torchkge_amd import optim
    E, P, h, t, r = tables(d)
    go = torch.randn(N_FACTS, generator=torch.Generator().manual_seed(5))
    with tk.deterministic():
        dE, dP = backward(d, E, P, h, t, r, go)
    m = build(d, E, P)
    with tk.row_gradients():
        loss = (m.scoring_function(h.cuda(), t.cuda(), r.cuda()) * go.cuda()).sum()
    loss.backward()
    row, dense = optim.split_parameters(m)
    assert len(row) == 2 and dense == []
    for p, want, n_ids in ((m.ent_emb.weight, dE, 2 * N_FACTS), (m.rel_emb.weight, dP, N_FACTS)):
        assert p.grad.is_sparse and p.grad._nnz() == n_ids and tuple(p.grad.shape) == tuple(p.shape)
        uniq, rows, count = optim.coalesce_rows(p.grad)
        scat = torch.zeros_like(want)
        scat[uniq[:int(count)]] = rows[:int(count)]
        assert torch.equal(bits(scat), bits(want))
    before = [p.detach().clone() for p in row]
    opt = optim.RowAdagrad(row, lr=0.1)
    opt.step()
    touched = torch.zeros(N_ENT, dtype=torch.bool)
    touched[torch.cat([h, t])] = True
    for p, b, live in zip(row, before, (touched, torch.ones(N_REL, dtype=torch.bool))):
        assert bool(torch.isfinite(p).all())
        assert torch.equal(bits(p.detach()[~live.cuda()]), bits(b[~live.cuda()])) and bool((p.detach()[live.cuda()] != b[live.cuda()]).any())


# ---- evaluation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', DIMS)
def test_link_prediction_evaluator_vs_float64_ranks_and_replay(hip, d):
    import torchkge_amd as tk
    E, P, h, t, r = tables(d)
    m = build(d, E, P)
    kg = graph(h, t, r)
    want = reference_ranks(d)
    ev = tk.LinkPredictionEvaluator(m, kg)
    ev.evaluate(b_size=128, verbose=False)
    excused = 0
    for nm in NAMES:
        got, (rank, lo, hi) = getattr(ev, nm).cpu(), want[nm]
        assert bool(((got == rank) | ((got >= lo) & (got <= hi))).all()), nm
        excused += int((got != rank).sum())
    assert excused == 0     # (the seeds leave no near-tie: tests/test_rotate_host.py)
    first = [getattr(ev, nm).clone() for nm in NAMES]
    ev.evaluate(b_size=128, verbose=False)     # the same objects again: the replay
    for nm, w in zip(NAMES, first):
        assert torch.equal(getattr(ev, nm), w), nm
    # the captured graph, the unfused path and one side at a time give the same ranks
    evg = tk.LinkPredictionEvaluator(m, kg, graph=True)
    for _ in range(3):
        evg.evaluate(b_size=128, verbose=False)
        for nm, w in zip(NAMES, first):
            assert torch.equal(getattr(evg, nm), w), nm
    for kw, b in (({'fused': False}, 7), ({'both_sides': False}, 300)):
        e2 = tk.LinkPredictionEvaluator(m, kg, **kw)
        e2.evaluate(b_size=b, verbose=False)
        for nm, w in zip(NAMES, first):
            assert torch.equal(getattr(e2, nm), w), (nm, kw)
    assert int(m.lp_problem(h.cuda(), t.cuda(), r.cuda(), 'both').desc.mode) == hip.LP_CMOD


@pytest.mark.parametrize('d', DIMS)
def test_inference_api_and_entity_topk_equal_the_materialised_matrix(hip, d):
    import torchkge_amd as tk
    E, P, h, t, r = tables(d)
    m = build(d, E, P)
    hc, tc, rc = h.cuda(), t.cuda(), r.cuda()
    S = {side: m.lp_problem(hc, tc, rc, side).scores() for side in ('tail', 'head')}
    assert close(S['tail'].cpu(), ref.scores64(E, P, h, t, r, 'tail')) and close(S['head'].cpu(), ref.scores64(E, P, h, t, r, 'head'))
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(hc, tc, rc, entities=True)
    assert tuple(cand.shape) == (N_FACTS, N_ENT, 2 * d) and cand.stride(0) == 0     # a view: no (b, N, 2d) tensor
    assert cand.data_ptr() == m.ent_emb.weight.data_ptr()
    for fn in (m.inference_scoring_function, m.lp_scoring_function):
        assert torch.equal(bits(fn(h_e, cand, r_e)), bits(S['tail'])) and torch.equal(bits(fn(cand, t_e, r_e)), bits(S['head']))
    # a real (b, N, 2d) tensor, as a user may pass it: the generic batched kernel (its own summation order)
    C = cand[:9].contiguous()
    assert close(m.inference_scoring_function(h_e[:9], C, r_e[:9]).cpu(), S['tail'][:9].cpu().double())
    assert close(m.inference_scoring_function(C, t_e[:9], r_e[:9]).cpu(), S['head'][:9].cpu().double())
    none = torch.zeros(0, dtype=torch.int64, device='cuda')
    assert tuple(m.inference_prepare_candidates(hc, none, rc)[1].shape) == (0, 2 * d)
    for missing, side in (('tails', 'tail'), ('heads', 'head')):
        for dictionary in (None, graph(h, t, r).dict_of_tails if side == 'tail' else graph(h, t, r).dict_of_heads):
            e = h if side == 'tail' else t
            a = tk.EntityInference(m, e, r, top_k=9, missing=missing, dictionary=dictionary)
            a.evaluate(b_size=64, verbose=False)
            M = S[side].cpu().clone()
            if dictionary is not None:
                for i, (a_, b_) in enumerate(zip(e.tolist(), r.tolist())):
                    M[i, sorted(dictionary[(a_, b_)])] = -float('inf')
            v, _ = M.sort(dim=1, descending=True)
            assert torch.equal(a.scores, v[:, :9]), (side, dictionary is None)
            assert bool((M.gather(1, a.predictions) == a.scores).all())


@pytest.mark.parametrize('d', DIMS)
def test_relation_prediction_vs_float64(hip, d):
    import torchkge_amd as tk
    E, P, h, t, r = tables(d)
    m = build(d, E, P)
    hc, tc, rc = h.cuda(), t.cuda(), r.cuda()
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(hc, tc, rc, entities=False)
    assert tuple(cand.shape) == (N_FACTS, N_REL, d) and cand.stride(0) == 0
    S = m.inference_scoring_function(h_e, t_e, cand)
    assert close(S.cpu(), ref.relation_scores64(E, P, h, t))
    assert torch.equal(bits(S[torch.arange(N_FACTS), rc]), bits(m.scoring_function(hc, tc, rc).detach()))
    # chunked, and on a materialised (b, n_rel, d) tensor: the same bits
    m.RELATION_CHUNK = 64
    assert torch.equal(bits(m.inference_scoring_function(h_e, t_e, cand)), bits(S))
    assert torch.equal(bits(m.inference_scoring_function(h_e, t_e, cand.contiguous())), bits(S))
    del m.RELATION_CHUNK
    want = reference_ranks(d)
    ev = tk.RelationPredictionEvaluator(m, graph(h, t, r))
    ev.evaluate(b_size=128, verbose=False)
    for nm in ('rank_true_rels', 'filt_rank_true_rels'):
        assert torch.equal(getattr(ev, nm).cpu(), want[nm][0]), nm
    from torchkge_amd.inference import RelationInference
    a = RelationInference(m, h, t, top_k=3, dictionary=None)
    a.evaluate(b_size=100, verbose=False)
    v, _ = S.cpu().sort(dim=1, descending=True)
    assert torch.equal(a.scores, v[:, :3])


# ---- training ----------------------------------------------------------------------------------------------------------
def train(d, grouped_forward=False, epochs=2, row=False):
    import torchkge_amd as tk
    from torchkge_amd import optim
    from torchkge_amd.utils.training import Trainer
    from torchkge_amd.utils.group_losses import SelfAdversarialLoss
    E, P, h, t, r = tables(d)
    m = build(d, E, P)
    torch.manual_seed(9)
    opt = optim.RowAdagrad(m.parameters(), lr=0.1) if row else torch.optim.Adagrad(m.parameters(), lr=0.1)
    tr = Trainer(m, SelfAdversarialLoss(margin=6.0), graph(h, t, r), epochs, 100, opt, use_cuda='all', verbose=False, n_neg=8)
    tr.grouped_forward = grouped_forward
    tr.run()
    return tr.epoch_losses, [p.detach().clone() for p in m.parameters()]


@pytest.mark.parametrize('d', DIMS)
def test_training_with_eight_negatives_and_the_self_adversarial_loss(hip, d):
    import torchkge_amd as tk
    losses, tabs = train(d)
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[1] < losses[0]
    E, P = tables(d)[:2]
    assert all(bool(torch.isfinite(x).all()) for x in tabs) and not torch.equal(tabs[0].cpu(), E) and not torch.equal(tabs[1].cpu(), P)
    with tk.deterministic():
        l1, a = train(d)
        l2, b = train(d)
        l3, c = train(d, grouped_forward=True)
    assert l1 == l2 == l3
    for x, y, z in zip(a, b, c):
        assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x), bits(z))
    lr_, tabs_r = train(d, row=True)
    assert len(lr_) == 2 and lr_[1] < lr_[0] and all(bool(torch.isfinite(x).all()) for x in tabs_r)


@pytest.mark.parametrize('d', DIMS)
def test_forward_grouped_falls_back_to_forward_bit_for_bit(hip, d):
    E, P, h, t, r = tables(d)
    m = build(d, E, P)
    g = torch.Generator().manual_seed(2)
    K, B = 8, 100
    hc, tc, rc = h[:B].cuda(), t[:B].cuda(), r[:B].cuda()
    side = torch.rand(K * B, generator=g) < 0.5
    draw = torch.randint(0, N_ENT, (K * B,), generator=g)
    nh, nt = torch.where(side, draw, h[:B].repeat(K)).cuda(), torch.where(side, t[:B].repeat(K), draw).cuda()
    p1, n1 = m(hc, tc, rc, nh, nt)
    p2, n2 = m.forward_grouped(hc, tc, rc, nh, nt)
    assert torch.equal(bits(p1), bits(p2)) and torch.equal(bits(n1), bits(n2)) and tuple(n2.shape) == (K * B,)
    assert close(n2.detach().cpu(), ref.sf64(E, P, nh.cpu(), nt.cpu(), r[:B].repeat(K)))


# ---- row-sharded entity tables -------------------------------------------------------------------------------------------
WORKER = r'''
import math, os, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
rank, world, port, out_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = port
torch.cuda.set_device(0)
dist.init_process_group('gloo', rank=rank, world_size=world)
import torchkge_amd as tk
from torchkge_amd import distributed as kd
from oracle import kge_oracle as orc
n_ent, n_rel, d = 601, 7, 18
g = torch.Generator().manual_seed(3)
E = torch.rand(n_ent, 2 * d, generator=g) * 2 - 1
rel = (torch.rand(n_rel, d, generator=g) * 2 - 1) * math.pi
m = tk.RotatEModel(d, n_ent, n_rel)
m.load_state_dict({'ent_emb.weight': E, 'rel_emb.weight': rel})
m = m.cuda()
h, t, r = orc.synthetic_triples_zipf(n_ent, n_rel, 4000, 9, hubs=((200, 'head'), (80, 'tail')))
kg = tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                       rel2ix={i: i for i in range(n_rel)})
_, kg_test = kg.split_kg(sizes=(len(h) - 300, 300))
ref = tk.LinkPredictionEvaluator(m, kg_test, graph=False)
ref.evaluate(b_size=128, verbose=False)
want = [ref.rank_true_heads, ref.rank_true_tails, ref.filt_rank_true_heads, ref.filt_rank_true_tails]
kd.shard_model_(m)
ok = True
for exchange, graph, qx in (('counts', False, 'evaluate'), ('counts', True, 'evaluate'), ('counts', False, 'batch')):
    ev = tk.LinkPredictionEvaluator(m, kg_test, shard='entities', exchange=exchange, graph=graph, query_exchange=qx)
    for _ in range(2):
        ev.evaluate(b_size=128, verbose=False)
    got = [ev.rank_true_heads, ev.rank_true_tails, ev.filt_rank_true_heads, ev.filt_rank_true_tails]
    for a, b in zip(want, got):
        if not torch.equal(a, b):
            ok = False
            print('MISMATCH', rank, exchange, graph, qx, int((a != b).sum()), flush=True)
dist.barrier()
dist.destroy_process_group()
open(out_path, 'w').write('ok' if ok else 'bad')
sys.exit(0 if ok else 1)
'''


def test_row_sharded_two_ranks_on_one_gpu(tmp_path):
    """Two ranks (gloo) sharing the one GPU, each holding half of ent_emb: ranks equal the unsharded ones.  Each child
    runs under a time limit of its own."""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'root': ROOT})
    port = str(32400 + (os.getpid() % 50) * 7)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('KGE_FORCE_COLLECTIVES', None)
    procs = [subprocess.Popen(['timeout', '-k', '10', '240', sys.executable, str(script), str(r), '2', port,
                               str(tmp_path / ('r%d' % r))], env=env, cwd=ROOT) for r in range(2)]
    codes = [p.wait(timeout=300) for p in procs]
    assert codes == [0, 0]
