"""GPU tests of TorusE on the HIP engine (run with -m gpu on an MI355X): scoring_function forward / backward, the
inference API, LinkPredictionEvaluator with the reference's in-place frac (also across a graph replay), relation
prediction, the torus dissimilarities of torchkge_amd.utils, top-k inference, positive scores, an FB15k-237-shaped
graph and row-sharded entity tables on two ranks.  float64 restatements are written from the reference's formulas
(utils/dissimilarities.py:28-54), applied literally to x = a - b."""
import math
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
TYPES = ('L1', 'torus_L1', 'torus_L2', 'torus_eL2')
TAG = {'L1': 'l1', 'torus_L1': 'tl1', 'torus_L2': 'tl2', 'torus_eL2': 'tel2'}
NAMES = ['rank_true_heads', 'rank_true_tails', 'filt_rank_true_heads', 'filt_rank_true_tails']


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


def diss64(diss, x):
    if diss == 'L1':
        return x.abs().sum(-1)
    if diss == 'torus_L1':
        return 2 * torch.minimum(x.abs(), 1 - x.abs()).sum(-1)
    if diss == 'torus_L2':
        return 4 * torch.minimum(x ** 2, 1 - x ** 2).sum(-1)
    u = torch.minimum(x, 1 - x)
    return (2 * (1 - torch.cos(2 * math.pi * u))).sum(-1) / 4


def close(a, ref, tol=TOL):
    """|a - ref| <= tol * max(1, |ref|): fp32 scores of d = 32 torus terms reach ~100 (ulp 7.6e-6)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return (np.abs(a - ref) / np.maximum(1.0, np.abs(ref))).max() < tol


def scores64(diss, E, R, h, t, r, side, chunk=64):
    """(b, N) float64 -diss(h + r, c) (tail side) / -diss(c + r, t) (head side); x rounded to fp32 as the engine forms
    it when E / R are fp32."""
    out = []
    for c0 in range(0, h.shape[0], chunk):
        sl = slice(c0, c0 + chunk)
        if side == 'tail':
            x = (E[h[sl]] + R[r[sl]]).unsqueeze(1) - E.unsqueeze(0)
        else:
            x = (E.unsqueeze(0) + R[r[sl]].unsqueeze(1)) - E[t[sl]].unsqueeze(1)
        out.append(-diss64(diss, x.double()))
    return torch.cat(out)


def build(diss, E, R, n_ent, n_rel, d, dev='cuda'):
    import torchkge_amd as tk
    m = tk.TorusEModel(d, n_ent, n_rel, diss)
    m.load_state_dict({'ent_emb.weight': torch.as_tensor(E).float().clone(), 'rel_emb.weight': torch.as_tensor(R).float().clone()})
    return m.to(dev)


def load(diss, tables='table'):
    import torchkge_amd as tk
    z = np.load(os.path.join(GOLDEN, 'ref_toruse_%s.npz' % TAG[diss]))
    n_ent, n_rel, d = int(z['n_ent']), int(z['n_rel']), int(z['dim'])
    m = build(diss, z[tables + '0'], z[tables + '1'], n_ent, n_rel, d)
    heads, tails, rels = (torch.from_numpy(z[k]) for k in ('heads', 'tails', 'rels'))
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    nt = int(z['n_test'])
    _, kg_test = kg.split_kg(sizes=(len(heads) - nt, nt))
    return z, m, kg, kg_test


def first_batch(z, kg_test):
    B = int(z['b_size'])
    return kg_test.head_idx[:B].cuda(), kg_test.tail_idx[:B].cuda(), kg_test.relations[:B].cuda()


@pytest.mark.parametrize('diss', TYPES)
def test_scoring_function_and_forward_vs_reference(hip, diss):
    z, m, kg, kg_test = load(diss)
    h, t, r = first_batch(z, kg_test)
    raw = m.ent_emb.weight.detach().clone()
    s = m.scoring_function(h, t, r)
    assert m.normalized is False and torch.equal(m.ent_emb.weight.detach(), raw)     # the tables are not changed
    assert close(s.detach().cpu(), z['sf'])
    pos, neg = m(h, t, r, torch.from_numpy(z['neg_heads']).cuda(), torch.from_numpy(z['neg_tails']).cuda())
    assert close(pos.detach().cpu(), z['fwd_pos']) and close(neg.detach().cpu(), z['fwd_neg'])


@pytest.mark.parametrize('diss', TYPES)
def test_backward_vs_reference_and_repeatable(hip, diss):
    grads = []
    for _ in range(2):
        z, m, kg, kg_test = load(diss)
        h, t, r = first_batch(z, kg_test)
        (m.scoring_function(h, t, r) * torch.from_numpy(z['grad_out']).cuda()).sum().backward()
        gE, gR = m.ent_emb.weight.grad.cpu(), m.rel_emb.weight.grad.cpu()
        assert np.abs(gE.numpy() - z['grad_ent']).max() < TOL * max(1.0, np.abs(z['grad_ent']).max())
        assert np.abs(gR.numpy() - z['grad_rel']).max() < TOL * max(1.0, np.abs(z['grad_rel']).max())
        grads.append((gE, gR))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


@pytest.mark.parametrize('diss', TYPES)
def test_backward_large_batch_vs_float64_autograd(hip, diss):
    n_ent, n_rel, d, B = 500, 9, 40, 5000
    g = torch.Generator().manual_seed(11)
    E = torch.rand(n_ent, d, generator=g) * 5 - 2.5
    R = torch.rand(n_rel, d, generator=g) * 5 - 2.5
    h, t, r = (torch.randint(0, n, (B,), generator=g) for n in (n_ent, n_ent, n_rel))
    go = torch.randn(B, generator=g)
    E64, R64 = E.double().requires_grad_(), R.double().requires_grad_()
    f = lambda x: x - torch.trunc(x).detach()      # noqa: E731 (frac with the identity gradient, as .data.frac_())
    # x rounded as the kernel forms it; the gradient's branches are taken on those fp32 values
    xf = ((E - E.trunc())[h] + (R - R.trunc())[r]) - (E - E.trunc())[t]
    x64 = (f(E64)[h] + f(R64)[r]) - f(E64)[t]
    x64 = x64 + (xf.double() - x64).detach()
    (-diss64(diss, x64) * go.double()).sum().backward()
    m = build(diss, E, R, n_ent, n_rel, d)
    s = m.scoring_function(h.cuda(), t.cuda(), r.cuda())
    assert close(s.detach().cpu(), -diss64(diss, xf.double()))
    (s * go.cuda()).sum().backward()
    for got, ref in ((m.ent_emb.weight.grad.cpu(), E64.grad), (m.rel_emb.weight.grad.cpu(), R64.grad)):
        assert (got.double() - ref).abs().max().item() < 1e-4 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize('diss', TYPES)
def test_inference_api_vs_reference(hip, diss):
    from torchkge_amd.models import EntityCandidates
    z, m, kg, kg_test = load(diss, 'after_table')
    h, t, r = first_batch(z, kg_test)
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=True)
    assert isinstance(cand, EntityCandidates) and tuple(cand.shape) == (h.shape[0], m.n_ent, m.emb_dim)
    for fn in (m.inference_scoring_function, m.lp_scoring_function):
        assert close(fn(h_e, cand, r_e).cpu(), z['s_tail'])
        assert close(fn(cand, t_e, r_e).cpu(), z['s_head'])
    # a real (b, N, d) tensor, as a user may pass it: the generic batched kernel
    C = m.ent_emb.weight.data.view(1, m.n_ent, m.emb_dim).expand(h.shape[0], m.n_ent, m.emb_dim).contiguous()
    assert close(m.inference_scoring_function(h_e, C, r_e).cpu(), z['s_tail'])
    # inference_prepare_candidates frac's un-normalized tables in place (translation.py:752-753)
    z2, m2, _, _ = load(diss)
    m2.scoring_function(h, t, r)
    m2.inference_prepare_candidates(h, t, r)
    assert m2.normalized is True
    assert np.array_equal(m2.ent_emb.weight.detach().cpu().numpy(), z['after_table0'])
    assert np.array_equal(m2.rel_emb.weight.detach().cpu().numpy(), z['after_table1'])


def rank_bounds(diss, z, kg, kg_test):
    E, R = (torch.from_numpy(z['after_table%d' % k]) for k in (0, 1))
    h, t, r = kg_test.head_idx, kg_test.tail_idx, kg_test.relations
    dh, dt, _ = orc.build_filter_dicts(kg.head_idx, kg.tail_idx, kg.relations)
    st, sh = scores64(diss, E, R, h, t, r, 'tail'), scores64(diss, E, R, h, t, r, 'head')
    return {'rank_true_tails': orc._tie_interval(st, t, TIE), 'rank_true_heads': orc._tie_interval(sh, h, TIE),
            'filt_rank_true_tails': orc._tie_interval(orc.filter_scores_vec(st, dt, h, r, t), t, TIE),
            'filt_rank_true_heads': orc._tie_interval(orc.filter_scores_vec(sh, dh, t, r, h), h, TIE)}


@pytest.mark.parametrize('diss', TYPES)
def test_link_prediction_evaluator_vs_reference_and_in_place_frac(hip, diss):
    import torchkge_amd as tk
    z, m, kg, kg_test = load(diss)
    B = int(z['b_size'])
    h, t, r = first_batch(z, kg_test)
    m.scoring_function(h, t, r)                  # the fixture's sequence: tables not normalized when evaluate() starts
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=B, verbose=False)
    after = [torch.from_numpy(z['after_table%d' % k]) for k in (0, 1)]
    assert m.normalized is True
    assert torch.equal(m.ent_emb.weight.data.cpu(), after[0]) and torch.equal(m.rel_emb.weight.data.cpu(), after[1])
    bounds = rank_bounds(diss, z, kg, kg_test)
    for nm in NAMES:
        got, ref = getattr(ev, nm), torch.from_numpy(z[nm])
        lo, hi = bounds[nm]
        assert bool(((got == ref) | ((got >= lo) & (got <= hi))).all()), nm
    assert np.abs(np.array(ev.mrr()) - z['mrr']).max() < TOL
    assert np.abs(np.array(ev.hit_at_k(10)) - z['hit10']).max() < TOL
    want = [getattr(ev, nm).clone() for nm in NAMES]

    def same(e, b_size=B, n=1):
        for _ in range(n):
            e.evaluate(b_size=b_size, verbose=False)
            for nm, w in zip(NAMES, want):
                assert torch.equal(getattr(e, nm), w), nm
    same(tk.LinkPredictionEvaluator(m, kg_test, fused=False), b_size=7)
    same(tk.LinkPredictionEvaluator(m, kg_test, both_sides=False), b_size=5)
    # the captured graph: warm-up, capture, replays -- then the RAW tables written back in place (same addresses) and a
    # scoring_function call: the next evaluate() is a steady-state replay and must still frac first (lp_eval_prepare)
    evg = tk.LinkPredictionEvaluator(m, kg_test, graph=True)
    same(evg, n=3)
    raw = [torch.from_numpy(z['table%d' % k]).cuda() for k in (0, 1)]
    ptrs = (m.ent_emb.weight.data_ptr(), m.rel_emb.weight.data_ptr())
    with torch.no_grad():
        m.ent_emb.weight.copy_(raw[0])
        m.rel_emb.weight.copy_(raw[1])
    m.scoring_function(h, t, r)
    assert m.normalized is False
    same(evg)
    assert (m.ent_emb.weight.data_ptr(), m.rel_emb.weight.data_ptr()) == ptrs
    assert torch.equal(m.ent_emb.weight.data.cpu(), after[0]) and torch.equal(m.rel_emb.weight.data.cpu(), after[1])


@pytest.mark.parametrize('diss', TYPES)
def test_relation_prediction_vs_float64(hip, diss):
    """The reference raises AttributeError here (translation.py:765); the engine scores -diss(h + r_c, t)."""
    import torchkge_amd as tk
    z, m, kg, kg_test = load(diss, 'after_table')
    h, t, r = first_batch(z, kg_test)
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=False)
    assert tuple(cand.shape) == (h.shape[0], m.n_rel, m.emb_dim)
    s = m.inference_scoring_function(h_e, t_e, cand).cpu()
    E, R = (torch.from_numpy(z['after_table%d' % k]).double() for k in (0, 1))
    x = (E[h.cpu()].unsqueeze(1) + R.unsqueeze(0)) - E[t.cpu()].unsqueeze(1)
    assert close(s, -diss64(diss, x), 2e-5)
    ev = tk.RelationPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=int(z['b_size']), verbose=False)
    assert ev.rank_true_rels.shape[0] == kg_test.n_facts and int(ev.rank_true_rels.min()) >= 1


@pytest.mark.parametrize('fn_name,diss', [('l1_torus_dissimilarity', 'torus_L1'), ('l2_torus_dissimilarity', 'torus_L2'),
                                          ('el2_torus_dissimilarity', 'torus_eL2')])
def test_utils_dissimilarities_and_gradients_vs_float64(hip, fn_name, diss):
    from torchkge_amd import utils
    fn = getattr(utils, fn_name)
    g = torch.Generator().manual_seed(5)
    a = (torch.rand(37, 3, 24, generator=g) * 4 - 2)
    b = (torch.rand(37, 1, 24, generator=g) * 2 - 1)
    go = torch.randn(37, 3, generator=g)
    A, Bv = a.cuda().requires_grad_(), b.cuda().requires_grad_()
    D = fn(A, Bv)
    a64, b64 = a.double().requires_grad_(), b.double().requires_grad_()
    D64 = diss64(diss, a64 - b64)
    assert close(D.detach().cpu(), D64.detach())
    (D * go.cuda()).sum().backward()
    (D64 * go.double()).sum().backward()
    assert (A.grad.cpu().double() - a64.grad).abs().max().item() < 1e-4
    assert (Bv.grad.cpu().double() - b64.grad).abs().max().item() < 1e-4 * max(1.0, float(b64.grad.abs().max()))
    with torch.no_grad():
        assert torch.equal(fn(A, Bv), D.detach())


@pytest.mark.parametrize('diss', TYPES)
def test_entity_inference_topk_equals_materialised(hip, diss):
    import torchkge_amd as tk
    z, m, kg, kg_test = load(diss, 'after_table')
    e, r = kg.head_idx[:200], kg.relations[:200]
    for missing, side in (('tails', 'tail'), ('heads', 'head')):
        a = tk.EntityInference(m, e, r, top_k=9, missing=missing, dictionary=None)
        a.evaluate(b_size=64, verbose=False)
        S = m.lp_problem(e.cuda(), e.cuda(), r.cuda(), side).scores().cpu()
        v, i = S.sort(dim=1, descending=True)
        assert torch.equal(a.scores.cpu(), v[:, :9])
        assert bool((S.gather(1, a.predictions.cpu()) == a.scores.cpu()).all())


@pytest.mark.parametrize('diss', ['torus_L1', 'torus_L2'])
def test_mostly_negative_terms_positive_scores_ranked(hip, diss):
    """Tables near +-0.9: |(h + r) - c| > 1 for most elements, most torus terms are negative and most scores positive;
    the ranks are still those of the materialised scores (nothing assumes s <= 0)."""
    import torchkge_amd as tk
    n_ent, n_rel, d = 400, 5, 16
    g = torch.Generator().manual_seed(2)
    sgn = torch.randint(0, 2, (n_ent, d), generator=g).float() * 2 - 1
    E = sgn * (0.8 + 0.19 * torch.rand(n_ent, d, generator=g))
    R = 0.8 + 0.19 * torch.rand(n_rel, d, generator=g)
    m = build(diss, E, R, n_ent, n_rel, d)
    h, t, r = orc.synthetic_triples_zipf(n_ent, n_rel, 3000, seed=4)
    kg = tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                           rel2ix={i: i for i in range(n_rel)})
    _, kg_test = kg.split_kg(sizes=(2800, 200))
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=64, verbose=False)
    hh, tt, rr = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    for side, nm, tr in (('tail', 'rank_true_tails', tt), ('head', 'rank_true_heads', hh)):
        S = m.lp_problem(hh, tt, rr, side).scores()
        assert (S > 0).float().mean().item() > 0.5
        s_true = S.gather(1, tr.view(-1, 1))
        assert torch.equal(getattr(ev, nm).cuda(), (S >= s_true).sum(1))


def test_fb15k237_shape_ranks_pair_scores_and_memory(hip):
    import torchkge_amd as tk
    from torchkge_amd import _hip
    n_ent, n_rel, d, n_test = 14541, 237, 200, 20466
    heads, tails, rels = orc.synthetic_triples_zipf(n_ent, n_rel, 310116, seed=237)
    g = torch.Generator().manual_seed(5)
    E = torch.rand(n_ent, d, generator=g) * 2 - 1
    R = torch.rand(n_rel, d, generator=g) * 2 - 1
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    _, kg_test = kg.split_kg(sizes=(len(heads) - n_test, n_test))
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    Ed, Rd = E.cuda(), R.cuda()
    for diss in TYPES:
        m = build(diss, E, R, n_ent, n_rel, d)
        ev = tk.LinkPredictionEvaluator(m, kg_test)
        ev.evaluate(b_size=2048, verbose=False)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ev.evaluate(b_size=2048, verbose=False)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base < (1 << 30), diss
        # raw ranks of a sample of the facts inside the tie interval of a float64 restatement on the GPU
        sl = slice(0, 512)
        for side, nm, tr in (('tail', 'rank_true_tails', t), ('head', 'rank_true_heads', h)):
            S = scores64(diss, Ed, Rd, h[sl], t[sl], r[sl], side, chunk=16)
            # (200-term fp32 sums of magnitude ~100: the tie band is relative to the largest score)
            lo, hi = orc._tie_interval(S, tr[sl], TIE * max(1.0, float(S.abs().max())))
            got = getattr(ev, nm).cuda()[sl]
            assert bool(((got >= lo) & (got <= hi)).all()), (diss, nm)
        # the pair kernel scores sampled pairs with the bits of the tile kernel
        prob = m.lp_problem(h[:300], t[:300], r[:300], 'tail')
        S = prob.scores()
        qi = torch.randint(0, 300, (4096,), generator=g).cuda()
        ci = torch.randint(0, n_ent, (4096,), generator=g).cuda()
        assert torch.equal(prob.pair_scores(ci, qi), S[qi, ci]), diss
        assert int(prob.desc.mode) == m._direct_mode() and int(prob.desc.mode) not in _hip.LP_MFMA_MODES
        del m, ev, prob, S


WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
rank, world, port, diss, out_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = port
torch.cuda.set_device(0)
dist.init_process_group('gloo', rank=rank, world_size=world)
import torchkge_amd as tk
from torchkge_amd import distributed as kd
from oracle import kge_oracle as orc
n_ent, n_rel, d = 3001, 11, 48
g = torch.Generator().manual_seed(3)
E = torch.rand(n_ent, d, generator=g) * 2 - 1
rel = torch.rand(n_rel, d, generator=g) * 2 - 1
m = tk.TorusEModel(d, n_ent, n_rel, diss)
m.load_state_dict({'ent_emb.weight': E, 'rel_emb.weight': rel})
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
            print('MISMATCH', rank, diss, exchange, graph, qx, int((a != b).sum()), flush=True)
dist.barrier()
dist.destroy_process_group()
open(out_path, 'w').write('ok' if ok else 'bad')
sys.exit(0 if ok else 1)
'''


@pytest.mark.parametrize('diss', ['torus_L2', 'torus_eL2'])
def test_row_sharded_two_ranks_on_one_gpu(diss, tmp_path):
    """Two ranks (gloo) sharing the one GPU, each holding half of ent_emb: ranks equal the unsharded ones."""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'root': ROOT})
    port = str(31900 + (os.getpid() % 50) * 7 + TYPES.index(diss))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('KGE_FORCE_COLLECTIVES', None)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', port, diss, str(tmp_path / ('r%d' % r))],
                              env=env, cwd=ROOT) for r in range(2)]
    codes = [p.wait(timeout=600) for p in procs]
    assert codes == [0, 0]
