"""GPU tests of TransR on the HIP engine (run with -m gpu on an MI355X): scoring_function forward / backward, the
projected-norm and query-transform kernels against float64 and for order independence, the inference API, both
evaluators and top-k inference against the reference fixture, an FB15k-237-shaped graph on the expanded and on the exact
relation-grouped path, and row-sharded entity tables on two ranks.  The float64 restatements are the formulas of
tests/test_transr_host.py, which pins them to the fixture on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.helpers import ROOT, GOLDEN, raw
from tests.test_transr_host import scoring64, side_scores64, relation_scores64

pytestmark = pytest.mark.gpu

TOL = 1e-5
TIE = 2e-5
NAMES = ['rank_true_heads', 'rank_true_tails', 'filt_rank_true_heads', 'filt_rank_true_tails']


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


def close(a, ref, tol=TOL):
    """|a - ref| <= tol * max(1, max |ref|): the project's relative form for scores above 1 in magnitude."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, bound = np.abs(a - ref).max(), tol * max(1.0, np.abs(ref).max())
    print('max err %.3e (bound %.3e)' % (err, bound))
    return err <= bound


def build(E, R, P, de, dr, dev='cuda'):
    import torchkge_amd as tk
    m = tk.TransRModel(de, dr, E.shape[0], R.shape[0])
    m.load_state_dict({'ent_emb.weight': torch.as_tensor(E), 'rel_emb.weight': torch.as_tensor(R),
                       'proj_mat.weight': torch.as_tensor(P)})
    return m.to(dev)


def load():
    import torchkge_amd as tk
    z = np.load(os.path.join(GOLDEN, 'ref_transr.npz'))
    n_ent, n_rel, de, dr = int(z['n_ent']), int(z['n_rel']), int(z['dim']), int(z['dim_rel'])
    m = build(z['table0'], z['table1'], z['table2'], de, dr)
    heads, tails, rels = (torch.from_numpy(z[k]) for k in ('heads', 'tails', 'rels'))
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    nt = int(z['n_test'])
    _, kg_test = kg.split_kg(sizes=(len(heads) - nt, nt))
    return z, m, kg, kg_test


def first_batch(z, kg_test):
    B = int(z['b_size'])
    return kg_test.head_idx[:B].cuda(), kg_test.tail_idx[:B].cuda(), kg_test.relations[:B].cuda()


def random_tables(n_ent, n_rel, de, dr, seed, scale=1.0):
    """Tables with the fixture's norms whatever the sizes: the fixture's standard deviations (0.25, 0.2, 0.15 at
    (32, 24)) scaled by sqrt(32 / d_e) for ent_emb and sqrt(24 / d_r) for rel_emb and proj_mat, so that ||e||^2 = d_e s_E^2,
    ||r||^2 = d_r s_R^2 and ||M e||^2 = d_r s_M^2 ||e||^2 keep their magnitude."""
    g = torch.Generator().manual_seed(seed)
    E = torch.randn(n_ent, de, generator=g) * (0.25 * (32.0 / de) ** 0.5 * scale)
    R = torch.randn(n_rel, dr, generator=g) * (0.2 * (24.0 / dr) ** 0.5 * scale)
    P = torch.randn(n_rel, dr * de, generator=g) * (0.15 * (24.0 / dr) ** 0.5 * scale)
    return E, R, P


def test_scoring_function_and_forward_vs_reference(hip):
    z, m, kg, kg_test = load()
    h, t, r = first_batch(z, kg_test)
    with torch.no_grad():
        assert close(m.scoring_function(h, t, r).cpu(), z['sf'])
        pos, neg = m(h, t, r, torch.from_numpy(z['neg_heads']).cuda(), torch.from_numpy(z['neg_tails']).cuda())
    assert close(pos.cpu(), z['fwd_pos']) and close(neg.cpu(), z['fwd_neg'])


def _backward_case(hip, n_ent, n_rel, de, dr, B, seed):
    E, R, P = random_tables(n_ent, n_rel, de, dr, seed)
    g = torch.Generator().manual_seed(seed + 1)
    h = torch.randint(0, n_ent, (B,), generator=g)
    t = torch.randint(0, n_ent, (B,), generator=g)
    r = torch.randint(0, n_rel, (B,), generator=g)
    r[torch.rand(B, generator=g) < 0.75] = 1            # one relation holds three quarters of the triples
    go = torch.randn(B, generator=g)
    E64, R64, P64 = (x.double().requires_grad_(True) for x in (E, R, P))
    (scoring64(E64, R64, P64.view(n_rel, dr, de), h, t, r) * go.double()).sum().backward()
    runs = []
    for _ in range(2):
        m = build(E, R, P, de, dr)
        (m.scoring_function(h.cuda(), t.cuda(), r.cuda()) * go.cuda()).sum().backward()
        runs.append([p.grad.detach().cpu() for p in (m.ent_emb.weight, m.rel_emb.weight, m.proj_mat.weight)])
    for got, want, name in zip(runs[0], (E64.grad, R64.grad, P64.grad), ('ent_emb', 'rel_emb', 'proj_mat')):
        err = (got.double() - want).abs().max().item()
        bound = 1e-4 * max(1.0, want.abs().max().item())
        print(name, 'B', B, 'max err %.3e (bound %.3e)' % (err, bound))
        assert err <= bound, name
    assert torch.equal(runs[0][2], runs[1][2])          # proj_mat.grad: the same bits on every run


def test_backward_vs_reference_fixture(hip):
    z, m, kg, kg_test = load()
    h, t, r = first_batch(z, kg_test)
    (m.scoring_function(h, t, r) * torch.from_numpy(z['grad_out']).cuda()).sum().backward()
    for p, name in ((m.ent_emb.weight, 'grad_ent'), (m.rel_emb.weight, 'grad_rel'), (m.proj_mat.weight, 'grad_proj')):
        assert close(p.grad.cpu(), z[name], 1e-4), name


def test_backward_small_batch_vs_float64_autograd(hip):
    _backward_case(hip, 200, 6, 17, 9, 300, seed=11)


def test_backward_large_batch_vs_float64_autograd(hip):
    assert 5000 > hip.BWD_SORTED_MIN_BATCH
    _backward_case(hip, 500, 6, 40, 24, 5000, seed=12)


DIMS = [(1, 1), (8, 5), (17, 32), (32, 24), (100, 100), (200, 100), (128, 256), (512, 512)]


@pytest.mark.parametrize('de,dr', DIMS)
def test_projected_norms_vs_float64_and_order_independence(hip, de, dr):
    n_rel, n = 5, 333                                   # n is no multiple of the 128-row tile
    E, R, P = random_tables(n, n_rel, de, dr, seed=de * 1000 + dr)
    Xd, Rd, Pd = E.cuda(), R.cuda(), P.cuda()
    M64 = Pd.double().view(n_rel, dr, de)
    for bias in (None, Rd):
        out = hip.transr_proj_sqnorm(Pd, Xd, de, dr, b=bias)
        p = torch.einsum('rck,nk->rnc', M64, Xd.double())
        if bias is not None:
            p = p + Rd.double().unsqueeze(1)
        assert close(out.cpu(), (p * p).sum(2).cpu()), (de, dr, bias is not None)
        # the same rows in another order, and in another batch size: bit-identical per (relation, row)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).cuda()
        assert torch.equal(hip.transr_proj_sqnorm(Pd, Xd[perm].contiguous(), de, dr, b=bias), out[:, perm])
        assert torch.equal(hip.transr_proj_sqnorm(Pd, Xd[40:141].contiguous(), de, dr, b=bias), out[:, 40:141])
        # strided output, one relation list entry, rows by (row, relation)
        assert torch.equal(hip.transr_proj_sqnorm(Pd, Xd, de, dr, b=bias, by_row=True), out.t())
        sub = hip.transr_proj_sqnorm(Pd, Xd, de, dr, b=bias, rels=torch.tensor([3, 1]).cuda())
        assert torch.equal(sub[3], out[3]) and torch.equal(sub[1], out[1]) and not sub[0].any()


@pytest.mark.parametrize('de,dr', DIMS)
def test_query_transform_vs_float64_and_order_independence(hip, de, dr):
    n_ent, n_rel, B = 150, 5, 400
    E, R, P = random_tables(n_ent, n_rel, de, dr, seed=de * 1000 + dr + 7)
    g = torch.Generator().manual_seed(3)
    h = torch.randint(0, n_ent, (B,), generator=g)
    t = torch.randint(0, n_ent, (B,), generator=g)
    r = torch.randint(0, n_rel, (B,), generator=g)
    r[torch.rand(B, generator=g) < 0.6] = 2             # one relation owns far more than 64 rows
    Ed, Rd, Pd, hd, td, rd = (x.cuda() for x in (E, R, P, h, t, r))
    Q, U = hip.transr_query(hip.SIDE_BOTH, Ed, Pd, Rd, de, dr, hd, td, rd)
    M64 = Pd.double().view(n_rel, dr, de)[rd]
    qt = torch.einsum('bck,bk->bc', M64, Ed.double()[hd]) + Rd.double()[rd]
    qh = torch.einsum('bck,bk->bc', M64, Ed.double()[td]) - Rd.double()[rd]
    q64 = torch.cat([qt, qh])
    u64 = torch.einsum('bck,bc->bk', torch.cat([M64, M64]), q64)
    assert close(Q.cpu(), q64.cpu()) and close(U.cpu(), u64.cpu())
    qn = hip.row_sqnorm(Q)
    assert close(qn.cpu(), (q64 * q64).sum(1).cpu())
    # rows depend on (entity row, relation, side) only: unsorted, one side at a time, a permuted and a shorter batch,
    # gathered rows instead of indices
    Q2, U2 = hip.transr_query(hip.SIDE_BOTH, Ed, Pd, Rd, de, dr, hd, td, rd, sort=False)
    assert torch.equal(Q2, Q) and torch.equal(U2, U)
    Qt, Ut = hip.transr_query(hip.SIDE_TAIL, Ed, Pd, Rd, de, dr, hd, td, rd)
    Qh, Uh = hip.transr_query(hip.SIDE_HEAD, Ed, Pd, Rd, de, dr, hd, td, rd)
    assert torch.equal(torch.cat([Qt, Qh]), Q) and torch.equal(torch.cat([Ut, Uh]), U)
    perm = torch.randperm(B, generator=g).cuda()
    Qp, Up = hip.transr_query(hip.SIDE_TAIL, Ed, Pd, Rd, de, dr, hd[perm], td[perm], rd[perm])
    assert torch.equal(Qp, Qt[perm]) and torch.equal(Up, Ut[perm])
    assert torch.equal(hip.row_sqnorm(Qp), qn[:B][perm])
    Qs, Us = hip.transr_query(hip.SIDE_HEAD, Ed, Pd, Rd, de, dr, hd[:77], td[:77], rd[:77])
    assert torch.equal(Qs, Qh[:77]) and torch.equal(Us, Uh[:77])
    rows = torch.cat([Ed[hd], Ed[td]]).contiguous()
    Qg, Ug = hip.transr_query(hip.SIDE_BOTH, rows, Pd, Rd, de, dr, None, None, rd)
    assert torch.equal(Qg, Q) and torch.equal(Ug, U)
    _, U3 = hip.transr_query(hip.SIDE_TAIL, None, Pd, None, de, dr, None, None, rd, Q=Qt)
    assert torch.equal(U3, Ut)


@pytest.mark.parametrize('dr,de', [(1, 1), (24, 24), (64, 64), (65, 64), (70, 130)])
def test_rel_grad_reduction_tiles_and_segments(hip, dr, de):
    """kge_transr_rel_grad / kge_rescal_rel_grad called directly: one 64 x 64 tile, an exact tile, one column past a
    tile, 2 x 3 ragged tiles; per relation an empty, a single-triple, a 16, 17, 33 and 133 triple segment (the reduction
    stages 16 triples per step) of shuffled triples.  Every element is an n-term fp32 fmaf chain: its error against
    float64 is at most n 2^-24 (|U|^T |V|), asserted doubled.  The square shapes give the same bits through both exports."""
    lib = hip.load_library()
    n_rel, lens = 6, [16, 0, 133, 1, 33, 17]
    B = sum(lens)
    g = torch.Generator().manual_seed(dr * 1000 + de)
    r = torch.repeat_interleave(torch.arange(n_rel), torch.tensor(lens))[torch.randperm(B, generator=g)]
    U = torch.randn(B, dr + 3, generator=g).cuda()[:, :dr]      # row stride width + 3
    V = torch.randn(B, de + 3, generator=g).cuda()[:, :de]
    rd = r.cuda()
    perm = hip._key_perm(rd, None, n_rel)
    assert not torch.equal(perm.cpu(), torch.arange(B))

    def run(name):
        gM = torch.full((n_rel, dr * de), float('nan'), device='cuda')
        if name == 'kge_transr_rel_grad':
            rc = raw(lib, name, U, U.stride(0), V, V.stride(0), dr, de, rd, perm, B, n_rel, gM, gM.stride(0))
        else:
            rc = raw(lib, name, U, V, U.stride(0), de, rd, perm, B, n_rel, gM, gM.stride(0))
        assert rc == 0, name
        return gM

    gM = run('kge_transr_rel_grad')
    assert torch.equal(run('kge_transr_rel_grad'), gM)
    if dr == de:
        assert V.stride(0) == U.stride(0) and torch.equal(run('kge_rescal_rel_grad'), gM)
    got = gM.cpu().double().view(n_rel, dr, de)
    U64, V64 = U.cpu().double(), V.cpu().double()
    for rho, n in enumerate(lens):
        sel = r == rho
        assert int(sel.sum()) == n
        ref = U64[sel].t() @ V64[sel]
        bound = n * 2.0 ** -23 * (U64[sel].abs().t() @ V64[sel].abs())
        err = (got[rho] - ref).abs()
        print('relation %d n %d max err %.3e (max bound %.3e)' % (rho, n, err.max().item(), bound.max().item()))
        assert bool((err <= bound).all()), (rho, n)
        if n == 0:
            assert not gM[rho].view(torch.int32).any()


def test_dimension_limits(hip):
    E, R, P = random_tables(4, 2, 513, 3, seed=1)
    with pytest.raises(RuntimeError, match=r'code -3'):
        hip.transr_proj_sqnorm(P.cuda(), E.cuda(), 513, 3)


def test_inference_api_vs_reference(hip):
    from torchkge_amd.models.interfaces import EntityCandidates, RelationProjections
    z, m, kg, kg_test = load()
    h, t, r = first_batch(z, kg_test)
    with torch.no_grad():
        ph, pt, rr, cand = m.inference_prepare_candidates(h, t, r, entities=True)
        assert isinstance(cand, EntityCandidates) and cand.shape == (h.shape[0], m.n_ent, m.rel_emb_dim)
        assert tuple(ph.shape) == (h.shape[0], m.rel_emb_dim) and m.evaluated_projections is True
        assert close(m.inference_scoring_function(ph, cand, rr).cpu(), z['s_tail'])
        assert close(m.inference_scoring_function(cand, pt, rr).cpu(), z['s_head'])
        assert m.lp_last_path == 'expand'
        ph, pt, rr, cand = m.inference_prepare_candidates(h, t, r, entities=False)
        assert isinstance(ph, RelationProjections) and isinstance(pt, RelationProjections)
        fused = m.inference_scoring_function(ph, pt, cand)
        assert close(fused.cpu(), z['s_rel'])
        # a relation table that is not the model's own: the materialised composition
        other = cand.clone()
        assert close(m.inference_scoring_function(ph, pt, other).cpu(), z['s_rel'])
        E64, R64, P64 = (torch.from_numpy(z['table%d' % k]).double() for k in range(3))
        mat = ph.materialize().cpu()
        want = torch.einsum('rck,bk->brc', P64.view(m.n_rel, m.rel_emb_dim, m.ent_emb_dim), E64[h.cpu()])
        assert close(mat, want)
    assert sorted(m.state_dict().keys()) == ['ent_emb.weight', 'proj_mat.weight', 'rel_emb.weight']


def test_link_prediction_evaluator_equals_reference_ranks(hip):
    import torchkge_amd as tk
    z, m, kg, kg_test = load()
    B = int(z['b_size'])
    ev = tk.LinkPredictionEvaluator(m, kg_test, graph=False)
    ev.evaluate(b_size=B, verbose=False)
    assert m.lp_last_path == 'expand' and not ev._last_redo
    for nm in NAMES:
        diff = (getattr(ev, nm) != torch.from_numpy(z[nm])).sum().item()
        print(nm, 'ranks differing from the fixture:', diff)
        assert torch.equal(getattr(ev, nm), torch.from_numpy(z[nm])), nm
    assert np.abs(np.array(ev.mrr()) - z['mrr']).max() < 1e-6
    assert np.abs(np.array(ev.hit_at_k(10)) - z['hit10']).max() < 1e-6
    assert np.abs(np.array(ev.mean_rank()) - z['mean_rank']).max() < 1e-6 * max(1.0, float(np.max(z['mean_rank'])))
    # the captured graph: a first evaluation and replays
    evg = tk.LinkPredictionEvaluator(m, kg_test, graph=True)
    for i in range(3):
        evg.evaluate(b_size=B, verbose=False)
        for nm in NAMES:
            assert torch.equal(getattr(evg, nm), torch.from_numpy(z[nm])), (nm, i)
    # other compositions of the same problems
    for kw, b in (({'fused': False}, 7), ({'both_sides': False}, 5)):
        e2 = tk.LinkPredictionEvaluator(m, kg_test, **kw)
        e2.evaluate(b_size=b, verbose=False)
        for nm in NAMES:
            assert torch.equal(getattr(e2, nm), torch.from_numpy(z[nm])), (nm, kw)
    # the exact relation-grouped path gives the same ranks
    m.l2_mode = 'direct'
    e3 = tk.LinkPredictionEvaluator(m, kg_test, graph=False)
    e3.evaluate(b_size=B, verbose=False)
    assert m.lp_last_path == 'exact'
    for nm in NAMES:
        assert torch.equal(getattr(e3, nm), torch.from_numpy(z[nm])), nm


def test_relation_prediction_evaluator_equals_reference_ranks(hip):
    import torchkge_amd as tk
    z, m, kg, kg_test = load()
    for directed, tag in ((True, 'rel_dir'), (False, 'rel_undir')):
        ev = tk.RelationPredictionEvaluator(m, kg_test, directed=directed)
        ev.evaluate(b_size=int(z['b_size']), verbose=False)
        assert torch.equal(ev.rank_true_rels, torch.from_numpy(z[tag + '_rank'])), tag
        assert torch.equal(ev.filt_rank_true_rels, torch.from_numpy(z[tag + '_frank'])), tag
        assert abs(ev.mrr()[0] - float(z[tag + '_mrr'][0])) < 1e-6


def test_entity_inference_topk_equals_materialised(hip):
    import torchkge_amd as tk
    z, m, kg, kg_test = load()
    e, r = kg.head_idx[:200], kg.relations[:200]
    for missing, side in (('tails', 'tail'), ('heads', 'head')):
        a = tk.EntityInference(m, e, r, top_k=9, missing=missing, dictionary=None)
        a.evaluate(b_size=64, verbose=False)
        S = m.lp_problem(e.cuda(), e.cuda(), r.cuda(), side).scores().cpu()
        v, i = S.sort(dim=1, descending=True)
        assert torch.equal(a.scores.cpu(), v[:, :9])
        assert bool((S.gather(1, a.predictions.cpu()) == a.scores.cpu()).all())


FB = dict(n_ent=14541, n_rel=237, de=200, dr=100, n_test=20466)


def _fb15k(scale):
    import torchkge_amd as tk
    n_ent, n_rel, de, dr, n_test = (FB[k] for k in ('n_ent', 'n_rel', 'de', 'dr', 'n_test'))
    heads, tails, rels = orc.synthetic_triples_zipf(n_ent, n_rel, 310116, seed=237)
    E, R, P = random_tables(n_ent, n_rel, de, dr, seed=17, scale=scale)
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    _, kg_test = kg.split_kg(sizes=(len(heads) - n_test, n_test))
    return build(E, R, P, de, dr), kg_test


def _side64(m, h, t, r, side, chunk=16):
    E, R = m.ent_emb.weight.data.double(), m.rel_emb.weight.data.double()
    M = m.proj_mat.weight.data.double().view(m.n_rel, m.rel_emb_dim, m.ent_emb_dim)
    out = []
    for c0 in range(0, h.shape[0], chunk):
        sl = slice(c0, c0 + chunk)
        out.append(side_scores64(E, R, M, h[sl], t[sl], r[sl])[0 if side == 'tail' else 1])
    return torch.cat(out)


def _check_sample(m, ev, kg_test):
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    sl = slice(0, 512)
    for side, nm, tr in (('tail', 'rank_true_tails', t), ('head', 'rank_true_heads', h)):
        S = _side64(m, h[sl], t[sl], r[sl], side)
        band = TIE * max(1.0, float(S.abs().max()))
        lo, hi = orc._tie_interval(S, tr[sl], band)
        got = getattr(ev, nm).cuda()[sl]
        print(nm, 'max |S| %.3f' % float(S.abs().max()), 'outside the interval:', int(((got < lo) | (got > hi)).sum()))
        assert bool(((got >= lo) & (got <= hi)).all()), nm       # all 512 facts, none left out
    return h, t, r


def test_fb15k237_shape_expanded_path_ranks_pair_scores_and_memory(hip):
    """Tables with the fixture's norms (random_tables): max ||q||^2 + max Z stays inside L2_EXPAND_LIMIT, the expansion
    is taken (asserted), and the second evaluate allocates far less than a quarter of the (n_rel, n_ent, d_r) cache."""
    import torchkge_amd as tk
    m, kg_test = _fb15k(1.0)
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=2048, verbose=False)
    assert m.lp_last_path == 'expand' and not ev._last_redo
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ev.evaluate(b_size=2048, verbose=False)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    cache = FB['n_rel'] * FB['n_ent'] * FB['dr'] * 4
    print('peak extra bytes of the second evaluate: %d (cache %d)' % (extra, cache))
    assert extra < cache // 4
    assert m.lp_last_path == 'expand' and not ev._last_redo
    h, t, r = _check_sample(m, ev, kg_test)
    with m.lp_session():
        prob = m.lp_problem(h[:300], t[:300], r[:300], 'tail')
        assert int(prob.desc.mode) == hip.LP_L2_PROJH and prob.split is None
        S = prob.scores()
        g = torch.Generator().manual_seed(5)
        qi = torch.randint(0, 300, (4096,), generator=g).cuda()
        ci = torch.randint(0, FB['n_ent'], (4096,), generator=g).cuda()
        assert torch.equal(prob.pair_scores(ci, qi), S[qi, ci])


def test_fb15k237_shape_exact_path_beyond_the_expansion_limit(hip):
    """All three tables times 4: ||q||^2 + max Z exceeds L2_EXPAND_LIMIT, the guard flags the expansion and the
    evaluation is redone on the exact relation-grouped path."""
    import torchkge_amd as tk
    m, kg_test = _fb15k(4.0)
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=2048, verbose=False)
    assert ev._last_redo and m.lp_last_path == 'exact'
    _check_sample(m, ev, kg_test)


WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
rank, world, port, out_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = port
torch.cuda.set_device(0)
dist.init_process_group('gloo', rank=rank, world_size=world)
import torchkge_amd as tk
from torchkge_amd import distributed as kd
from oracle import kge_oracle as orc
n_ent, n_rel, de, dr = 3001, 11, 48, 20
g = torch.Generator().manual_seed(3)
E = torch.randn(n_ent, de, generator=g) * 0.2
rel = torch.randn(n_rel, dr, generator=g) * 0.2
P = torch.randn(n_rel, dr * de, generator=g) * 0.12
m = tk.TransRModel(de, dr, n_ent, n_rel)
m.load_state_dict({'ent_emb.weight': E, 'rel_emb.weight': rel, 'proj_mat.weight': P})
m = m.cuda()
h, t, r = orc.synthetic_triples_zipf(n_ent, n_rel, 20000, 9, hubs=((900, 'head'), (300, 'tail')))
kg = tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                       rel2ix={i: i for i in range(n_rel)})
_, kg_test = kg.split_kg(sizes=(19000, 1000))
ref = tk.LinkPredictionEvaluator(m, kg_test, graph=False)
ref.evaluate(b_size=256, verbose=False)
ok = m.lp_last_path == 'expand'
want = [ref.rank_true_heads, ref.rank_true_tails, ref.filt_rank_true_heads, ref.filt_rank_true_tails]
kd.shard_model_(m)
for exchange, graph, qx in (('counts', False, 'evaluate'), ('counts', True, 'evaluate'), ('counts', False, 'batch')):
    ev = tk.LinkPredictionEvaluator(m, kg_test, shard='entities', exchange=exchange, graph=graph, query_exchange=qx)
    for _ in range(2):
        ev.evaluate(b_size=256, verbose=False)
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
    """Two ranks (gloo) sharing the one GPU, each holding half of ent_emb (Z built for the local rows only): ranks equal
    the unsharded evaluator's, with and without graph."""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'root': ROOT})
    port = str(32300 + (os.getpid() % 50) * 7)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('KGE_FORCE_COLLECTIVES', None)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', port, str(tmp_path / ('r%d' % r))],
                              env=env, cwd=ROOT) for r in range(2)]
    codes = [p.wait(timeout=600) for p in procs]
    assert codes == [0, 0]
