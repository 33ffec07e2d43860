"""GPU tests of ANALOGY on the HIP engine (run with -m gpu on an MI355X): the pack / query / score kernels of
include/kge_hip_analogy.h, scoring_function forward / backward, the inference API, LinkPredictionEvaluator and
RelationPredictionEvaluator against the reference's fixture, top-k inference, the packed candidate rows after an
in-place update of the tables under a captured graph, a medium shape whose width is a multiple of neither 4 nor 8, and
row-sharded entity tables on two ranks.  The float64 restatement is tests/analogy_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.helpers import ROOT
from tests import analogy_ref as ar

pytestmark = pytest.mark.gpu

TOL = 1e-5
TIE = 2e-5
NAMES = ['rank_true_heads', 'rank_true_tails', 'filt_rank_true_heads', 'filt_rank_true_tails']
SHAPES = [(0, 1), (1, 0), (1, 1), (3, 4), (9, 23), (16, 16), (100, 100), (512, 256)]


@pytest.fixture(scope='module')
def A():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_analogy
    _hip_analogy.load_library()
    return _hip_analogy


def build(tabs, dev='cuda'):
    """AnalogyModel holding the six tables ``tabs``."""
    import torchkge_amd as tk
    tabs = [torch.as_tensor(x).float() for x in tabs]
    d_sc, d_c = tabs[0].shape[1], tabs[1].shape[1]
    m = tk.AnalogyModel(d_sc + d_c, tabs[0].shape[0], tabs[3].shape[0], scalar_share=(d_sc + 0.5) / (d_sc + d_c))
    assert (m.scalar_dim, m.complex_dim) == (d_sc, d_c)
    m.load_state_dict({n + '.weight': t.clone() for n, t in zip(ar.NAMES, tabs)})
    return m.to(dev)


def random_tables(n_ent, n_rel, d_sc, d_c, g, scale):
    return [torch.randn(n, d, generator=g) * scale for n, d in ((n_ent, d_sc), (n_ent, d_c), (n_ent, d_c),
                                                                (n_rel, d_sc), (n_rel, d_c), (n_rel, d_c))]


def load():
    import torchkge_amd as tk
    z = ar.fixture()
    n_ent, n_rel = int(z['n_ent']), int(z['n_rel'])
    m = build(ar.fixture_tables(z))
    heads, tails, rels = (torch.from_numpy(z[k]) for k in ('heads', 'tails', 'rels'))
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    nt = int(z['n_test'])
    _, kg_test = kg.split_kg(sizes=(len(heads) - nt, nt))
    return z, m, kg, kg_test


def torch_queries(tabs, side, h, t, r):
    """The reference's fp32 expressions (bilinear.py:695-711), one torch kernel per operation."""
    sc_e, re_e, im_e, sc_r, re_r, im_r = tabs
    if side == 'tail':
        sc_h, re_h, im_h, sc_rr, re_rr, im_rr = sc_e[h], re_e[h], im_e[h], sc_r[r], re_r[r], im_r[r]
        return torch.cat([sc_h * sc_rr, re_h * re_rr - im_h * im_rr, re_h * im_rr + im_h * re_rr], dim=1)
    if side == 'head':
        sc_t, re_t, im_t, sc_rr, re_rr, im_rr = sc_e[t], re_e[t], im_e[t], sc_r[r], re_r[r], im_r[r]
        return torch.cat([sc_rr * sc_t, re_rr * re_t + im_rr * im_t, re_rr * im_t - im_rr * re_t], dim=1)
    sc_h, re_h, im_h, sc_t, re_t, im_t = sc_e[h], re_e[h], im_e[h], sc_e[t], re_e[t], im_e[t]
    return torch.cat([sc_h * sc_t, re_h * re_t + im_h * im_t, re_h * im_t - im_h * re_t], dim=1)


@pytest.mark.parametrize('B', [1, 63, 65, 700])
@pytest.mark.parametrize('d_sc,d_c', SHAPES)
def test_query_and_pack_kernels_are_bit_equal_to_torch(A, d_sc, d_c, B):
    from torchkge_amd import _hip
    n_ent, n_rel = 400, 6
    g = torch.Generator().manual_seed(1000 * d_sc + d_c)
    tabs = [x.cuda() for x in random_tables(n_ent, n_rel, d_sc, d_c, g, 0.7)]
    ent, rel = tabs[:3], tabs[3:]
    K = d_sc + 2 * d_c
    h = torch.randint(0, n_ent, (B,), generator=g)
    t = torch.randint(0, n_ent, (B,), generator=g)
    r = torch.randint(0, 5, (B,), generator=g)
    h[B // 2:] = h[: B - B // 2].clone()                     # repeated entities (odd B: the two slices overlap)
    t[::7] = h[::7]                                          # some h == t
    r[0] = 5                                                 # relation 5 holds exactly one row
    h, t, r = h.cuda(), t.cuda(), r.cuda()
    Q = A.query(_hip.SIDE_BOTH, ent, rel, h, t, r)
    want = torch.cat([torch_queries(tabs, 'tail', h, t, r), torch_queries(tabs, 'head', h, t, r)])
    assert Q.shape == (2 * B, K) and torch.equal(Q, want)
    assert torch.equal(A.query(A.SIDE_REL, ent, None, h, t, None), torch_queries(tabs, 'rel', h, t, r))
    # (entity, relation, side) alone fixes the row: a permuted sub-batch, one side at a time
    perm = torch.randperm(B, generator=g).cuda()[:333]
    assert torch.equal(A.query(_hip.SIDE_TAIL, ent, rel, h[perm], t[perm], r[perm]), Q[:B][perm])
    assert torch.equal(A.query(_hip.SIDE_HEAD, ent, rel, h[perm], t[perm], r[perm]), Q[B:][perm])
    # already-gathered rows (what inference_scoring_function passes)
    gh, gt, gr = [x[h] for x in ent], [x[t] for x in ent], [x[r] for x in rel]
    assert torch.equal(A.query(_hip.SIDE_TAIL, gh, gr, None, None, None, B=B), Q[:B])
    assert torch.equal(A.query(_hip.SIDE_HEAD, gt, gr, None, None, None, B=B), Q[B:])
    assert torch.equal(A.query(A.SIDE_REL, gh, gt, None, None, None, B=B), torch_queries(tabs, 'rel', h, t, r))
    # the row-sharded contract: owners write their rows, everyone else zeros
    lo, hi = 100, 250
    Qs = A.query(_hip.SIDE_BOTH, [x[lo:hi].contiguous() for x in ent], rel, h, t, r, ent_lo=lo, ent_n=hi - lo)
    own = torch.cat([(h >= lo) & (h < hi), (t >= lo) & (t < hi)])
    assert torch.equal(Qs[own], Q[own]) and bool((Qs[~own] == 0).all())
    # pack: torch.cat of the three tables' rows, with and without an index; pad columns of a fresh matrix are zero
    P = A.pack_rows(ent)
    assert P.shape == (n_ent, (K + 3) // 4 * 4) and torch.equal(P[:, :K], torch.cat(ent, dim=1))
    assert bool((P[:, K:] == 0).all())
    assert torch.equal(A.pack_rows(ent, h)[:, :K], torch.cat(ent, dim=1)[h])
    assert torch.equal(A.pack_rows(rel, r)[:, :K], torch.cat(rel, dim=1)[r])


def test_unsupported_and_invalid_arguments_are_refused(A):
    from torchkge_amd import _hip
    from tests.helpers import raw
    lib = A.load_library()
    x = torch.zeros(4, 600, device='cuda')
    i = torch.zeros(4, dtype=torch.int64, device='cuda')
    out = torch.zeros(4, 2048, device='cuda')
    t3 = [x, 600, x, 600, x, 600]
    for d_sc, d_c in ((513, 1), (1, 513), (0, 0), (-1, 4)):
        assert raw(lib, 'kge_analogy_pack_rows', *t3, d_sc, d_c, None, 4, out, 2048) == _hip.KGE_EUNSUPPORTED
        assert raw(lib, 'kge_analogy_query', _hip.SIDE_TAIL, *t3, *t3, d_sc, d_c, i, i, i, 4, 0, -1, out, 2048) == \
            _hip.KGE_EUNSUPPORTED
        assert raw(lib, 'kge_analogy_score_triples', *t3, *t3, d_sc, d_c, i, i, i, 4, out) == _hip.KGE_EUNSUPPORTED
        assert raw(lib, 'kge_analogy_score_triples_bwd', *t3, *t3, d_sc, d_c, i, i, i, 4, out, out, 2048) == \
            _hip.KGE_EUNSUPPORTED
    EINVAL = -1
    assert raw(lib, 'kge_analogy_pack_rows', *t3, 3, 4, None, 4, out, 10) == EINVAL                 # ldp < K
    assert raw(lib, 'kge_analogy_query', 2, *t3, *t3, 3, 4, i, i, i, 4, 0, -1, out, 2048) == EINVAL  # not a side of this entry
    assert raw(lib, 'kge_analogy_query', A.SIDE_REL, *t3, *t3, 3, 4, i, i, None, 4, 0, 4, out, 2048) == EINVAL   # sharded relation side
    assert raw(lib, 'kge_analogy_query', _hip.SIDE_TAIL, *t3, *t3, 3, 4, None, None, None, 4, 0, 4, out, 2048) == EINVAL
    assert raw(lib, 'kge_analogy_query', _hip.SIDE_TAIL, *t3, *t3, 3, 4, i, i, i, 4, 0, -1, out, 10) == EINVAL
    assert raw(lib, 'kge_analogy_score_triples_bwd', *t3, *t3, 3, 4, i, i, i, 4, out, out, 10) == EINVAL
    # a zero-width segment's pointers may be NULL
    assert raw(lib, 'kge_analogy_pack_rows', None, 0, x, 600, x, 600, 0, 4, None, 4, out, 2048) == 0
    assert raw(lib, 'kge_analogy_pack_rows', x, 600, None, 0, None, 0, 4, 0, None, 4, out, 2048) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('prefix', ['', 'u_'])
def test_scoring_function_and_forward_vs_reference(A, prefix):
    z = ar.fixture()
    m = build(ar.fixture_tables(z, prefix))
    B = int(z['b_size'])
    h, t, r = (x[:B].cuda() for x in ar.fixture_test_triples(z))
    s = m.scoring_function(h, t, r)
    assert np.abs(s.detach().cpu().numpy() - z[prefix + 'sf']).max() < TOL
    pos, neg = m(h, t, r, torch.from_numpy(z[prefix + 'neg_heads']).cuda(), torch.from_numpy(z[prefix + 'neg_tails']).cuda())
    assert np.abs(pos.detach().cpu().numpy() - z[prefix + 'fwd_pos']).max() < TOL
    assert np.abs(neg.detach().cpu().numpy() - z[prefix + 'fwd_neg']).max() < TOL


@pytest.mark.parametrize('B', [300, 5000])
def test_backward_vs_float64_autograd(A, B):
    from torchkge_amd import _hip
    assert (B < _hip.BWD_SORTED_MIN_BATCH) == (B == 300)
    n_ent, n_rel, d_sc, d_c = 700, 9, 7, 10
    g = torch.Generator().manual_seed(11)
    tabs = random_tables(n_ent, n_rel, d_sc, d_c, g, 0.5)
    h = torch.randint(0, n_ent, (B,), generator=g)
    t = torch.randint(0, n_ent, (B,), generator=g)
    r = torch.randint(0, n_rel, (B,), generator=g)
    r[: (3 * B) // 4] = 4                                    # one relation holds most of the triples
    go = torch.randn(B, generator=g)
    t64 = [x.double().requires_grad_() for x in tabs]
    (ar.sf64(t64, h, t, r) * go.double()).sum().backward()
    m = build(tabs)
    s = m.scoring_function(h.cuda(), t.cuda(), r.cuda())
    assert (s.detach().cpu().double() - ar.sf64(tabs, h, t, r)).abs().max().item() < TOL
    (s * go.cuda()).sum().backward()
    for name, ref in zip(ar.NAMES, t64):
        got = getattr(m, name).weight.grad.cpu().double()
        assert got.shape == ref.grad.shape
        assert (got - ref.grad).abs().max().item() < 1e-5 * max(1.0, float(ref.grad.abs().max())) * 10, name


def test_backward_of_a_zero_width_segment_and_partial_needs(A):
    """scalar_share = 0 / 1: the empty tables get empty gradients; frozen tables get none."""
    g = torch.Generator().manual_seed(5)
    for d_sc, d_c in ((0, 5), (5, 0)):
        tabs = random_tables(50, 4, d_sc, d_c, g, 0.5)
        h, t, r = (torch.randint(0, n, (40,), generator=g) for n in (50, 50, 4))
        t64 = [x.double().requires_grad_() for x in tabs]
        ar.sf64(t64, h, t, r).sum().backward()
        m = build(tabs)
        m.im_rel_emb.weight.requires_grad_(False)
        m.scoring_function(h.cuda(), t.cuda(), r.cuda()).sum().backward()
        assert m.im_rel_emb.weight.grad is None
        for name, ref in zip(ar.NAMES[:5], t64):
            got = getattr(m, name).weight.grad.cpu().double()
            assert got.shape == ref.grad.shape, name
            if got.numel():     # the tolerance of the test above
                assert (got - ref.grad).abs().max().item() < 1e-5 * max(1.0, float(ref.grad.abs().max())) * 10, name


def test_inference_api_vs_reference(A):
    z, m, kg, kg_test = load()
    B = int(z['b_size'])
    h, t, r = kg_test.head_idx[:B].cuda(), kg_test.tail_idx[:B].cuda(), kg_test.relations[:B].cuda()
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=True)
    assert all(len(x) == 3 for x in (h_e, t_e, r_e, cand))
    tabs = [x.data for x in m._tables()]
    for k in range(3):
        assert cand[k].stride(0) == 0 and tuple(cand[k].shape) == (B, m.n_ent, tabs[k].shape[1])
        assert torch.equal(h_e[k], tabs[k][h]) and torch.equal(t_e[k], tabs[k][t]) and torch.equal(r_e[k], tabs[3 + k][r])
    for fn in (m.inference_scoring_function, m.lp_scoring_function):
        assert np.abs(fn(h_e, cand, r_e).cpu().numpy() - z['s_tail']).max() < TOL
        assert np.abs(fn(cand, t_e, r_e).cpu().numpy() - z['s_head']).max() < TOL
    # real materialised tensors, as a user may pass them
    C = tuple(c.contiguous() for c in cand)
    contig = lambda x: tuple(v.contiguous() for v in x)     # noqa: E731
    assert np.abs(m.inference_scoring_function(contig(h_e), C, contig(r_e)).cpu().numpy() - z['s_tail']).max() < TOL
    assert np.abs(m.inference_scoring_function(C, contig(t_e), contig(r_e)).cpu().numpy() - z['s_head']).max() < TOL
    h2, t2, r2, c2 = m.lp_prep_cands(h, t, r)
    for k in range(3):
        assert torch.equal(h2[k], h_e[k]) and torch.equal(r2[k], r_e[k]) and torch.equal(c2[k], cand[k])
        assert c2[k].stride(0) == 0
    # relation candidates
    h_e, t_e, r_e, rc = m.inference_prepare_candidates(h, t, r, entities=False)
    assert all(rc[k].stride(0) == 0 and rc[k].shape[1] == m.n_rel for k in range(3))
    assert np.abs(m.inference_scoring_function(h_e, t_e, rc).cpu().numpy() - z['s_rel']).max() < TOL
    RC = tuple(c.contiguous() for c in rc)
    assert np.abs(m.inference_scoring_function(h_e, t_e, RC).cpu().numpy() - z['s_rel']).max() < TOL


def test_inference_api_serves_an_uneven_split(A):
    """9 | 24 | 24: the documented score, which the reference's own inference_scoring_function cannot compute."""
    z = ar.fixture()
    tabs = ar.fixture_tables(z, 'u_')
    m = build(tabs)
    B = int(z['b_size'])
    h, t, r = (x[:B] for x in ar.fixture_test_triples(z))
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(h.cuda(), t.cuda(), r.cuda(), entities=True)
    st = m.inference_scoring_function(h_e, cand, r_e).cpu().double()
    sh = m.inference_scoring_function(tuple(c.contiguous() for c in cand), t_e, r_e).cpu().double()
    assert (st - ar.scores64(tabs, 'tail', h=h, r=r)).abs().max().item() < TOL
    assert (sh - ar.scores64(tabs, 'head', t=t, r=r)).abs().max().item() < TOL
    h_e, t_e, r_e, rc = m.inference_prepare_candidates(h.cuda(), t.cuda(), r.cuda(), entities=False)
    sr = m.inference_scoring_function(h_e, t_e, rc).cpu().double()
    assert (sr - ar.scores64(tabs, 'rel', h=h, t=t)).abs().max().item() < TOL


def tie_bounds(tabs, kg, kg_test):
    h, t, r = kg_test.head_idx, kg_test.tail_idx, kg_test.relations
    dh, dt, _ = orc.build_filter_dicts(kg.head_idx, kg.tail_idx, kg.relations)
    st, sh = ar.scores64(tabs, 'tail', h=h, r=r), ar.scores64(tabs, 'head', t=t, r=r)
    return {'rank_true_tails': orc._tie_interval(st, t, TIE), 'rank_true_heads': orc._tie_interval(sh, h, TIE),
            'filt_rank_true_tails': orc._tie_interval(orc.filter_scores_vec(st, dt, h, r, t), t, TIE),
            'filt_rank_true_heads': orc._tie_interval(orc.filter_scores_vec(sh, dh, t, r, h), h, TIE)}


def test_link_prediction_evaluator_vs_reference(A):
    import torchkge_amd as tk
    z, m, kg, kg_test = load()
    B = int(z['b_size'])
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=B, verbose=False)
    # the reference's ranks, or inside the tie interval of the float64 restatement's scores
    bounds = tie_bounds(ar.fixture_tables(z), kg, kg_test)
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


def test_relation_prediction_vs_reference(A):
    import torchkge_amd as tk
    z, m, kg, kg_test = load()
    B = int(z['b_size'])
    for directed, tag in ((True, 'dir'), (False, 'undir')):
        ev = tk.RelationPredictionEvaluator(m, kg_test, directed=directed)
        ev.evaluate(b_size=B, verbose=False)
        assert np.array_equal(ev.rank_true_rels.numpy(), z[tag + '_rank'])
        assert np.array_equal(ev.filt_rank_true_rels.numpy(), z[tag + '_frank'])
        assert abs(ev.mrr()[1] - z[tag + '_mrr'][1]) < TOL and abs(ev.mrr()[0] - z[tag + '_mrr'][0]) < TOL
        assert abs(ev.hit_at_k(3)[1] - z[tag + '_hit3'][1]) < TOL


def test_entity_inference_topk_equals_materialised(A):
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


def test_packed_rows_follow_an_in_place_update_under_a_captured_graph(A):
    """The packed candidate rows are a COPY of the tables: a captured evaluation must rebuild them at every replay (the
    pack launch is inside the graph and reads the parameters at their addresses), or an optimizer step between two
    evaluations would be ranked against stale candidates."""
    import torchkge_amd as tk
    z, m, kg, kg_test = load()
    B = int(z['b_size'])
    ev = tk.LinkPredictionEvaluator(m, kg_test, graph=True)
    for _ in range(3):
        ev.evaluate(b_size=B, verbose=False)
    before = [getattr(ev, nm).clone() for nm in NAMES]
    ptrs = [p.data_ptr() for p in m.parameters()]
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():
            p.add_((0.5 * torch.randn(p.shape, generator=g)).to(p.device))
    assert ptrs == [p.data_ptr() for p in m.parameters()]
    ev.evaluate(b_size=B, verbose=False)
    after = [getattr(ev, nm).clone() for nm in NAMES]
    assert any(not torch.equal(a, b) for a, b in zip(before, after))        # the update moved some rank
    fresh = tk.LinkPredictionEvaluator(m, kg_test, graph=False)
    fresh.evaluate(b_size=B, verbose=False)
    for nm, a in zip(NAMES, after):
        assert torch.equal(a, getattr(fresh, nm)), nm


def medium_model_and_graph():
    import torchkge_amd as tk
    n_ent, n_rel, d = 3001, 11, 50                           # K = 25 + 2 * 25 = 75
    g = torch.Generator().manual_seed(3)
    tabs = random_tables(n_ent, n_rel, 25, 25, g, 0.5)       # scores O(1)
    h, t, r = orc.synthetic_triples_zipf(n_ent, n_rel, 20000, 9, hubs=((900, 'head'), (300, 'tail')))
    kg = tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                           rel2ix={i: i for i in range(n_rel)})
    _, kg_test = kg.split_kg(sizes=(19000, 1000))
    return tabs, kg, kg_test


def test_medium_shape_split_equals_fp32_and_ranks_vs_float64(A):
    import torchkge_amd as tk
    tabs, kg, kg_test = medium_model_and_graph()
    m = build(tabs)
    assert m._lp_width() == 75
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=256, verbose=False)
    ev.evaluate(b_size=256, verbose=False)
    m.split_filter = False
    ev2 = tk.LinkPredictionEvaluator(m, kg_test)
    ev2.evaluate(b_size=256, verbose=False)
    m.split_filter = True
    for nm in NAMES:
        assert torch.equal(getattr(ev, nm), getattr(ev2, nm)), nm
    # raw ranks inside the tie interval of the float64 restatement (on the GPU)
    t64 = [x.cuda() for x in tabs]
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    for side, nm, tr, kw in (('tail', 'rank_true_tails', t, {'h': h, 'r': r}), ('head', 'rank_true_heads', h, {'t': t, 'r': r})):
        lo, hi = orc._tie_interval(ar.scores64(t64, side, **kw), tr, TIE)
        got = getattr(ev, nm).cuda()
        assert bool(((got >= lo) & (got <= hi)).all()), nm


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
from tests.test_gpu_analogy import medium_model_and_graph, build
tabs, kg, kg_test = medium_model_and_graph()
m = build(tabs)
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
            print('MISMATCH', rank, exchange, graph, qx, int((a != b).sum()), flush=True)
dist.barrier()
dist.destroy_process_group()
open(out_path, 'w').write('ok' if ok else 'bad')
sys.exit(0 if ok else 1)
'''


def test_row_sharded_two_ranks_on_one_gpu(tmp_path):
    """Two ranks (gloo) sharing the one GPU, each holding half of the three entity tables: the owner builds the query row
    (kge_analogy_query on the shard, zeros elsewhere) or every rank builds it from the replicas; each rank packs and
    scores its own candidates; ranks equal the unsharded ones."""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'root': ROOT})
    port = str(32300 + (os.getpid() % 50) * 7)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('KGE_FORCE_COLLECTIVES', None)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', port, str(tmp_path / ('r%d' % r))],
                              env=env, cwd=ROOT) for r in range(2)]
    codes = [p.wait(timeout=600) for p in procs]
    assert codes == [0, 0]
