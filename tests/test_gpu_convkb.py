"""GPU tests of ConvKB on the HIP engine (run with -m gpu on an MI355X): the entry points of include/kge_hip_convkb.h
agree bit for bit with each other, and with the float64 restatement (tests/convkb_ref.py) within the project's score
tolerance; saturated scores; the reference's fixture; scoring_function's backward; argument checks; top-k inference;
graph replays after in-place weight updates; a medium shape."""
import itertools

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests import convkb_ref as cr
from tests.helpers import assert_guard_intact, carve, guarded_out, raw

pytestmark = pytest.mark.gpu

TOL = 1e-5
TIE = 2e-5
NAMES = ['rank_true_heads', 'rank_true_tails', 'filt_rank_true_heads', 'filt_rank_true_tails']
DIMS = [1, 3, 8, 33, 64]
FILTERS = [1, 2, 5, 32]
# (B, N): B = 1 and one below / at / one above the query tile (4), N = 1 and one below / at / one above the candidate
# tile (1024) of csrc/convkb.hip -- tests/test_convkb_host.py pins the two constants to the source
BN = [(1, 1025), (3, 1024), (4, 1023), (5, 1), (5, 1025), (4, 1024)]
MODES = ['tail', 'head', 'rel', 'both']


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_convkb
    _hip_convkb.load_library()
    assert (_hip_convkb.TILE_Q, _hip_convkb.TILE_C) == (4, 1024)
    return _hip_convkb


def rand_params(n_ent, n_rel, d, F, g, gain=1.0):
    """[ent, rel, conv weight (F, 3, 1), conv bias (F), linear weight (2, F d), linear bias (2)], scores O(1) apart"""
    return [torch.randn(n_ent, d, generator=g) * 0.7, torch.randn(n_rel, d, generator=g) * 0.7,
            torch.randn(F, 3, 1, generator=g) * 0.6, torch.randn(F, generator=g) * 0.3,
            torch.randn(2, F * d, generator=g) * (gain / (F * d) ** 0.5), torch.randn(2, generator=g) * 0.2]


def build(params, dev='cuda'):
    """ConvKBModel holding ``params``."""
    import torchkge_amd as tk
    params = [torch.as_tensor(x).float() for x in params]
    m = tk.ConvKBModel(params[0].shape[1], params[2].shape[0], params[0].shape[0], params[1].shape[0])
    m.load_state_dict({n: t.clone() for n, t in zip(cr.PARAMS, params)})
    return m.to(dev)


def load():
    import torchkge_amd as tk
    z = cr.fixture()
    n_ent, n_rel = int(z['n_ent']), int(z['n_rel'])
    m = build(cr.fixture_params(z))
    heads, tails, rels = (torch.from_numpy(z[k]) for k in ('heads', 'tails', 'rels'))
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    nt = int(z['n_test'])
    _, kg_test = kg.split_kg(sizes=(len(heads) - nt, nt))
    return z, m, kg, kg_test


def make_problem(K, params, mode, B, N, c_base, g):
    """A ConvKBProblem of ``mode`` on operands carved out of poisoned buffers (odd leading dimensions, bases off a
    16-byte boundary), and the float64 restatement's (B', N) scores.  'tail' / 'head' / 'both' are index-driven over the
    entity rows [c_base, c_base + N); 'rel' takes already-gathered rows and the relation table as candidates."""
    ent, rel = params[0], params[1]
    n_ent, n_rel = ent.shape[0], rel.shape[0]
    d, F = ent.shape[1], params[2].shape[0]
    ws = K.prepare(*[x.cuda() for x in params[2:]], d)
    E, R = carve(ent, pad=3, off=1, device='cuda'), carve(rel, pad=5, off=3, device='cuda')
    h = torch.randint(0, n_ent, (B,), generator=g)
    t = torch.randint(0, n_ent, (B,), generator=g)
    r = torch.randint(0, n_rel, (B,), generator=g)
    p64 = [x.cuda() for x in params]
    hc, tc, rc = h.cuda(), t.cuda(), r.cuda()
    if mode == 'rel':
        T = carve(torch.randn(N, d, generator=g) * 0.7, pad=1, off=2, device='cuda')
        prob = K.ConvKBProblem(K.SLOT_REL, carve(ent[h], pad=2, off=3, device='cuda'), None,
                               carve(ent[t], pad=7, off=1, device='cuda'), None, T, ws, d, F, B, c_base=c_base)
        ref = cr.scores64(p64, 'rel', h=hc, t=tc, cand=T)
        return prob, ref, None
    T = E[c_base:c_base + N]
    if mode == 'tail':
        prob = K.ConvKBProblem(K.SLOT_TAIL, E, hc, R, rc, T, ws, d, F, B, c_base=c_base)
        ref = cr.scores64(p64, 'tail', h=hc, r=rc, cand=T)
    elif mode == 'head':
        prob = K.ConvKBProblem(K.SLOT_HEAD, E, tc, R, rc, T, ws, d, F, B, c_base=c_base)
        ref = cr.scores64(p64, 'head', t=tc, r=rc, cand=T)
    else:
        prob = K.ConvKBProblem(K.SLOT_BOTH, E, torch.cat([hc, tc]), R, torch.cat([rc, rc]), T, ws, d, F, 2 * B,
                               c_base=c_base, B_tail=B)
        ref = torch.cat([cr.scores64(p64, 'tail', h=hc, r=rc, cand=T), cr.scores64(p64, 'head', t=tc, r=rc, cand=T)])
    return prob, ref, (hc, tc, rc)


def check_entries_agree(K, prob, g):
    """scores / chunks / row blocks / pairs / counts / filter correction of one problem, bit for bit."""
    B, N, c_base = prob.B, prob.N, int(prob.desc.c_base)
    out = guarded_out(B, N, pad=3, off=1)
    S = prob.scores(out=out)
    assert_guard_intact(out)
    assert bool(torch.isfinite(S).all())
    S = S.contiguous()
    for c0, c1 in zip((0, 1, N // 2), (1, N // 2, N)):
        if c1 > c0:
            part = guarded_out(B, c1 - c0, pad=1, off=2)
            prob.scores_chunk(c0, c1, part)
            assert_guard_intact(part)
            assert torch.equal(part, S[:, c0:c1]), ('chunk', c0, c1)
    cuts = sorted({0, 1, int(prob.desc.B_tail) + 1 if prob.desc.slot == K.SLOT_BOTH else B // 2, B})
    for q0, q1 in zip(cuts[:-1], cuts[1:]):
        if q1 > q0 and q1 <= B:
            part = guarded_out(q1 - q0, N, pad=2, off=3)
            prob.scores_rows(q0, q1, part)
            assert_guard_intact(part)
            assert torch.equal(part, S[q0:q1]), ('rows', q0, q1)
    qi = torch.arange(B, device='cuda').repeat_interleave(N)
    ci = c_base + torch.arange(N, device='cuda').repeat(B)
    assert torch.equal(prob.pair_scores(ci, qi), S.view(-1))
    outside = torch.tensor([c_base - 1, c_base + N, c_base + N + 5], device='cuda')
    assert torch.equal(prob.pair_scores(outside, torch.zeros(3, dtype=torch.long, device='cuda')), torch.zeros(3, device='cuda'))
    true_idx = c_base + torch.randint(0, N, (B,), generator=g).cuda()
    s_true = prob.pair_scores(true_idx)                     # qi = NULL: pair p belongs to query p
    assert torch.equal(s_true, S.gather(1, (true_idx - c_base).view(-1, 1)).view(-1))
    raw_cnt = prob.count_ge(s_true)
    assert raw_cnt.dtype == torch.int32 and torch.equal(raw_cnt.long(), (S >= s_true[:, None]).sum(1))
    # filter segments: a few in-range targets, the true id for every other query, ids outside the candidate range
    segs, lo, hi = [], [], []
    for i in range(B):
        tg = (c_base + torch.randint(0, N, (int(torch.randint(0, 12, (1,), generator=g)),), generator=g)).tolist()
        tg += [c_base - 1, c_base + N] + ([int(true_idx[i])] if i % 2 == 0 else [])
        lo.append(sum(len(s) for s in segs))
        segs.append(tg)
        hi.append(lo[-1] + len(tg))
    targets = torch.tensor(list(itertools.chain(*segs)), dtype=torch.int32).cuda()
    seg_lo, seg_hi = torch.tensor(lo).cuda(), torch.tensor(hi).cuda()
    sub, found = prob.filter_sub(s_true, true_idx, seg_lo, seg_hi, targets, grouped=True, plan=None)
    Sc, st, ti = S.cpu(), s_true.cpu(), true_idx.cpu()
    for i in range(B):
        inside = [c for c in segs[i] if c_base <= c < c_base + N]
        want = sum(1 for c in inside if c != int(ti[i]) and float(Sc[i, c - c_base]) >= float(st[i]))
        assert int(sub[i]) == want and int(found[i]) == int(int(ti[i]) in inside), i
    return S


@pytest.mark.parametrize('F', FILTERS)
@pytest.mark.parametrize('d', DIMS)
def test_kernel_entries_agree_bit_for_bit_and_with_float64(K, d, F):
    g = torch.Generator().manual_seed(100 * d + F)
    worst = 0.0
    for (B, N), mode in itertools.product(BN, MODES):
        c_base = 0 if (B + N) % 2 else 7
        params = rand_params(N + c_base + 3, 6, d, F, g)
        prob, ref, idx = make_problem(K, params, mode, B, N, c_base, g)
        S = check_entries_agree(K, prob, g)
        err = (S.double() - ref).abs().max().item()
        worst = max(worst, err)
        assert err < TOL, (mode, B, N, err)
        if mode == 'tail' and c_base == 0:      # scoring_function is the tail-side score at column t
            m = build(params)
            h, t, r = idx
            t = t % N
            sf = m.scoring_function(h, t, r)
            assert torch.equal(sf, S.gather(1, t.view(-1, 1)).view(-1))
            assert torch.equal(m.lp_problem(h, t, r, 'tail').scores()[:, :N], S)
    print('d = %d, F = %d: max |score - float64| = %.3g' % (d, F, worst))


@pytest.mark.parametrize('variant', ['w_zero', 'dead_relu', 'D_zero'])
@pytest.mark.parametrize('F', FILTERS)
@pytest.mark.parametrize('d', DIMS)
def test_degenerate_filters_vs_float64(K, d, F, variant):
    g = torch.Generator().manual_seed(7 * d + F)
    for (B, N), mode in itertools.product([(5, 1025), (4, 1023)], MODES):
        params = rand_params(N + 3, 6, d, F, g)
        f = F - 1
        if variant == 'w_zero':             # the candidate's weight of one filter is exactly zero (every slot a mode uses)
            for s in {'tail': (2,), 'head': (0,), 'rel': (1,), 'both': (0, 2)}[mode]:
                params[2][f, s, 0] = 0.0
        elif variant == 'dead_relu':        # one filter's ReLU is dead for every pair
            params[3][f] = -1e3
        else:                               # D = L[1] - L[0] = 0: every score is sigmoid(db)
            params[4][1] = params[4][0]
        prob, ref, _ = make_problem(K, params, mode, B, N, 0, g)
        S = prob.scores()
        assert (S.double() - ref).abs().max().item() < TOL, (mode, B, N)
        if variant == 'dead_relu':
            live = [x.clone() for x in params]
            live[4] = live[4].clone()
            live[4].view(2, F, d)[:, f, :] = 0.0        # the dead filter contributes nothing, bit for bit
            ws = K.prepare(*[x.cuda() for x in live[2:]], d)
            p2 = K.ConvKBProblem(prob.desc.slot, prob.keep[0], prob.keep[1], prob.keep[2], prob.keep[3], prob.keep[4], ws,
                                 d, F, prob.B, B_tail=int(prob.desc.B_tail))
            assert torch.equal(p2.scores(), S)
        if variant == 'D_zero':
            db = (params[5][1] - params[5][0]).double()
            assert S.unique().numel() == 1 and abs(float(S[0, 0]) - float(torch.sigmoid(db))) < 2e-7
            assert torch.equal(prob.count_ge(S[:, 0].contiguous()).long(), torch.full((prob.B,), N, device='cuda'))


def small_graph(n_ent, n_rel, n_facts, n_test, seed):
    import torchkge_amd as tk
    heads, tails, rels = orc.synthetic_triples(n_ent, n_rel, n_facts, seed=seed)
    kg = tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    _, kg_test = kg.split_kg(sizes=(n_facts - n_test, n_test))
    return kg, kg_test


def ranks_from_own_scores(m, kg_test):
    """The four rank vectors from the engine's own materialised score matrices (kge_filtered_rank_from_scores), filtered
    with the dictionaries the evaluator uses (those of the evaluated graph: split_kg hands the whole graph's on)."""
    from torchkge_amd import _hip
    from torchkge_amd.filter_index import filter_index_for
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    out = {}
    for side, true, key1, dic in (('tail', t, h, kg_test.dict_of_tails), ('head', h, t, kg_test.dict_of_heads)):
        S = m.lp_problem(h, t, r, side).scores()
        index = filter_index_for(dic, S.device)
        seg_lo, seg_hi = index.lookup(key1, r)
        rank, filt = _hip.filtered_rank_from_scores(S, true, seg_lo, seg_hi, index.targets)
        assert torch.equal(rank, _hip.get_rank(S, true))
        out['rank_true_%ss' % side], out['filt_rank_true_%ss' % side] = rank.cpu(), filt.cpu()
    return out


def test_saturated_scores_rank_like_the_engines_own_matrix(K):
    """A head gain that drives |z| past 40: fp32 scores saturate to 1 (and towards 0), whole groups of candidates tie.
    The fused counts still equal kge_get_rank / kge_filtered_rank_from_scores on the engine's own score matrix,
    position by position.  No comparison with the reference here."""
    import torchkge_amd as tk
    g = torch.Generator().manual_seed(5)
    n_ent, n_rel, d, F = 1100, 5, 16, 4
    params = rand_params(n_ent, n_rel, d, F, g, gain=400.0)
    kg, kg_test = small_graph(n_ent, n_rel, 3000, 120, seed=3)
    m = build(params)
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    S = m.lp_problem(h, t, r, 'tail').scores()
    z = cr.z64([x.cuda() for x in params], params[0].cuda()[h].unsqueeze(1), params[1].cuda()[r].unsqueeze(1),
               params[0].cuda().unsqueeze(0))
    assert float(z.abs().max()) > 40 and bool((S == 1.0).any()) and float(S.min()) < 1e-12
    want = ranks_from_own_scores(m, kg_test)
    assert int(max(v.max() for v in want.values())) > 50        # ties: many candidates share the saturated score
    for b_size in (32, 120):
        ev = tk.LinkPredictionEvaluator(m, kg_test)
        ev.evaluate(b_size=b_size, verbose=False)
        for nm in NAMES:
            assert torch.equal(getattr(ev, nm), want[nm]), (nm, b_size)


def test_scoring_function_forward_and_inference_api_vs_reference(K):
    z, m, kg, kg_test = load()
    B = int(z['b_size'])
    h, t, r = kg_test.head_idx[:B].cuda(), kg_test.tail_idx[:B].cuda(), kg_test.relations[:B].cuda()
    assert np.abs(m.scoring_function(h, t, r).detach().cpu().numpy() - z['sf']).max() < TOL
    nh, nt = torch.from_numpy(z['neg_heads']).cuda(), torch.from_numpy(z['neg_tails']).cuda()
    pos, neg = m(h, t, r, nh, nt)
    assert pos.shape == neg.shape == (2 * B,)
    assert np.abs(pos.detach().cpu().numpy() - z['fwd_pos']).max() < TOL
    assert np.abs(neg.detach().cpu().numpy() - z['fwd_neg']).max() < TOL
    h_e, t_e, r_e, cand = m.inference_prepare_candidates(h, t, r, entities=True)
    ent, rel = m.get_embeddings()
    assert tuple(cand.shape) == (B, m.n_ent, 1, m.emb_dim) and cand.stride(0) == 0
    assert torch.equal(h_e, ent[h]) and torch.equal(t_e, ent[t]) and torch.equal(r_e, rel[r])
    for fn in (m.inference_scoring_function, m.lp_scoring_function):
        assert np.abs(fn(h_e, cand, r_e).cpu().numpy() - z['s_tail']).max() < TOL
        assert np.abs(fn(cand, t_e, r_e).cpu().numpy() - z['s_head']).max() < TOL
    # a truly materialised (b, N, 1, d) tensor: the pair path, the same bits
    C = cand.contiguous()
    assert torch.equal(m.inference_scoring_function(h_e, C, r_e), m.inference_scoring_function(h_e, cand, r_e))
    assert torch.equal(m.inference_scoring_function(C, t_e, r_e), m.inference_scoring_function(cand, t_e, r_e))
    h2, t2, r2, c2 = m.lp_prep_cands(h, t, r)
    assert torch.equal(h2, h_e) and torch.equal(r2, r_e) and torch.equal(c2, cand) and c2.stride(0) == 0
    h_e, t_e, r_e, rc = m.inference_prepare_candidates(h, t, r, entities=False)
    assert tuple(rc.shape) == (B, m.n_rel, 1, m.emb_dim) and rc.stride(0) == 0
    s_rel = m.inference_scoring_function(h_e, t_e, rc)
    assert np.abs(s_rel.cpu().numpy() - z['s_rel']).max() < TOL
    assert torch.equal(m.inference_scoring_function(h_e, t_e, rc.contiguous()), s_rel)


def rank64(scores, true_idx):
    return (scores >= scores.gather(1, true_idx.view(-1, 1))).sum(dim=1)


def test_link_prediction_evaluator_vs_reference(K):
    import torchkge_amd as tk
    z, m, kg, kg_test = load()
    B = int(z['b_size'])
    params = cr.fixture_params(z)
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=B, verbose=False)
    h, t, r = kg_test.head_idx, kg_test.tail_idx, kg_test.relations
    dh, dt, _ = orc.build_filter_dicts(kg.head_idx, kg.tail_idx, kg.relations)
    st, sh = cr.scores64(params, 'tail', h=h, r=r), cr.scores64(params, 'head', t=t, r=r)
    fst, fsh = orc.filter_scores_vec(st, dt, h, r, t), orc.filter_scores_vec(sh, dh, t, r, h)
    scores = {'rank_true_tails': (st, t), 'rank_true_heads': (sh, h), 'filt_rank_true_tails': (fst, t),
              'filt_rank_true_heads': (fsh, h)}
    for nm in NAMES:                        # EVERY rank inside the tie interval, no exclusions
        lo, hi = orc._tie_interval(*scores[nm], TIE)
        got = getattr(ev, nm)
        assert bool(((got >= lo) & (got <= hi)).all()), nm
    # ... and, for the queries whose score rows the fixture holds, inside the tie intervals of the REFERENCE's scores
    for nm, key, true in (('rank_true_tails', 's_tail', t), ('rank_true_heads', 's_head', h)):
        lo, hi = orc._tie_interval(torch.from_numpy(z[key]).double(), true[:B], TIE)
        got = getattr(ev, nm)[:B]
        assert bool(((got >= lo) & (got <= hi)).all()), nm
    # MRR and Hits@10 of the restatement, given its own ranks
    r64 = {nm: rank64(*scores[nm]).double() for nm in NAMES}
    for col, (a, b) in enumerate((('rank_true_heads', 'rank_true_tails'), ('filt_rank_true_heads', 'filt_rank_true_tails'))):
        mrr = float(((1 / r64[a]).mean() + (1 / r64[b]).mean()) / 2)
        hit = float(((r64[a] <= 10).double().mean() + (r64[b] <= 10).double().mean()) / 2)
        print('mrr %.9f vs %.9f, hit@10 %.6f vs %.6f' % (ev.mrr()[col], mrr, ev.hit_at_k(10)[col], hit))
        assert abs(ev.mrr()[col] - mrr) < 1e-6 and abs(ev.hit_at_k(10)[col] - hit) < 1e-6
    want = [getattr(ev, nm).clone() for nm in NAMES]
    for kw, b_size in (({'fused': False}, 7), ({'both_sides': False}, 5), ({'graph': True}, B)):
        e2 = tk.LinkPredictionEvaluator(m, kg_test, **kw)
        e2.evaluate(b_size=b_size, verbose=False)
        for nm, w in zip(NAMES, want):
            assert torch.equal(getattr(e2, nm), w), (nm, kw)


def test_relation_prediction_vs_reference(K):
    import torchkge_amd as tk
    z, m, kg, kg_test = load()
    B = int(z['b_size'])
    params = cr.fixture_params(z)
    h, t, r = kg_test.head_idx, kg_test.tail_idx, kg_test.relations
    s_ht, s_th = cr.scores64(params, 'rel', h=h, t=t), cr.scores64(params, 'rel', h=t, t=h)
    _, _, dr = orc.build_filter_dicts(kg.head_idx, kg.tail_idx, kg.relations)
    f_ht, f_th = orc.filter_scores_vec(s_ht, dr, h, t, r), orc.filter_scores_vec(s_th, dr, h, t, r)
    for directed, tag in ((True, 'dir'), (False, 'undir')):
        ev = tk.RelationPredictionEvaluator(m, kg_test, directed=directed)
        ev.evaluate(b_size=B, verbose=False)
        raw_s = s_ht if directed else torch.cat([s_ht, s_th], dim=1)
        filt_s = f_ht if directed else torch.cat([f_ht, f_th], dim=1)
        for got, s in ((ev.rank_true_rels, raw_s), (ev.filt_rank_true_rels, filt_s)):
            lo, hi = orc._tie_interval(s, r, TIE)
            assert bool(((got >= lo) & (got <= hi)).all()), tag        # every rank
        for col, s in enumerate((raw_s, filt_s)):
            mrr = float((1 / rank64(s, r).double()).mean())
            assert abs(ev.mrr()[col] - mrr) < 1e-6, tag


GRAD_TOL = 1e-5 * 10        # x max(1, |grad|max): tests/test_gpu_analogy.py::test_backward_vs_float64_autograd


def backward_case(B, d, F, g, n_ent=40, n_rel=5):
    params = rand_params(n_ent, n_rel, d, F, g, gain=3.0)
    h = torch.randint(0, n_ent, (B,), generator=g)
    t = torch.randint(0, n_ent, (B,), generator=g)
    r = torch.randint(0, n_rel, (B,), generator=g)
    h[B // 2:] = h[: B - B // 2].clone()        # repeated entities
    t[::7] = h[::7]                             # some h == t
    go = torch.randn(B, generator=g)
    return params, h, t, r, go


def grads_of(m):
    return [p.grad for p in m._tables()]


@pytest.mark.parametrize('B', [1, 65, 700])
def test_backward_vs_float64_autograd(K, B):
    g = torch.Generator().manual_seed(11 + B)
    params, h, t, r, go = backward_case(B, 9, 6, g)
    p64 = [x.double().requires_grad_() for x in params]
    (cr.sf64(p64, h, t, r) * go.double()).sum().backward()
    m = build(params)
    s = m.scoring_function(h.cuda(), t.cuda(), r.cuda())
    assert (s.detach().cpu().double() - cr.sf64(params, h, t, r)).abs().max().item() < TOL
    (s * go.cuda()).sum().backward()
    for name, got, ref in zip(cr.PARAMS, grads_of(m), p64):
        assert got.shape == ref.grad.shape, name
        err = (got.cpu().double() - ref.grad).abs().max().item()
        print('B = %d %s: max |grad - float64| = %.3g (|grad|max %.3g)' % (B, name, err, float(ref.grad.abs().max())))
        assert err < GRAD_TOL * max(1.0, float(ref.grad.abs().max())), name
    # a second run: the four layer gradients are fixed-order reductions -- equal bits
    m2 = build(params)
    (m2.scoring_function(h.cuda(), t.cuda(), r.cuda()) * go.cuda()).sum().backward()
    for name, a, b in list(zip(cr.PARAMS, grads_of(m), grads_of(m2)))[2:]:
        assert torch.equal(a, b), name


@pytest.mark.parametrize('d,F', [(1, 4), (7, 1), (1, 1)])
def test_backward_of_single_column_and_single_filter_and_partial_needs(K, d, F):
    g = torch.Generator().manual_seed(5)
    params, h, t, r, go = backward_case(40, d, F, g)
    p64 = [x.double().requires_grad_() for x in params]
    (cr.sf64(p64, h, t, r) * go.double()).sum().backward()
    for frozen in ((), (0, 3), (2, 3, 4, 5), (0, 1)):
        m = build(params)
        for k in frozen:
            m._tables()[k].requires_grad_(False)
        (m.scoring_function(h.cuda(), t.cuda(), r.cuda()) * go.cuda()).sum().backward()
        for k, (name, got, ref) in enumerate(zip(cr.PARAMS, grads_of(m), p64)):
            if k in frozen:
                assert got is None, name
            else:
                assert got.shape == ref.grad.shape, name
                assert (got.cpu().double() - ref.grad).abs().max().item() < GRAD_TOL * max(1.0, float(ref.grad.abs().max())), name


def test_bad_arguments_are_refused_and_outputs_untouched(K):
    from torchkge_amd import _hip
    lib = K.load_library()
    EINVAL, EUNSUPPORTED = -1, -3
    g = torch.Generator().manual_seed(2)
    d, F, B, N = 8, 3, 5, 40
    params = rand_params(N, 4, d, F, g)
    prob, _, _ = make_problem(K, params, 'both', B, N, 0, g)
    good = prob.desc
    out = guarded_out(2 * B, N, pad=2)
    pairs, cnt = guarded_out(2 * B), guarded_out(2 * B, dtype=torch.int32)
    sub, found = guarded_out(2 * B, dtype=torch.int32), guarded_out(2 * B, dtype=torch.int32)
    s_true = torch.zeros(2 * B, device='cuda')
    ci = torch.zeros(2 * B, dtype=torch.long, device='cuda')
    seg = torch.zeros(2 * B, dtype=torch.long, device='cuda')
    tg = torch.zeros(4, dtype=torch.int32, device='cuda')

    def variants():
        for field, value, code in (('d', 513, EUNSUPPORTED), ('F', 513, EUNSUPPORTED), ('d', 0, EINVAL), ('F', -1, EINVAL),
                                   ('slot', 4, EINVAL), ('slot', -1, EINVAL), ('B', -1, EINVAL), ('N', -2, EINVAL),
                                   ('B_tail', 2 * B + 1, EINVAL), ('B_tail', -1, EINVAL), ('ld_qe', d - 1, EINVAL),
                                   ('ld_qr', 0, EINVAL), ('ldt', d - 1, EINVAL), ('QE', 0, EINVAL), ('T', 0, EINVAL),
                                   ('wp', 0, EINVAL), ('Dt', 0, EINVAL), ('db', 0, EINVAL)):
            p = K.ConvKBDesc.from_buffer_copy(good)
            setattr(p, field, value)
            yield field, p, code
    for field, p, code in variants():
        assert raw(lib, 'kge_convkb_scores', p, out, out.stride(0)) == code, field
        assert raw(lib, 'kge_convkb_pair_scores', p, None, ci, 2 * B, pairs) == code, field
        assert raw(lib, 'kge_convkb_count_ge', p, s_true, cnt) == code, field
        assert raw(lib, 'kge_convkb_filter_sub', p, s_true, ci, seg, seg, tg, sub, found) == code, field
    assert raw(lib, 'kge_convkb_scores', good, None, N) == EINVAL
    assert raw(lib, 'kge_convkb_scores', good, out, N - 1) == EINVAL
    assert raw(lib, 'kge_convkb_scores', None, out, N) == EINVAL
    assert raw(lib, 'kge_convkb_count_ge', good, None, cnt) == EINVAL
    assert raw(lib, 'kge_convkb_count_ge', good, s_true, None) == EINVAL
    assert raw(lib, 'kge_convkb_pair_scores', good, None, None, 3, pairs) == EINVAL
    assert raw(lib, 'kge_convkb_pair_scores', good, None, ci, -1, pairs) == EINVAL
    assert raw(lib, 'kge_convkb_filter_sub', good, s_true, ci, seg, seg, tg, None, found) == EINVAL
    ws = prob.keep[5]
    E, R = params[0].cuda(), params[1].cuda()
    sf = guarded_out(B)
    for dd, ff, code in ((513, F, EUNSUPPORTED), (d, 513, EUNSUPPORTED), (0, F, EINVAL)):
        assert raw(lib, 'kge_convkb_score_triples', E, d, R, d, dd, ff, ws, ci, ci, ci, B, sf) == code
        assert raw(lib, 'kge_convkb_prepare', params[2].cuda(), params[3].cuda(), params[4].cuda(), F * d, params[5].cuda(),
                   dd, ff, out) == code
    assert raw(lib, 'kge_convkb_score_triples', E, d - 1, R, d, d, F, ws, ci, ci, ci, B, sf) == EINVAL
    assert raw(lib, 'kge_convkb_score_triples', E, d, R, d, d, F, ws, ci, None, ci, B, sf) == EINVAL
    assert raw(lib, 'kge_convkb_prepare', params[2].cuda(), params[3].cuda(), params[4].cuda(), F * d - 1, params[5].cuda(),
               d, F, out) == EINVAL
    gbuf, rows = guarded_out(B), guarded_out(3 * B, d)
    dL = guarded_out(2, F * d)
    assert raw(lib, 'kge_convkb_score_triples_bwd', E, d, R, d, d, F, ws, ci, ci, ci, B, s_true, s_true, gbuf, rows, d,
               dL, None, None, None) == EINVAL         # the four layer gradients: all or none
    assert raw(lib, 'kge_convkb_score_triples_bwd', E, d, R, d, d, F, ws, ci, ci, ci, B, s_true, s_true, gbuf, rows, d - 1,
               None, None, None, None) == EINVAL
    assert raw(lib, 'kge_convkb_score_triples_bwd', E, d, R, d, 513, F, ws, ci, ci, ci, B, s_true, s_true, gbuf, rows, d,
               None, None, None, None) == EUNSUPPORTED
    torch.cuda.synchronize()
    for view in (out, pairs, cnt, sub, found, sf, gbuf, rows, dL):
        assert_guard_intact(view, rows=0)
    # empty problems are valid and launch nothing
    p = K.ConvKBDesc.from_buffer_copy(good)
    p.N = 0
    assert raw(lib, 'kge_convkb_scores', p, out, out.stride(0)) == 0 and raw(lib, 'kge_convkb_count_ge', p, s_true, cnt) == 0
    torch.cuda.synchronize()
    assert_guard_intact(out, rows=0)
    assert_guard_intact(cnt, rows=0)
    with pytest.raises(RuntimeError, match='emb_dim <= 512'):
        K.prepare(torch.zeros(2, 3, 1).cuda(), torch.zeros(2).cuda(), torch.zeros(2, 2 * 513).cuda(), torch.zeros(2).cuda(), 513)
    assert _hip.ABI_VERSION == 33


def test_entity_inference_topk_equals_materialised(K):
    import torchkge_amd as tk
    g = torch.Generator().manual_seed(9)
    n_ent, n_rel = 700, 5
    m = build(rand_params(n_ent, n_rel, 12, 3, g, gain=8.0))
    kg, _ = small_graph(n_ent, n_rel, 800, 100, seed=2)
    e, r = kg.head_idx[:90], kg.relations[:90]
    for missing, side in (('tails', 'tail'), ('heads', 'head')):
        a = tk.EntityInference(m, e, r, top_k=9, missing=missing, dictionary=None, tile=256)
        assert a._tile(64, n_ent) == 256                    # several chunks: 700 candidates in tiles of 256
        a.evaluate(b_size=64, verbose=False)
        S = m.lp_problem(e.cuda(), e.cuda(), r.cuda(), side).scores().cpu()
        v, i = S.sort(dim=1, descending=True)
        assert torch.equal(a.scores.cpu(), v[:, :9])
        assert bool((S.gather(1, a.predictions.cpu()) == a.scores.cpu()).all())


def test_replays_are_stable_and_follow_in_place_weight_updates(K):
    """Three consecutive evaluate() calls (eager or capturing, then replays) give equal ranks; after an in-place change
    of output.0.weight and of ent_emb.weight the next one -- a replay: kge_convkb_prepare is inside the graph -- gives
    the ranks of a fresh model holding the new weights."""
    import torchkge_amd as tk
    z, m, kg, kg_test = load()
    B = int(z['b_size'])
    for kw in ({}, {'graph': True}):
        tk.clear_eval_state()
        ev = tk.LinkPredictionEvaluator(m, kg_test, **kw)
        runs = []
        for _ in range(3):
            ev.evaluate(b_size=B, verbose=False)
            runs.append([getattr(ev, nm).clone() for nm in NAMES])
        for other in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(runs[0], other))
        ptrs = [p.data_ptr() for p in m.parameters()]
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for p in (m.output[0].weight, m.ent_emb.weight):
                p.add_((0.3 * p.abs().mean().cpu() * torch.randn(p.shape, generator=g)).to(p.device))
        assert ptrs == [p.data_ptr() for p in m.parameters()]
        ev.evaluate(b_size=B, verbose=False)
        after = [getattr(ev, nm).clone() for nm in NAMES]
        assert any(not torch.equal(a, b) for a, b in zip(runs[0], after))       # the update moved some rank
        fresh_model = build([p.detach().cpu() for p in m._tables()])
        fresh = tk.LinkPredictionEvaluator(fresh_model, kg_test, graph=False)
        fresh.evaluate(b_size=B, verbose=False)
        for nm, a in zip(NAMES, after):
            assert torch.equal(a, getattr(fresh, nm)), (nm, kw)


def test_medium_shape_ranks_vs_float64_and_own_scores(K):
    """N = 2000, 150 facts, both sides, d = 50, F = 16, x32 head."""
    import torchkge_amd as tk
    n_ent, n_rel, d, F = 2000, 11, 50, 16
    torch.manual_seed(3)
    m = tk.ConvKBModel(d, F, n_ent, n_rel)                 # the reference's initialisation ...
    with torch.no_grad():
        m.output[0].weight.mul_(32.0)                       # ... with the x32 head: scores spread, nothing saturates
    m = m.cuda()
    params = [p.detach().cpu() for p in m._tables()]
    kg, kg_test = small_graph(n_ent, n_rel, 6000, 150, seed=9)
    ev = tk.LinkPredictionEvaluator(m, kg_test)
    ev.evaluate(b_size=64, verbose=False)
    want = ranks_from_own_scores(m, kg_test)
    for nm in NAMES:
        assert torch.equal(getattr(ev, nm), want[nm]), nm
    p64 = [x.cuda() for x in params]
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    for side, nm, tr, kw in (('tail', 'rank_true_tails', t, {'h': h, 'r': r}), ('head', 'rank_true_heads', h, {'t': t, 'r': r})):
        s64 = cr.scores64(p64, side, **kw)
        assert 0.1 < float(s64.max() - s64.min()) and 1e-3 < float(s64.min()) and float(s64.max()) < 1 - 1e-3
        lo, hi = orc._tie_interval(s64, tr, TIE)
        got = getattr(ev, nm).cuda()
        assert bool(((got >= lo) & (got <= hi)).all()), nm
    dh, dt, _ = orc.build_filter_dicts(kg.head_idx, kg.tail_idx, kg.relations)
    hc, tc, rc = kg_test.head_idx, kg_test.tail_idx, kg_test.relations
    for side, nm, dic, k1, tr, kw in (('tail', 'filt_rank_true_tails', dt, hc, tc, {'h': h, 'r': r}),
                                      ('head', 'filt_rank_true_heads', dh, tc, hc, {'t': t, 'r': r})):
        fs = orc.filter_scores_vec(cr.scores64(p64, side, **kw).cpu(), dic, k1, rc, tr)
        lo, hi = orc._tie_interval(fs, tr, TIE)
        got = getattr(ev, nm)
        assert bool(((got >= lo) & (got <= hi)).all()), nm
