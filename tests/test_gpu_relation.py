"""GPU tests of the relation side: kge_relation_corrupt (include/kge_hip_relation.h) against the reference fixture
(tests/golden/ref_relation.npz) and the plain-Python restatement of tests/relation_ref.py, the
BernoulliRelationNegativeSampler object, and RelationInference on the five fixture models and on every exported model
class."""
import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests import relation_ref as rr
from tests.helpers import assert_guard_intact, guarded_out, raw

pytestmark = pytest.mark.gpu

TOL = 1e-5          # the project's score tolerance (tests/test_gpu_parity.py)
KGE_EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_relation
    return _hip_relation.load_library()


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x))       # (a copy: the fixture's arrays are read-only)
    return (t if dtype is None else t.to(dtype)).cuda()


# ---------------------------------------------------------------------------------------------------------------
# kge_relation_corrupt
# ---------------------------------------------------------------------------------------------------------------
def run_corrupt(lib, heads, tails, rels, mask_ent, mask_head, draws_r, draws_h, draws_t, n_neg=1):
    """The raw entry point on guarded outputs: (neg_heads, neg_tails, neg_rels) as numpy; guards and inputs checked.
    An optional array that is None or empty goes in as NULL."""
    B = len(heads)
    n = B * n_neg
    ins = [dev(heads), dev(tails), dev(rels), dev(mask_ent)] + \
        [None if x is None or len(x) == 0 else dev(x) for x in (mask_head, draws_r, draws_h, draws_t)]
    before = [None if x is None else x.clone() for x in ins]
    outs = [guarded_out(n, dtype=torch.int64) for _ in range(3)]
    ws = guarded_out(int(lib.kge_relation_corrupt_ws_elems(n)), dtype=torch.int32)
    rc = raw(lib, 'kge_relation_corrupt', *[0 if x is None else x for x in ins], B, n_neg, *outs, ws)
    assert rc == 0
    torch.cuda.synchronize()
    for o in outs + [ws]:
        assert_guard_intact(o)
    for a, b in zip(ins, before):
        assert a is None or torch.equal(a, b)
    return tuple(o.cpu().numpy() for o in outs)


@pytest.mark.parametrize('which', [64, 'all'])
def test_corrupt_equals_the_reference_on_both_recorded_batches(lib, which):
    d = rr.fixture_batch(which)
    B = len(d['heads'])
    want = (d['neg_heads'], d['neg_tails'], d['neg_rels'])
    got = run_corrupt(lib, d['heads'], d['tails'], d['rels'], d['mask_ent'], d['mask_head'], d['draws_r'], d['draws_h'], d['draws_t'])
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # the same arrays padded to n entries: the caller that does not know the split
    got = run_corrupt(lib, d['heads'], d['tails'], d['rels'], d['mask_ent'], rr.pad_to(d['mask_head'], B, 1, np.uint8),
                      rr.pad_to(d['draws_r'], B, -7, np.int64), rr.pad_to(d['draws_h'], B, -8, np.int64),
                      rr.pad_to(d['draws_t'], B, -9, np.int64))
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # ... and through the tensor-level wrapper
    from torchkge_amd import _hip_relation
    got = _hip_relation.relation_corrupt(*[dev(d[nm]) for nm in ('heads', 'tails', 'rels', 'mask_ent', 'mask_head', 'draws_r',
                                                                 'draws_h', 'draws_t')])
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w)


def mask_bytes(rng, mode, n):
    """zeros / ones / random: a random mask's non-zero bytes take every value of 1 .. 255."""
    if mode == 'zeros':
        return np.zeros(n, dtype=np.uint8)
    if mode == 'ones':
        return np.ones(n, dtype=np.uint8)
    return (rng.randint(0, 2, n) * rng.randint(1, 256, n)).astype(np.uint8)


MODES = [('zeros', None), ('ones', 'zeros'), ('ones', 'ones'), ('ones', 'random'), ('random', 'ones'), ('random', 'random')]


def check_against_restatement(lib, B, n_neg, modes):
    n = B * n_neg
    rng = np.random.RandomState(B * 7 + n_neg)
    heads, tails = rng.randint(0, 1000, B).astype(np.int64), rng.randint(0, 1000, B).astype(np.int64)
    rels = rng.randint(0, 50, B).astype(np.int64)
    for ent_mode, head_mode in modes:
        mask_ent = mask_bytes(rng, ent_mode, n)
        k = int((mask_ent != 0).sum())
        # n_neg == 1: n-long arrays (the split is not known); otherwise compact ones of exactly the consumed length
        mask_head = None if head_mode is None else mask_bytes(rng, head_mode, n if n_neg == 1 else k)
        q = 0 if mask_head is None else int((mask_head[:k] != 0).sum())
        lens = (n, n, n) if n_neg == 1 else (n - k, q, k - q)
        draws = [rng.randint(1000, 1 << 40, ln).astype(np.int64) for ln in lens]
        # an array whose branch cannot be taken is NULL
        if ent_mode == 'ones':
            draws[0] = None
        if ent_mode == 'zeros' or head_mode == 'zeros':
            draws[1] = None
        if ent_mode == 'zeros' or head_mode == 'ones':
            draws[2] = None
        want = rr.relation_corrupt(heads, tails, rels, mask_ent, mask_head, *draws, n_neg=n_neg)
        got = run_corrupt(lib, heads, tails, rels, mask_ent, mask_head, *draws, n_neg=n_neg)
        for g, w, nm in zip(got, want, ('neg_heads', 'neg_tails', 'neg_rels')):
            assert np.array_equal(g, w), (B, n_neg, ent_mode, head_mode, nm)
        # every draw of a taken branch was consumed in order, every other component is the fact's own
        rep = lambda a: np.tile(a, n_neg)       # noqa: E731
        ent = mask_ent != 0
        assert np.array_equal(got[2][ent], rep(rels)[ent])
        assert np.array_equal(got[0][~ent], rep(heads)[~ent]) and np.array_equal(got[1][~ent], rep(tails)[~ent])
        if draws[0] is not None:
            assert np.array_equal(got[2][~ent], draws[0][:n - k])


@pytest.mark.parametrize('n_neg', [1, 3])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 1023, 1024, 1025, 4096 + 3])
def test_corrupt_equals_the_restatement_across_the_scan_boundaries(lib, B, n_neg):
    """Across the wave (64), the block (1024 positions) and, with n_neg = 3, several blocks; masks all-0 / all-1 / random
    on both levels; NULL for the arrays of branches that cannot be taken."""
    check_against_restatement(lib, B, n_neg, MODES)


@pytest.mark.parametrize('B,n_neg', [(256 * 1024 + 5, 1), (87385, 3)])
def test_corrupt_equals_the_restatement_past_one_chunk_of_block_counts(lib, B, n_neg):
    """n > 256 * 1024: more than 256 block counts, so the one-block scan of the counts carries across its own chunks --
    for both prefix counts (all-ones masks put 1024 into every count)."""
    assert B * n_neg > 256 * 1024
    check_against_restatement(lib, B, n_neg, [('zeros', None), ('ones', 'ones'), ('random', 'random')])


def test_corrupt_of_zero_positions_touches_nothing(lib):
    outs = [guarded_out(8, dtype=torch.int64) for _ in range(3)]
    ws = guarded_out(8, dtype=torch.int32)
    e64, e8 = torch.zeros(1, dtype=torch.int64, device='cuda'), torch.zeros(1, dtype=torch.uint8, device='cuda')
    for n_neg in (1, 3):
        assert raw(lib, 'kge_relation_corrupt', e64, e64, e64, e8, e8, e64, e64, e64, 0, n_neg, *outs, ws) == 0
        assert raw(lib, 'kge_relation_corrupt', 0, 0, 0, 0, 0, 0, 0, 0, 0, n_neg, 0, 0, 0, 0) == 0
    torch.cuda.synchronize()
    for o in outs + [ws]:
        assert_guard_intact(o, rows=0)
    assert int(lib.kge_relation_corrupt_ws_elems(0)) == 0
    from torchkge_amd import _hip_relation
    e = torch.zeros(0, dtype=torch.int64, device='cuda')
    got = _hip_relation.relation_corrupt(e, e, e, e.to(torch.uint8), e.to(torch.uint8), e, e, e, n_neg=2)
    assert all(tuple(g.shape) == (0,) and g.dtype == torch.int64 for g in got)


def test_corrupt_refuses_bad_arguments_and_leaves_the_outputs_alone(lib):
    B = 5
    ins = [torch.arange(B, device='cuda')] * 3 + [torch.ones(B, dtype=torch.uint8, device='cuda')] * 2 + \
        [torch.arange(B, device='cuda')] * 3
    outs = [guarded_out(B, dtype=torch.int64) for _ in range(3)]
    ws = guarded_out(int(lib.kge_relation_corrupt_ws_elems(3 * B)), dtype=torch.int32)
    assert raw(lib, 'kge_relation_corrupt', *ins, -1, 1, *outs, ws) == KGE_EINVAL
    for n_neg in (0, -2):
        assert raw(lib, 'kge_relation_corrupt', *ins, B, n_neg, *outs, ws) == KGE_EINVAL
    assert raw(lib, 'kge_relation_corrupt', *ins, B, (1 << 31) // B + 1, *outs, ws) == KGE_EINVAL     # B * n_neg past int32
    for i in (0, 1, 2, 3):                      # a NULL heads / tails / rels / mask_ent
        a = list(ins)
        a[i] = 0
        assert raw(lib, 'kge_relation_corrupt', *a, B, 1, *outs, ws) == KGE_EINVAL, i
    for i in range(3):                          # a NULL output
        o = list(outs)
        o[i] = 0
        assert raw(lib, 'kge_relation_corrupt', *ins, B, 1, *o, ws) == KGE_EINVAL, i
    assert raw(lib, 'kge_relation_corrupt', *ins, B, 1, *outs, 0) == KGE_EINVAL
    torch.cuda.synchronize()
    for o in outs + [ws]:
        assert_guard_intact(o, rows=0)


def test_corrupt_gives_identical_bytes_from_launch_to_launch(lib):
    B, n_neg = 4096 + 3, 3
    n = B * n_neg
    rng = np.random.RandomState(5)
    args = [rng.randint(0, 1000, B).astype(np.int64) for _ in range(3)] + [mask_bytes(rng, 'random', n), mask_bytes(rng, 'random', n)] + \
        [rng.randint(0, 1 << 40, n).astype(np.int64) for _ in range(3)]
    first = run_corrupt(lib, *args, n_neg=n_neg)
    for _ in range(2):
        again = run_corrupt(lib, *args, n_neg=n_neg)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


# ---------------------------------------------------------------------------------------------------------------
# BernoulliRelationNegativeSampler
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def graph():
    import torchkge_amd as tk
    kg = rr.fixture_kg(tk)
    return kg, kg.head_idx.cuda(), kg.tail_idx.cuda(), kg.relations.cuda()


@pytest.fixture()
def recorded(monkeypatch):
    """The arguments of every kge_relation_corrupt call the sampler makes."""
    from torchkge_amd import sampling
    calls = []
    inner = sampling._hip_relation.relation_corrupt

    def recording(*args):
        calls.append(args)
        return inner(*args)
    monkeypatch.setattr(sampling._hip_relation, 'relation_corrupt', recording)
    return calls


@pytest.mark.parametrize('sync_free', [False, True])
def test_sampler_same_seed_same_samples_and_untouched_components(graph, recorded, sync_free):
    from torchkge_amd.sampling import BernoulliRelationNegativeSampler
    kg, h, t, r = graph
    s = BernoulliRelationNegativeSampler(kg, n_neg=2)
    s.sync_free = sync_free
    torch.manual_seed(3)
    a = s.corrupt_batch(h, t, r)
    torch.manual_seed(3)
    b = s.corrupt_batch(h, t, r)
    torch.manual_seed(4)
    c = s.corrupt_batch(h, t, r)
    n = 2 * kg.n_facts
    assert all(x.dtype == torch.int64 and x.is_cuda and tuple(x.shape) == (n,) for x in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not all(torch.equal(x, y) for x, y in zip(a, c))
    # what the kernel was given explains what came back
    heads, tails, rels, mask_ent, mask_head, draws_r, draws_h, draws_t, n_neg = recorded[0]
    assert n_neg == 2 and mask_ent.dtype == torch.uint8 and mask_head.dtype == torch.uint8
    k = int(mask_ent.sum())
    q = int(mask_head[:k].sum())
    want_lens = (n, n, n, n) if sync_free else (k, n - k, q, k - q)
    assert tuple(x.shape[0] for x in (mask_head, draws_r, draws_h, draws_t)) == want_lens
    want = rr.relation_corrupt(*[x.cpu().numpy() for x in (heads, tails, rels, mask_ent, mask_head, draws_r, draws_h, draws_t)],
                               n_neg=2)
    nh, nt, nr = (x.cpu().numpy() for x in a)
    assert np.array_equal(nh, want[0]) and np.array_equal(nt, want[1]) and np.array_equal(nr, want[2])
    ent = mask_ent.cpu().numpy() != 0
    is_head = np.zeros(n, dtype=bool)
    is_head[np.flatnonzero(ent)] = mask_head[:k].cpu().numpy() != 0
    H, T, R = (np.tile(x.cpu().numpy(), 2) for x in (h, t, r))
    assert np.array_equal(nr[ent], R[ent]) and np.array_equal(nh[~ent], H[~ent]) and np.array_equal(nt[~ent], T[~ent])
    assert np.array_equal(nt[ent & is_head], T[ent & is_head]) and np.array_equal(nh[ent & ~is_head], H[ent & ~is_head])
    # the reference's quirk: randint(1, .) never draws id 0
    assert nr[~ent].min() >= 1 and nr[~ent].max() < kg.n_rel
    assert nh[ent & is_head].min() >= 1 and nt[ent & ~is_head].min() >= 1 and max(nh.max(), nt.max()) < kg.n_ent


def test_sampler_sync_free_reads_nothing_back(graph, monkeypatch):
    from torchkge_amd.sampling import BernoulliRelationNegativeSampler
    kg, h, t, r = graph
    s = BernoulliRelationNegativeSampler(kg)
    s.sync_free = True
    s.corrupt_batch(h, t, r)                    # (library loaded, probabilities on the device)
    torch.cuda.synchronize()

    def refuse(*a, **kw):
        raise AssertionError('the sync-free path read a value back')
    with monkeypatch.context() as mp:           # the host reads of the other path are not taken ...
        for name in ('item', 'tolist', 'cpu', 'numpy', 'nonzero'):
            mp.setattr(torch.Tensor, name, refuse)
        out = s.corrupt_batch(h, t, r)
    assert tuple(out[0].shape) == (kg.n_facts,)
    # ... and where this build can tell, no synchronising call is made at all
    detects = False
    try:
        torch.cuda.set_sync_debug_mode('error')
    except Exception:                           # (a build without the switch)
        return
    try:
        try:
            torch.ones(1, device='cuda').item()
        except RuntimeError:
            detects = True
        if detects:
            out = s.corrupt_batch(h, t, r, n_neg=3)
            s.sync_free = False
            with pytest.raises(RuntimeError):
                s.corrupt_batch(h, t, r)        # the reference's host read
    finally:
        torch.cuda.set_sync_debug_mode('default')
    print('sync debug mode detects a host read on this build:', detects)
    assert tuple(out[2].shape) == ((3 if detects else 1) * kg.n_facts,)


@pytest.mark.parametrize('sync_free', [False, True])
def test_sampler_shares_lie_within_their_binomial_bounds(graph, recorded, sync_free):
    """n = 200,000 positions under a fixed seed: the share of entity-corrupted positions against rel_share, and among
    them the share of heads against the mean of bern_probs[relations], each within 5 standard deviations."""
    from torchkge_amd.sampling import BernoulliRelationNegativeSampler
    kg, h, t, r = graph
    n = 200000
    reps = -(-n // kg.n_facts)
    h, t, r = (x.repeat(reps)[:n] for x in (h, t, r))
    s = BernoulliRelationNegativeSampler(kg)
    s.sync_free = sync_free
    torch.manual_seed(17)
    nh, nt, nr = s.corrupt_batch(h, t, r)
    assert tuple(nr.shape) == (n,)
    mask_ent, mask_head = recorded[0][3], recorded[0][4]
    k = int(mask_ent.sum())
    share = k / n
    sigma = (s.rel_share * (1 - s.rel_share) / n) ** 0.5
    print('entity share %.5f (rel_share %.2f, sigma %.5f)' % (share, s.rel_share, sigma))
    assert abs(share - s.rel_share) <= 5 * sigma
    m = float(s.bern_probs[r].double().mean())
    head_share = int(mask_head[:k].sum()) / k           # (compact in both modes: entry p is the p-th entity position's)
    sigma = (m * (1 - m) / k) ** 0.5
    print('head share %.5f (mean probability %.5f, sigma %.5f)' % (head_share, m, sigma))
    assert abs(head_share - m) <= 5 * sigma
    # ... and relation by relation against bern_probs[relation]: a position uses the probability of its OWN relation
    ent_rels, is_head = r[mask_ent != 0], mask_head[:k] != 0
    for rel in range(kg.n_rel):
        sel = ent_rels == rel
        cnt, p = int(sel.sum()), float(s.bern_probs[rel])
        assert cnt > 1000
        assert abs(int(is_head[sel].sum()) / cnt - p) <= 5 * (p * (1 - p) / cnt) ** 0.5, (rel, p)
    assert float(s.bern_probs.max() - s.bern_probs.min()) > 0.05      # (the relations do differ: ten of these sigmas)
    # a corrupted relation is uniform over 1 .. n_rel - 1
    rel_pos = (mask_ent == 0)
    counts = torch.bincount(nr[rel_pos], minlength=kg.n_rel).double()
    assert counts[0] == 0
    p = 1.0 / (kg.n_rel - 1)
    assert ((counts[1:] / (n - k) - p).abs() <= 5 * (p * (1 - p) / (n - k)) ** 0.5).all()


def test_sampler_n_neg_rows_are_what_forward_scores(graph):
    import torchkge_amd as tk
    from torchkge_amd.sampling import BernoulliRelationNegativeSampler
    kg, h, t, r = graph
    B = 200
    h, t, r = h[:B], t[:B], r[:B]
    s = BernoulliRelationNegativeSampler(kg, n_neg=3)
    torch.manual_seed(9)
    nh, nt, nr = s.corrupt_batch(h, t, r)
    assert tuple(nh.shape) == tuple(nt.shape) == tuple(nr.shape) == (3 * B,)
    assert tuple(s.corrupt_batch(h, t, r, n_neg=1)[0].shape) == (B,)
    torch.manual_seed(0)
    m = tk.TransEModel(16, kg.n_ent, kg.n_rel, 'L2').cuda()
    with torch.no_grad():
        pos, neg = m(h, t, r, nh, nt, nr)
        assert tuple(neg.shape) == (3 * B,) and torch.equal(neg, m.scoring_function(nh, nt, nr))
        assert torch.equal(pos[:B], m.scoring_function(h, t, r))


def test_sampler_corrupt_kg_returns_three_vectors(graph):
    from torchkge_amd.sampling import BernoulliRelationNegativeSampler
    kg, h, t, r = graph
    s = BernoulliRelationNegativeSampler(kg, n_neg=4)       # corrupt_kg draws one negative per fact whatever n_neg is
    torch.manual_seed(2)
    out = s.corrupt_kg(500, True)
    assert len(out) == 3 and all(x.dtype == torch.int64 and not x.is_cuda and tuple(x.shape) == (kg.n_facts,) for x in out)
    torch.manual_seed(2)
    dev_out = s.corrupt_kg(500, True, which='main', on_device=True)
    assert all(x.is_cuda and torch.equal(x.cpu(), y) for x, y in zip(dev_out, out))
    changed = (out[0] != kg.head_idx).long() + (out[1] != kg.tail_idx).long() + (out[2] != kg.relations).long()
    assert int(changed.max()) == 1 and 0.7 < float(changed.double().mean()) < 1.0      # one component at most, most rows changed


def test_sampler_with_one_relation_raises_torchs_own_error():
    import torchkge_amd as tk
    from torchkge_amd.sampling import BernoulliRelationNegativeSampler
    h = torch.arange(10)
    kg = tk.KnowledgeGraph(kg={'heads': h, 'tails': (h + 1) % 10, 'relations': torch.zeros(10, dtype=torch.int64)},
                           ent2ix={i: i for i in range(10)}, rel2ix={0: 0})
    s = BernoulliRelationNegativeSampler(kg)
    with pytest.raises(RuntimeError, match='from'):
        s.corrupt_batch(kg.head_idx.cuda(), kg.tail_idx.cuda(), kg.relations.cuda())


# ---------------------------------------------------------------------------------------------------------------
# RelationInference
# ---------------------------------------------------------------------------------------------------------------
def fixture_model(kind):
    import torchkge_amd as tk
    z = rr.fixture()
    tables = rr.fixture_tables(kind)
    n_ent, n_rel, d = int(z['n_ent']), int(z['n_rel']), tables[0].shape[1]
    if kind == 'transe':
        m, names = tk.TransEModel(d, n_ent, n_rel, dissimilarity_type='L2'), ['ent_emb', 'rel_emb']
    elif kind == 'transh':
        m, names = tk.TransHModel(d, n_ent, n_rel), ['ent_emb', 'rel_emb', 'norm_vect']
    elif kind == 'transd':
        m, names = tk.TransDModel(d, tables[1].shape[1], n_ent, n_rel), ['ent_emb', 'rel_emb', 'ent_proj_vect', 'rel_proj_vect']
    elif kind == 'distmult':
        m, names = tk.DistMultModel(d, n_ent, n_rel), ['ent_emb', 'rel_emb']
    else:
        m, names = tk.ComplExModel(d, n_ent, n_rel), ['re_ent_emb', 'im_ent_emb', 're_rel_emb', 'im_rel_emb']
    m.load_state_dict({n + '.weight': t.clone() for n, t in zip(names, tables)})
    return m.cuda()


@pytest.mark.parametrize('kind', rr.KINDS)
def test_relation_inference_equals_the_reference(graph, kind):
    """Scores within 1e-5 of the reference's at the predicted ids; the predicted id is the reference's, or the reference
    itself holds the two relations within NEAR of each other -- in no more rows than the fixture counted as near ties."""
    from torchkge_amd.inference import RelationInference
    z = rr.fixture()
    kg = graph[0]
    n, k, b, near = int(z['n_pairs']), int(z['top_k']), int(z['b_size']), float(z['near'])
    e1, e2 = kg.head_idx[-n:], kg.tail_idx[-n:]
    m = fixture_model(kind)
    for variant, dictionary in (('raw', None), ('filt', kg.dict_of_rels)):
        tag = '%s_%s_' % (kind, variant)
        inf = RelationInference(m, e1, e2, top_k=k, dictionary=dictionary)
        inf.evaluate(b_size=b, verbose=False)
        pred, val = inf.predictions.numpy(), inf.scores.numpy()
        assert pred.shape == (n, k) and val.shape == (n, k) and pred.dtype == np.int64 and val.dtype == np.float32
        ref_mat, ref_ids, ref_vals = z[tag + 'scores'], z[tag + 'top_ids'], z[tag + 'top_vals']
        rows = np.arange(n)[:, None]
        at_pred = ref_mat[rows, pred]                   # the reference's score of the relation the engine predicts
        masked = np.isinf(ref_vals)
        assert np.array_equal(np.isinf(val), masked) and (val[masked] < 0).all()
        err = np.abs(val[~masked] - at_pred[~masked]).max()
        swapped = (pred != ref_ids) & ~masked
        assert (np.abs(at_pred[swapped] - ref_vals[swapped]) <= near).all()
        near_rows = int(swapped.any(axis=1).sum())
        print(tag, 'max score error %.3g' % err, 'rows ordered differently', near_rows, 'near-tie rows of the reference', int(z[tag + 'near']))
        assert err < TOL
        assert near_rows <= int(z[tag + 'near'])
        for i, j in zip(*np.nonzero(masked)):           # a masked entry: one of the pair's known relations
            assert variant == 'filt' and int(pred[i, j]) in kg.dict_of_rels[(int(e1[i]), int(e2[i]))]
        assert all(len(set(row)) == k for row in pred.tolist())


def tiny_models(tk, n_ent, n_rel, d):
    return [('TransE', lambda: tk.TransEModel(d, n_ent, n_rel, 'L2')), ('TransE-L1', lambda: tk.TransEModel(d, n_ent, n_rel, 'L1')),
            ('TransH', lambda: tk.TransHModel(d, n_ent, n_rel)), ('TransD', lambda: tk.TransDModel(d, d - 8, n_ent, n_rel)),
            ('TransR', lambda: tk.TransRModel(d, d - 8, n_ent, n_rel)), ('TorusE', lambda: tk.TorusEModel(d, n_ent, n_rel, 'torus_L2')),
            ('DistMult', lambda: tk.DistMultModel(d, n_ent, n_rel)), ('ComplEx', lambda: tk.ComplExModel(d, n_ent, n_rel)),
            ('RESCAL', lambda: tk.RESCALModel(d, n_ent, n_rel)), ('HolE', lambda: tk.HolEModel(d, n_ent, n_rel)),
            ('ANALOGY', lambda: tk.AnalogyModel(d, n_ent, n_rel)), ('ConvKB', lambda: tk.ConvKBModel(d, 3, n_ent, n_rel))]


def test_tiny_model_list_covers_every_exported_model_class():
    import torchkge_amd as tk
    exported = {n for n in dir(tk) if n.endswith('Model') and isinstance(getattr(tk, n), type)}
    built = {type(make()).__name__ for _, make in tiny_models(tk, 50, 4, 16)}
    assert built == exported and len(exported) == 11


def relation_matrix(m, e1, e2):
    with torch.no_grad():
        none = torch.zeros(0, dtype=torch.long, device='cuda')
        h_emb, t_emb, _, cand = m.inference_prepare_candidates(e1.cuda(), e2.cuda(), none, entities=False)
        return m.inference_scoring_function(h_emb, t_emb, cand).cpu()


@pytest.mark.parametrize('name', ['TransE', 'TransE-L1', 'TransH', 'TransD', 'TransR', 'TorusE', 'DistMult', 'ComplEx', 'RESCAL',
                                  'HolE', 'ANALOGY', 'ConvKB'])
def test_relation_inference_is_the_sort_of_the_models_own_scores(graph, name):
    """n_ent 300, n_rel 7, d 32, 64 pairs: predictions and scores equal the stable descending sort (value descending, id
    ascending) of the model's own relation-score matrix, raw and after the oracle's filter_scores, bit for bit, for
    every top_k (9 clips to n_rel) and both batch sizes."""
    import torchkge_amd as tk
    from torchkge_amd.inference import RelationInference
    kg = graph[0]
    n_ent, n_rel, d, n = kg.n_ent, kg.n_rel, 32, 64
    assert (n_ent, n_rel) == (300, 7)
    torch.manual_seed(0)
    m = dict(tiny_models(tk, n_ent, n_rel, d))[name]().cuda()
    e1, e2 = kg.head_idx[:n].clone(), kg.tail_idx[:n].clone()
    e1[-4:], e2[-4:] = torch.tensor([0, 1, 2, 3]), torch.tensor([0, 0, 1, 1])     # (some pairs need not be facts)
    mat = relation_matrix(m, e1, e2)
    assert tuple(mat.shape) == (n, n_rel) and mat.dtype == torch.float32 and bool(torch.isfinite(mat).all())
    filt = orc.filter_scores(mat, kg.dict_of_rels, e1, e2, None)
    assert int(torch.isinf(filt).sum()) >= n - 4
    for dictionary, full in ((None, mat), (kg.dict_of_rels, filt)):
        vals, ids = torch.sort(full, dim=1, descending=True, stable=True)
        for top_k in (1, 3, 7, 9):
            k = min(top_k, n_rel)
            for b_size in (16, 64):
                inf = RelationInference(m, e1, e2, top_k=top_k, dictionary=dictionary)
                inf.evaluate(b_size=b_size, verbose=False)
                assert tuple(inf.predictions.shape) == (n, k) and not inf.predictions.is_cuda
                assert torch.equal(inf.predictions, ids[:, :k]), (top_k, b_size, dictionary is not None)
                assert torch.equal(inf.scores.view(torch.int32), vals[:, :k].contiguous().view(torch.int32)), (top_k, b_size)
    assert torch.equal(relation_matrix(m, e1, e2), mat)        # the mask went into the batch's own tile, nothing the model keeps
    assert all(p.grad is None for p in m.parameters())         # scored under no_grad
    # a prebuilt index is taken as it is
    from torchkge_amd.filter_index import filter_index_for
    inf = RelationInference(m, e1, e2, top_k=3, dictionary=filter_index_for(kg.dict_of_rels, torch.device('cuda', 0)))
    inf.evaluate(b_size=64, verbose=False)
    assert torch.equal(inf.predictions, torch.sort(filt, dim=1, descending=True, stable=True)[1][:, :3])


def test_relation_inference_of_nothing_and_of_a_sharded_model(graph):
    import torchkge_amd as tk
    from torchkge_amd.inference import RelationInference
    kg = graph[0]
    torch.manual_seed(0)
    m = tk.TransEModel(32, kg.n_ent, kg.n_rel, 'L2').cuda()
    e = torch.zeros(0, dtype=torch.int64)
    for top_k, k in ((3, 3), (9, 7)):
        inf = RelationInference(m, e, e, top_k=top_k, dictionary=kg.dict_of_rels)
        inf.evaluate(b_size=16, verbose=False)
        assert tuple(inf.predictions.shape) == (0, k) and inf.predictions.dtype == torch.int64
        assert tuple(inf.scores.shape) == (0, k) and inf.scores.dtype == torch.float32
    m._row_shard = (0, 150)         # what distributed.shard_model_ leaves behind: refused by the model's own check
    try:
        with pytest.raises(RuntimeError, match='needs the whole entity tables'):
            RelationInference(m, kg.head_idx[:8], kg.tail_idx[:8]).evaluate(b_size=8, verbose=False)
    finally:
        m._row_shard = None
