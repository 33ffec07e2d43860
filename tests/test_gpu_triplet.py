"""GPU tests of triplet classification: the three entry points of include/kge_hip_triplet.h against the reference
fixture (tests/golden/ref_triplet.npz) and the numpy restatement of tests/triplet_ref.py, the PositionalNegativeSampler
object, and TripletClassificationEvaluator on the six fixture models and on every exported model class."""
import numpy as np
import pytest
import torch

from tests import triplet_ref as tr
from tests.helpers import assert_guard_intact, guarded_out, raw

pytestmark = pytest.mark.gpu

TOL = 1e-5          # the project's score tolerance (tests/test_gpu_parity.py)
KGE_EINVAL = -1
ONE_BELOW = np.nextafter(np.float32(1.0), np.float32(0.0))     # the largest fp32 below 1


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_triplet
    return _hip_triplet.load_library()


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x))       # (a copy: the fixture's arrays are read-only)
    return (t if dtype is None else t.to(dtype)).cuda()


def fixture_index():
    z = tr.fixture()
    return [dev(z[k]) for k in ('poss_heads_offsets', 'poss_heads_values', 'poss_tails_offsets', 'poss_tails_values')]


# ---------------------------------------------------------------------------------------------------------------
# kge_positional_corrupt
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['main', 'test'])
def test_positional_corrupt_equals_the_reference_on_every_recorded_batch(lib, which):
    from torchkge_amd import _hip_triplet
    off_h, val_h, off_t, val_t = fixture_index()
    n_rel = int(tr.fixture()['n_rel'])
    for d in tr.fixture_batches(which):
        nh, nt = _hip_triplet.positional_corrupt(dev(d['heads']), dev(d['tails']), dev(d['rels']), dev(d['mask']), dev(d['u_h']),
                                                 dev(d['u_t']), dev(d['fb_h']), dev(d['fb_t']), off_h, val_h, off_t, val_t, n_rel)
        assert np.array_equal(nh.cpu().numpy(), d['neg_heads']) and np.array_equal(nt.cpu().numpy(), d['neg_tails'])


def synthetic_index(n_rel, seed):
    """Two dense CSRs with segments of length 0, 1 and 2**k + 1 (n_rel = 1: one segment of 9)."""
    lens = [9] if n_rel == 1 else [0, 1, 3, 5, 9, 17, 1][:n_rel]
    rng = np.random.RandomState(seed)
    out = []
    for side in range(2):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        val = np.concatenate([np.sort(rng.choice(1000, n, replace=False)) for n in lens] + [[]]).astype(np.int32)
        out += [off, val]
    return lens, out


def run_corrupt(lib, n_rel, heads, tails, rels, mask, u_h, u_t, fb_h, fb_t, index):
    """The raw entry point on guarded outputs: (neg_heads, neg_tails) as numpy; guards and inputs checked."""
    B = len(heads)
    ins = [dev(heads), dev(tails), dev(rels), dev(mask), dev(u_h), dev(u_t), None if fb_h is None else dev(fb_h),
           None if fb_t is None else dev(fb_t)] + [dev(x) for x in index]
    before = [None if x is None else x.clone() for x in ins]
    nh, nt = guarded_out(B, dtype=torch.int64), guarded_out(B, dtype=torch.int64)
    ws = guarded_out(int(lib.kge_positional_ws_elems(B)), dtype=torch.int32)
    rc = raw(lib, 'kge_positional_corrupt', *[0 if x is None else x for x in ins[:8]], *ins[8:], n_rel, B, nh, nt, ws)
    assert rc == 0
    torch.cuda.synchronize()
    assert_guard_intact(nh)
    assert_guard_intact(nt)
    assert_guard_intact(ws)
    for a, b in zip(ins, before):
        assert a is None or torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    return nh.cpu().numpy(), nt.cpu().numpy()


@pytest.mark.parametrize('B', [1, 63, 64, 1023, 1024, 1025, 2049])
def test_positional_corrupt_equals_the_restatement_on_synthetic_shapes(lib, B):
    """Across the scan's block boundary (1024 positions per block), masks all-0 / all-1 / random, one and seven
    relations with segments of length 0, 1 and 2**k + 1, draws 0, the largest fp32 below 1, and 1.0 on segments that
    are not the last of their value array (a missing clamp gives a wrong value, not a read past the array)."""
    for n_rel in (1, 7):
        lens, index = synthetic_index(n_rel, 100 + n_rel)
        rng = np.random.RandomState(B * 10 + n_rel)
        heads, tails = rng.randint(0, 1000, B).astype(np.int64), rng.randint(0, 1000, B).astype(np.int64)
        rels = rng.randint(0, n_rel, B).astype(np.int64)
        if B >= n_rel:
            rels[:n_rel] = np.arange(n_rel)             # every segment is drawn from
        for mode in ('zeros', 'ones', 'random'):
            mask = {'zeros': np.zeros(B), 'ones': np.ones(B), 'random': rng.randint(0, 2, B) * rng.randint(1, 256, B)}[mode]
            mask = mask.astype(np.uint8)
            k = int((mask != 0).sum())
            sides = []
            for sel in (mask != 0, mask == 0):
                u = rng.rand(B).astype(np.float32)      # B-long arrays: the caller that does not know the split
                u[0::5], u[1::5] = 0.0, ONE_BELOW
                r_side = rels[sel]
                one = np.flatnonzero(r_side < n_rel - 1)[2::7]      # 1.0 only where the segment is not the last one
                u[one] = 1.0
                fb = rng.randint(0, 1000, B).astype(np.int64) if n_rel > 1 else None
                sides.append((u, fb))
            (u_h, fb_h), (u_t, fb_t) = sides
            want = tr.positional_corrupt(heads, tails, rels, mask, u_h, u_t, fb_h, fb_t, *index)
            got = run_corrupt(lib, n_rel, heads, tails, rels, mask, u_h, u_t, fb_h, fb_t, index)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n_rel, mode)
            assert np.array_equal(got[1][mask != 0], tails[mask != 0]) and np.array_equal(got[0][mask == 0], heads[mask == 0])
            if n_rel == 1 and B > 1:                    # every replacement lies in the one segment
                assert set(got[0][mask != 0].tolist()) <= set(index[1].tolist())
            assert k + int((mask == 0).sum()) == B


def test_positional_corrupt_without_fallback_arrays_keeps_positions_of_empty_relations(lib):
    lens, index = synthetic_index(7, 3)
    B = 70
    rng = np.random.RandomState(1)
    heads, tails = rng.randint(0, 1000, B).astype(np.int64), rng.randint(0, 1000, B).astype(np.int64)
    rels = (np.arange(B) % 7).astype(np.int64)
    rels[5], rels[6] = 7, -1                    # ids outside [0, n_rel): treated as an empty relation
    mask = (np.arange(B) % 2).astype(np.uint8)
    u = rng.rand(B).astype(np.float32)
    want = tr.positional_corrupt(heads, tails, rels, mask, u, u, None, None, *index)
    got = run_corrupt(lib, 7, heads, tails, rels, mask, u, u, None, None, index)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    stay = (rels == 0) | (rels == 7) | (rels == -1)
    assert np.array_equal(got[0][stay], heads[stay]) and np.array_equal(got[1][stay], tails[stay])


# ---------------------------------------------------------------------------------------------------------------
# kge_relation_max
# ---------------------------------------------------------------------------------------------------------------
def run_relation_max(lib, scores, rels, n_rel):
    s, r = dev(scores), dev(rels)
    thr = guarded_out(n_rel, dtype=torch.float32)
    ws = guarded_out(int(lib.kge_relation_max_ws_elems(n_rel)), dtype=torch.int32)
    assert raw(lib, 'kge_relation_max', s, r, len(scores), n_rel, thr, ws) == 0
    torch.cuda.synchronize()
    assert_guard_intact(thr)
    assert_guard_intact(ws)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), np.asarray(scores, np.float32).view(np.uint32))
    return thr.cpu().numpy()


@pytest.mark.parametrize('n_rel', [1, 7, 1345, 70000])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 4097])
def test_relation_max_equals_numpy(lib, n, n_rel):
    """n_rel = 70000 is beyond the LDS table (4096 relations); all scores negative; absent relations take the overall
    maximum; -inf present; all scores equal; a NaN in one relation; two launches give the same bits."""
    rng = np.random.RandomState(n * 7 + n_rel)
    rels = rng.randint(0, n_rel, n).astype(np.int64)
    if n_rel >= 4:
        rels[rels == 3] = 2                     # relation 3 is absent whatever n
    base = (-10.0 * rng.rand(n) - 0.5).astype(np.float32)
    cases = {'negative': base, 'equal': np.full(n, -2.5, np.float32)}
    with_inf = base.copy()
    with_inf[::3] = -np.inf
    cases['minus_inf'] = with_inf
    with_nan = base.copy()
    with_nan[n // 2] = np.nan
    cases['nan'] = with_nan
    for name, scores in cases.items():
        want = tr.relation_max(scores, rels, n_rel)
        got = run_relation_max(lib, scores, rels, n_rel)
        assert tr.same_values(got, want), name
        again = run_relation_max(lib, scores, rels, n_rel)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), name
        if name == 'nan':
            hit = int(rels[n // 2])
            absent = np.bincount(rels, minlength=n_rel) == 0
            assert np.isnan(got[hit]) and np.isnan(got[absent]).all()
            assert int(np.isnan(got).sum()) == 1 + int(absent.sum())
        elif name == 'negative':
            assert (got < 0).all()              # the maximum starts below every score, not at 0
            if n_rel >= 4:
                assert got[3] == scores.max()


def test_relation_max_of_only_minus_inf_and_of_ids_outside_the_range(lib):
    scores = np.array([-np.inf, -np.inf, -1.0, -7.0], np.float32)
    got = run_relation_max(lib, scores[:2], np.array([0, 0]), 3)
    assert tr.same_values(got, [-np.inf] * 3)
    rels = np.array([0, 1, 5, -2])              # the two ids outside [0, 3) count for the overall maximum only
    got = run_relation_max(lib, scores, rels, 3)
    assert tr.same_values(got, tr.relation_max(scores, rels, 3)) and tr.same_values(got, [-np.inf, -np.inf, -1.0])


# ---------------------------------------------------------------------------------------------------------------
# kge_threshold_count
# ---------------------------------------------------------------------------------------------------------------
def run_threshold_count(lib, pos, neg, rels, thr):
    counts = guarded_out(2, dtype=torch.int64)
    assert raw(lib, 'kge_threshold_count', dev(pos), dev(neg), dev(rels), dev(thr), len(pos), len(thr), counts) == 0
    torch.cuda.synchronize()
    assert_guard_intact(counts)
    return tuple(counts.cpu().tolist())


@pytest.mark.parametrize('n', [1, 257, 4097])
def test_threshold_count_equals_numpy(lib, n):
    """Thresholds at each relation's median (about half the decisions fall each way), exact ties, a NaN threshold, NaN
    scores."""
    n_rel = 7
    rng = np.random.RandomState(n)
    rels = rng.randint(0, n_rel, n).astype(np.int64)
    pos = (-10.0 * rng.rand(n)).astype(np.float32)
    neg = (-10.0 * rng.rand(n)).astype(np.float32)
    thr = np.full(n_rel, -5.0, np.float32)
    for r in range(n_rel):
        if (rels == r).any():
            thr[r] = np.median(np.concatenate([pos[rels == r], neg[rels == r]])).astype(np.float32)
    pos[::4] = thr[rels[::4]]                   # exact ties count for neither side
    neg[1::4] = thr[rels[1::4]]
    for name in ('plain', 'nan_threshold', 'nan_scores'):
        p, q, t = pos.copy(), neg.copy(), thr.copy()
        if name == 'nan_threshold':
            t[2] = np.nan
        if name == 'nan_scores':
            p[n // 2], q[n // 3] = np.nan, np.nan
        want = tr.threshold_count(p, q, rels, t)
        assert run_threshold_count(lib, p, q, rels, t) == want, name
        if name == 'plain' and n > 1:
            assert 0.25 * n < want[0] < 0.75 * n and 0.25 * n < want[1] < 0.75 * n


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_touch_nothing(lib):
    B, n_rel = 8, 3
    i64 = lambda: torch.zeros(B, dtype=torch.int64, device='cuda')      # noqa: E731
    f32 = lambda: torch.zeros(B, dtype=torch.float32, device='cuda')    # noqa: E731
    mask = torch.zeros(B, dtype=torch.uint8, device='cuda')
    off = torch.zeros(n_rel + 1, dtype=torch.int64, device='cuda')
    val = torch.zeros(1, dtype=torch.int32, device='cuda')
    nh, nt = guarded_out(B, dtype=torch.int64), guarded_out(B, dtype=torch.int64)
    ws = guarded_out(int(lib.kge_positional_ws_elems(B)), dtype=torch.int32)
    good = [i64(), i64(), i64(), mask, f32(), f32(), 0, 0, off, val, off, val, n_rel, B, nh, nt, ws]
    required = (0, 1, 2, 3, 4, 5, 8, 10, 14, 15, 16)
    for pos in required:
        args = list(good)
        args[pos] = 0
        assert raw(lib, 'kge_positional_corrupt', *args) == KGE_EINVAL, pos
    for pos, bad in ((12, 0), (12, -1), (13, -1)):
        args = list(good)
        args[pos] = bad
        assert raw(lib, 'kge_positional_corrupt', *args) == KGE_EINVAL, (pos, bad)
    args = list(good)
    args[13] = 0                                    # an empty batch: success, nothing written
    assert raw(lib, 'kge_positional_corrupt', *args) == 0
    thr = guarded_out(n_rel, dtype=torch.float32)
    ws2 = guarded_out(int(lib.kge_relation_max_ws_elems(n_rel)), dtype=torch.int32)
    good = [f32(), i64(), B, n_rel, thr, ws2]
    for pos, bad in ((0, 0), (1, 0), (4, 0), (5, 0), (2, -1), (3, 0), (3, -5)):
        args = list(good)
        args[pos] = bad
        assert raw(lib, 'kge_relation_max', *args) == KGE_EINVAL, (pos, bad)
    args = list(good)
    args[2] = 0
    assert raw(lib, 'kge_relation_max', *args) == 0
    counts = guarded_out(2, dtype=torch.int64)
    good = [f32(), f32(), i64(), torch.zeros(n_rel, dtype=torch.float32, device='cuda'), B, n_rel, counts]
    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (6, 0), (4, -1), (5, 0), (5, -1)):
        args = list(good)
        args[pos] = bad
        assert raw(lib, 'kge_threshold_count', *args) == KGE_EINVAL, (pos, bad)
    args = list(good)
    args[4] = 0
    assert raw(lib, 'kge_threshold_count', *args) == 0
    torch.cuda.synchronize()
    for out in (nh, nt, ws, thr, ws2, counts):      # nothing was launched: the views still hold their sentinel too
        assert_guard_intact(out, rows=0)


# ---------------------------------------------------------------------------------------------------------------
# the sampler object
# ---------------------------------------------------------------------------------------------------------------
def check_sample(z, h, t, r, nh, nt):
    """Every output differs from its input on at most one side, and every replacement lies in the relation's set (any
    entity for the empty relation)."""
    h, t, r, nh, nt = (x.cpu().numpy() for x in (h, t, r, nh, nt))
    n_ent, empty = int(z['n_ent']), int(z['empty_rel'])
    assert not ((nh != h) & (nt != t)).any()
    sets = {}
    for side in ('heads', 'tails'):
        off, val = z['poss_%s_offsets' % side], z['poss_%s_values' % side]
        sets[side] = [set(val[off[k]:off[k + 1]].tolist()) for k in range(int(z['n_rel']))]
    for j in range(len(h)):
        for new, old, side in ((nh[j], h[j], 'heads'), (nt[j], t[j], 'tails')):
            if new != old:
                assert (0 <= new < n_ent) if r[j] == empty else (new in sets[side][r[j]]), (j, side)


def test_sampler_object_draws_valid_reproducible_samples():
    import torchkge_amd as tk
    from torchkge_amd.sampling import PositionalNegativeSampler
    z = tr.fixture()
    kg_val, kg_test = tr.fixture_kgs(tk)
    s = PositionalNegativeSampler(kg_val, kg_test=kg_test)
    h, t, r = kg_test.head_idx.cuda(), kg_test.tail_idx.cuda(), kg_test.relations.cuda()
    for sync_free in (False, True):
        s.sync_free = sync_free
        torch.manual_seed(5)
        nh, nt = s.corrupt_batch(h, t, r)
        torch.manual_seed(5)
        nh2, nt2 = s.corrupt_batch(h, t, r)
        assert torch.equal(nh, nh2) and torch.equal(nt, nt2)
        assert nh.dtype == torch.int64 and nh.is_cuda and tuple(nh.shape) == tuple(h.shape)
        check_sample(z, h, t, r, nh, nt)
        changed = int(((nh != h) | (nt != t)).sum())
        assert changed > 0.8 * len(h)                      # (a draw can hit the original entity)
        torch.manual_seed(6)
        nh3, _ = s.corrupt_batch(h, t, r)
        assert not torch.equal(nh, nh3)
    # which side is replaced follows the Bernoulli mask of the same seed
    s.sync_free = False
    torch.manual_seed(5)
    mask = torch.bernoulli(s.bern_probs.cuda()[r])
    torch.manual_seed(5)
    nh, nt = s.corrupt_batch(h, t, r)
    assert torch.equal(nt[mask == 1], t[mask == 1]) and torch.equal(nh[mask == 0], h[mask == 0])


def test_sampler_index_built_on_the_device_and_the_corrupt_kg_driver():
    import torchkge_amd as tk
    from torchkge_amd.sampling import PositionalNegativeSampler
    z = tr.fixture()
    kg_val, kg_test = tr.fixture_kgs(tk, device='cuda')     # graph vectors on the GPU: the engine's own index builder
    s = PositionalNegativeSampler(kg_val, kg_test=kg_test)
    ih, it = s._indices(torch.device('cuda', torch.cuda.current_device()))
    for idx, side in ((ih, 'heads'), (it, 'tails')):
        assert idx.offsets.is_cuda and idx.values.is_cuda
        assert np.array_equal(idx.offsets.cpu().numpy(), z['poss_%s_offsets' % side])
        assert np.array_equal(idx.values.cpu().numpy(), z['poss_%s_values' % side])
    assert np.array_equal(s.n_poss_heads.numpy(), z['n_poss_heads']) and s.possible_tails[int(z['empty_rel'])] == []
    kg_val, kg_test = tr.fixture_kgs(tk)
    s = PositionalNegativeSampler(kg_val, kg_test=kg_test)
    for which, kg in (('main', kg_val), ('test', kg_test)):
        torch.manual_seed(9)
        nh, nt = s.corrupt_kg(64, True, which=which)        # the reference's driver: host tensors
        torch.manual_seed(9)
        dh, dt = s.corrupt_kg(64, True, which=which, on_device=True)
        assert not nh.is_cuda and dh.is_cuda and nh.dtype == torch.int64 and tuple(nh.shape) == (kg.n_facts,)
        assert torch.equal(nh, dh.cpu()) and torch.equal(nt, dt.cpu())
        check_sample(z, kg.head_idx, kg.tail_idx, kg.relations, nh, nt)


# ---------------------------------------------------------------------------------------------------------------
# the evaluator
# ---------------------------------------------------------------------------------------------------------------
def fixed_negatives(ev):
    """Substitute the fixture's negatives for the sampler's output."""
    z = tr.fixture()

    def corrupt_kg(batch_size, use_cuda, which='main', on_device=False):
        assert on_device and use_cuda and which in ('main', 'test')
        return dev(z[which + '_neg_heads']), dev(z[which + '_neg_tails'])
    ev.sampler.corrupt_kg = corrupt_kg


@pytest.mark.parametrize('kind,p', tr.CASES)
def test_evaluator_against_the_reference_fixture(kind, p):
    import torchkge_amd as tk
    from torchkge_amd.evaluation import TripletClassificationEvaluator
    from tests.test_gpu_parity import build_model
    z, t = tr.fixture(), tr.tag(kind, p)
    n_ent, n_rel, b = int(z['n_ent']), int(z['n_rel']), int(z['b_size'])
    kg_val, kg_test = tr.fixture_kgs(tk)
    m = build_model(kind, p, tr.fixture_tables(kind, p), n_ent, n_rel)
    ev = TripletClassificationEvaluator(m, kg_val, kg_test)
    assert ev.evaluated is False and ev.thresholds is None
    fixed_negatives(ev)
    ev.evaluate(b)
    assert ev.evaluated is True
    thr = ev.thresholds.cpu().numpy()
    assert thr.dtype == np.float32 and thr.shape == (n_rel,) and ev.thresholds.is_cuda and not ev.thresholds.requires_grad
    print(t, 'max |threshold - reference| =', float(np.abs(thr - z[t + '_thresholds']).max()))
    assert np.abs(thr - z[t + '_thresholds']).max() <= TOL
    # ... and they are the per-relation maxima of the engine's own scores, by value
    val_neg = ev.get_scores(dev(z['main_neg_heads']), dev(z['main_neg_tails']), kg_val.relations, b).cpu().numpy()
    assert np.abs(val_neg - z[t + '_val_neg_scores']).max() <= TOL
    assert tr.same_values(thr, tr.relation_max(val_neg, z['val_rels'], n_rel))
    acc = ev.accuracy(b)
    n = kg_test.n_facts
    count = int(round(acc * 2 * n))
    assert abs(acc - count / (2 * n)) < 1e-12
    print(t, 'correct decisions', count, 'reference', int(z[t + '_correct']), 'near-threshold', int(z[t + '_near']))
    assert abs(count - int(z[t + '_correct'])) <= int(z[t + '_near'])
    pos = ev.get_scores(kg_test.head_idx, kg_test.tail_idx, kg_test.relations, b).cpu().numpy()
    neg = ev.get_scores(dev(z['test_neg_heads']), dev(z['test_neg_tails']), kg_test.relations, b).cpu().numpy()
    assert count == sum(tr.threshold_count(pos, neg, z['test_rels'], thr))       # exactly, on the engine's own scores
    assert ev.evaluated is True and torch.equal(ev.thresholds.cpu(), torch.from_numpy(thr))


def tiny_models(tk, n_ent, n_rel, d):
    return [('TransE', lambda: tk.TransEModel(d, n_ent, n_rel, 'L2')), ('TransE-L1', lambda: tk.TransEModel(d, n_ent, n_rel, 'L1')),
            ('TransH', lambda: tk.TransHModel(d, n_ent, n_rel)), ('TransD', lambda: tk.TransDModel(d, d - 2, n_ent, n_rel)),
            ('TransR', lambda: tk.TransRModel(d, d - 2, n_ent, n_rel)), ('TorusE', lambda: tk.TorusEModel(d, n_ent, n_rel, 'torus_L2')),
            ('DistMult', lambda: tk.DistMultModel(d, n_ent, n_rel)), ('ComplEx', lambda: tk.ComplExModel(d, n_ent, n_rel)),
            ('RESCAL', lambda: tk.RESCALModel(d, n_ent, n_rel)), ('HolE', lambda: tk.HolEModel(d, n_ent, n_rel)),
            ('ANALOGY', lambda: tk.AnalogyModel(d, n_ent, n_rel)), ('ConvKB', lambda: tk.ConvKBModel(d, 3, n_ent, n_rel))]


def test_tiny_model_list_covers_every_exported_model_class():
    import torchkge_amd as tk
    exported = {n for n in dir(tk) if n.endswith('Model') and isinstance(getattr(tk, n), type)}
    built = {type(make()).__name__ for _, make in tiny_models(tk, 50, 4, 8)}
    assert built == exported and len(exported) == 11


@pytest.mark.parametrize('name', ['TransE', 'TransE-L1', 'TransH', 'TransD', 'TransR', 'TorusE', 'DistMult', 'ComplEx', 'RESCAL',
                                  'HolE', 'ANALOGY', 'ConvKB'])
def test_evaluator_runs_on_every_exported_model_class(name):
    """N = 50, d = 8; relation 3 has no validation fact (fallback draws and the overall-maximum threshold)."""
    import torchkge_amd as tk
    from torchkge_amd.evaluation import TripletClassificationEvaluator
    n_ent, n_rel, d, b = 50, 4, 8, 32
    g = torch.Generator().manual_seed(3)
    mk = lambda n, rels: tk.KnowledgeGraph(kg={'heads': torch.randint(0, n_ent, (n,), generator=g),      # noqa: E731
                                               'tails': torch.randint(0, n_ent, (n,), generator=g),
                                               'relations': torch.randint(0, rels, (n,), generator=g)},
                                           ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})
    kg_val, kg_test = mk(90, n_rel - 1), mk(70, n_rel)
    torch.manual_seed(0)
    m = dict(tiny_models(tk, n_ent, n_rel, d))[name]().cuda()
    ev = TripletClassificationEvaluator(m, kg_val, kg_test)
    seen = {}
    inner = ev.sampler.corrupt_kg

    def recording(batch_size, use_cuda, which='main', on_device=False):
        seen[which] = inner(batch_size, use_cuda, which=which, on_device=on_device)
        return seen[which]
    ev.sampler.corrupt_kg = recording
    torch.manual_seed(1)
    ev.evaluate(b)
    acc = ev.accuracy(b)
    thr = ev.thresholds.cpu().numpy()
    val_neg = ev.get_scores(seen['main'][0], seen['main'][1], kg_val.relations, b).cpu().numpy()
    assert np.isfinite(thr).all() and tr.same_values(thr, tr.relation_max(val_neg, kg_val.relations.numpy(), n_rel))
    assert thr[n_rel - 1] == val_neg.max()
    pos = ev.get_scores(kg_test.head_idx, kg_test.tail_idx, kg_test.relations, b).cpu().numpy()
    neg = ev.get_scores(seen['test'][0], seen['test'][1], kg_test.relations, b).cpu().numpy()
    count = sum(tr.threshold_count(pos, neg, kg_test.relations.numpy(), thr))
    assert acc == count / (2 * kg_test.n_facts) and 0.0 <= acc <= 1.0
    assert all(p.grad is None for p in m.parameters())      # scored under no_grad
