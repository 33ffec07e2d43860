"""GPU tests of the data-redundancy analytics: torchkge_amd.utils.data_redundancy against every result the real reference
recorded (tests/golden/ref_redundancy.npz), and the three entry points of include/kge_hip_redundancy.h against the numpy
restatement of tests/redundancy_ref.py.  Every comparison is integer or list equality."""
import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests import redundancy_ref as rd
from tests.helpers import assert_guard_intact, guarded_out, raw

pytestmark = pytest.mark.gpu

KGE_EINVAL, KGE_EUNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_redundancy
    return _hip_redundancy.load_library()


def dev(x, dtype=torch.int64):
    return torch.from_numpy(np.array(x)).to(dtype).cuda()      # (a copy: the fixture's arrays are read-only)


def pairs(a):
    return [tuple(p) for p in np.asarray(a).tolist()]


def run_overlap(lib, a, b, n_ent, n_rel, want_rev=True, pad=3, rc_want=0):
    """The raw entry point on guarded outputs of leading dimension n_rel + pad: (same, rev) as numpy; guards, pad
    columns, workspace guard and inputs checked.  b None: B = A (NULL); an empty B keeps a non-NULL pointer."""
    ins_a = [dev(x) for x in a]
    ins_b = None if b is None else [dev(x) if len(x) else torch.zeros(1, dtype=torch.int64, device='cuda') for x in b]
    n_a, n_b = len(a[0]), 0 if b is None else len(b[0])
    before = [x.clone() for x in ins_a + (ins_b or [])]
    same = guarded_out(n_rel, n_rel, pad=pad, dtype=torch.int32)
    rev = guarded_out(n_rel, n_rel, pad=pad, dtype=torch.int32) if want_rev else None
    ws_bytes = int(lib.kge_relation_overlap_ws_bytes(n_a, n_b))
    ws = guarded_out(max(ws_bytes, 16), dtype=torch.uint8)
    rc = raw(lib, 'kge_relation_overlap', *ins_a, n_a, *(ins_b or [None, None, None]), n_b, n_ent, n_rel, same,
             rev, n_rel + pad, ws, ws_bytes)
    assert rc == rc_want
    torch.cuda.synchronize()
    assert_guard_intact(ws)
    for x, y in zip(ins_a + (ins_b or []), before):
        assert torch.equal(x, y)
    if rc != 0:         # a refusal touches nothing: the sentinel also fills the views
        assert_guard_intact(same, rows=0)
        if rev is not None:
            assert_guard_intact(rev, rows=0)
        return None, None
    assert_guard_intact(same)
    if rev is not None:
        assert_guard_intact(rev)
    return same.cpu().numpy().astype(np.int64), None if rev is None else rev.cpu().numpy().astype(np.int64)


def check_overlap(lib, a, b, n_ent, n_rel, **kw):
    want_same, want_rev = rd.overlap(a, b, n_ent, n_rel)
    same, rev = run_overlap(lib, a, b, n_ent, n_rel, **kw)
    assert np.array_equal(same, want_same)
    assert rev is None or np.array_equal(rev, want_rev)
    return same, rev


def run_stats(lib, h, t, r, n_ent, n_rel):
    ins = [dev(h), dev(t), dev(r)]
    before = [x.clone() for x in ins]
    out = guarded_out(3, n_rel, dtype=torch.int64)
    ws_bytes = int(lib.kge_relation_stats_ws_bytes(len(h)))
    ws = guarded_out(max(ws_bytes, 16), dtype=torch.uint8)
    assert raw(lib, 'kge_relation_stats', *ins, len(h), n_ent, n_rel, out, ws, ws_bytes) == 0
    torch.cuda.synchronize()
    assert_guard_intact(out)
    assert_guard_intact(ws)
    for x, y in zip(ins, before):
        assert torch.equal(x, y)
    return out.cpu().numpy()


def run_select(lib, counts, lengths, theta1, theta2, cap, pad=3):
    """(pairs written, true count); counts go in with leading dimension n_rel + pad."""
    n_rel = len(lengths)
    c = guarded_out(n_rel, n_rel, pad=pad, dtype=torch.int32)
    c.copy_(dev(counts, torch.int32))
    ln = dev(lengths)
    out = guarded_out(max(cap, 1), 2, dtype=torch.int32)
    n_out = guarded_out(1, dtype=torch.int64)
    ws_bytes = int(lib.kge_overlap_select_ws_bytes(n_rel))
    ws = guarded_out(ws_bytes, dtype=torch.uint8)
    assert raw(lib, 'kge_overlap_select', c, n_rel + pad, ln, n_rel, float(theta1), float(theta2), out, cap, n_out, ws, ws_bytes) == 0
    torch.cuda.synchronize()
    n = int(n_out.cpu()[0])
    assert_guard_intact(out, rows=min(n, cap))
    assert_guard_intact(n_out)
    assert_guard_intact(ws)
    assert_guard_intact(c)
    assert torch.equal(c.cpu(), torch.from_numpy(np.asarray(counts)).int()) and torch.equal(ln.cpu(), torch.from_numpy(np.asarray(lengths)).long())
    return pairs(out.cpu().numpy()[:min(n, cap)]), n


# ---------------------------------------------------------------------------------------------------------------
# 1. the module against the real reference's recorded results
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fixture_kgs():
    import torchkge_amd as tk
    z = rd.fixture()
    n_ent, n_rel = int(z['n_ent']), int(z['n_rel'])
    out = []
    for s in ('train', 'valid', 'test'):
        h, t, r = (torch.from_numpy(z[s + nm].astype(np.int64)) for nm in ('_heads', '_tails', '_rels'))
        out.append(tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                                     rel2ix={i: i for i in range(n_rel)}))
    return out


def test_module_equals_every_recorded_result_of_the_reference(lib, fixture_kgs):
    from torchkge_amd.utils import data_redundancy as dr
    z = rd.fixture()
    kgs = fixture_kgs
    dup, rev = dr.duplicates(*kgs)
    assert dup == pairs(z['dup_08_08']) and rev == pairs(z['rev_08_08'])
    assert all(type(p) is tuple and type(p[0]) is int and type(p[1]) is int for p in dup + rev)
    dup2, rev2 = dr.duplicates(*kgs, theta1=0.5, theta2=0.9)
    assert dup2 == pairs(z['dup_05_09']) and rev2 == pairs(z['rev_05_09'])
    dup3, rev3 = dr.duplicates(*kgs, reverses=pairs(z['reverses']))
    assert dup3 == pairs(z['dup_08_08_reverses']) and rev3 == pairs(z['rev_08_08_reverses'])
    cart = dr.cartesian_product_relations(*kgs)
    assert cart == z['cart_08'].tolist() and all(type(c) is int for c in cart)
    assert dr.cartesian_product_relations(*kgs, theta=0.5) == z['cart_05'].tolist()
    for nm, (k1, k2) in (('train_train', (kgs[0], kgs[0])), ('train_test', (kgs[0], kgs[2])), ('test_test', (kgs[2], kgs[2]))):
        got = dr.count_triplets(k1, k2, dup, rev)
        assert type(got) is tuple and all(type(g) is int for g in got) and list(got) == z['count_' + nm].tolist(), nm
    # the matrices themselves, for other thresholds without recounting
    lengths, same, rv = dr.relation_overlaps(*kgs)
    h, t, r = rd.concat_kgs(*rd.fixture_graphs())
    want_same, want_rev = rd.overlap((h, t, r), None, 48, 1345)
    assert lengths.dtype == torch.int64 and same.dtype == torch.int32 and same.is_cuda and rv.is_cuda
    assert np.array_equal(lengths.cpu().numpy(), rd.stats(h, t, r, 48, 1345)[0])
    assert np.array_equal(same.cpu().numpy(), want_same) and np.array_equal(rv.cpu().numpy(), want_rev)
    assert dr.relation_overlaps(*kgs, rev=False)[2] is None


def test_duplicates_with_counts_prints_the_references_lines_and_takes_device_tensors(lib, fixture_kgs, capsys):
    from torchkge_amd.utils import data_redundancy as dr
    z = rd.fixture()
    on_gpu = []
    for g in rd.fixture_graphs():           # the light graph objects, ids already on the device
        for nm in ('head_idx', 'tail_idx', 'relations'):
            setattr(g, nm, torch.from_numpy(getattr(g, nm)).cuda())
        on_gpu.append(g)
    dup, rev = dr.duplicates(*on_gpu, verbose=True, counts=True)
    assert dup == pairs(z['dup_08_08']) and rev == pairs(z['rev_08_08'])
    lines = [ln for ln in capsys.readouterr().out.split('\n') if ln]
    n_tr, n_te = len(on_gpu[0]), len(on_gpu[2])
    want = ['Computing Ts', 'Finding duplicate relations', 'Duplicate relations: %d' % len(dup),
            'Reverse duplicate relations: %d' % len(rev)]
    for nm, what, where, n in (('train_train', 'train', 'train', n_tr), ('train_test', 'test', 'train', n_te),
                               ('test_test', 'test', 'test', n_te)):
        d, r = z['count_' + nm].tolist()
        want.append('%d %s triplets have duplicate in %s set (%d%%)' % (d, what, where, int(d / n * 100)))
        want.append('%d %s triplets have reverse duplicate in %s set (%d%%)' % (r, what, where, int(r / n * 100)))
    assert lines == want


# ---------------------------------------------------------------------------------------------------------------
# 2. kge_relation_overlap on hand-made graphs
# ---------------------------------------------------------------------------------------------------------------
# n_ent = 8, n_rel = 6; relation 4 is empty
HAND = [(0, 1, 0), (1, 0, 0),                   # (a, b) and (b, a) in one relation: rev[0][0]
        (2, 2, 1), (2, 2, 2), (7, 7, 1),        # self-loops, one shared by two relations
        (3, 4, 3), (3, 4, 3), (3, 4, 3),        # a fact three times
        (3, 4, 1), (4, 3, 2),
        (7, 0, 5), (0, 7, 5), (7, 6, 5), (6, 7, 0)]     # ids n_ent - 1 and n_rel - 1


def cols(facts):
    f = np.array(facts, dtype=np.int64).reshape(-1, 3)
    return f[:, 0], f[:, 1], f[:, 2]


def test_overlap_on_the_hand_made_graph(lib):
    same, rev = check_overlap(lib, cols(HAND), None, 8, 6)
    want_same = np.zeros((6, 6), dtype=np.int64)
    want_rev = np.zeros((6, 6), dtype=np.int64)
    for d, v in (((0, 0), 3), ((1, 1), 3), ((2, 2), 2), ((3, 3), 1), ((5, 5), 3), ((1, 2), 1), ((2, 1), 1), ((3, 1), 1),
                 ((1, 3), 1)):
        want_same[d] = v
    for d, v in (((0, 0), 2), ((1, 1), 2), ((2, 2), 1), ((1, 2), 2), ((2, 1), 2), ((5, 5), 2), ((3, 2), 1), ((2, 3), 1),
                 ((5, 0), 1), ((0, 5), 1)):
        want_rev[d] = v
    assert same.tolist() == want_same.tolist() and rev.tolist() == want_rev.tolist()      # written out by hand
    assert same[4].sum() == 0 and same[:, 4].sum() == 0
    # rev = NULL: the same `same`, nothing else written
    same2, none = check_overlap(lib, cols(HAND), None, 8, 6, want_rev=False)
    assert none is None and np.array_equal(same2, same)
    # no pad columns
    check_overlap(lib, cols(HAND), None, 8, 6, pad=0)


def test_overlap_of_one_fact_of_an_empty_b_and_of_two_different_lists(lib):
    same, rev = check_overlap(lib, cols([(7, 7, 5)]), None, 8, 6)           # n = 1, a self-loop at the last ids
    assert same[5, 5] == 1 and rev[5, 5] == 1 and same.sum() == 1 and rev.sum() == 1
    same, rev = check_overlap(lib, cols([(6, 7, 0)]), None, 8, 6)
    assert same[0, 0] == 1 and same.sum() == 1 and rev.sum() == 0
    empty = (np.zeros(0, dtype=np.int64),) * 3
    for a, b in ((cols(HAND), empty), (empty, cols(HAND)), (empty, None)):
        same, rev = run_overlap(lib, a, b, 8, 6)
        assert not same.any() and not rev.any()
    # rectangular: A = the first 9 facts, B = the rest and two of A's; the expected matrix is not symmetric
    a, b = cols(HAND[:9]), cols(HAND[9:] + [(2, 2, 1), (1, 0, 3)])
    same, rev = check_overlap(lib, a, b, 8, 6)
    assert same.tolist() != same.T.tolist() and rev.tolist() != rev.T.tolist()
    assert same[2, 1] == 1 and same[1, 2] == 0 and same[0, 3] == 1 and rev[0, 3] == 1 and rev[3, 2] == 1 and rev[2, 3] == 0
    check_overlap(lib, a, b, 8, 6, want_rev=False)
    check_overlap(lib, b, a, 8, 6)


def test_overlap_refuses_bad_arguments_and_touches_nothing(lib):
    a = cols(HAND)
    x = dev(a[0])
    same = guarded_out(6, 6, pad=3, dtype=torch.int32)
    ws = guarded_out(1 << 16, dtype=torch.uint8)
    for args in ((x, x, x, -1, None, None, None, 0, 8, 6, same, None, 9, ws, 1 << 16),            # nA < 0
                 (x, x, x, 14, None, None, None, 0, 8, 6, same, None, 5, ws, 1 << 16),            # ld < n_rel
                 (x, x, x, 14, None, None, None, 0, 8, 0, same, None, 9, ws, 1 << 16),            # n_rel = 0
                 (x, x, x, 14, None, None, None, 0, 8, 6, None, None, 9, ws, 1 << 16),            # same = NULL
                 (x, x, x, 14, None, None, None, 0, 8, 6, same, None, 9, ws, 64),                 # short workspace
                 (x, x, x, 1 << 30, x, x, x, 1 << 30, 8, 6, same, None, 9, ws, 1 << 16)):         # nA + nB >= 2^31
        assert raw(lib, 'kge_relation_overlap', *args) == KGE_EINVAL
    torch.cuda.synchronize()
    assert_guard_intact(same, rows=0)
    assert_guard_intact(ws, rows=0)


# ---------------------------------------------------------------------------------------------------------------
# 3. sizes across block and scan-chunk boundaries, dense groups
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [255, 256, 257, 1023, 1024, 1025, 4097])
def test_overlap_and_stats_across_block_boundaries(lib, n):
    rng = np.random.RandomState(n)
    n_ent, n_rel = 50, 7
    h, t, r = rng.randint(0, n_ent, n), rng.randint(0, n_ent, n), rng.randint(0, n_rel, n)
    same, rev = check_overlap(lib, (h, t, r), None, n_ent, n_rel)
    assert rev.diagonal().sum() > 0 and same.sum() > same.diagonal().sum()
    k = n // 3
    check_overlap(lib, (h[:k], t[:k], r[:k]), (h[k:], t[k:], r[k:]), n_ent, n_rel)
    assert np.array_equal(run_stats(lib, h, t, r, n_ent, n_rel), rd.stats(h, t, r, n_ent, n_rel))


# ---------------------------------------------------------------------------------------------------------------
# 4. one group that holds every relation in both orientations
# ---------------------------------------------------------------------------------------------------------------
def test_one_group_holding_all_1345_relations_in_both_orientations(lib):
    rng = np.random.RandomState(4)
    n_ent, n_rel = 300, 1345
    rel = np.arange(n_rel)
    h = np.concatenate([np.full(n_rel, 17), np.full(n_rel, 230), rng.randint(0, n_ent, 2000)])
    t = np.concatenate([np.full(n_rel, 230), np.full(n_rel, 17), rng.randint(0, n_ent, 2000)])
    r = np.concatenate([rel, rel, rng.randint(0, n_rel, 2000)])
    perm = rng.permutation(len(h))
    same, rev = check_overlap(lib, (h[perm], t[perm], r[perm]), None, n_ent, n_rel)
    assert same.min() >= 2 and rev.min() >= 2           # every cell holds the two pairs of the big group


# ---------------------------------------------------------------------------------------------------------------
# 5. a Zipf-skewed graph at FB15k's relation count
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def zipf_case():
    n_ent, n_rel, n = 15000, 1345, 200000
    h, t, r = (x.numpy() for x in orc.synthetic_triples_zipf(n_ent, n_rel, n, seed=19))
    # plant duplicate and reverse pairs among the rare relations: relation q becomes a copy (a reversed copy) of p
    cnt = np.bincount(r, minlength=n_rel)
    rare = [int(i) for i in np.argsort(cnt, kind='stable') if cnt[i] >= 5][:8]
    keep = ~np.isin(r, rare[4:])
    hs, ts, rs = [h[keep]], [t[keep]], [r[keep]]
    for i, (p, q) in enumerate(zip(rare[:4], rare[4:])):
        m = r == p
        hs.append(t[m] if i % 2 else h[m])
        ts.append(h[m] if i % 2 else t[m])
        rs.append(np.full(int(m.sum()), q))
    h, t, r = np.concatenate(hs), np.concatenate(ts), np.concatenate(rs)
    h, t, r = np.concatenate([h, h[:500]]), np.concatenate([t, t[:500]]), np.concatenate([r, r[:500]])       # repeats
    same, rev = rd.overlap((h, t, r), None, n_ent, n_rel)
    st = rd.stats(h, t, r, n_ent, n_rel)
    return dict(n_ent=n_ent, n_rel=n_rel, h=h, t=t, r=r, same=same, rev=rev, stats=st,
                dup=rd.select(same, st[0], 0.8, 0.8), rdup=rd.select(rev, st[0], 0.8, 0.8))


def test_zipf_graph_of_200000_facts_equals_the_restatement(lib, zipf_case):
    from torchkge_amd.utils import data_redundancy as dr
    c = zipf_case
    assert len(c['dup']) >= 2 and len(c['rdup']) >= 2
    same, rev = run_overlap(lib, (c['h'], c['t'], c['r']), None, c['n_ent'], c['n_rel'])
    assert np.array_equal(same, c['same']) and np.array_equal(rev, c['rev'])
    assert np.array_equal(run_stats(lib, c['h'], c['t'], c['r'], c['n_ent'], c['n_rel']), c['stats'])
    n = len(c['h'])
    cut = (0, int(0.8 * n), int(0.9 * n), n)
    kgs = []
    for lo, hi in zip(cut[:-1], cut[1:]):
        g = rd.Graph(c['h'][lo:hi], c['t'][lo:hi], c['r'][lo:hi], c['n_ent'], c['n_rel'])
        for nm in ('head_idx', 'tail_idx', 'relations'):
            setattr(g, nm, torch.from_numpy(getattr(g, nm)))
        kgs.append(g)
    dup, rdup = dr.duplicates(*kgs)
    assert dup == c['dup'] and rdup == c['rdup']
    # thresholds that select thousands of pairs: more than the first read of duplicates() fetches per list
    lengths, same_d, rev_d = dr.relation_overlaps(*kgs)
    got = dr._select_both(lengths, same_d, rev_d, 0.0, 0.0)
    assert [tuple(p) for p in got[0]] == rd.select(c['same'], c['stats'][0], 0.0, 0.0)
    assert [tuple(p) for p in got[1]] == rd.select(c['rev'], c['stats'][0], 0.0, 0.0)
    assert max(len(got[0]), len(got[1])) > dr._FIRST_CAP


# ---------------------------------------------------------------------------------------------------------------
# 6. the 64-bit key budget
# ---------------------------------------------------------------------------------------------------------------
def test_key_budget_of_exactly_64_bits_passes_and_65_bits_are_refused(lib):
    n_ent, n_rel = 1 << 26, 1024                 # bits(n_ent^2 - 1) + 2 + bits(n_rel - 1) = 52 + 2 + 10
    e, r = n_ent - 1, n_rel - 1
    facts = [(e, e, r), (e, e, 0), (e, e - 1, r), (e - 1, e, r), (e - 1, e, 0), (0, e, r), (e, 0, r), (0, 0, r), (0, 0, 0),
             (e, e - 1, r), (e - 1, e - 1, 1), (0, 1, r)]
    same, rev = check_overlap(lib, cols(facts), None, n_ent, n_rel)
    assert same[r, r] == 7 and same[r, 0] == 3 and rev[r, r] == 6 and rev[r, 0] == 3 and rev[0, r] == 3
    check_overlap(lib, cols(facts[:6]), cols(facts[4:]), n_ent, n_rel)
    run_overlap(lib, cols(facts), None, n_ent, n_rel + 1, rc_want=KGE_EUNSUPPORTED)
    run_overlap(lib, cols(facts[:6]), cols(facts[4:]), n_ent, n_rel + 1, rc_want=KGE_EUNSUPPORTED)


# ---------------------------------------------------------------------------------------------------------------
# 7. kge_overlap_select
# ---------------------------------------------------------------------------------------------------------------
def test_select_thresholds_zero_lengths_cap_and_order(lib):
    #          0  1  2  3  4  5
    counts = [[9, 4, 5, 0, 4, 4],
              [4, 9, 4, 3, 0, 5],
              [5, 4, 9, 4, 4, 4],
              [0, 3, 4, 9, 4, 1],
              [9, 9, 9, 9, 9, 4],           # the lower triangle is never read as a pair
              [4, 5, 4, 1, 4, 9]]
    lengths = [5, 5, 5, 5, 0, 5]            # relation 4 holds no fact: never selected, whatever its counts
    # c = 4, len = 5, theta = 0.8: 4 / 5 > 0.8 is false
    got, n = run_select(lib, counts, lengths, 0.8, 0.8, cap=15)
    assert got == [(0, 2), (1, 5)] and n == 2 and got == rd.select(counts, lengths, 0.8, 0.8)
    # theta one ulp below 0.8: every c = 4 cell of the upper triangle whose two lengths are 5, in row-major order
    below = float(np.nextafter(0.8, 0))
    want = [(0, 1), (0, 2), (0, 5), (1, 2), (1, 5), (2, 3), (2, 5)]
    got, n = run_select(lib, counts, lengths, below, below, cap=15)
    assert got == want and n == 7 and got == rd.select(counts, lengths, below, below)
    # theta1 applies to r1's length, theta2 to r2's
    got, n = run_select(lib, counts, [5, 4, 5, 5, 0, 5], 0.9, below, cap=15)
    assert got == [(0, 2), (1, 2), (1, 5)] and got == rd.select(counts, [5, 4, 5, 5, 0, 5], 0.9, below)
    got, n = run_select(lib, counts, [5, 4, 5, 5, 0, 5], below, 0.9, cap=15)
    assert got == [(0, 1), (0, 2), (1, 5)] and got == rd.select(counts, [5, 4, 5, 5, 0, 5], below, 0.9)
    # a cap below the true count: the first cap pairs, the true count, nothing past the cap
    got, n = run_select(lib, counts, lengths, below, below, cap=3)
    assert got == want[:3] and n == 7
    got, n = run_select(lib, counts, lengths, below, below, cap=0)
    assert got == [] and n == 7
    got, n = run_select(lib, counts, lengths, 1.0, 1.0, cap=4)
    assert got == [] and n == 0


def test_select_across_scan_blocks(lib):
    """n_rel = 71: 5,041 cells, five blocks of the prefix count; every third cell of the upper triangle qualifies."""
    rng = np.random.RandomState(71)
    n_rel = 71
    lengths = rng.randint(0, 9, n_rel)
    counts = rng.randint(0, 9, (n_rel, n_rel))
    want = rd.select(counts, lengths, 0.5, 0.25)
    got, n = run_select(lib, counts, lengths, 0.5, 0.25, cap=n_rel * n_rel)
    assert got == want and n == len(want) and 100 < n < 2000
    got, n = run_select(lib, counts, lengths, 0.5, 0.25, cap=n - 1)
    assert got == want[:-1] and n == len(want)


# ---------------------------------------------------------------------------------------------------------------
# 8. kge_relation_stats
# ---------------------------------------------------------------------------------------------------------------
def test_stats_count_repeats_as_facts_and_once_as_heads_and_tails(lib):
    h, t, r = cols(HAND)
    got = run_stats(lib, h, t, r, 8, 6)
    assert got.tolist() == [[3, 3, 2, 3, 0, 3],         # facts, the triple repeat of relation 3 included
                            [3, 3, 2, 1, 0, 2],         # distinct heads
                            [3, 3, 2, 1, 0, 3]]         # distinct tails
    assert np.array_equal(got, rd.stats(h, t, r, 8, 6))
    assert run_stats(lib, h[:1], t[:1], r[:1], 8, 6).tolist() == [[1, 0, 0, 0, 0, 0]] * 3
    assert not run_stats(lib, h[:0], t[:0], r[:0], 8, 6).any()
    # one relation over many waves and blocks, every fact repeated
    rng = np.random.RandomState(8)
    h, t = rng.randint(0, 40, 3000), rng.randint(0, 40, 3000)
    h, t, r = np.tile(h, 2), np.tile(t, 2), np.full(6000, 2)
    got = run_stats(lib, h, t, r, 40, 3)
    assert got.tolist() == [[0, 0, 6000], [0, 0, 40], [0, 0, 40]]
