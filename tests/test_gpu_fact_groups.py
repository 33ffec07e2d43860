"""GPU tests of the grouped scorer of torchkge_amd/csrc/score_fact_groups.hip (include/kge_hip_factgroup.h; run with
-m gpu on an MI355X): kge_score_fact_groups and kge_score_fact_groups_bwd for the ten kinds they serve.

Forward: pos and neg are BIT-equal to kge_score_triples on the concatenated B (K + 1) triples -- every kind, both
register buckets on both load paths, B and K on both sides of the block's four wavefronts (empty slices, ragged
slices), corruption all-head / all-tail / mixed, negatives equal to the fact's own entities, facts with h == t, one
entity as every negative of a fact, a padded score matrix whose pad must keep its NaN payload.

Backward: the reference, the metric and the bound are those of tests/test_gpu_triple_kernels.py -- the float64 autograd
restatement over the concatenated triples with the gathered rows as leaves, per table |got - ref| <= GRAD_TOL S_rho with
S_rho the summed scales of the triples that hit row rho, rows nothing hits bit-zero (``Case``) -- applied to the tables
the rows buffer reduces to; the same tables from kge_score_triples_bwd must lie within the same bound of them.  A fact
row's gradient is here ONE sum over up to K + 1 triples with the normalisation's derivative applied to the sum; the
bound already scales with the number of triples that hit a row, so it is not widened.

For TransE-L1 the go of every triple inside the kink band is zeroed by ``Case`` (l1_kinks, at most 3 % of the batch;
the seeds below stay under it in float64 alone -- checked on the CPU, where ``Case`` runs without a GPU); the TorusE
reference takes its branches on the fp32 x, as there."""
import pytest
import torch

from tests.helpers import raw, carve
from tests.test_gpu_triple_kernels import KINDS, CODE, SENTINEL, Case, bits, make_tables
from tests.test_gpu_layout_contract import GRAD_TOL

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -3
N_ENT, N_REL = 50, 5
WIDTHS = [1, 5, 64, 200, 203, 260, 512]
# (B, K, corruption, pad of the score matrix): B in {1, 7, 300}, K in {1, 2, 5, 67}; K = 1, 2, 3 leave wavefronts of the
# block without a negative, 5 and 67 are no multiple of the four; 129 and 300 are two and three chunks of the forward
# (64 + 65 negatives, whose second has ragged slices; 100 each)
SHAPES = [(1, 1, 'mixed', 0), (1, 67, 'head', 3), (7, 2, 'tail', 1), (7, 3, 'mixed', 0), (7, 5, 'mixed', 5), (300, 1, 'mixed', 0),
          (300, 2, 'head', 4), (300, 5, 'tail', 0), (300, 67, 'mixed', 1), (1, 129, 'tail', 0), (7, 300, 'mixed', 2)]
BWD_KINDS = ['transe_l1', 'transe_l2', 'transh', 'complex', 'transd', 'toruse_tl2', 'distmult']
BWD_WIDTHS = [5, 64, 203, 260]


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


@pytest.fixture(scope='module')
def fg(hip):
    from torchkge_amd import _hip_factgroup
    _hip_factgroup.load_library()
    return _hip_factgroup


def make_groups(B, K, g, corruption='mixed', n_ent=N_ENT, n_rel=N_REL):
    """(h, t, r, neg_h, neg_t) on the host, inside the contract: facts with h == t, a fact whose negatives are all one
    entity, negatives equal to the fact's own head / tail (the fact itself, and (t, r, t) / (h, r, h))."""
    h = torch.randint(0, n_ent, (B,), generator=g)
    t = torch.randint(0, n_ent, (B,), generator=g)
    r = torch.randint(0, n_rel, (B,), generator=g)
    t[::5] = h[::5]                                                 # h == t (fact 0 included)
    draw = torch.randint(0, n_ent, (K, B), generator=g)
    if B > 1:
        draw[:, 1] = 7                                              # one entity as every negative of fact 1
    draw[0, ::3] = h[::3]                                           # the fact's own head as the replacement ...
    if K > 1:
        draw[1, ::4] = t[::4]                                       # ... and its own tail
    head = {'head': torch.ones(K, B, dtype=torch.bool), 'tail': torch.zeros(K, B, dtype=torch.bool),
            'mixed': torch.rand(K, B, generator=g) < 0.5}[corruption]
    nh = torch.where(head, draw, h.expand(K, B)).reshape(-1)
    nt = torch.where(head, t.expand(K, B), draw).reshape(-1)
    assert not bool(((nh != h.repeat(K)) & (nt != t.repeat(K))).any())
    return h, t, r, nh, nt


def concat(h, t, r, nh, nt):
    K = nh.shape[0] // h.shape[0]
    return torch.cat([h, nh]), torch.cat([t, nt]), torch.cat([r, r.repeat(K)])


def tables_for(kind, de, dr, seed, off=0):
    g = torch.Generator().manual_seed(seed)
    tabs = make_tables(kind, de, dr, g, N_ENT, N_REL)
    if off:
        tabs = [carve(x, 0, off, device='cuda') for x in tabs]
        assert all(x.is_contiguous() and x.data_ptr() % 16 == 4 * off for x in tabs)
        return tabs, g
    return [x.cuda() for x in tabs], g


def raw_forward(fg, kind, tabs, de, dr, h, t, r, nh, nt, pad=0):
    """kge_score_fact_groups through the C entry into sentinel-filled outputs: (rc, pos, neg as (K, B + pad))."""
    B, K = h.shape[0], nh.shape[0] // h.shape[0]
    pos = torch.full((B,), SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)
    neg = torch.full((K, B + pad), SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)
    tb = list(tabs) + [None] * (4 - len(tabs))
    rc = raw(fg.load_library(), 'kge_score_fact_groups', CODE[kind], tb[0], tb[1], tb[2], tb[3], de, dr, h, t, r, B, nh, nt, K,
             pos, neg, B + pad)
    return rc, pos, neg


def check_forward(hip, fg, kind, tabs, de, dr, groups, pad, tag):
    h, t, r, nh, nt = (x.cuda() for x in groups)
    B = h.shape[0]
    H, T, R = concat(h, t, r, nh, nt)
    want = hip.score_triples(CODE[kind], tabs, de, dr, H, T, R)
    rc, pos, neg = raw_forward(fg, kind, tabs, de, dr, h, t, r, nh, nt, pad)
    assert rc == 0, (tag, rc)
    assert bool(torch.isfinite(want).all()), tag
    assert torch.equal(bits(pos), bits(want[:B])), (tag, 'pos')
    assert torch.equal(bits(neg[:, :B]), bits(want[B:].view(-1, B))), (tag, 'neg', int((bits(neg[:, :B]) != bits(want[B:].view(-1, B))).sum()))
    assert bool((bits(neg[:, B:]) == SENTINEL).all()), (tag, 'the pad of the score matrix was written')
    return pos, neg


# ---------------------------------------------------------------------------
# forward: the bits of kge_score_triples
# ---------------------------------------------------------------------------
def forward_params():
    out = [pytest.param(kind, d, d, 0, id='%s-%d' % (kind, d)) for kind in KINDS for d in WIDTHS]
    out += [pytest.param(kind, 64, 64, 1, id='%s-64-one-float-off' % kind) for kind in KINDS]
    out += [pytest.param('transd', 64, 24, 0, id='transd-64-24'), pytest.param('transd', 260, 5, 0, id='transd-260-5')]
    return out


@pytest.mark.parametrize('kind,de,dr,off', forward_params())
def test_forward_scores_are_bit_equal_to_kge_score_triples(hip, fg, kind, de, dr, off):
    tabs, g = tables_for(kind, de, dr, 7919 * CODE[kind] + 31 * de + dr + off, off)
    for B, K, corruption, pad in SHAPES:
        groups = make_groups(B, K, g, corruption)
        if B >= 7:
            assert bool((groups[0] == groups[1]).any())
        check_forward(hip, fg, kind, tabs, de, dr, groups, pad, '%s d %d/%d B %d K %d %s' % (kind, de, dr, B, K, corruption))


@pytest.mark.parametrize('kind', KINDS)
def test_wrapper_returns_flat_tile_order_and_the_sixteen_register_bucket_is_refused(hip, fg, kind):
    """The Python wrapper's (pos, neg) at d = 200; at d = 516 (the 16-register bucket) the C entries answer
    KGE_EUNSUPPORTED, write nothing, and the wrapper raises Unsupported."""
    tabs, g = tables_for(kind, 200, 200, 11 + CODE[kind])
    h, t, r, nh, nt = (x.cuda() for x in make_groups(40, 9, g))
    H, T, R = concat(h, t, r, nh, nt)
    want = hip.score_triples(CODE[kind], tabs, 200, 200, H, T, R)
    pos, neg = fg.score_fact_groups(CODE[kind], tabs, 200, 200, h, t, r, nh, nt)
    assert pos.shape == (40,) and neg.shape == (360,)
    assert torch.equal(bits(pos), bits(want[:40])) and torch.equal(bits(neg), bits(want[40:]))
    tabs, g = tables_for(kind, 516, 516, 13 + CODE[kind])
    rc, pos, neg = raw_forward(fg, kind, tabs, 516, 516, h, t, r, nh, nt)
    assert rc == EUNSUPPORTED
    rows = torch.full((fg.rows_per_fact(CODE[kind], 9) * 40, 516), SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)
    ids = torch.full((40 * 11,), -77, dtype=torch.int64, device='cuda')
    tb = list(tabs) + [None] * (4 - len(tabs))
    go = torch.ones(400, device='cuda')
    assert raw(fg.load_library(), 'kge_score_fact_groups_bwd', CODE[kind], tb[0], tb[1], tb[2], tb[3], 516, 516, h, t, r, 40, nh, nt,
               9, go[:40], go[40:], 40, rows, 516, ids) == EUNSUPPORTED
    with pytest.raises(fg.Unsupported):
        fg.score_fact_groups(CODE[kind], tabs, 516, 516, h, t, r, nh, nt)
    torch.cuda.synchronize()
    for x in (pos, neg, rows):
        assert bool((bits(x) == SENTINEL).all())
    assert bool((ids == -77).all())
    # ... and the triples are still scored by the general path
    assert bool(torch.isfinite(hip.score_triples(CODE[kind], tabs, 516, 516, H, T, R)).all())


@pytest.mark.parametrize('kind', ['transe_l2', 'complex', 'transd', 'toruse_tl1'])
def test_a_negative_that_breaks_the_contract_is_scored_with_the_facts_tail(hip, fg, kind):
    """Both head and tail differ: an ordinary in-bounds input, scored as (neg_h, r, t) as the header says, neg_t unused."""
    de, dr = 64, (24 if kind == 'transd' else 64)
    tabs, g = tables_for(kind, de, dr, 17 + CODE[kind])
    B, K = 7, 5
    h, t, r, nh, nt = make_groups(B, K, g)
    broken = torch.zeros(K * B, dtype=torch.bool)
    broken[[2, 9, 17, 30]] = True
    nh = torch.where(broken, (h.repeat(K) + 1) % N_ENT, nh)
    nt = torch.where(broken, (t.repeat(K) + 2) % N_ENT, nt)
    assert bool(((nh != h.repeat(K)) & (nt != t.repeat(K)))[broken].all())
    h, t, r, nh, nt = (x.cuda() for x in (h, t, r, nh, nt))
    rc, pos, neg = raw_forward(fg, kind, tabs, de, dr, h, t, r, nh, nt)
    assert rc == 0
    as_doc = torch.where(broken.cuda(), t.repeat(K), nt)
    H, T, R = concat(h, t, r, nh, as_doc)
    want = hip.score_triples(CODE[kind], tabs, de, dr, H, T, R)
    assert torch.equal(bits(pos), bits(want[:B])) and torch.equal(bits(neg.view(-1)), bits(want[B:]))


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
def group_case(kind, de, dr, B, K, seed, device='cuda'):
    """``Case`` of tests/test_gpu_triple_kernels.py over the concatenated triples of B facts with K negatives, go =
    [go_pos | go_neg] with a few exact zeros; returns (case, groups on the device)."""
    g = torch.Generator().manual_seed(seed)
    tabs = [x.to(device) for x in make_tables(kind, de, dr, g, N_ENT, N_REL)]
    groups = make_groups(B, K, g)
    go = torch.randn(B * (K + 1), generator=g)
    go[::11] = 0
    groups = tuple(x.to(device) for x in groups)
    H, T, R = concat(*groups)
    tag = '%s d %d/%d B %d K %d' % (kind, de, dr, B, K)
    return Case(kind, tabs, de, dr, H, T, R, go.to(device), tag), groups


def bwd_seed(kind, de, dr, B, K):
    return 104729 * CODE[kind] + 31 * de + dr + 7 * B + K


def backward_params():
    out = [pytest.param(kind, d, d, id='%s-%d' % (kind, d)) for kind in BWD_KINDS for d in BWD_WIDTHS]
    return out + [pytest.param('transd', 64, 24, id='transd-64-24')]


BWD_SHAPES = [(37, 6), (5, 67), (9, 3)]


def rows_views(fg, kind, rows, ld, B, K):
    """The blocks of the rows buffer: [(table, (n, ld) view, is an entity block)]."""
    ent, rel = fg.tables_of(CODE[kind])
    rows = rows.view(-1, ld)
    n = (K + 2) * B
    out = [(ti, rows[s * n:(s + 1) * n], True) for s, ti in enumerate(ent)]
    return out + [(ti, rows[len(ent) * n + q * B:len(ent) * n + (q + 1) * B], False) for q, ti in enumerate(rel)]


@pytest.mark.parametrize('kind,de,dr', backward_params())
def test_backward_vs_float64_autograd_and_vs_kge_score_triples_bwd(hip, fg, monkeypatch, kind, de, dr):
    for B, K in BWD_SHAPES:
        case, (h, t, r, nh, nt) = group_case(kind, de, dr, B, K, bwd_seed(kind, de, dr, B, K))
        nt_ = len(case.tabs)
        go_pos, go_neg = case.go[:B].contiguous(), case.go[B:].contiguous()
        grads = fg.score_fact_groups_bwd(CODE[kind], case.tabs, de, dr, h, t, r, nh, nt, go_pos, go_neg, (True,) * nt_)
        case.check_grads(grads, 'fact groups')
        # the existing backward over the concatenated triples, reduced per table: within the same bound of each other
        monkeypatch.setattr(hip, 'BWD_SORTED_MIN_BATCH', 0)
        old = hip.score_triples_bwd(CODE[kind], case.tabs, de, dr, case.h, case.t, case.r, case.go, (True,) * nt_)
        for X, (a, b) in enumerate(zip(grads, old)):
            S = case.rows[X][1]
            err = (a.double() - b.double()).abs().amax(1)
            assert bool((err <= GRAD_TOL * S).all()), (case.tag, 'table', X, float((err / S.clamp_min(1e-300)).max()))
        # the rows buffer: the id vector of the contract, the row counts of the header
        rows, ids, ld = fg.fact_group_rows(CODE[kind], case.tabs, de, dr, h, t, r, nh, nt, go_pos, go_neg)
        head = nh != h.repeat(K)
        assert torch.equal(ids, torch.cat([h, t, torch.where(head, nh, nt)]))
        assert rows.numel() == B * fg.rows_per_fact(CODE[kind], K) * ld and ids.numel() == B * (K + 2)
        # ... reduced on the host in float64 it gives the same tables (what is in the buffer is what the wrapper summed)
        for ti, blk, is_ent in rows_views(fg, kind, rows, ld, B, K):
            d = case.tabs[ti].shape[1]
            keys = ids if is_ent else r
            ref = torch.zeros(case.tabs[ti].shape, dtype=torch.float64).index_add_(0, keys.cpu(), blk[:, :d].double().cpu())
            err = (grads[ti].double().cpu() - ref).abs().amax(1)
            assert bool((err <= GRAD_TOL * case.rows[ti][1].cpu()).all()), (case.tag, 'rows buffer of table', ti)


@pytest.mark.parametrize('kind,de,dr', [('transe_l2', 200, 200), ('transh', 64, 64), ('complex', 203, 203), ('transd', 64, 24),
                                        ('toruse_tl2', 5, 5), ('distmult', 260, 260)])
def test_two_runs_give_the_same_bits_and_a_fact_does_not_depend_on_its_batch(hip, fg, kind, de, dr):
    """Determinism: the forward and the rows buffer of two runs are bit-identical.  Independence: the facts [a, b) run
    alone give the bits they have inside the batch -- pos, neg and every gradient row."""
    tabs, g = tables_for(kind, de, dr, 23 + CODE[kind])
    B, K, a, b = 41, 7, 13, 30
    h, t, r, nh, nt = (x.cuda() for x in make_groups(B, K, g))
    go = torch.randn(B * (K + 1), generator=g).cuda()
    code = CODE[kind]

    def run(h, t, r, nh, nt, gp, gn):
        pos, neg = fg.score_fact_groups(code, tabs, de, dr, h, t, r, nh, nt)
        rows, ids, ld = fg.fact_group_rows(code, tabs, de, dr, h, t, r, nh, nt, gp, gn)
        return pos, neg, rows, ids, ld
    gp, gn = go[:B].contiguous(), go[B:].contiguous()
    one, two = run(h, t, r, nh, nt, gp, gn), run(h, t, r, nh, nt, gp, gn)
    assert torch.equal(bits(one[0]), bits(two[0])) and torch.equal(bits(one[1]), bits(two[1])) and torch.equal(one[3], two[3])
    for (ti, x, _), (_, y, _) in zip(rows_views(fg, kind, one[2], one[4], B, K), rows_views(fg, kind, two[2], two[4], B, K)):
        d = tabs[ti].shape[1]       # (a relation row of TransD is d_rel floats: the rest of the row is never written)
        assert torch.equal(bits(x[:, :d]), bits(y[:, :d])), (kind, 'table', ti)

    def cut(x):
        return x.view(K, B)[:, a:b].reshape(-1).contiguous()
    sub = run(h[a:b].contiguous(), t[a:b].contiguous(), r[a:b].contiguous(), cut(nh), cut(nt), gp[a:b].contiguous(), cut(gn))
    n = b - a
    assert torch.equal(bits(sub[0]), bits(one[0][a:b]))
    assert torch.equal(bits(sub[1]), bits(cut(one[1])))
    assert torch.equal(sub[3].view(K + 2, n), one[3].view(K + 2, B)[:, a:b])
    ld = one[4]
    for (ti, big, is_ent), (_, small, _) in zip(rows_views(fg, kind, one[2], ld, B, K), rows_views(fg, kind, sub[2], ld, n, K)):
        d = tabs[ti].shape[1]
        big = big.view(K + 2, B, ld)[:, a:b] if is_ent else big[a:b]
        small = small.view(K + 2, n, ld) if is_ent else small
        assert torch.equal(bits(small[..., :d]), bits(big[..., :d])), (kind, 'table', ti)
