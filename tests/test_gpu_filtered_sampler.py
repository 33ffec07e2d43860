"""GPU tests of filtered negative sampling (run with -m gpu on an MI355X): kge_filtered_corrupt against the pure-Python
restatement of its seven steps (tests/filtered_ref.py) -- ``torch.equal`` on all three outputs, integer work has no
tolerance -- over every list length at which a branch changes, the draws at the edges of the modulo, batch sizes around
the wavefront and the workgroup and one list longer than 2^16 entries; kge_triples_known against Python sets;
``FilteredNegativeSampler`` against the sets of its graph; and a ``Trainer`` run on it."""
import numpy as np
import pytest
import torch

from tests import filtered_ref as ref

pytestmark = pytest.mark.gpu

N_ENT = 37
ALL = list(range(N_ENT))
TOP, NEGATIVE = (1 << 62) - 1, -5        # the largest draw of the sampler; a bit pattern above 2^63


def without(*gone):
    return [e for e in ALL if e not in gone]


# (h, t, the known tails of (h, r), the known heads of (t, r)); c = the free entities of the (tail side, head side)
CATALOGUE = [
    (5, 9, [], []),                                             # both keys absent: c = 36, 36
    (4, 9, [9], [3]),                                           # one entry: the own entity inside / outside
    (36, 0, [0, 36], [0, 36]),                                  # two entries, entity 0 and entity 36, both inside
    (2, 20, [17, 18], [17, 18]),                                # two entries, both outside
    (9, 15, list(range(10, 20)), list(range(10, 20))),          # a run of consecutive ids: inside / just below it
    (20, 10, list(range(10, 20)), list(range(10, 20))),         # ... at its first id / just above it
    (5, 8, without(7, 30), without(0, 36)),                     # 35 entries, inside: two free
    (36, 7, without(7, 30), without(0, 36)),                    # 35 entries, outside: one free (30; 0)
    (36, 0, without(36), without(0)),                           # 36 entries, inside: one free (36; 0)
    (0, 12, without(12), without(0)),                           # 36 entries, outside: none free
    (3, 4, ALL, ALL),                                           # 37 entries: none free
    (3, 4, ALL, []),                                            # exhausted on one side only
]
SENTINEL = 99       # between the segments: a search that left its segment would meet it


def device_lists(lists):
    """One int32 target array of the distinct lists with a sentinel between them, and every list's (lo, hi); the empty
    list is (0, 0), what a lookup gives for an absent key."""
    flat, where = [SENTINEL], []
    for L in lists:
        if not L:
            where.append((0, 0))
            continue
        where.append((len(flat), len(flat) + len(L)))
        flat += list(L) + [SENTINEL]
    return torch.tensor(flat, dtype=torch.int32, device='cuda'), where


def launch(h, t, n_neg, mask, draws, tail_lists, head_lists, n_ent, want_exhausted=True):
    """kge_filtered_corrupt on per-fact Python lists: (neg_h, neg_t, exhausted) as Python lists."""
    from torchkge_amd import _hip_filtered as hf
    tt, tw = device_lists(tail_lists)
    ht, hw = device_lists(head_lists)
    dev = lambda x, dt=torch.int64: torch.tensor(x, dtype=dt, device='cuda')
    nh, nt, ex = hf.filtered_corrupt(dev(h), dev(t), dev(mask, torch.uint8), dev(draws), dev([a for a, _ in tw]),
                                     dev([b for _, b in tw]), tt, dev([a for a, _ in hw]), dev([b for _, b in hw]), ht,
                                     n_ent, n_neg, want_exhausted=want_exhausted)
    return nh, nt, ex


def free_count(x, L, n_ent):
    return n_ent - len(L) - (0 if x in L else 1)


def edge_draws(B, n_neg, h, t, mask, tail_lists, head_lists, n_ent, seed):
    """Per position one of: 0, c - 1, c, 2^62 - 1, a negative bit pattern, a random 62-bit draw -- the kind cycles with
    k, so every fact meets every kind on both sides once n_neg reaches 12."""
    rng = np.random.RandomState(seed)
    out = []
    for p in range(B * n_neg):
        i, k = p % B, p // B
        c = free_count(h[i], head_lists[i], n_ent) if mask[p] else free_count(t[i], tail_lists[i], n_ent)
        out.append([0, c - 1, c, TOP, NEGATIVE, int(rng.randint(0, 1 << 62, dtype=np.int64))][(k // 2 + i) % 6])
    return out


@pytest.mark.parametrize('n_neg', [1, 3, 64])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 257])
def test_kernel_agrees_with_the_restatement_at_every_list_length_and_draw(B, n_neg):
    facts = [CATALOGUE[(i + B) % len(CATALOGUE)] for i in range(B)]
    h, t = [f[0] for f in facts], [f[1] for f in facts]
    tails, heads = [f[2] for f in facts], [f[3] for f in facts]
    mask = [(p // B + (p % B) // len(CATALOGUE)) % 2 for p in range(B * n_neg)]
    draws = edge_draws(B, n_neg, h, t, mask, tails, heads, N_ENT, seed=B * 100 + n_neg)
    want = ref.corrupt(h, t, n_neg, mask, draws, tails, heads, N_ENT)
    nh, nt, ex = launch(h, t, n_neg, mask, draws, tails, heads, N_ENT)
    assert ex.dtype == torch.uint8 and nh.dtype == nt.dtype == torch.int64
    assert torch.equal(nh.cpu(), torch.tensor(want[0])) and torch.equal(nt.cpu(), torch.tensor(want[1]))
    assert torch.equal(ex.cpu(), torch.tensor(want[2], dtype=torch.uint8))
    # the properties themselves, not only the agreement: a replacement is free, an exhausted position keeps its fact
    for p, (a, b, x) in enumerate(zip(*want)):
        i = p % B
        if x:
            assert (a, b) == (h[i], t[i])
        elif mask[p]:
            assert b == t[i] and a != h[i] and a not in heads[i] and 0 <= a < N_ENT
        else:
            assert a == h[i] and b != t[i] and b not in tails[i] and 0 <= b < N_ENT
    if B == 257 and n_neg == 64:        # the largest case meets every catalogue entry exhausted and not, on both sides
        assert {(p % B + B) % len(CATALOGUE) for p, x in enumerate(want[2]) if x} == {9, 10, 11}
        assert sum(want[2]) > 0 and len(set(want[0])) > 30 and len(set(want[1])) > 30
    # without the flag array (NULL) the two id outputs are the same
    nh2, nt2, none = launch(h, t, n_neg, mask, draws, tails, heads, N_ENT, want_exhausted=False)
    assert none is None and torch.equal(nh2, nh) and torch.equal(nt2, nt)


def test_kernel_agrees_with_the_restatement_on_a_list_longer_than_two_to_the_sixteen():
    """n_ent = 70,001 with a list of 65,537 entries: 17 search levels, an index past 2^16."""
    n_ent, m, B, n_neg = 70001, 65537, 4, 8
    rng = np.random.RandomState(5)
    L = np.sort(rng.choice(n_ent, m, replace=False)).tolist()
    known = set(L)
    outside = [e for e in range(n_ent) if e not in known]
    # facts 0, 1: the own entity inside the list (the last entry; one past 2^16); facts 2, 3: outside it (the first and the last free entity)
    h = [L[-1], L[65536 // 2], outside[0], outside[-1]]
    t = [L[0], L[-1], outside[-1], outside[1]]
    tails, heads = [L] * B, [L] * B
    mask = [(p // B + p % B) % 2 for p in range(B * n_neg)]
    draws = edge_draws(B, n_neg, h, t, mask, tails, heads, n_ent, seed=6)
    assert {free_count(x, L, n_ent) for x in h + t} == {n_ent - m, n_ent - m - 1}
    want = ref.corrupt(h, t, n_neg, mask, draws, tails, heads, n_ent)
    nh, nt, ex = launch(h, t, n_neg, mask, draws, tails, heads, n_ent)
    assert torch.equal(nh.cpu(), torch.tensor(want[0])) and torch.equal(nt.cpu(), torch.tensor(want[1]))
    assert torch.equal(ex.cpu(), torch.zeros(B * n_neg, dtype=torch.uint8)) and sum(want[2]) == 0
    for p, (a, b) in enumerate(zip(want[0], want[1])):
        e = a if mask[p] else b
        assert e not in known and e != (h if mask[p] else t)[p % B] and 0 <= e < n_ent
    assert max(max(want[0]), max(want[1])) > (1 << 16)


@pytest.mark.parametrize('side', ['tail', 'head'])
@pytest.mark.parametrize('inside', [True, False])
def test_the_draws_zero_to_c_minus_one_return_the_free_entities_in_ascending_order(side, inside):
    L = [0, 5, 6, 7, 20, 36]
    x = 6 if inside else 21
    free = ref.free_entities(x, L, N_ENT)
    c = len(free)
    assert c == N_ENT - len(L) - (0 if inside else 1)
    other = 3
    h, t = ([other], [x]) if side == 'tail' else ([x], [other])
    tails, heads = ([L], [[1, 2]]) if side == 'tail' else ([[1, 2]], [L])
    nh, nt, ex = launch(h, t, c, [int(side == 'head')] * c, list(range(c)), tails, heads, N_ENT)
    got, kept = (nt, nh) if side == 'tail' else (nh, nt)
    assert got.cpu().tolist() == free and kept.cpu().tolist() == [other] * c and int(ex.sum()) == 0


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
G_ENT, G_REL, G_FACTS = 60, 4, 300


@pytest.fixture(scope='module')
def tk():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import torchkge_amd
    return torchkge_amd


@pytest.fixture(scope='module')
def kg(tk):
    """300 distinct facts over 60 entities and 4 relations, 40 of them the tails of one hub key (0, 0)."""
    g = torch.Generator().manual_seed(21)
    facts = {(0, t, 0) for t in range(1, 41)}
    while len(facts) < G_FACTS:
        h, t, r = (int(torch.randint(0, n, (1,), generator=g)) for n in (G_ENT, G_ENT, G_REL))
        facts.add((h, t, r))
    trip = torch.tensor(sorted(facts))[torch.randperm(G_FACTS, generator=g)]
    return tk.KnowledgeGraph(kg={'heads': trip[:, 0].contiguous(), 'tails': trip[:, 1].contiguous(),
                                 'relations': trip[:, 2].contiguous()},
                             ent2ix={i: i for i in range(G_ENT)}, rel2ix={i: i for i in range(G_REL)})


def fact_set(kg):
    return set(zip(kg.head_idx.tolist(), kg.tail_idx.tolist(), kg.relations.tolist()))


def blocks(kg, nh, nt, batch_size, n_neg):
    """(h, t, r, negative head, negative tail) of every position of a corrupt_kg output (batches laid end to end, each in
    tile order)."""
    nh, nt = nh.cpu().tolist(), nt.cpu().tolist()
    h, t, r = kg.head_idx.tolist(), kg.tail_idx.tolist(), kg.relations.tolist()
    out, at = [], 0
    for lo in range(0, kg.n_facts, batch_size):
        b = min(batch_size, kg.n_facts - lo)
        for p in range(b * n_neg):
            i = lo + p % b
            out.append((h[i], t[i], r[i], nh[at + p], nt[at + p]))
        at += b * n_neg
    return out


def test_known_agrees_with_a_python_set_on_a_thousand_triples(tk, kg):
    from torchkge_amd.sampling import FilteredNegativeSampler
    facts = fact_set(kg)
    g = torch.Generator().manual_seed(8)
    pick = torch.randint(0, G_FACTS, (500,), generator=g)
    h = torch.cat([kg.head_idx[pick], torch.randint(0, G_ENT, (500,), generator=g)])
    t = torch.cat([kg.tail_idx[pick], torch.randint(0, G_ENT, (500,), generator=g)])
    r = torch.cat([kg.relations[pick], torch.randint(0, G_REL, (500,), generator=g)])
    want = [(a, b, c) in facts for a, b, c in zip(h.tolist(), t.tolist(), r.tolist())]
    keys = {(a, c) for a, _, c in facts}
    assert sum(want) >= 500 and sum((a, c) not in keys for a, c in zip(h.tolist(), r.tolist())) > 20     # absent keys too
    got = FilteredNegativeSampler(kg).known(h.cuda(), t.cuda(), r.cuda())
    assert got.dtype == torch.bool and got.cpu().tolist() == want


def test_no_negative_of_the_sampler_is_a_fact_and_the_bernoulli_samplers_are(tk, kg):
    from torchkge_amd.sampling import FilteredNegativeSampler
    facts = fact_set(kg)
    sampler = FilteredNegativeSampler(kg)
    assert sampler.exhaustible == 0
    torch.manual_seed(3)
    nh, nt = sampler.corrupt_kg(128, True, on_device=True, n_neg=4)
    assert nh.is_cuda and nh.shape == nt.shape == (4 * G_FACTS,) and sampler.last_exhausted is None
    heads = 0
    for h, t, r, a, b in blocks(kg, nh, nt, 128, 4):
        assert (a, b, r) not in facts and (a, b) != (h, t)
        assert (a == h) != (b == t) and 0 <= a < G_ENT and 0 <= b < G_ENT       # exactly one place replaced
        heads += a != h
    assert 0 < heads < 4 * G_FACTS
    rep = kg.relations.cuda()
    rep = torch.cat([rep[lo:lo + 128].repeat(4) for lo in range(0, G_FACTS, 128)])
    assert int(sampler.known(nh, nt, rep).sum()) == 0
    # the same seed gives the same samples
    torch.manual_seed(3)
    nh2, nt2 = sampler.corrupt_kg(128, True, on_device=True, n_neg=4)
    assert torch.equal(nh, nh2) and torch.equal(nt, nt2)
    torch.manual_seed(4)
    nh3, _ = sampler.corrupt_kg(128, True, on_device=True, n_neg=4)
    assert not torch.equal(nh, nh3)
    # bernoulli=False draws the side with probability 1 / 2 and filters the same way
    nhu, ntu = FilteredNegativeSampler(kg, bernoulli=False, n_neg=2).corrupt_kg(128, True, on_device=True, n_neg=2)
    assert nhu.shape == (2 * G_FACTS,) and all((a, b, r) not in facts for _, _, r, a, b in blocks(kg, nhu, ntu, 128, 2))
    # what the feature is for: the unfiltered sampler hands out known facts on the same graph
    bern = tk.BernoulliNegativeSampler(kg)
    bern.sync_free = True
    torch.manual_seed(3)
    bh, bt = bern.corrupt_kg(128, True, on_device=True, n_neg=4)
    flagged = sampler.known(bh, bt, rep).cpu().tolist()
    assert flagged == [(a, b, r) in facts for _, _, r, a, b in blocks(kg, bh, bt, 128, 4)]
    print('Bernoulli sampler: %d of %d negatives are train facts' % (sum(flagged), len(flagged)))
    assert sum(flagged) > 0


def test_exhausted_positions_keep_their_fact_and_are_flagged(tk):
    """A graph whose key (0, 0) knows every entity but one as a tail: replacing the tail of (0, 0, t) has one free entity
    when t is known -- and the head side of a tail that every entity points to has none."""
    from torchkge_amd.sampling import FilteredNegativeSampler
    n_ent = 6
    h = [0] * 5 + list(range(1, 6))
    t = list(range(5)) + [0] * 5
    kg = tk.KnowledgeGraph(kg={'heads': torch.tensor(h), 'tails': torch.tensor(t), 'relations': torch.zeros(10, dtype=torch.int64)},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={0: 0})
    sampler = FilteredNegativeSampler(kg)
    assert sampler.exhaustible == 2             # (0, r0) -> 5 tails; tail 0 of r0 <- all 6 heads
    hd, td, rd = kg.head_idx.cuda(), kg.tail_idx.cuda(), kg.relations.cuda()
    torch.manual_seed(1)
    nh, nt = sampler.corrupt_batch(hd, td, rd, n_neg=16)
    ex = sampler.last_exhausted
    assert ex is not None and ex.dtype == torch.uint8 and ex.shape == (160,)
    facts = fact_set(kg)
    seen = 0
    for p, (a, b, x) in enumerate(zip(nh.cpu().tolist(), nt.cpu().tolist(), ex.cpu().tolist())):
        i = p % 10
        if x:       # only a head replacement of a fact with tail 0 can be exhausted
            assert (a, b) == (h[i], t[i]) and t[i] == 0
            seen += 1
        else:
            assert (a, b, 0) not in facts and (a == h[i]) != (b == t[i])
            if h[i] == 0 and b != t[i]:
                assert b == 5       # the one free tail of (0, r0)
    assert seen > 0


# ---------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------
DIM, N_NEG, B_SIZE, N_EPOCHS = 8, 4, 128, 2


def trainer(tk, kg, sync_free, seed=0, lr=0.01):
    from torchkge_amd.sampling import FilteredNegativeSampler
    from torchkge_amd.utils.group_losses import SelfAdversarialLoss
    from torchkge_amd.utils.training import Trainer
    torch.manual_seed(seed)
    model = tk.TransEModel(DIM, G_ENT, G_REL, 'L2').cuda()
    return Trainer(model, SelfAdversarialLoss(2.0, 0.5), kg, N_EPOCHS, B_SIZE, torch.optim.SGD(model.parameters(), lr=lr),
                   use_cuda='all', sampler=FilteredNegativeSampler(kg), verbose=False, sync_free=sync_free, n_neg=N_NEG)


def tables(tr):
    return [p.detach().clone() for p in tr.model.parameters()]


def test_a_sync_free_trainer_run_reads_nothing_back_and_its_losses_decrease(tk, kg):
    tr = trainer(tk, kg, True)
    assert tr._check_negatives is False             # one of the package's own samplers
    tr.run()                    # the warm-up: library loading, the graph's upload, the index build (its one host read)
    first = tr.epoch_losses
    torch.cuda.set_sync_debug_mode('error')
    try:
        tr.run()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert tr._loader.sampler.sync_free is True and tr._epoch_sums is not None
    losses = first + tr.epoch_losses
    print('filtered sampler, TransE d = 8, n_neg = 4: epoch losses', losses)
    assert len(losses) == 2 * N_EPOCHS and np.isfinite(losses).all()
    assert first[1] < first[0] and losses[-1] < losses[0]


def test_two_deterministic_runs_give_the_same_table_bits(tk, kg):
    out = []
    with tk.deterministic():
        for _ in range(2):
            tr = trainer(tk, kg, True, seed=5)
            torch.manual_seed(9)
            tr.run()
            out.append((tr.epoch_losses, tables(tr)))
    assert out[0][0] == out[1][0]
    for x, y in zip(out[0][1], out[1][1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_the_grouped_forward_runs_with_the_contract_check_on(tk, kg):
    tr = trainer(tk, kg, False)
    tr.grouped_forward = True
    tr._check_negatives = True          # what a sampler from elsewhere gets: every step checks its negatives
    tr.run()
    assert len(tr.epoch_losses) == N_EPOCHS and np.isfinite(tr.epoch_losses).all()
