"""GPU tests of torchkge_amd.utils.training (run with -m gpu on an MI355X): the reference's recorded training loop
(tests/golden/ref_trainer.npz) replayed through Trainer on both criterion paths; Trainer(fused=False) bit for bit against
the tutorial loop written out here; the fused path against the generic one under a bound taken from a float64 run of the
same loop in plain torch; a ``sync_free`` run under torch's sync debug mode; and the counter-examples API.

The bound on trained tables is the project's usual one: 4 * (2 * |fp32 run - fp64 run| + one ulp of the largest
entry), in max-norm over all tables; on mean losses the same rule relative to the loss, with the ulp of 1.0."""
import os

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests import convkb_ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

ULP1 = 2.0 ** -23
FIXTURE_CASES = {
    'transe': ('MarginLoss', ('ent_emb', 'rel_emb')),
    'distmult': ('LogisticLoss', ('ent_emb', 'rel_emb')),
    'complex': ('BinaryCrossEntropyLoss', ('re_ent_emb', 'im_ent_emb', 're_rel_emb', 'im_rel_emb')),
}


@pytest.fixture(scope='module')
def tk():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import torchkge_amd
    return torchkge_amd


@pytest.fixture(scope='module')
def Z():
    return np.load(os.path.join(GOLDEN, 'ref_trainer.npz'))


def ulp_of(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def make_kg(tk, heads, tails, rels, n_ent, n_rel):
    return tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels}, ent2ix={i: i for i in range(n_ent)},
                             rel2ix={i: i for i in range(n_rel)})


class Replay(object):
    """A sampler that hands out recorded negatives, epoch after epoch; they lie on the device from the start."""

    def __init__(self, epochs):
        self.host = [(nh.long(), nt.long()) for nh, nt in epochs]
        self.dev = [(nh.cuda(), nt.cuda()) for nh, nt in self.host]
        self.calls, self.sync_free = 0, False

    def corrupt_kg(self, batch_size, use_cuda, which='main', on_device=False):
        i = self.calls % len(self.host)
        self.calls += 1
        return self.dev[i] if on_device else self.host[i]


def criterion_of(tk, name, margin=0.5):
    from torchkge_amd.utils import losses
    return losses.MarginLoss(margin) if name == 'MarginLoss' else getattr(losses, name)()


def tables_of(model, names):
    return [getattr(model, nm).weight.detach().cpu() for nm in names]


def table_bound(ref32, ref64):
    """4 * (2 * |ref32 - ref64| + one ulp of the largest entry), max-norm over the tables; also the distance itself."""
    dist = max(float((a.double() - b.double()).abs().max()) for a, b in zip(ref32, ref64))
    return 4 * (2 * dist + ulp_of(max(float(b.abs().max()) for b in ref64))), dist


def distance(tables, ref64):
    return max(float((a.double() - b.double()).abs().max()) for a, b in zip(tables, ref64))


# ---------------------------------------------------------------------------
# 1. the reference's recorded loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'generic'])
@pytest.mark.parametrize('case', sorted(FIXTURE_CASES))
def test_replay_of_the_reference_training_loop(tk, Z, case, fused):
    from torchkge_amd.utils.training import Trainer
    crit_name, names = FIXTURE_CASES[case]
    n_ent, n_rel, dim, b_size, n_epochs = (int(Z[k]) for k in ('n_ent', 'n_rel', 'dim', 'b_size', 'n_epochs'))
    kg = make_kg(tk, *(torch.from_numpy(Z[k]) for k in ('heads', 'tails', 'rels')), n_ent, n_rel)
    model = {'transe': lambda: tk.TransEModel(dim, n_ent, n_rel, 'L2'), 'distmult': lambda: tk.DistMultModel(dim, n_ent, n_rel),
             'complex': lambda: tk.ComplExModel(dim, n_ent, n_rel)}[case]()
    for i, nm in enumerate(names):
        getattr(model, nm).weight.data = torch.from_numpy(Z['%s_init%d' % (case, i)]).clone()
    model = model.cuda()
    sampler = Replay([(torch.from_numpy(Z[case + '_nh32'][e]), torch.from_numpy(Z[case + '_nt32'][e])) for e in range(n_epochs)])
    trainer = Trainer(model, criterion_of(tk, crit_name, float(Z['margin'])), kg, n_epochs, b_size,
                      torch.optim.SGD(model.parameters(), lr=float(Z['lr'])), use_cuda='all', fused=fused, sampler=sampler,
                      verbose=False)
    assert (trainer._fused_criterion is not None) == fused
    trainer.run()
    assert sampler.calls == n_epochs
    ref32 = [torch.from_numpy(Z['%s_final32_%d' % (case, i)]) for i in range(len(names))]
    ref64 = [torch.from_numpy(Z['%s_final64_%d' % (case, i)]) for i in range(len(names))]
    bound, ref_dist = table_bound(ref32, ref64)
    got = distance(tables_of(model, names), ref64)
    l32, l64 = Z[case + '_loss32'], Z[case + '_loss64']
    losses = np.array(trainer.epoch_losses)
    loss_bound = 4 * (2 * np.abs(l32 - l64) / l64 + ULP1)
    loss_dist = np.abs(losses - l64) / l64
    print('trainer replay %-8s %-7s tables |engine - ref64| %.3g (ref32 %.3g, bound %.3g); mean losses relative %.3g '
          '(ref32 %.3g, bound %.3g)' % (case, 'fused' if fused else 'generic', got, ref_dist, bound, loss_dist.max(),
                                        (np.abs(l32 - l64) / l64).max(), loss_bound.min()))
    assert got <= bound
    assert losses.shape == (n_epochs,) and bool((loss_dist <= loss_bound).all())
    ce = trainer.get_counter_examples()
    assert torch.equal(ce.head_idx.cpu(), sampler.host[-1][0]) and torch.equal(ce.tail_idx.cpu(), sampler.host[-1][1])


# ---------------------------------------------------------------------------
# a small graph for the rest: 500 entities, d = 40, B = 512, two epochs, a short last batch
# ---------------------------------------------------------------------------
N_ENT, N_REL, DIM, N_FACTS, B_SIZE, N_EPOCHS, LR = 500, 9, 40, 1200, 512, 2, 0.01
BUILD = {
    'transe': lambda tk: tk.TransEModel(DIM, N_ENT, N_REL, 'L2'),
    'complex': lambda tk: tk.ComplExModel(DIM, N_ENT, N_REL),
    'analogy': lambda tk: tk.AnalogyModel(DIM, N_ENT, N_REL),
    'convkb': lambda tk: tk.ConvKBModel(DIM, 3, N_ENT, N_REL),
}


def graph(tk):
    h, t, r = orc.synthetic_triples(N_ENT, N_REL, N_FACTS, 5)
    return make_kg(tk, h, t, r, N_ENT, N_REL)


def build(tk, name, seed=0):
    torch.manual_seed(seed)
    return BUILD[name](tk).cuda()


def optimizer_of(tk, model, row):
    from torchkge_amd import optim
    return optim.RowAdagrad(model.parameters(), lr=0.05) if row else torch.optim.SGD(model.parameters(), lr=LR)


def host_negatives(kg, seed):
    """Recorded negatives made on the host: every fact has its head or its tail replaced."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(N_EPOCHS):
        side = torch.rand(kg.n_facts, generator=g) < 0.5
        draw = torch.randint(0, N_ENT, (kg.n_facts,), generator=g)
        out.append((torch.where(side, draw, kg.head_idx), torch.where(side, kg.tail_idx, draw)))
    return out


# ---------------------------------------------------------------------------
# 2. the generic path IS the tutorial loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name,row', [('transe', False), ('analogy', False), ('transe', True)],
                         ids=['transe', 'analogy', 'transe-RowAdagrad'])
def test_the_generic_path_is_the_tutorial_loop_bit_for_bit(tk, name, row):
    from torchkge_amd.utils.training import Trainer
    kg = graph(tk)
    crit = tk.MarginLoss(0.5)
    # (the row path is bit-reproducible by itself; the dense one under the deterministic switch)
    with tk.deterministic(not row):
        model = build(tk, name)
        torch.manual_seed(77)
        trainer = Trainer(model, crit, kg, N_EPOCHS, B_SIZE, optimizer_of(tk, model, row), sampling_type='bern',
                          use_cuda='all', fused=False, verbose=False)
        trainer.run()

        hand = build(tk, name)
        opt = optimizer_of(tk, hand, row)
        sampler = tk.BernoulliNegativeSampler(kg)
        H, T, R = kg.head_idx.cuda(), kg.tail_idx.cuda(), kg.relations.cuda()
        torch.manual_seed(77)
        means = []
        for _ in range(N_EPOCHS):
            nh, nt = sampler.corrupt_kg(B_SIZE, True, on_device=True)
            total = 0
            for lo in range(0, kg.n_facts, B_SIZE):
                sl = slice(lo, lo + B_SIZE)
                with tk.row_gradients(row):
                    opt.zero_grad()
                    p, n = hand(H[sl], T[sl], R[sl], nh[sl], nt[sl])
                    loss = crit(p, n)
                    loss.backward()
                    opt.step()
                total += loss.item()
            means.append(total / 3)
            hand.normalize_parameters()
    assert hand.ent_emb.weight.grad.is_sparse == row if name == 'transe' else True
    for a, b in zip(model.parameters(), hand.parameters()):
        assert torch.equal(a.detach(), b.detach())
    ce = trainer.get_counter_examples()
    assert torch.equal(ce.head_idx, nh) and torch.equal(ce.tail_idx, nt) and torch.equal(ce.relations, R)
    assert not torch.equal(nh, H) and trainer.epoch_losses == means


# ---------------------------------------------------------------------------
# 3. fused against generic
# ---------------------------------------------------------------------------
FUSED_CASES = {'transe': 'MarginLoss', 'complex': 'BinaryCrossEntropyLoss', 'convkb': 'LogisticLoss'}
MIN_HINGE = 1e-4


def plain_float64_loop(tk, name, crit, init, kg, negatives):
    """The generic loop in plain torch on the host, float64: the oracle's scores (tests/convkb_ref.py for ConvKB) under
    autograd, SGD written out, TransE's normalisation after every epoch.  Returns the tables and the smallest
    |margin - p + n| met (inf without a margin)."""
    tabs = [x.double().clone().requires_grad_() for x in init]
    min_hinge = float('inf')
    for nh, nt in negatives:
        for lo in range(0, kg.n_facts, B_SIZE):
            sl = slice(lo, lo + B_SIZE)
            h, t, r = torch.cat([kg.head_idx[sl], nh[sl]]), torch.cat([kg.tail_idx[sl], nt[sl]]), kg.relations[sl].repeat(2)
            s = convkb_ref.sf64(tabs, h, t, r) if name == 'convkb' else orc.score_triples(name, tabs, h, t, r)
            b = s.shape[0] // 2
            if hasattr(crit, 'margin'):
                min_hinge = min(min_hinge, float((crit.margin - s[:b] + s[b:]).detach().abs().min()))
            grads = torch.autograd.grad(crit(s[:b], s[b:]), tabs)
            with torch.no_grad():
                for x, g in zip(tabs, grads):
                    x -= LR * g
        if name == 'transe':
            with torch.no_grad():
                tabs[0].copy_(torch.nn.functional.normalize(tabs[0], p=2, dim=1))
    return [x.detach() for x in tabs], min_hinge


@pytest.mark.parametrize('name', sorted(FUSED_CASES))
def test_fused_against_generic_under_the_float64_bound(tk, name):
    from torchkge_amd.utils.training import Trainer
    kg = graph(tk)
    crit = criterion_of(tk, FUSED_CASES[name])
    # the same seed draws the same counter-examples on both paths
    drawn = []
    for fused in (True, False):
        model = build(tk, name)
        torch.manual_seed(123)
        tr = Trainer(model, crit, kg, N_EPOCHS, B_SIZE, optimizer_of(tk, model, False), use_cuda='all', fused=fused, verbose=False)
        tr.run()
        drawn.append(tr.get_counter_examples())
    assert torch.equal(drawn[0].head_idx, drawn[1].head_idx) and torch.equal(drawn[0].tail_idx, drawn[1].tail_idx)
    assert drawn[0].head_idx.is_cuda and not torch.equal(drawn[0].head_idx, kg.head_idx.cuda())
    # recorded negatives: both paths and the float64 loop see the same ones
    negatives = host_negatives(kg, 9)
    init = [p.detach().cpu().clone() for p in build(tk, name).parameters()]
    ref64, min_hinge = plain_float64_loop(tk, name, crit, init, kg, negatives)
    assert min_hinge >= MIN_HINGE, 'a hinge of the float64 run lies inside float noise (%.3g): choose other negatives' % min_hinge
    runs = {}
    for fused in (False, True):
        model = build(tk, name)
        assert all(torch.equal(a.detach().cpu(), b) for a, b in zip(model.parameters(), init))
        tr = Trainer(model, crit, kg, N_EPOCHS, B_SIZE, optimizer_of(tk, model, False), use_cuda='all', fused=fused,
                     sampler=Replay(negatives), verbose=False)
        tr.run()
        runs[fused] = [p.detach().cpu() for p in model.parameters()]
    bound, generic_dist = table_bound(runs[False], ref64)
    got = distance(runs[True], ref64)
    print('trainer fused vs generic %-8s tables |fused - f64| %.3g (generic %.3g, bound %.3g)' % (name, got, generic_dist, bound))
    assert distance(init, ref64) > 1e-4        # it trained
    assert got <= bound


# ---------------------------------------------------------------------------
# 4. sync_free reads nothing back
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('row', [False, True], ids=['SGD', 'RowAdagrad'])
def test_a_sync_free_run_reads_nothing_back(tk, row):
    from torchkge_amd.utils.training import Trainer
    kg = graph(tk)
    crit = tk.MarginLoss(0.5)
    negatives = host_negatives(kg, 4)

    def trainer(sync_free, sampler):
        model = build(tk, 'transe')
        return Trainer(model, crit, kg, N_EPOCHS, B_SIZE, optimizer_of(tk, model, row), use_cuda='all', sync_free=sync_free,
                       sampler=sampler, verbose=False)
    own, replayed = trainer(True, None), trainer(True, Replay(negatives))
    own.run()                   # the warm-up: library loading, the graph's upload, the allocator's growth
    replayed.run()
    assert len(own.epoch_losses) == N_EPOCHS == len(replayed.epoch_losses)
    detects = False
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            torch.ones(1, device='cuda').item()
        except RuntimeError:
            detects = True
        own.run()               # the engine's Bernoulli sampler, drawing without its host read
        replayed.run()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    print('sync debug mode detects a host read on this build:', detects)
    assert own._loader.sampler.sync_free is True and own._epoch_sums is not None          # nothing fetched yet
    assert np.isfinite(own.epoch_losses).all() and own._epoch_sums is None and len(own.epoch_losses) == N_EPOCHS
    # the epoch means against the per-step losses of an ordinary run on the same negatives.  With one summation order
    # in the backward (the row path has it by itself, the dense one under the switch) the steps are the same launches
    # on the same bits; the device sum adds the k fp32 losses in order: k - 1 roundings of half an ulp of the sum.
    with tk.deterministic(not row):
        replayed = trainer(True, Replay(negatives))
        replayed.run()
        plain = trainer(False, Replay(negatives))
        steps = []
        plain.process_batch = (lambda f: lambda b: steps.append(f(b)) or steps[-1])(plain.process_batch)
        plain.run()
    k = len(steps) // N_EPOCHS
    assert k == 3 and len(replayed.epoch_losses) == N_EPOCHS
    for e in range(N_EPOCHS):
        total = sum(steps[e * k:(e + 1) * k])
        assert plain.epoch_losses[e] == total / k
        dist, bound = abs(replayed.epoch_losses[e] - total / k), 0.5 * (k - 1) * ulp_of(total) / k
        print('sync_free epoch %d mean loss %.9g: |device sum - step losses| %.3g (bound %.3g)' % (e, total / k, dist, bound))
        assert dist <= bound, e


# ---------------------------------------------------------------------------
# 5. the counter-examples
# ---------------------------------------------------------------------------
def test_counter_examples_before_and_after_run(tk):
    from torchkge_amd.utils.training import Trainer, TrainDataLoader
    kg = graph(tk)
    model = build(tk, 'transe')
    for use_cuda in ('all', 'batch'):
        # the reference tutorial's call, positional arguments and all ('batch': with the progress bar when tqdm imports)
        tr = Trainer(model, tk.MarginLoss(0.5), kg, 1, B_SIZE, optimizer_of(tk, model, False), 'unif', use_cuda,
                     verbose=use_cuda == 'batch')
        assert tr.get_counter_examples() is None
        tr.run()
        ce = tr.get_counter_examples()
        assert isinstance(ce, tk.SmallKG) and len(ce) == kg.n_facts and ce.head_idx.is_cuda
        assert torch.equal(ce.relations.cpu(), kg.relations)
        changed = (ce.head_idx.cpu() != kg.head_idx) | (ce.tail_idx.cpu() != kg.tail_idx)
        assert int(changed.sum()) > 0.9 * kg.n_facts and len(tr.epoch_losses) == 1 and tr.epoch_losses[0] > 0
    loader = TrainDataLoader(kg, B_SIZE, 'bern', use_cuda='batch')
    batches = list(loader)
    assert [b['h'].shape[0] for b in batches] == [512, 512, 176] and all(v.is_cuda for b in batches for v in b.values())
    assert not loader.h.is_cuda and TrainDataLoader(kg, B_SIZE, 'bern', use_cuda='all').h.is_cuda
