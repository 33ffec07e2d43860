"""GPU tests of training with K negatives per fact (run with -m gpu on an MI355X): Trainer(n_neg=4) with the grouped
criteria of torchkge_amd.utils.group_losses against the same loop with the criterion written out in torch
(tests/group_loss_ref.py ``written_out``), under the bound of tests/test_gpu_trainer.py taken from a float64 run of the
written-out loop in plain torch: 4 * (2 * |fp32 run - fp64 run| + one ulp of the largest entry) in max-norm over all
tables, and the same rule relative to the loss, with the ulp of 1.0, on the epochs' mean losses.  Then ``sync_free``,
``deterministic()``, ``RowAdagrad``, and the engine's own Bernoulli sampler with ``n_neg=4``."""
import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.group_loss_ref import written_out
from tests.test_gpu_trainer import make_kg, table_bound, distance, ulp_of, ULP1

pytestmark = pytest.mark.gpu

N_ENT, N_REL, DIM, N_FACTS, B_SIZE, N_EPOCHS, LR, N_NEG = 300, 7, 16, 700, 256, 2, 0.05, 4
SIZES = (256, 256, 188)
MARGIN, ALPHA = 2.0, 0.5
BUILD = {
    'transe': lambda tk: tk.TransEModel(DIM, N_ENT, N_REL, 'L2'),
    'complex': lambda tk: tk.ComplExModel(DIM, N_ENT, N_REL),
}
CASES = [(m, k) for m in sorted(BUILD) for k in ('nssa', 'softmax')]


@pytest.fixture(scope='module')
def tk():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import torchkge_amd
    return torchkge_amd


@pytest.fixture(scope='module')
def kg(tk):
    h, t, r = orc.synthetic_triples(N_ENT, N_REL, N_FACTS, 5)
    return make_kg(tk, h, t, r, N_ENT, N_REL)


class Replay(object):
    """A sampler that hands out recorded negatives (the blocks of n_neg * B_b per batch, laid end to end)."""

    def __init__(self, epochs):
        self.host = [(nh.long(), nt.long()) for nh, nt in epochs]
        self.dev = [(nh.cuda(), nt.cuda()) for nh, nt in self.host]
        self.calls, self.sync_free, self.asked = 0, False, []

    def corrupt_kg(self, batch_size, use_cuda, which='main', on_device=False, *, n_neg=1):
        i = self.calls % len(self.host)
        self.calls += 1
        self.asked.append(n_neg)
        return self.dev[i] if on_device else self.host[i]


def recorded_negatives(kg, seed):
    """Per epoch the batches' blocks in tile order: negative k of the batch's fact i at k * B_b + i, head or tail replaced."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(N_EPOCHS):
        nhs, nts = [], []
        for lo in range(0, kg.n_facts, B_SIZE):
            h, t = kg.head_idx[lo:lo + B_SIZE].repeat(N_NEG), kg.tail_idx[lo:lo + B_SIZE].repeat(N_NEG)
            side = torch.rand(h.shape[0], generator=g) < 0.5
            draw = torch.randint(0, N_ENT, (h.shape[0],), generator=g)
            nhs.append(torch.where(side, draw, h))
            nts.append(torch.where(side, t, draw))
        out.append((torch.cat(nhs), torch.cat(nts)))
    return out


def build(tk, name, seed=0):
    torch.manual_seed(seed)
    return BUILD[name](tk).cuda()


def grouped(kind, **kw):
    from torchkge_amd.utils import group_losses
    return group_losses.SelfAdversarialLoss(MARGIN, ALPHA, **kw) if kind == 'nssa' else group_losses.SampledSoftmaxLoss(**kw)


class WrittenOut(object):
    """The criterion a user writes today, on what Model.forward returns: the generic path of the Trainer."""

    def __init__(self, kind):
        self.kind = kind

    def __call__(self, p, n):
        b = n.shape[0] // N_NEG
        return written_out(self.kind, MARGIN, ALPHA, p[:b], n.view(N_NEG, b)).sum()


def float64_loop(name, kind, init, kg, negatives):
    """The written-out loop in plain torch on the host, float64: the oracle's scores under autograd, torch's Adagrad,
    TransE's normalisation after every epoch.  Returns the tables and the epochs' mean losses."""
    tabs = [x.double().clone().requires_grad_() for x in init]
    opt = torch.optim.Adagrad(tabs, lr=LR)
    means = []
    for nh, nt in negatives:
        total = 0.0
        for lo in range(0, kg.n_facts, B_SIZE):
            sl = slice(lo, lo + B_SIZE)
            b = kg.head_idx[sl].shape[0]
            nsl = slice(N_NEG * lo, N_NEG * (lo + b))
            h, t = torch.cat([kg.head_idx[sl], nh[nsl]]), torch.cat([kg.tail_idx[sl], nt[nsl]])
            s = orc.score_triples(name, tabs, h, t, kg.relations[sl].repeat(N_NEG + 1))
            loss = written_out(kind, MARGIN, ALPHA, s[:b], s[b:].view(N_NEG, b)).sum()
            opt.zero_grad()
            loss.backward()
            opt.step()
            total += float(loss.detach())
        means.append(total / len(SIZES))
        if name == 'transe':
            with torch.no_grad():
                tabs[0].copy_(torch.nn.functional.normalize(tabs[0], p=2, dim=1))
    return [x.detach() for x in tabs], means


def run(tk, kg, name, criterion, negatives, row=False, **kw):
    from torchkge_amd import optim
    from torchkge_amd.utils.training import Trainer
    model = build(tk, name)
    opt = optim.RowAdagrad(model.parameters(), lr=LR) if row else torch.optim.Adagrad(model.parameters(), lr=LR)
    sampler = Replay(negatives)
    tr = Trainer(model, criterion, kg, N_EPOCHS, B_SIZE, opt, use_cuda='all', sampler=sampler, verbose=False, n_neg=N_NEG, **kw)
    tr.run()
    assert sampler.asked == [N_NEG] * N_EPOCHS
    return tr, [p.detach().cpu() for p in model.parameters()]


_SHARED = {}


def reference(tk, kg, name, kind):
    """(negatives, init, float64 tables, float64 mean losses, fp32 written-out tables and losses): once per case."""
    key = (name, kind)
    if key not in _SHARED:
        negatives = recorded_negatives(kg, 9)
        init = [p.detach().cpu().clone() for p in build(tk, name).parameters()]
        ref64, l64 = float64_loop(name, kind, init, kg, negatives)
        tr, tabs32 = run(tk, kg, name, WrittenOut(kind), negatives)
        assert tr._fused_criterion is None and not tr._grouped
        _SHARED[key] = (negatives, init, ref64, l64, tabs32, list(tr.epoch_losses))
    return _SHARED[key]


# ---------------------------------------------------------------------------
# the grouped criteria against the written-out loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name,kind', CASES)
def test_grouped_against_written_out_under_the_float64_bound(tk, kg, name, kind):
    negatives, init, ref64, l64, tabs32, l32 = reference(tk, kg, name, kind)
    crit = grouped(kind)
    tr, tabs = run(tk, kg, name, crit, negatives)
    assert crit.n_neg == N_NEG and tr._grouped
    bound, written_dist = table_bound(tabs32, ref64)
    got = distance(tabs, ref64)
    l64, l32, losses = np.array(l64), np.array(l32), np.array(tr.epoch_losses)
    loss_bound = 4 * (2 * np.abs(l32 - l64) / l64 + ULP1)
    loss_dist = np.abs(losses - l64) / l64
    print('group trainer %-8s %-7s tables |grouped - f64| %.3g (written out %.3g, bound %.3g); mean losses %s relative %.3g '
          '(written out %.3g, bound %.3g)' % (name, kind, got, written_dist, bound, l64.tolist(), loss_dist.max(),
                                              (np.abs(l32 - l64) / l64).max(), loss_bound.min()))
    assert distance(init, ref64) > 1e-3        # it trained
    assert got <= bound
    assert losses.shape == (N_EPOCHS,) and bool((loss_dist <= loss_bound).all())
    # the loader's blocks and the counter-examples
    assert [b['nh'].shape[0] for b in tr._loader] == [N_NEG * s for s in SIZES]
    ce = tr.get_counter_examples()
    assert len(ce) == N_NEG * N_FACTS and ce.relations.shape == ce.head_idx.shape


# ---------------------------------------------------------------------------
# sync_free, deterministic mode, the row optimizer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ('nssa', 'softmax'))
def test_a_sync_free_run_adds_the_same_losses_on_the_device(tk, kg, kind):
    negatives = recorded_negatives(kg, 4)
    with tk.deterministic():
        sf, tabs_sf = run(tk, kg, 'transe', grouped(kind), negatives, sync_free=True)
        assert sf._epoch_sums is not None                       # nothing fetched yet
        from torchkge_amd.utils.training import Trainer
        model = build(tk, 'transe')
        plain = Trainer(model, grouped(kind), kg, N_EPOCHS, B_SIZE, torch.optim.Adagrad(model.parameters(), lr=LR),
                        use_cuda='all', sampler=Replay(negatives), verbose=False, n_neg=N_NEG)
        steps = []
        plain.process_batch = (lambda f: lambda b: steps.append(f(b)) or steps[-1])(plain.process_batch)
        plain.run()
    k = len(SIZES)
    assert len(steps) == k * N_EPOCHS and len(sf.epoch_losses) == N_EPOCHS and sf._epoch_sums is None
    for a, b in zip(tabs_sf, [p.detach().cpu() for p in model.parameters()]):
        assert torch.equal(a, b)
    for e in range(N_EPOCHS):
        total = sum(steps[e * k:(e + 1) * k])
        # the device sum adds the k fp32 losses in order: k - 1 roundings of half an ulp of the sum
        dist, bound = abs(sf.epoch_losses[e] - total / k), 0.5 * (k - 1) * ulp_of(total) / k
        print('group sync_free %-7s epoch %d mean loss %.9g: |device sum - step losses| %.3g (bound %.3g)'
              % (kind, e, total / k, dist, bound))
        assert dist <= bound, e


def test_a_sync_free_run_reads_nothing_back(tk, kg):
    negatives = recorded_negatives(kg, 4)
    from torchkge_amd.utils.training import Trainer
    model = build(tk, 'transe')
    # (SGD, as tests/test_gpu_trainer.py has it under the sync debug mode)
    tr = Trainer(model, grouped('nssa'), kg, N_EPOCHS, B_SIZE, torch.optim.SGD(model.parameters(), lr=0.01),
                 use_cuda='all', sampler=Replay(negatives), verbose=False, sync_free=True, n_neg=N_NEG)
    tr.run()                    # the warm-up: library loading, the graph's upload, the allocator's growth
    torch.cuda.set_sync_debug_mode('error')
    try:
        tr.run()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert tr._epoch_sums is not None and np.isfinite(tr.epoch_losses).all()


@pytest.mark.parametrize('name', sorted(BUILD))
def test_two_deterministic_runs_give_the_same_table_bits(tk, kg, name):
    negatives = recorded_negatives(kg, 6)
    with tk.deterministic():
        a = run(tk, kg, name, grouped('nssa'), negatives)
        b = run(tk, kg, name, grouped('nssa'), negatives)
    assert a[0].epoch_losses == b[0].epoch_losses
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize('kind', ('nssa', 'softmax'))
def test_row_adagrad_agrees_with_dense_adagrad_under_the_bound(tk, kg, kind):
    negatives, init, ref64, l64, tabs32, l32 = reference(tk, kg, 'transe', kind)
    tr, tabs = run(tk, kg, 'transe', grouped(kind, n_neg=N_NEG), negatives, row=True)
    assert tr._row_mode
    bound, written_dist = table_bound(tabs32, ref64)
    got = distance(tabs, ref64)
    print('group trainer RowAdagrad %-7s tables |row - f64| %.3g (dense written out %.3g, bound %.3g)' % (kind, got, written_dist, bound))
    assert distance(init, ref64) > 1e-3 and got <= bound


# ---------------------------------------------------------------------------
# the engine's own sampler
# ---------------------------------------------------------------------------
def test_the_bernoulli_sampler_draws_four_negatives_per_fact_through_the_trainer(tk, kg):
    from torchkge_amd.utils.training import Trainer
    model = build(tk, 'transe')
    sampler = tk.BernoulliNegativeSampler(kg, n_neg=N_NEG)
    torch.manual_seed(11)
    tr = Trainer(model, grouped('nssa'), kg, 1, B_SIZE, torch.optim.Adagrad(model.parameters(), lr=LR), use_cuda='all',
                 sampler=sampler, verbose=False, n_neg=N_NEG)
    tr.run()
    assert len(tr.epoch_losses) == 1 and np.isfinite(tr.epoch_losses[0]) and tr.epoch_losses[0] > 0
    ce = tr.get_counter_examples()
    assert len(ce) == N_NEG * N_FACTS and ce.head_idx.is_cuda
    blocks = list(tr._loader)
    assert [b['nh'].shape[0] for b in blocks] == [N_NEG * s for s in SIZES] and [b['h'].shape[0] for b in blocks] == list(SIZES)
    # tile order: negative k of the batch's fact i keeps the head or the tail of fact i
    for b in blocks:
        h, t = b['h'].repeat(N_NEG), b['t'].repeat(N_NEG)
        assert bool(((b['nh'] == h) | (b['nt'] == t)).all()) and int(((b['nh'] != h) | (b['nt'] != t)).sum()) > 0.9 * h.shape[0]
    # corrupt_kg itself: the default is one negative per fact, n_neg=4 four blocks' worth, on both paths
    nh1, _ = sampler.corrupt_kg(B_SIZE, True, on_device=True)
    nh4, nt4 = sampler.corrupt_kg(B_SIZE, True, on_device=True, n_neg=N_NEG)
    hh4, _ = sampler.corrupt_kg(B_SIZE, True, n_neg=N_NEG)
    assert nh1.shape == (N_FACTS,) and nh4.shape == nt4.shape == (N_NEG * N_FACTS,) == hh4.shape and not hh4.is_cuda
    # the pairwise criteria see n_neg pairs per fact through Model.forward's repeat
    model = build(tk, 'transe')
    tr = Trainer(model, tk.MarginLoss(0.5), kg, 1, B_SIZE, torch.optim.Adagrad(model.parameters(), lr=LR), use_cuda='all',
                 sampler=sampler, verbose=False, n_neg=N_NEG)
    tr.run()
    assert tr._fused_criterion is not None and np.isfinite(tr.epoch_losses[0]) and tr.epoch_losses[0] > 0
