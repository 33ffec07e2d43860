"""GPU tests of ``Model.forward_grouped`` and ``Trainer.grouped_forward`` (run with -m gpu on an MI355X): the
outputs have the bits of ``Model.forward``, the dense gradients agree with its gradients, inside ``row_gradients()`` an
entity table's gradient carries B (K + 2) rows instead of 2 B (K + 1), the models the grouped kernels do not serve fall
back, ``check=True`` refuses a negative corrupted on both sides, and the Trainer's switch changes nothing when off.

The bound between two fp32 gradients of one quantity is GRAD_TOL in the form tests/test_gpu_layout_contract.py defines
it: |a - b| <= GRAD_TOL * max(1, max |b|) per table."""
import pytest
import torch

from oracle import kge_oracle as orc
from tests.test_gpu_layout_contract import GRAD_TOL
from tests.test_gpu_trainer import make_kg

pytestmark = pytest.mark.gpu

N_ENT, N_REL, DIM, B, K = 60, 5, 24, 64, 8
BUILD = {
    'transe_l1': lambda tk: tk.TransEModel(DIM, N_ENT, N_REL, 'L1'),
    'transe_l2': lambda tk: tk.TransEModel(DIM, N_ENT, N_REL, 'L2'),
    'transh': lambda tk: tk.TransHModel(DIM, N_ENT, N_REL),
    'transd': lambda tk: tk.TransDModel(DIM, 16, N_ENT, N_REL),
    'distmult': lambda tk: tk.DistMultModel(DIM, N_ENT, N_REL),
    'complex': lambda tk: tk.ComplExModel(DIM, N_ENT, N_REL),
    'toruse': lambda tk: tk.TorusEModel(DIM, N_ENT, N_REL, 'torus_L2'),
}


@pytest.fixture(scope='module')
def tk():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import torchkge_amd
    return torchkge_amd


def bits(x):
    return x.contiguous().view(torch.int32)


def batch(seed=3):
    """B facts and their K negatives in tile order, one side replaced per negative."""
    g = torch.Generator().manual_seed(seed)
    h, t = torch.randint(0, N_ENT, (B,), generator=g), torch.randint(0, N_ENT, (B,), generator=g)
    r = torch.randint(0, N_REL, (B,), generator=g)
    side = torch.rand(K * B, generator=g) < 0.5
    draw = torch.randint(0, N_ENT, (K * B,), generator=g)
    nh, nt = torch.where(side, draw, h.repeat(K)), torch.where(side, t.repeat(K), draw)
    wp, wn = torch.randn(K * B, generator=g), torch.randn(K * B, generator=g)
    return tuple(x.cuda() for x in (h, t, r, nh, nt, wp, wn))


def build(tk, name, seed=0):
    torch.manual_seed(seed)
    return BUILD[name](tk).cuda()


def grads_of(model, grouped, data, **kw):
    h, t, r, nh, nt, wp, wn = data
    model.zero_grad()
    p, n = (model.forward_grouped(h, t, r, nh, nt, **kw) if grouped else model(h, t, r, nh, nt))
    ((p * wp).sum() + (n * wn).sum()).backward()
    return p.detach(), n.detach(), [x.grad for x in model.parameters()]


def close(a, b):
    return bool(((a.double() - b.double()).abs() <= GRAD_TOL * max(1.0, float(b.abs().max()))).all())


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('name', sorted(BUILD))
def test_forward_grouped_has_the_bits_of_forward_and_its_dense_gradients(tk, name, det):
    model, data = build(tk, name), batch()
    import contextlib
    with tk.deterministic() if det else contextlib.nullcontext():
        p0, n0, g0 = grads_of(model, False, data)
        g0 = [x.clone() for x in g0]
        p1, n1, g1 = grads_of(model, True, data)
    assert p1.shape == p0.shape == (K * B,) and n1.shape == n0.shape == (K * B,)
    assert torch.equal(bits(p1), bits(p0)) and torch.equal(bits(n1), bits(n0))
    for a, b in zip(g1, g0):
        assert a.shape == b.shape and not a.is_sparse and bool(torch.isfinite(a).all())
        assert close(a, b), (name, float((a - b).abs().max()))
    if det:     # the ordered reduction: the same bits again
        _, _, g2 = grads_of(model, True, data)
        for a, b in zip(g1, [x.clone() for x in g2]):
            assert torch.equal(bits(a), bits(b))
    if name == 'toruse':
        assert model.normalized is False


@pytest.mark.parametrize('name', ['transe_l2', 'complex', 'transd'])
def test_row_gradients_carry_k_plus_two_rows_per_fact(tk, name):
    from torchkge_amd.rowgrad import row_gradients
    model, data = build(tk, name), batch()
    ent = [getattr(model, n).weight for n in model._ENT_TABLES]
    with row_gradients():
        grads_of(model, False, data)
        old = [w.grad for w in ent]
        assert all(g.is_sparse and g._nnz() == 2 * B * (K + 1) for g in old)
        old = [g.coalesce().to_dense() for g in old]
        _, _, all_g = grads_of(model, True, data)
    for w, o in zip(ent, old):
        g = w.grad
        assert g.is_sparse and not g.is_coalesced() and g._nnz() == B * (K + 2)
        assert close(g.coalesce().to_dense(), o)
    for g in all_g:         # the relation tables: one row per fact
        assert g.is_sparse and g._nnz() in (B, B * (K + 2))


def test_models_outside_the_ten_kinds_and_negative_relations_fall_back(tk):
    data = batch()
    h, t, r, nh, nt = data[:5]
    torch.manual_seed(0)
    model = tk.RESCALModel(DIM, N_ENT, N_REL).cuda()
    p0, n0, g0 = grads_of(model, False, data)
    g0 = [x.clone() for x in g0]
    p1, n1, g1 = grads_of(model, True, data)
    assert torch.equal(bits(p1), bits(p0)) and torch.equal(bits(n1), bits(n0))
    # one negative per fact with its own relations: forward's path, forward's bits
    model = build(tk, 'transe_l2')
    nr = (r + 1) % N_REL
    a = model(h, t, r, nh[:B], nt[:B], nr)
    b = model.forward_grouped(h, t, r, nh[:B], nt[:B], nr)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    # rows wider than 512 floats: the kernels answer KGE_EUNSUPPORTED and forward serves
    torch.manual_seed(0)
    wide = tk.TransEModel(516, N_ENT, N_REL, 'L2').cuda()
    a, b = wide(h, t, r, nh, nt), wide.forward_grouped(h, t, r, nh, nt)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    # n_neg = 1 through the kernels: pos is not repeated
    p, n = model.forward_grouped(h, t, r, nh[:B], nt[:B])
    q, m = model(h, t, r, nh[:B], nt[:B])
    assert p.shape == (B,) and torch.equal(bits(p), bits(q)) and torch.equal(bits(n), bits(m))


def test_check_refuses_a_negative_corrupted_on_both_sides(tk):
    model, (h, t, r, nh, nt, _, _) = build(tk, 'transe_l2'), batch()
    nh, nt = nh.clone(), nt.clone()
    nh[5 * B + 3], nt[5 * B + 3] = (h[3] + 1) % N_ENT, (t[3] + 1) % N_ENT
    with pytest.raises(ValueError):
        model.forward_grouped(h, t, r, nh, nt)
    with pytest.raises(ValueError):
        model.forward_grouped(h, t, r, nh, nt, check=True)
    # unchecked it runs, scoring that negative with the fact's tail
    p, n = model.forward_grouped(h, t, r, nh, nt, check=False)
    fixed = nt.clone()
    fixed[5 * B + 3] = t[3]
    q, m = model(h, t, r, nh, fixed)
    assert torch.equal(bits(n), bits(m)) and torch.equal(bits(p), bits(q))
    shard = build(tk, 'transe_l2').shard_entities_(0, N_ENT // 2)
    with pytest.raises(RuntimeError):
        shard.forward_grouped(h, t, r, nh, fixed)


# ---------------------------------------------------------------------------
# the Trainer
# ---------------------------------------------------------------------------
LR, N_NEG, N_FACTS, B_SIZE = 0.05, 4, 300, 128


@pytest.fixture(scope='module')
def kg(tk):
    h, t, r = orc.synthetic_triples(N_ENT, N_REL, N_FACTS, 5)
    return make_kg(tk, h, t, r, N_ENT, N_REL)


def one_step(tk, kg, name, grouped_forward=None):
    """A Trainer from one seed, its loader's first batch through one plain-SGD step: (loss, tables before, tables after,
    the batch).  ``grouped_forward``: None leaves the attribute alone."""
    from torchkge_amd.utils import group_losses
    from torchkge_amd.utils.training import Trainer, TrainDataLoader
    model = build(tk, name, seed=1)
    before = [p.detach().clone() for p in model.parameters()]
    tr = Trainer(model, group_losses.SelfAdversarialLoss(2.0, 0.5), kg, 1, B_SIZE, torch.optim.SGD(model.parameters(), lr=LR),
                 sampling_type='bern', use_cuda='all', verbose=False, n_neg=N_NEG)
    if grouped_forward is not None:
        tr.grouped_forward = grouped_forward
    torch.manual_seed(7)
    loader = TrainDataLoader(kg, B_SIZE, 'bern', use_cuda='all', n_neg=N_NEG)
    first = next(iter(loader))
    loss = tr._step(first)
    return loss, before, [p.detach().clone() for p in model.parameters()], first, tr


@pytest.mark.parametrize('name', ['transe_l2', 'complex'])
def test_trainer_grouped_forward_first_step(tk, kg, name):
    with tk.deterministic():
        l_old, w0, w_old, b_old, tr_old = one_step(tk, kg, name)
        l_off, _, w_off, _, tr_off = one_step(tk, kg, name, grouped_forward=False)
        l_new, _, w_new, b_new, tr_new = one_step(tk, kg, name, grouped_forward=True)
        l_again, _, w_again, _, _ = one_step(tk, kg, name, grouped_forward=True)
    assert tr_new.grouped_forward and not tr_off.grouped_forward and not tr_old.grouped_forward
    assert not tr_new._check_negatives          # the package's own sampler: no host read
    for k in b_old:
        assert torch.equal(b_old[k], b_new[k])  # one seed, one batch
    # the sampler's negatives keep the contract the unchecked path relies on
    hh, tt = b_new['h'].repeat(N_NEG), b_new['t'].repeat(N_NEG)
    assert not bool(((b_new['nh'] != hh) & (b_new['nt'] != tt)).any())
    # off is the parent's behaviour, bit for bit
    assert torch.equal(bits(l_off), bits(l_old))
    for a, b in zip(w_off, w_old):
        assert torch.equal(bits(a), bits(b))
    # on: the same scores, hence the same loss bits; the step within the gradient bound times the learning rate
    assert torch.equal(bits(l_new), bits(l_old))
    moved = 0.0
    for a, b, w in zip(w_new, w_old, w0):
        gmax = float((b - w).abs().max()) / LR          # plain SGD: the step is lr * grad
        moved = max(moved, gmax)
        assert bool(((a.double() - b.double()).abs() <= LR * GRAD_TOL * max(1.0, gmax)).all()), name
    assert moved > 0
    for a, b in zip(w_new, w_again):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(l_new), bits(l_again))


def test_trainer_checks_a_foreign_sampler_unless_sync_free(tk, kg):
    from torchkge_amd.utils import group_losses
    from torchkge_amd.utils.training import Trainer

    class Foreign(object):
        sync_free = False

        def corrupt_kg(self, batch_size, use_cuda, which='main', on_device=False, *, n_neg=1):
            n = N_FACTS * n_neg
            return (torch.zeros(n, dtype=torch.int64, device='cuda' if on_device else 'cpu'),) * 2

    def trainer(**kw):
        model = build(tk, 'transe_l2')
        tr = Trainer(model, group_losses.SampledSoftmaxLoss(), kg, 1, B_SIZE, torch.optim.SGD(model.parameters(), lr=LR),
                     use_cuda='all', verbose=False, n_neg=N_NEG, **kw)
        tr.grouped_forward = True
        return tr
    assert trainer(sampler=Foreign())._check_negatives
    assert not trainer(sampler=Foreign(), sync_free=True)._check_negatives
    assert not trainer(sampler=tk.UniformNegativeSampler(kg, n_neg=N_NEG))._check_negatives
    assert not trainer()._check_negatives
