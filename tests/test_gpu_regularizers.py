"""GPU tests of torchkge_amd.utils.regularizers on every model class and inside the three trainers, against the float64
yardstick of tests/penalty_ref.py.

The loss bound, derived (u = 2 ** -24): every term is within (16 + ceil(d / 256)) u of float64
(tests/test_gpu_penalty_kernels.py) and non-negative, the fp64 tree adds them without a visible error and rounds once
(u), and a model of more than eight streams adds two launches' sums (u): |loss - ref| <= (18 + ceil(d_max / 256)) u ref,
d_max the widest penalised row of the model.  Gradients: the project's own metric of the backward tests,
|got - want| <= 1e-4 * max(1, max |want|) (tests/test_gpu_layout_contract.py: GRAD_TOL)."""
import math

import pytest
import torch

from tests import penalty_ref as ref
from tests import group_loss_ref as gref
from tests.penalty_ref import N_ENT, N_REL

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GRAD_TOL = 1e-4
B = 37


def facts(seed=0, n=B):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(0, hi, (n,), generator=g).cuda() for hi in (N_ENT, N_ENT, N_REL))


def build(name, d, seed=0):
    torch.manual_seed(seed)
    return ref.zoo(d)[name][0]().cuda()


def groups64(model, reg):
    """The model's groups on float64 leaves: ((entity groups, relation groups) as (layout, t0, t1), {parameter id: leaf})."""
    leaves = {}

    def leaf(x):
        if id(x) not in leaves:
            leaves[id(x)] = x.detach().double().clone().requires_grad_()
        return leaves[id(x)]
    sides = [[(layout, leaf(t0), None if t1 is None else leaf(t1)) for layout, t0, t1 in side] for side in reg._groups(model)]
    return sides, leaves


def reference(model, reg, ent_ids, rel_ids):
    """(float64 penalty, {parameter id: float64 gradient}, widest penalised row)."""
    sides, leaves = groups64(model, reg)
    loss = ref.penalty64(sides, reg.p, (reg.weight, reg.relation_weight), (ent_ids, rel_ids))
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in leaves.items()}, max(t0.shape[1] for side in sides for _, t0, _ in side)


def close(got, want):
    return float((got.double() - want).abs().max()) <= GRAD_TOL * max(1.0, float(want.abs().max()))


def loss_ok(got, want, d_max, extra=0.0):
    return abs(float(got.detach()) - want) <= (18 + math.ceil(d_max / 256)) * U * want + extra


CASES = [(name, d) for name in sorted(ref.zoo(5)) for d in (5, 64)]


@pytest.mark.parametrize('name,d', CASES)
@pytest.mark.parametrize('p', [2, 3])
def test_loss_and_gradients_of_every_model_class_dense_and_row_mode(name, d, p):
    import torchkge_amd as tk
    from torchkge_amd.utils.regularizers import LpRegularizer
    model = build(name, d)
    reg = LpRegularizer(p=p, weight=0.05, relation_weight=0.02)
    h, t, r = facts()
    want, grads, d_max = reference(model, reg, (h, t), (r,))
    loss = reg(model, (h, t), (r,))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss_ok(loss, want, d_max), (float(loss), want)
    loss.backward()
    hit = {'ent': torch.cat([h, t]).unique(), 'rel': r.unique()}
    dense = {}
    for pname, param in model.named_parameters():
        if id(param) not in grads:
            assert param.grad is None, pname            # RotatE's phases, ConvKB's layers
            continue
        g = dense[pname] = param.grad
        assert not g.is_sparse and close(g, grads[id(param)]), pname
        rows = hit['ent'] if param.shape[0] == N_ENT else hit['rel']
        untouched = torch.ones(param.shape[0], dtype=torch.bool, device='cuda')
        untouched[rows] = False
        assert bool((g[untouched].view(torch.int32) == 0).all()), pname
    assert dense
    # row mode: B rows per (group, id vector), the coalesced rows are the dense gradient; rel_mat / proj_mat stay dense
    model.zero_grad(set_to_none=True)
    with tk.row_gradients():
        loss_rows = reg(model, (h, t), (r,))
    assert float(loss_rows.detach()) == float(loss.detach())
    loss_rows.backward()        # outside the context: the mode was read by the forward
    stays_dense = {n + '.weight' for n in model._DENSE_GRAD_TABLES}
    for pname, param in model.named_parameters():
        if pname not in dense:
            assert param.grad is None, pname
        elif pname in stays_dense:
            assert not param.grad.is_sparse and close(param.grad, grads[id(param)]), pname
        else:
            g = param.grad
            assert g.is_sparse and not g.is_coalesced(), pname
            assert g._values().shape == ((2 if param.shape[0] == N_ENT else 1) * B, param.shape[1]), pname
            assert close(g.coalesce().to_dense(), grads[id(param)]), pname
    assert stays_dense <= set(dense)


@pytest.mark.parametrize('name', ['ComplEx', 'RotatE', 'ANALOGY'])
@pytest.mark.parametrize('p', [2, 3])
def test_modulus_false_is_the_elementwise_form(name, p):
    """ANALOGY element by element is nine streams: two launches, their sums added."""
    from torchkge_amd.utils.regularizers import LpRegularizer
    model = build(name, 64)
    reg = LpRegularizer(p=p, weight=0.03, modulus=False)
    assert all(layout == ref.REAL for side in reg._groups(model) for layout, _, _ in side)
    h, t, r = facts(1)
    want, grads, d_max = reference(model, reg, (h, t), (r,))
    with_modulus = reference(model, LpRegularizer(p=p, weight=0.03), (h, t), (r,))[0]
    assert (abs(with_modulus - want) <= 1e-12 * want) == (p == 2)       # the two forms coincide for p = 2 only
    loss = reg(model, (h, t), (r,))
    assert loss_ok(loss, want, d_max)
    loss.backward()
    for pname, param in model.named_parameters():
        if id(param) in grads:
            assert close(param.grad, grads[id(param)]), pname
        else:
            assert param.grad is None, pname


def test_accumulator_unequal_id_vectors_and_zero_weights():
    from torchkge_amd.utils.regularizers import N3Regularizer, LpRegularizer
    model = build('ComplEx', 5)
    h, t, r = facts(2)
    acc = torch.tensor(1.5, device='cuda')
    reg = N3Regularizer(0.1, relation_weight=0.0)
    loss = reg(model, (h, t[:5]), r, acc)           # a tensor for one side, vectors of different lengths on the other
    want, grads, d_max = reference(model, reg, (h, t[:5]), (r,))
    assert loss_ok(loss, want, d_max) and float(acc) == float(torch.tensor(1.5) + loss.detach().cpu())
    loss.backward()
    assert model.re_rel_emb.weight.grad is None and close(model.im_ent_emb.weight.grad, grads[id(model.im_ent_emb.weight)])
    zero = LpRegularizer(p=2, weight=0.0)(model, (h, t), (r,))
    assert float(zero.detach()) == 0.0 and zero.is_cuda


# ---------------------------------------------------------------------------
# inside the trainers
# ---------------------------------------------------------------------------
def small_kg(n=B, seed=3):
    import torchkge_amd as tk
    g = torch.Generator().manual_seed(seed)
    h, t, r = (torch.randint(0, hi, (n,), generator=g) for hi in (N_ENT, N_ENT, N_REL))
    return tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(N_ENT)},
                             rel2ix={i: i for i in range(N_REL)})


def score64(name, leaves, model, h, t, r):
    """ComplEx / RotatE scores in float64 on the leaves of the model's tables."""
    if name == 'ComplEx':
        re_e, im_e, re_r, im_r = (leaves[id(x)] for x in model._tables())
        return (re_e[h] * (re_r[r] * re_e[t] + im_r[r] * im_e[t]) + im_e[h] * (re_r[r] * im_e[t] - im_r[r] * re_e[t])).sum(1)
    E, P = (leaves[id(x)] for x in model._tables())
    Ec = torch.view_as_complex(E.view(E.shape[0], -1, 2))
    return -(Ec[h] * torch.polar(torch.ones_like(P[r]), P[r]) - Ec[t]).abs().sum(-1)


def nssa_trainer(model, kg, optimizer, n_epochs=1, batch=B, **kw):
    from torchkge_amd.utils.group_losses import SelfAdversarialLoss
    from torchkge_amd.utils.training import Trainer
    return Trainer(model, SelfAdversarialLoss(2.0, temperature=0.5), kg, n_epochs, batch, optimizer, sampling_type='unif',
                   use_cuda='all', verbose=False, n_neg=8, **kw)


@pytest.mark.parametrize('name', ['ComplEx', 'RotatE'])
@pytest.mark.parametrize('grouped', [False, True])
def test_one_row_sgd_step_of_the_trainer_is_the_float64_step(name, grouped):
    """Score gradient and penalty gradient arrive as two sparse gradients on one parameter; RowSGD coalesces their sum.
    One step from fixed tables against the float64 written-out step: criterion (tests/group_loss_ref.py) plus penalty."""
    from torchkge_amd import optim
    from torchkge_amd.utils.regularizers import N3Regularizer
    lr, K = 0.1, 8
    model, kg = build(name, 64), small_kg()
    before = {id(x): x.detach().double().clone().requires_grad_() for x in model._tables()}
    tr = nssa_trainer(model, kg, optim.RowSGD(model.parameters(), lr=lr))
    tr.regularizer = reg = N3Regularizer(0.05, relation_weight=0.02)
    tr.grouped_forward = grouped
    tr.run()
    neg = tr.get_counter_examples()
    h, t, r = kg.head_idx.cuda(), kg.tail_idx.cuda(), kg.relations.cuda()
    nh, nt = neg.head_idx.cuda(), neg.tail_idx.cuda()
    assert nh.shape[0] == K * B
    pos64 = score64(name, before, model, h, t, r)
    neg64 = score64(name, before, model, nh, nt, r.repeat(K)).view(K, B)
    sides = [[(layout, before[id(t0)], None if t1 is None else before[id(t1)]) for layout, t0, t1 in side] for side in reg._groups(model)]
    pen64 = ref.penalty64(sides, 3, (0.05, 0.02), ((h, t), (r,)))
    total = gref.written_out('nssa', 2.0, 0.5, pos64, neg64).sum() + pen64
    total.backward()
    # the epoch's loss holds the penalty: the project's metric on the sum of criterion and penalty
    assert abs(tr.epoch_losses[0] - float(total.detach())) <= GRAD_TOL * max(1.0, abs(float(total.detach())))
    assert float(pen64.detach()) > 10 * GRAD_TOL
    for x in model._tables():
        want = before[id(x)].detach() - lr * before[id(x)].grad
        err = float((x.detach().double() - want).abs().max())
        # (+ 2 u |table|: the updated table is stored in fp32, half an ulp, and lr * g is rounded before it is subtracted)
        assert err <= GRAD_TOL * lr * max(1.0, float(before[id(x)].grad.abs().max())) + 2 * U * float(want.abs().max()), name


@pytest.mark.parametrize('name', ['ComplEx', 'RotatE'])
def test_row_adagrad_training_with_a_regularizer_runs_and_shrinks_the_penalty(name):
    from torchkge_amd import optim
    from torchkge_amd.utils.regularizers import N3Regularizer
    model, kg = build(name, 64), small_kg(n=3 * B)
    reg = N3Regularizer(0.5)
    ids = ((kg.head_idx.cuda(), kg.tail_idx.cuda()), (kg.relations.cuda(),))
    first = float(reg(model, *ids).detach())
    tr = nssa_trainer(model, kg, optim.RowAdagrad(model.parameters(), lr=0.05), n_epochs=3)
    tr.regularizer = reg
    tr.run()
    assert len(tr.epoch_losses) == 3 and all(math.isfinite(x) for x in tr.epoch_losses)
    assert all(bool(torch.isfinite(x).all()) for x in model._tables())
    assert float(reg(model, *ids).detach()) < first


def train_once(name, row_mode, seed=4):
    from torchkge_amd import optim
    from torchkge_amd.utils.regularizers import N3Regularizer
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    model, kg = build(name, 64, seed=seed), small_kg(n=3 * B)
    opt = optim.RowAdagrad(model.parameters(), lr=0.05) if row_mode else torch.optim.Adagrad(model.parameters(), lr=0.05)
    tr = nssa_trainer(model, kg, opt, n_epochs=2, batch=16)
    tr.regularizer = N3Regularizer(0.05)
    tr.run()
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}, list(tr.epoch_losses)


@pytest.mark.parametrize('name', ['ComplEx', 'RotatE'])
@pytest.mark.parametrize('row_mode', [False, True])
def test_two_deterministic_trainings_with_a_regularizer_give_the_same_bits(name, row_mode):
    import torchkge_amd as tk
    from torchkge_amd import _hip_det
    before = dict(_hip_det.CALLS)
    with tk.deterministic():
        a, la = train_once(name, row_mode)
        b, lb = train_once(name, row_mode)
    if not row_mode:
        assert _hip_det.CALLS['ordered'] > before['ordered'] and _hip_det.CALLS['atomic'] == before['atomic']
    assert la == lb and sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def dense_trainer(cls, model, kg, sync_free=False, n_epochs=1, batch=1000, lr=0.1):
    return cls(model, kg, n_epochs, batch, torch.optim.SGD(model.parameters(), lr=lr), side='tail', use_cuda='all',
               sync_free=sync_free, verbose=False)


@pytest.mark.parametrize('regime', ['one_vs_all', 'k_vs_all'])
def test_dense_gradient_trainers_add_the_penalty_on_both_loss_paths(regime):
    import torchkge_amd as tk
    from torchkge_amd.utils.regularizers import N3Regularizer
    from torchkge_amd.utils.training import OneVsAllTrainer, KvsAllTrainer
    cls = OneVsAllTrainer if regime == 'one_vs_all' else KvsAllTrainer
    kg = small_kg(n=3 * B)
    start = build('DistMult', 64)
    state = {k: v.clone() for k, v in start.state_dict().items()}

    def fresh():
        m = build('DistMult', 64)
        m.load_state_dict(state)
        return m
    reg = N3Regularizer(0.05, relation_weight=0.02)
    plain = dense_trainer(cls, fresh(), kg)
    plain.run()
    model = fresh()
    with_reg = dense_trainer(cls, model, kg)
    with_reg.regularizer = reg
    if regime == 'one_vs_all':
        ids = ((kg.head_idx.cuda(), kg.tail_idx.cuda()), (kg.relations.cuda(),))
    else:
        plain_keys = next(KvsAllTrainer.key_batches(plain._indexes['tail'], 1000))
        ids = ((plain_keys[0].cuda(),), (plain_keys[1].cuda(),))
    pen64, _, d_max = reference(fresh(), reg, *ids)
    with_reg.run()
    assert len(plain.epoch_losses) == len(with_reg.epoch_losses) == 1
    crit, total = plain.epoch_losses[0], with_reg.epoch_losses[0]
    # the criterion's own bits, the penalty within its bound, their fp32 sum rounded once
    assert abs(total - (crit + pen64)) <= (18 + math.ceil(d_max / 256)) * U * pen64 + U * abs(crit + pen64)
    assert pen64 > 100 * U * abs(crit)      # the penalty is visible in the sum
    # sync_free: the same step losses, criterion and penalty added one by one in fp32 on the device (two roundings per
    # step, each at most u |sum|) instead of as fl(criterion + penalty) in double on the host (one): 3 u |sum| per step
    for batch in (1000, 16):
        host = dense_trainer(cls, fresh(), kg, batch=batch, n_epochs=2)
        free = dense_trainer(cls, fresh(), kg, batch=batch, n_epochs=2, sync_free=True)
        host.regularizer = free.regularizer = reg
        with tk.deterministic():        # (the second epoch starts from the first one's tables: the same bits on both paths)
            host.run()
            free.run()
        steps = host._n_batches()
        assert len(host.epoch_losses) == len(free.epoch_losses) == 2
        for x, y in zip(host.epoch_losses, free.epoch_losses):
            assert abs(x - y) <= 3 * steps * U * abs(x), (batch, x, y)
        if batch == 1000:
            assert abs(host.epoch_losses[0] - total) <= U * abs(total)


@pytest.mark.parametrize('name', ['ComplEx', 'RotatE'])
def test_regularizer_none_gives_the_bits_of_a_trainer_that_never_had_the_attribute_set(name):
    """Inside deterministic(): outside it the small-batch backward adds with float atomics, whose order is no
    function of the trainer."""
    import torchkge_amd as tk

    def one(set_none):
        torch.manual_seed(6)
        torch.cuda.manual_seed(6)
        model, kg = build(name, 64, seed=6), small_kg(n=3 * B)
        tr = nssa_trainer(model, kg, torch.optim.Adagrad(model.parameters(), lr=0.05), batch=16)
        if set_none:
            tr.regularizer = None
        else:
            assert 'regularizer' not in tr.__dict__
        tr.run()
        return {k: v.detach().cpu() for k, v in model.state_dict().items()}, list(tr.epoch_losses)
    with tk.deterministic():
        a, la = one(False)
        b, lb = one(True)
    assert la == lb
    for k in a:
        assert torch.equal(a[k], b[k]), k
