"""GPU tests of K-vs-all training at model level (run with -m gpu on an MI355X): ``k_vs_all_loss`` of DistMultModel and
ComplExModel, ``all_candidates_bce`` and ``KvsAllTrainer``.

Yardstick: float64 autograd on the CPU of the formula written out below (``formula``: the query rows of
inference_scoring_function, the materialised (B, N) score matrix, a dense label matrix scattered from the CSR, torch's
binary_cross_entropy_with_logits) on copies of the tables.  Comparator: the same formula in fp32 on the device.
Tolerance, the project's usual shape: 4 * (2 * |fp32 - float64| + one fp32 ulp of the value) -- in max-norm with the ulp
of the largest float64 entry for a loss vector, a gradient table or a trained table.

The graph: 150 entities (more than two candidate tiles), 5 relations, random facts and one hub key -- (0, 0) with 140
tails, a label segment longer than two tiles."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bce_ref

pytestmark = pytest.mark.gpu

N_ENT, N_REL, N_RANDOM, HUB = 150, 5, 260, 140
DIMS = {'distmult': 20, 'complex': 12}


@pytest.fixture(scope='module')
def tk():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import torchkge_amd
    from torchkge_amd import _hip_bce
    _hip_bce.load_library()
    return torchkge_amd


def ulp_of(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def build(tk, name, seed=0):
    torch.manual_seed(seed)
    cls = {'distmult': tk.DistMultModel, 'complex': tk.ComplExModel}[name]
    return cls(DIMS[name], N_ENT, N_REL).cuda()


def facts(seed=3):
    g = torch.Generator().manual_seed(seed)
    h, t, r = (torch.randint(0, m, (N_RANDOM,), generator=g) for m in (N_ENT, N_ENT, N_REL))
    hub_t = torch.randperm(N_ENT, generator=g)[:HUB]
    order = torch.randperm(N_RANDOM + HUB, generator=g)
    return (torch.cat([h, torch.zeros(HUB, dtype=torch.long)])[order], torch.cat([t, hub_t])[order],
            torch.cat([r, torch.zeros(HUB, dtype=torch.long)])[order])


def make_kg(tk, seed=3):
    h, t, r = facts(seed)
    return tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(N_ENT)},
                             rel2ix={i: i for i in range(N_REL)})


def host_index(kg, side):
    """The side's FilterIndex on the host (numpy): bit-identical to the one the trainer builds on the device."""
    from torchkge_amd.filter_index import FilterIndex
    h, t, r = kg.head_idx.numpy(), kg.tail_idx.numpy(), kg.relations.numpy()
    return FilterIndex.from_triples(h, r, t, 'cpu') if side == 'tail' else FilterIndex.from_triples(t, r, h, 'cpu')


def all_keys(index):
    from torchkge_amd.utils.training import KvsAllTrainer
    (batch,) = list(KvsAllTrainer.key_batches(index, index.n_keys))
    return batch


def scores(name, tabs, e, r, side):
    """The materialised (B, N) score matrix of inference_scoring_function for the keys (e, r)."""
    if name == 'distmult':
        E, R = tabs
        return (E[e] * R[r]) @ E.t()
    Ere, Eim, Rre, Rim = tabs
    if side == 'tail':
        q0, q1 = Ere[e] * Rre[r] - Eim[e] * Rim[r], Ere[e] * Rim[r] + Eim[e] * Rre[r]
    else:
        q0, q1 = Rre[r] * Ere[e] + Rim[r] * Eim[e], Rre[r] * Eim[e] - Rim[r] * Ere[e]
    return q0 @ Ere.t() + q1 @ Eim.t()


def formula(name, tabs, e, r, Y, side, eps, reduction='mean'):
    S = scores(name, tabs, e, r, side)
    Ys = ((1.0 - eps) * Y + eps / Y.shape[1]).to(S.dtype)
    rows = F.binary_cross_entropy_with_logits(S, Ys, reduction='none').sum(dim=1)
    if reduction == 'none':
        return rows
    return rows.sum() if reduction == 'sum' else rows.sum() / (Y.shape[0] * Y.shape[1])


def loss_and_grads(name, init, e, r, Y, w, side, eps, reduction, dtype, device):
    tabs = [x.to(device=device, dtype=dtype).clone().requires_grad_() for x in init]
    loss = formula(name, tabs, e.to(device), r.to(device), Y.to(device), side, eps, reduction)
    scalar = loss if loss.dim() == 0 else (loss * w.to(device=device, dtype=dtype)).sum()
    return loss.detach(), torch.autograd.grad(scalar, tabs)


@pytest.mark.parametrize('reduction', ['mean', 'sum', 'none'])
@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('side', ['tail', 'head'])
@pytest.mark.parametrize('name', ['distmult', 'complex'])
def test_loss_and_every_table_gradient_match_float64_autograd(tk, name, side, eps, reduction):
    kg = make_kg(tk)
    index = host_index(kg, side)
    e, r, lo, hi = all_keys(index)
    B = e.shape[0]
    assert B > 128 and (side == 'head' or int((hi - lo).max()) >= HUB > 128)     # more than two row panels, one hub key
    Y = bce_ref.dense_labels(lo, hi, index.targets, N_ENT)
    w = torch.rand(B, generator=torch.Generator().manual_seed(9)) + 0.5
    model = build(tk, name)
    params = list(model.parameters())
    init = [p.detach().cpu().clone() for p in params]
    labels = (lo.cuda(), hi.cuda(), index.targets.cuda())
    loss = model.k_vs_all_loss(e.cuda(), r.cuda(), labels, side, label_smoothing=eps, reduction=reduction)
    assert loss.dtype == torch.float32 and loss.shape == ((B,) if reduction == 'none' else ())
    (loss if loss.dim() == 0 else (loss * w.cuda()).sum()).backward()
    l64, g64 = loss_and_grads(name, init, e, r, Y, w, side, eps, reduction, torch.float64, 'cpu')
    l32, g32 = loss_and_grads(name, init, e, r, Y, w, side, eps, reduction, torch.float32, 'cuda')
    d_ours = float((loss.detach().double().cpu() - l64).abs().max())
    d_cmp = float((l32.double().cpu() - l64).abs().max())
    tol = 4 * (2 * d_cmp + ulp_of(l64.abs().max()))
    print('k_vs_all %-8s %-4s eps=%g %-4s loss %.9g: |engine - f64| %.3g (torch fp32 %.3g, bound %.3g)'
          % (name, side, eps, reduction, float(l64.abs().max()), d_ours, d_cmp, tol))
    assert d_ours <= tol
    for i, p in enumerate(params):
        assert p.grad is not None and not p.grad.is_sparse and p.grad.shape == p.shape     # dense, by nature
        d_ours = float((p.grad.double().cpu() - g64[i]).abs().max())
        d_cmp = float((g32[i].double().cpu() - g64[i]).abs().max())
        tol = 4 * (2 * d_cmp + ulp_of(g64[i].abs().max()))
        print('k_vs_all %-8s %-4s eps=%g %-4s table %d gradient: |engine - f64| %.3g (torch fp32 %.3g, bound %.3g, max %.3g)'
              % (name, side, eps, reduction, i, d_ours, d_cmp, tol, float(g64[i].abs().max())))
        assert d_ours <= tol, (name, side, eps, i)


def test_the_scores_are_the_engines_and_the_reductions_are_torchs(tk):
    """all_candidates_bce on explicit operands whose scores are integers 512 m +- 200: every softplus is max(s, 0) exactly
    (expf(-200) is 0), every sum is exact, so 'none' is fp32(sum_c max(s, 0) - sum over the labels of s) of the engine's
    ``scores()`` bit for bit; 'sum' / 'mean' are torch's reductions of it; only the wanted gradients come back."""
    from torchkge_amd import _hip
    from torchkge_amd.utils.k_vs_all import all_candidates_bce
    g = torch.Generator().manual_seed(8)
    B, K = 70, 9
    Q = torch.randint(-3, 4, (B, K), generator=g).float() * 512.0
    E = torch.randint(-3, 4, (N_ENT, K), generator=g).float()
    Q[:, -1], E[:, -1] = 1.0, (torch.randint(0, 2, (N_ENT,), generator=g).float() * 2 - 1) * 200.0
    lens = torch.randint(0, 6, (B,), generator=g)
    lens[0], lens[1] = N_ENT, 0
    sets = [torch.randperm(N_ENT, generator=g)[:int(n)].sort().values for n in lens]
    hi = torch.cumsum(lens, 0)
    labels = ((hi - lens).cuda(), hi.cuda(), torch.cat(sets).to(torch.int32).cuda())
    Q, E = Q.cuda().requires_grad_(), E.cuda()
    S = _hip.LpProblem(_hip.LP_DOT, Q.detach(), E).scores()
    assert float(S.abs().min()) >= 200 and bool((S == S.round()).all()) and float(S.abs().max()) < 2 ** 24
    Y = bce_ref.dense_labels(*labels, N_ENT).cuda()
    expect = (S.double().clamp(min=0).sum(dim=1) - (S.double() * Y).sum(dim=1)).float()
    rows = all_candidates_bce(Q, E, labels, reduction='none')
    assert torch.equal(rows.detach(), expect)
    assert torch.equal(all_candidates_bce(Q, E, labels, reduction='sum').detach(), rows.detach().sum())
    assert torch.equal(all_candidates_bce(Q, E, labels).detach(), rows.detach().sum() / float(B * N_ENT))
    rows.sum().backward()
    assert Q.grad is not None and Q.grad.shape == Q.shape and E.grad is None
    # two segments continue one chain: with K0 a multiple of 8 the k-order is that of the single segment, so are the bits
    Qd = Q.detach()
    two = all_candidates_bce((Qd[:, :8], Qd[:, 8:]), (E[:, :8], E[:, 8:]), labels, reduction='none')
    assert torch.equal(two, rows.detach())


@pytest.mark.parametrize('side', ['tail', 'head'])
@pytest.mark.parametrize('name', ['distmult', 'complex'])
def test_the_query_rows_are_the_evaluators(tk, name, side):
    """k_vs_all_loss is all_candidates_bce on the rows of _hip.lp_prep -- what the evaluator scores -- and the raw tables."""
    from torchkge_amd import _hip
    from torchkge_amd.utils.k_vs_all import all_candidates_bce
    kg = make_kg(tk)
    index = host_index(kg, side)
    e, r, lo, hi = (x.cuda() for x in all_keys(index))
    labels = (lo, hi, index.targets.cuda())
    model = build(tk, name)
    tabs = [x.detach() for x in model._tables()]
    q = _hip.lp_prep(model._hip_kind(), _hip.side_code(side), tabs, model._d_ent, model._d_rel, e, e, r,
                     want_q1=name == 'complex')
    n_et = len(model._ENT_TABLES)
    direct = all_candidates_bce(tuple(q[:n_et]), tuple(tabs[:n_et]), labels, 0.1, 'none')
    with torch.no_grad():
        got = model.k_vs_all_loss(e, r, labels, side, label_smoothing=0.1, reduction='none')
    assert torch.equal(got, direct)


# ---------------------------------------------------------------------------
# KvsAllTrainer
# ---------------------------------------------------------------------------
LR = 0.5


def trained(tk, name, kg, side, batch_size, n_epochs=2, sync_free=False, eps=0.1, use_cuda='all'):
    from torchkge_amd.utils.training import KvsAllTrainer
    model = build(tk, name)
    tr = KvsAllTrainer(model, kg, n_epochs, batch_size, torch.optim.SGD(model.parameters(), lr=LR), label_smoothing=eps,
                       side=side, use_cuda=use_cuda, sync_free=sync_free, verbose=False)
    tr.run()
    return tr, [p.detach().clone() for p in model.parameters()]


@pytest.mark.parametrize('name', ['distmult', 'complex'])
def test_two_deterministic_runs_give_the_same_bits(tk, name):
    kg = make_kg(tk)
    n_tail, n_head = host_index(kg, 'tail').n_keys, host_index(kg, 'head').n_keys
    bs = 100
    assert n_tail % bs and n_head % bs      # a short last batch on both sides
    k = -(-n_tail // bs) + -(-n_head // bs)
    with tk.deterministic():
        a, tabs_a = trained(tk, name, kg, 'both', bs)
        b, tabs_b = trained(tk, name, kg, 'both', bs)
        s, tabs_s = trained(tk, name, kg, 'both', bs, sync_free=True)
        c, tabs_c = trained(tk, name, kg, 'both', bs, use_cuda='batch')
    assert a.n_batches() == k
    init = [p.detach() for p in build(tk, name).parameters()]
    assert max(float((x - y).abs().max()) for x, y in zip(tabs_a, init)) > 1e-5      # it trained
    for x, y, z, u in zip(tabs_a, tabs_b, tabs_s, tabs_c):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, u)
    assert a.epoch_losses == b.epoch_losses == c.epoch_losses and len(a.epoch_losses) == 2
    assert np.isfinite(a.epoch_losses).all()
    # the sync_free epoch means: the same step losses added in fp32 on the device, k - 1 roundings of half an ulp
    assert s._epoch_sums is not None
    for ep in range(2):
        total = a.epoch_losses[ep] * k
        dist, bound = abs(s.epoch_losses[ep] - a.epoch_losses[ep]), 0.5 * (k - 1) * ulp_of(total) / k
        print('k_vs_all sync_free %-8s epoch %d mean loss %.9g: |device sum - step losses| %.3g (bound %.3g)'
              % (name, ep, a.epoch_losses[ep], dist, bound))
        assert dist <= bound, ep
    assert s._epoch_sums is None


def hand_loop(name, init, kg, side, batch_size, steps, eps, dtype, device):
    """`steps` SGD steps of the materialised formula in plain torch over the trainer's key batches, DistMult's
    normalisation at the end (one epoch)."""
    from torchkge_amd.utils.training import KvsAllTrainer
    tabs = [x.to(device=device, dtype=dtype).clone().requires_grad_() for x in init]
    index = host_index(kg, side)
    batches = list(KvsAllTrainer.key_batches(index, batch_size))
    assert len(batches) == steps
    for e, r, lo, hi in batches:
        Y = bce_ref.dense_labels(lo, hi, index.targets, N_ENT).to(device)
        grads = torch.autograd.grad(formula(name, tabs, e.to(device), r.to(device), Y, side, eps), tabs)
        with torch.no_grad():
            for x, g in zip(tabs, grads):
                x -= LR * g
    if name == 'distmult':
        with torch.no_grad():
            tabs[0].copy_(F.normalize(tabs[0], p=2, dim=1))
    return [x.detach().double().cpu() for x in tabs]


@pytest.mark.parametrize('name,side', [('distmult', 'tail'), ('complex', 'head')])
def test_three_steps_against_the_hand_written_loop(tk, name, side):
    kg = make_kg(tk, seed=6)
    eps = 0.1
    bs = -(-host_index(kg, side).n_keys // 3)
    init = [p.detach().cpu().clone() for p in build(tk, name).parameters()]
    tr, tabs = trained(tk, name, kg, side, bs, n_epochs=1, eps=eps)
    assert tr.n_batches() == 3
    # mean over B * N makes the gradients small: a learning rate that moves the tables is the test's, not a recommendation
    ref64 = hand_loop(name, init, kg, side, bs, 3, eps, torch.float64, 'cpu')
    ref32 = hand_loop(name, init, kg, side, bs, 3, eps, torch.float32, 'cuda')
    ref_dist = max(float((a - b).abs().max()) for a, b in zip(ref32, ref64))
    bound = 4 * (2 * ref_dist + ulp_of(max(float(b.abs().max()) for b in ref64)))
    got = max(float((a.double().cpu() - b).abs().max()) for a, b in zip(tabs, ref64))
    print('k_vs_all trainer %-8s tables after 3 steps |engine - f64| %.3g (torch fp32 %.3g, bound %.3g)'
          % (name, got, ref_dist, bound))
    assert max(float((a.double() - b).abs().max()) for a, b in zip(init, ref64)) > 1e-6      # it trained
    assert got <= bound
