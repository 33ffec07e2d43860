"""GPU tests of 1-vs-all training at model level (run with -m gpu on an MI355X): ``one_vs_all_loss`` of DistMultModel and
ComplExModel, ``all_candidates_cross_entropy`` and ``OneVsAllTrainer``.

Yardstick: float64 autograd on the CPU of the formula written out below (``formula``: the query rows of
inference_scoring_function, the materialised (B, N) score matrix, torch's cross_entropy) on copies of the tables.
Comparator: the same formula in fp32 on the device.  Tolerance, the project's usual shape: 4 * (2 * |fp32 - float64| +
one fp32 ulp of the value) -- of the loss for the loss, in max-norm with the ulp of the largest float64 entry for a
gradient table or a trained table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

N_ENT, N_REL, B = 300, 7, 70
DIMS = {'distmult': 20, 'complex': 12}


@pytest.fixture(scope='module')
def tk():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import torchkge_amd
    from torchkge_amd import _hip_xent
    _hip_xent.load_library()
    return torchkge_amd


def ulp_of(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def build(tk, name, seed=0):
    torch.manual_seed(seed)
    cls = {'distmult': tk.DistMultModel, 'complex': tk.ComplExModel}[name]
    return cls(DIMS[name], N_ENT, N_REL).cuda()


def facts(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, N_ENT, (n,), generator=g), torch.randint(0, N_ENT, (n,), generator=g),
            torch.randint(0, N_REL, (n,), generator=g))


def scores(name, tabs, h, t, r, side):
    """The materialised (B, N) -- 'both': (2B, N), tail side first -- score matrix of inference_scoring_function."""
    if side == 'both':
        return torch.cat([scores(name, tabs, h, t, r, 'tail'), scores(name, tabs, h, t, r, 'head')])
    if name == 'distmult':
        E, R = tabs
        q = E[h] * R[r] if side == 'tail' else R[r] * E[t]
        return q @ E.t()
    Ere, Eim, Rre, Rim = tabs
    if side == 'tail':
        q0, q1 = Ere[h] * Rre[r] - Eim[h] * Rim[r], Ere[h] * Rim[r] + Eim[h] * Rre[r]
    else:
        q0, q1 = Rre[r] * Ere[t] + Rim[r] * Eim[t], Rre[r] * Eim[t] - Rim[r] * Ere[t]
    return q0 @ Ere.t() + q1 @ Eim.t()


def formula(name, tabs, h, t, r, side, eps, reduction='mean'):
    target = {'tail': t, 'head': h, 'both': torch.cat([t, h])}[side]
    return F.cross_entropy(scores(name, tabs, h, t, r, side), target, label_smoothing=eps, reduction=reduction)


def loss_and_grads(name, init, h, t, r, side, eps, dtype, device):
    tabs = [x.to(device=device, dtype=dtype).clone().requires_grad_() for x in init]
    loss = formula(name, tabs, h.to(device), t.to(device), r.to(device), side, eps)
    return loss.detach(), torch.autograd.grad(loss, tabs)


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('side', ['both', 'tail', 'head'])
@pytest.mark.parametrize('name', ['distmult', 'complex'])
def test_loss_and_every_table_gradient_match_float64_autograd(tk, name, side, eps):
    model = build(tk, name)
    params = list(model.parameters())
    init = [p.detach().cpu().clone() for p in params]
    h, t, r = facts(B, 3)
    loss = model.one_vs_all_loss(h.cuda(), t.cuda(), r.cuda(), side=side, label_smoothing=eps)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    l64, g64 = loss_and_grads(name, init, h, t, r, side, eps, torch.float64, 'cpu')
    l32, g32 = loss_and_grads(name, init, h, t, r, side, eps, torch.float32, 'cuda')
    d_ours, d_cmp = abs(float(loss.detach()) - float(l64)), abs(float(l32) - float(l64))
    tol = 4 * (2 * d_cmp + ulp_of(l64))
    print('one_vs_all %-8s %-4s eps=%g loss %.9g: |engine - f64| %.3g (torch fp32 %.3g, bound %.3g)'
          % (name, side, eps, float(l64), d_ours, d_cmp, tol))
    assert d_ours <= tol
    for i, p in enumerate(params):
        assert p.grad is not None and not p.grad.is_sparse and p.grad.shape == p.shape     # dense, by nature
        d_ours = float((p.grad.double().cpu() - g64[i]).abs().max())
        d_cmp = float((g32[i].double().cpu() - g64[i]).abs().max())
        tol = 4 * (2 * d_cmp + ulp_of(g64[i].abs().max()))
        print('one_vs_all %-8s %-4s eps=%g table %d gradient: |engine - f64| %.3g (torch fp32 %.3g, bound %.3g, max %.3g)'
              % (name, side, eps, i, d_ours, d_cmp, tol, float(g64[i].abs().max())))
        assert d_ours <= tol, (name, side, eps, i)


def test_the_scores_are_the_evaluators_and_the_reductions_are_torchs(tk):
    """all_candidates_cross_entropy on explicit operands: 'none' is lse - (the pair kernel's target score) bit for bit,
    'sum' / 'mean' are torch's reductions of it; only the wanted gradients come back."""
    from torchkge_amd import _hip, _hip_xent
    from torchkge_amd.utils.one_vs_all import all_candidates_cross_entropy
    g = torch.Generator().manual_seed(8)
    Q = (torch.randn(B, 24, generator=g) * 0.6).cuda().requires_grad_()
    E = torch.randn(N_ENT, 24, generator=g).cuda()
    t = torch.randint(0, N_ENT, (B,), generator=g).cuda()
    rows = all_candidates_cross_entropy(Q, E, t, reduction='none')
    prob = _hip.LpProblem(_hip.LP_DOT, Q.detach(), E)
    lse, row_loss = _hip_xent.xent_fwd(prob, t)
    assert torch.equal(rows.detach(), row_loss) and torch.equal(row_loss, lse - prob.pair_scores(t))
    assert torch.equal(all_candidates_cross_entropy(Q, E, t, reduction='sum').detach(), rows.detach().sum())
    assert torch.equal(all_candidates_cross_entropy(Q, E, t).detach(), rows.detach().mean())
    rows.sum().backward()
    assert Q.grad is not None and Q.grad.shape == Q.shape and E.grad is None
    # two segments continue one chain: with K0 a multiple of 8 the k-order is that of the single segment, so are the bits
    two = all_candidates_cross_entropy((Q[:, :8], Q[:, 8:]), (E[:, :8], E[:, 8:]), t, reduction='none')
    assert torch.equal(two.detach(), rows.detach())


# ---------------------------------------------------------------------------
# OneVsAllTrainer
# ---------------------------------------------------------------------------
N_FACTS, B_SIZE, N_EPOCHS, LR = 200, 64, 2, 0.5


def make_kg(tk, n=N_FACTS, seed=5):
    h, t, r = facts(n, seed)
    return tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(N_ENT)},
                             rel2ix={i: i for i in range(N_REL)})


def trained(tk, name, kg, n_epochs=N_EPOCHS, sync_free=False, eps=0.1):
    from torchkge_amd.utils.training import OneVsAllTrainer
    model = build(tk, name)
    tr = OneVsAllTrainer(model, kg, n_epochs, B_SIZE, torch.optim.SGD(model.parameters(), lr=LR), label_smoothing=eps,
                         use_cuda='all', sync_free=sync_free, verbose=False)
    tr.run()
    return tr, [p.detach().clone() for p in model.parameters()]


@pytest.mark.parametrize('name', ['distmult', 'complex'])
def test_two_deterministic_runs_give_the_same_bits(tk, name):
    kg = make_kg(tk)
    assert N_FACTS % B_SIZE == 8        # a short last batch
    with tk.deterministic():
        a, tabs_a = trained(tk, name, kg)
        b, tabs_b = trained(tk, name, kg)
        s, tabs_s = trained(tk, name, kg, sync_free=True)
    init = [p.detach() for p in build(tk, name).parameters()]
    assert max(float((x - y).abs().max()) for x, y in zip(tabs_a, init)) > 1e-4      # it trained
    for x, y, z in zip(tabs_a, tabs_b, tabs_s):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert a.epoch_losses == b.epoch_losses and len(a.epoch_losses) == N_EPOCHS and np.isfinite(a.epoch_losses).all()
    # the sync_free epoch means: the same step losses added in fp32 on the device, k - 1 roundings of half an ulp
    assert s._epoch_sums is not None
    k = 4
    for e in range(N_EPOCHS):
        total = a.epoch_losses[e] * k
        dist, bound = abs(s.epoch_losses[e] - a.epoch_losses[e]), 0.5 * (k - 1) * ulp_of(total) / k
        print('one_vs_all sync_free %-8s epoch %d mean loss %.9g: |device sum - step losses| %.3g (bound %.3g)'
              % (name, e, a.epoch_losses[e], dist, bound))
        assert dist <= bound, e
    assert s._epoch_sums is None


def hand_loop(name, init, kg, steps, eps, dtype, device):
    """`steps` SGD steps of the materialised formula in plain torch, DistMult's normalisation at the end (one epoch)."""
    tabs = [x.to(device=device, dtype=dtype).clone().requires_grad_() for x in init]
    H, T, R = kg.head_idx.to(device), kg.tail_idx.to(device), kg.relations.to(device)
    for s in range(steps):
        sl = slice(s * B_SIZE, (s + 1) * B_SIZE)
        grads = torch.autograd.grad(formula(name, tabs, H[sl], T[sl], R[sl], 'both', eps), tabs)
        with torch.no_grad():
            for x, g in zip(tabs, grads):
                x -= LR * g
    if name == 'distmult':
        with torch.no_grad():
            tabs[0].copy_(F.normalize(tabs[0], p=2, dim=1))
    return [x.detach().double().cpu() for x in tabs]


@pytest.mark.parametrize('name', ['distmult', 'complex'])
def test_three_steps_against_the_hand_written_loop(tk, name):
    kg = make_kg(tk, n=3 * B_SIZE, seed=6)
    eps = 0.1
    init = [p.detach().cpu().clone() for p in build(tk, name).parameters()]
    _, tabs = trained(tk, name, kg, n_epochs=1, eps=eps)
    ref64 = hand_loop(name, init, kg, 3, eps, torch.float64, 'cpu')
    ref32 = hand_loop(name, init, kg, 3, eps, torch.float32, 'cuda')
    ref_dist = max(float((a - b).abs().max()) for a, b in zip(ref32, ref64))
    bound = 4 * (2 * ref_dist + ulp_of(max(float(b.abs().max()) for b in ref64)))
    got = max(float((a.double().cpu() - b).abs().max()) for a, b in zip(tabs, ref64))
    print('one_vs_all trainer %-8s tables after 3 steps |engine - f64| %.3g (torch fp32 %.3g, bound %.3g)'
          % (name, got, ref_dist, bound))
    assert max(float((a.double() - b).abs().max()) for a, b in zip(init, ref64)) > 1e-4      # it trained
    assert got <= bound
