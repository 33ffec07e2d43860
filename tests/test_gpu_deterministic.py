"""GPU tests of the deterministic training mode (run with -m gpu on an MI355X): kge_segment_sum_ordered
(include/kge_hip_det.h) against float64 with its layout contract, the same bits on repeated and on differently scheduled
calls, every model's backward twice inside ``tk.deterministic()`` against the reference its own backward test uses, two
trainings from one seed, and the untouched default path."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.helpers import load_golden, raw
from tests import analogy_ref as ar
from tests import convkb_ref as cr
from tests.test_transr_host import scoring64 as transr_sf64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24      # unit roundoff of fp32


@pytest.fixture(scope='module')
def D():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_det
    _hip_det.load_library()
    return _hip_det


# ---------------------------------------------------------------------------
# 1. the kernel against float64, with its layout contract
# ---------------------------------------------------------------------------
def key_cases():
    """(name, keys in caller order, n_keys).  Every case leaves some key of [0, n_keys) unused."""
    g = torch.Generator().manual_seed(7)
    out = []
    for M in (1, 31, 32, 33, 65):                           # below / at / above one chunk, three chunks
        k = torch.randint(0, 9, (M,), generator=g)         # (keys 9 and 10 never occur)
        k[0] = 0                                            # the lowest key ...
        if M > 1:
            k[-1] = 11                                      # ... and the highest, n_keys - 1
        out.append(('M%d' % M, k, 12))
    out.append(('distinct', torch.randperm(130, generator=g)[:100], 130))
    out.append(('equal2053', torch.full((2053,), 3, dtype=torch.int64), 5))      # 65 chunks -> 130 slots -> 10 -> 1 chunk
    runs = torch.cat([torch.full((n,), k, dtype=torch.int64) for k, n in ((0, 32), (1, 32), (2, 64), (4, 1))])
    out.append(('runs_on_boundaries', runs[torch.randperm(runs.shape[0], generator=g)], 6))
    runs = torch.cat([torch.full((n,), k, dtype=torch.int64) for k, n in ((1, 31), (2, 40), (6, 5))])
    out.append(('run_from_a_chunks_last_entry', runs[torch.randperm(runs.shape[0], generator=g)], 7))
    return out


def nan_padded(mat, pad):
    """(rows, cols + pad) buffer, NaN in the pad columns, and its [:, :cols] view holding ``mat``."""
    buf = torch.full((mat.shape[0], mat.shape[1] + pad), float('nan'), dtype=torch.float32, device='cuda')
    buf[:, :mat.shape[1]] = mat
    return buf


@pytest.mark.parametrize('d', [1, 63, 64, 65, 200, 256, 257, 512, 513, 1024])
def test_ordered_sum_vs_float64_and_layout_contract(D, d):
    g = torch.Generator().manual_seed(1000 + d)
    for name, keys, n_keys in key_cases():
        M = keys.shape[0]
        x = torch.randn(M, d, generator=g)
        perm = torch.sort(keys, stable=True).indices
        n_run = torch.bincount(keys, minlength=n_keys).double().view(-1, 1)
        sum64 = torch.zeros(n_keys, d, dtype=torch.float64).index_add_(0, keys, x.double())
        abs64 = torch.zeros(n_keys, d, dtype=torch.float64).index_add_(0, keys, x.double().abs())
        pattern = (torch.arange(n_keys * d, dtype=torch.float32).view(n_keys, d) % 13 - 6.25) * 0.37
        assert float(n_run.max()) * U < 0.01 and bool((n_run == 0).any())
        rows = nan_padded(x, 3)
        kd, pd = keys.cuda(), perm.cuda()
        for n0 in sorted({M, M // 3}):                      # n1 = 0 with k1 = NULL, and n1 > 0
            k0, k1 = kd[:n0].contiguous(), (kd[n0:].contiguous() if n0 < M else None)
            for fill in (torch.zeros(n_keys, d), pattern):
                out = nan_padded(fill, 5)
                before = out.clone()
                D.segment_sum_ordered(rows, d + 3, d, k0, n0, k1, M - n0, pd, out, d + 5)
                got = out[:, :d].cpu()
                tag = (name, d, n0)
                # the pads of `out` stay NaN bit for bit; rows whose key does not occur keep every bit
                bits = lambda x: x.contiguous().view(torch.int32)       # noqa: E731 (NaN pads compare as integers)
                assert torch.equal(bits(out[:, d:]), bits(before[:, d:])), tag
                absent = (n_run.view(-1) == 0).cuda()
                assert torch.equal(bits(out[absent]), bits(before[absent])), tag
                assert bool(torch.isfinite(got).all()), tag          # no pad column of `rows` reached a sum
                # forward bound of ANY fp32 summation order: n - 1 adds of the run's rows (<= n u sum |x|); a non-zero
                # `out` is one more term of the same sum
                fill64 = fill.double()
                err = (got.double() - (fill64 + sum64)).abs()
                bound = 1.01 * n_run * U * (abs64 + fill64.abs())
                assert bool((err <= bound).all()), (tag, float((err - bound).max()))
                if not fill.any():                          # a run of one row is that row
                    one = (n_run.view(-1) == 1)
                    assert torch.equal(got[one], sum64[one].float()), tag


def test_bad_arguments_are_refused_and_out_is_untouched(D):
    lib = D.load_library()
    M, d, n_keys = 100, 8, 5
    g = torch.Generator().manual_seed(3)
    keys = torch.randint(0, n_keys, (M,), generator=g).cuda()
    perm = torch.sort(keys, stable=True).indices
    rows = torch.randn(M, d + 3, generator=g).cuda()
    out = torch.full((n_keys, d + 5), 1.5, device='cuda')
    before = out.clone()
    nb = D.ws_bytes(M, d)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')

    def call(d_, ld, nbytes):
        return raw(lib, 'kge_segment_sum_ordered', rows, ld, d_, keys, M, None, 0, perm, out, d + 5, ws, nbytes)
    assert call(0, d + 3, nb) != 0 and call(1025, 1030, nb) != 0        # d outside [1, 1024]
    assert call(d, d - 1, nb) != 0                                      # ld < d
    assert call(d, d + 3, nb - 1) != 0                                  # workspace one byte short
    assert raw(lib, 'kge_segment_sum_ordered', rows, d + 3, d, keys, M, None, 0, perm, out, d - 1, ws, nb) != 0   # out_ld < d
    assert raw(lib, 'kge_segment_sum_ordered', rows, d + 3, d, keys, M, None, 0, perm, out, d + 5, None, nb) != 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    assert raw(lib, 'kge_segment_sum_ordered', None, d, d, None, 0, None, 0, None, None, d, None, 0) == 0   # M = 0: a no-op
    assert call(d, d + 3, nb) == 0
    torch.cuda.synchronize()
    assert not torch.equal(out, before)


# ---------------------------------------------------------------------------
# 2. the same bits under contention and beside other work
# ---------------------------------------------------------------------------
def test_same_bits_under_contention_and_beside_a_busy_stream(D):
    M, d, n_keys = 65536, 64, 501
    g = torch.Generator().manual_seed(5)
    keys = torch.where(torch.rand(M, generator=g) < 0.9, torch.zeros(M, dtype=torch.int64),
                       torch.randint(1, n_keys, (M,), generator=g))
    # magnitudes over 40 binades: the order of the additions shows in the low bits of the sum
    x = torch.randn(M, d, generator=g) * torch.exp2(torch.rand(M, d, generator=g) * 40 - 20)
    perm = torch.sort(keys, stable=True).indices.cuda()
    keys, x = keys.cuda(), x.cuda()

    def run():
        out = torch.zeros(n_keys, d, device='cuda')
        D.segment_sum_ordered(x, d, d, keys, M, None, 0, perm, out, d)
        return out
    outs = [run() for _ in range(4)]
    # (it is the sum: the forward bound of the kernel test, n u = 0.0035 for the 59,000 rows of key 0)
    ref = torch.zeros(n_keys, d, dtype=torch.float64, device='cuda').index_add_(0, keys, x.double())
    mag = torch.zeros(n_keys, d, dtype=torch.float64, device='cuda').index_add_(0, keys, x.double().abs())
    n_run = torch.bincount(keys, minlength=n_keys).double().view(-1, 1)
    assert float(n_run.max()) * U < 0.01
    assert bool(((outs[0].double() - ref).abs() <= 1.01 * n_run * U * mag).all())
    # a different scheduling: an unrelated 64 MB copy loop on another stream while the reduction runs
    a = torch.empty(16 << 20, device='cuda')
    b = torch.empty_like(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(40):
            b.copy_(a)
    outs += [run() for _ in range(4)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(outs[0], o)


# ---------------------------------------------------------------------------
# 3. every model: backward twice inside the mode, and against the reference of the model's own backward test
# ---------------------------------------------------------------------------
def skewed_triples(B, n_ent, n_rel, g):
    """Three quarters of the triples on one relation and one head."""
    h = torch.randint(0, n_ent, (B,), generator=g)
    t = torch.randint(0, n_ent, (B,), generator=g)
    r = torch.randint(0, n_rel, (B,), generator=g)
    r[: (3 * B) // 4] = min(4, n_rel - 1)
    h[: (3 * B) // 4] = 3
    return h, t, r, torch.randn(B, generator=g)


def rel_bound(tol):
    return lambda ref: tol * max(1.0, float(ref.abs().max()))


def case_parity(kind, p, B):
    """tests/test_gpu_parity.py::test_scoring_function_backward_vs_autograd: the oracle's formulas under autograd."""
    from tests.test_gpu_parity import build_model
    z, tables = load_golden(kind, p)
    n_ent, n_rel = int(z['n_ent']), int(z['n_rel'])
    h, t, r, go = skewed_triples(B, n_ent, n_rel, torch.Generator().manual_seed(11))
    ref_tabs = [x.clone().cuda().requires_grad_(True) for x in tables]
    (orc.score_triples(kind, ref_tabs, h.cuda(), t.cuda(), r.cuda(), p=p) * go.cuda()).sum().backward()
    return dict(build=lambda: build_model(kind, p, tables, n_ent, n_rel), tables=lambda m: m._tables(), idx=(h, t, r), go=go,
                ref=[x.grad.cpu() for x in ref_tabs], bound=rel_bound(1e-4))


def case_rescal_hole(kind, B):
    """tests/test_gpu_rescal_hole.py::test_backward_vs_float64_autograd_and_repeatable"""
    from tests.test_gpu_rescal_hole import build, sf64
    n_ent, n_rel, d = 700, 9, 24
    g = torch.Generator().manual_seed(11)
    E = torch.randn(n_ent, d, generator=g) * 0.3
    rel = torch.randn(n_rel, d * d if kind == 'rescal' else d, generator=g) * 0.3
    h, t, r, go = skewed_triples(B, n_ent, n_rel, g)
    E64, R64 = E.double().requires_grad_(), rel.double().requires_grad_()
    (sf64(kind, E64, R64, d, h, t, r) * go.double()).sum().backward()
    return dict(build=lambda: build(kind, E, rel, n_ent, n_rel, d), tables=lambda m: [m.ent_emb.weight, m._rel_param().weight],
                idx=(h, t, r), go=go, ref=[E64.grad, R64.grad], bound=rel_bound(1e-5 * 10))


def case_toruse(diss, B):
    """tests/test_gpu_toruse.py::test_backward_large_batch_vs_float64_autograd"""
    from tests.test_gpu_toruse import build, diss64
    n_ent, n_rel, d = 500, 9, 40
    g = torch.Generator().manual_seed(11)
    E = torch.rand(n_ent, d, generator=g) * 5 - 2.5
    R = torch.rand(n_rel, d, generator=g) * 5 - 2.5
    h, t, r, go = skewed_triples(B, n_ent, n_rel, g)
    E64, R64 = E.double().requires_grad_(), R.double().requires_grad_()
    f = lambda x: x - torch.trunc(x).detach()      # noqa: E731 (frac with the identity gradient, as .data.frac_())
    xf = ((E - E.trunc())[h] + (R - R.trunc())[r]) - (E - E.trunc())[t]
    x64 = (f(E64)[h] + f(R64)[r]) - f(E64)[t]
    x64 = x64 + (xf.double() - x64).detach()
    (-diss64(diss, x64) * go.double()).sum().backward()
    return dict(build=lambda: build(diss, E, R, n_ent, n_rel, d), tables=lambda m: [m.ent_emb.weight, m.rel_emb.weight],
                idx=(h, t, r), go=go, ref=[E64.grad, R64.grad], bound=rel_bound(1e-4))


def case_transr(B):
    """tests/test_gpu_transr.py::test_backward_small / large_batch_vs_float64_autograd"""
    from tests.test_gpu_transr import build, random_tables
    n_ent, n_rel, de, dr, seed = (200, 6, 17, 9, 11) if B < 2048 else (500, 6, 40, 24, 12)
    E, R, P = random_tables(n_ent, n_rel, de, dr, seed)
    h, t, r, go = skewed_triples(B, n_ent, n_rel, torch.Generator().manual_seed(seed + 1))
    E64, R64, P64 = (x.double().requires_grad_(True) for x in (E, R, P))
    (transr_sf64(E64, R64, P64.view(n_rel, dr, de), h, t, r) * go.double()).sum().backward()
    return dict(build=lambda: build(E, R, P, de, dr), tables=lambda m: [m.ent_emb.weight, m.rel_emb.weight, m.proj_mat.weight],
                idx=(h, t, r), go=go, ref=[E64.grad, R64.grad, P64.grad], bound=rel_bound(1e-4))


def case_analogy(B):
    """tests/test_gpu_analogy.py::test_backward_vs_float64_autograd"""
    from tests.test_gpu_analogy import build, random_tables
    n_ent, n_rel, d_sc, d_c = 700, 9, 7, 10
    g = torch.Generator().manual_seed(11)
    tabs = random_tables(n_ent, n_rel, d_sc, d_c, g, 0.5)
    h, t, r, go = skewed_triples(B, n_ent, n_rel, g)
    t64 = [x.double().requires_grad_() for x in tabs]
    (ar.sf64(t64, h, t, r) * go.double()).sum().backward()
    return dict(build=lambda: build(tabs), tables=lambda m: [getattr(m, n).weight for n in ar.NAMES], idx=(h, t, r), go=go,
                ref=[x.grad for x in t64], bound=rel_bound(1e-5 * 10))


def case_convkb(B):
    """tests/test_gpu_convkb.py::test_backward_vs_float64_autograd"""
    from tests.test_gpu_convkb import build, rand_params, GRAD_TOL
    n_ent, n_rel, d, F = 700, 9, 9, 6
    g = torch.Generator().manual_seed(11 + B)
    params = rand_params(n_ent, n_rel, d, F, g, gain=3.0)
    h, t, r, go = skewed_triples(B, n_ent, n_rel, g)
    p64 = [x.double().requires_grad_() for x in params]
    (cr.sf64(p64, h, t, r) * go.double()).sum().backward()
    return dict(build=lambda: build(params), tables=lambda m: m._tables(), idx=(h, t, r), go=go, ref=[x.grad for x in p64],
                bound=rel_bound(GRAD_TOL))


MODEL_CASES = {
    'transe_l2': functools.partial(case_parity, 'transe', 2), 'transe_l1': functools.partial(case_parity, 'transe', 1),
    'transh': functools.partial(case_parity, 'transh', 2), 'transd': functools.partial(case_parity, 'transd', 2),
    'distmult': functools.partial(case_parity, 'distmult', 2), 'complex': functools.partial(case_parity, 'complex', 2),
    'rescal': functools.partial(case_rescal_hole, 'rescal'), 'hole': functools.partial(case_rescal_hole, 'hole'),
    'toruse_l1': functools.partial(case_toruse, 'L1'), 'toruse_torus_l1': functools.partial(case_toruse, 'torus_L1'),
    'toruse_torus_l2': functools.partial(case_toruse, 'torus_L2'), 'toruse_torus_el2': functools.partial(case_toruse, 'torus_eL2'),
    'transr': case_transr, 'analogy': case_analogy, 'convkb': case_convkb,
}


@pytest.mark.parametrize('B', [300, 5000])
@pytest.mark.parametrize('name', sorted(MODEL_CASES))
def test_every_models_backward_twice_gives_the_same_bits(D, name, B):
    import torchkge_amd as tk
    from torchkge_amd import _hip
    assert (B < _hip.BWD_SORTED_MIN_BATCH) == (B == 300)
    case = MODEL_CASES[name](B)
    h, t, r = (x.cuda() for x in case['idx'])
    runs = []
    before = dict(D.CALLS)
    with tk.deterministic():
        for _ in range(2):
            m = case['build']()
            (m.scoring_function(h, t, r) * case['go'].cuda()).sum().backward()
            assert all(p.grad is not None for p in m.parameters())      # (every parameter of every model takes part in a score)
            runs.append((m, [p.grad.detach().clone() for p in m.parameters()]))
    assert D.CALLS['ordered'] > before['ordered'] and D.CALLS['atomic'] == before['atomic']
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    for k, (prm, ref) in enumerate(zip(case['tables'](runs[0][0]), case['ref'])):
        got = prm.grad.cpu().double()
        assert got.shape == ref.shape, k
        err, bound = float((got - ref.double()).abs().max()), case['bound'](ref)
        print('%s B = %d table %d: max |grad - reference| = %.3g (bound %.3g)' % (name, B, k, err, bound))
        assert err < bound, k


# ---------------------------------------------------------------------------
# 4. two trainings from one seed
# ---------------------------------------------------------------------------
N_ENT, N_REL, DIM = 500, 7, 32
TRAIN_MODELS = {
    'transe_l2': lambda tk: tk.TransEModel(DIM, N_ENT, N_REL, 'L2'), 'transe_l1': lambda tk: tk.TransEModel(DIM, N_ENT, N_REL, 'L1'),
    'transh': lambda tk: tk.TransHModel(DIM, N_ENT, N_REL), 'transd': lambda tk: tk.TransDModel(DIM, DIM, N_ENT, N_REL),
    'transr': lambda tk: tk.TransRModel(DIM, DIM, N_ENT, N_REL), 'toruse': lambda tk: tk.TorusEModel(DIM, N_ENT, N_REL, 'torus_L2'),
    'distmult': lambda tk: tk.DistMultModel(DIM, N_ENT, N_REL), 'complex': lambda tk: tk.ComplExModel(DIM, N_ENT, N_REL),
    'rescal': lambda tk: tk.RESCALModel(DIM, N_ENT, N_REL), 'hole': lambda tk: tk.HolEModel(DIM, N_ENT, N_REL),
    'analogy': lambda tk: tk.AnalogyModel(DIM, N_ENT, N_REL), 'convkb': lambda tk: tk.ConvKBModel(DIM, 8, N_ENT, N_REL),
}


@functools.lru_cache(maxsize=None)
def zipf_graph():
    import torchkge_amd as tk
    heads, tails, rels = orc.synthetic_triples_zipf(N_ENT, N_REL, 3000, seed=21)
    return tk.KnowledgeGraph(kg={'heads': heads, 'tails': tails, 'relations': rels},
                             ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})


def train(name, steps=20, batch=1024):
    """20 steps of the reference's training loop from a fixed seed; returns the state_dict on the host."""
    import torchkge_amd as tk
    kg = zipf_graph()
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    m = TRAIN_MODELS[name](tk).cuda()
    sampler = tk.BernoulliNegativeSampler(kg)
    loss_fn = tk.MarginLoss(0.5)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    H, T, R = kg.head_idx.cuda(), kg.tail_idx.cuda(), kg.relations.cuda()
    for step in range(steps):
        lo = (step * batch) % kg.n_facts
        h, t, r = H[lo:lo + batch], T[lo:lo + batch], R[lo:lo + batch]
        nh, nt = sampler.corrupt_batch(h, t, r)
        pos, neg = m(h, t, r, nh, nt)
        loss = loss_fn(pos, neg)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if (step + 1) % 5 == 0:
            m.normalize_parameters()
    assert math.isfinite(float(loss.detach()))
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('name', sorted(TRAIN_MODELS))
def test_two_trainings_from_one_seed_give_one_model(D, name):
    import torchkge_amd as tk
    before = dict(D.CALLS)
    with tk.deterministic():
        first = train(name)
        second = train(name)
    assert D.CALLS['ordered'] > before['ordered'] and D.CALLS['atomic'] == before['atomic']
    same_state(first, second)
    assert not tk.is_deterministic()
    if name == 'transe_l2':     # the mode entered through torch's flag, and through the package switch: the same bits
        assert not torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)
        try:
            assert tk.is_deterministic()
            through_torch = train(name)
        finally:
            torch.use_deterministic_algorithms(False)
        tk.set_deterministic(True)
        try:
            through_switch = train(name)
        finally:
            tk.set_deterministic(False)
        same_state(first, through_torch)
        same_state(first, through_switch)


# ---------------------------------------------------------------------------
# 5. off is today's path
# ---------------------------------------------------------------------------
def test_off_is_the_atomic_path_and_a_small_batch_takes_no_row_mode(D):
    import torchkge_amd as tk
    from torchkge_amd import _hip
    assert not tk.is_deterministic()
    z, tables = load_golden('transe', 2)
    n_ent, n_rel, d = int(z['n_ent']), int(z['n_rel']), tables[0].shape[1]
    tabs = [x.cuda() for x in tables]
    for B in (300, 5000):
        h, t, r, go = (x.cuda() for x in skewed_triples(B, n_ent, n_rel, torch.Generator().manual_seed(B)))
        before = dict(D.CALLS)
        grads = _hip.score_triples_bwd(_hip.TRANSE_L2, tabs, d, d, h, t, r, go, (True, True))
        assert D.CALLS['ordered'] == before['ordered']
        # B = 300: the per-element scatter, no row reduction at all; B = 5000: one kge_segment_sum_rows per table
        assert D.CALLS['atomic'] - before['atomic'] == (0 if B == 300 else 2)
        with tk.deterministic():
            det = _hip.score_triples_bwd(_hip.TRANSE_L2, tabs, d, d, h, t, r, go, (True, True))
        assert D.CALLS['ordered'] - before['ordered'] == 2
        for a, b in zip(grads, det):
            assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max()))
