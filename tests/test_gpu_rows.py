"""GPU tests of row gradients (run with -m gpu on an MI355X): kge_rows_coalesce (include/kge_hip_rows.h) against a
float64 index_add_ and, bit for bit, against kge_segment_sum_ordered; the row updates against torch's own sparse
optimizers in float64; every model's backward with the switch on, off and under ``deterministic()``; and a training
with RowAdagrad: the same bits twice, close to the dense deterministic path, and no host read in ``step()``."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.helpers import raw
from tests.test_gpu_deterministic import MODEL_CASES

pytestmark = pytest.mark.gpu

U = 2.0 ** -24      # unit roundoff of fp32


@pytest.fixture(scope='module')
def R():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_rows
    _hip_rows.load_library()
    return _hip_rows


def bits(x):
    return x.contiguous().view(torch.int32)


def ulp_of(x):
    """One float32 ulp at the magnitude |x| (of the largest entry of a table)."""
    return float(np.spacing(np.float32(abs(float(x)))))


# ---------------------------------------------------------------------------
# 1. kge_rows_coalesce
# ---------------------------------------------------------------------------
PATTERNS = ('distinct', 'equal', 'skewed', 'ends')


def make_ids(pattern, M, g):
    """(ids, n_rows): M ids of the pattern on the host."""
    if pattern == 'distinct':
        n_rows = M + 3
        return torch.randperm(n_rows, generator=g)[:M], n_rows
    if pattern == 'equal':
        return torch.full((M,), 5, dtype=torch.int64), 9
    if pattern == 'skewed':                 # three quarters on one id
        n_rows = max(8, M // 3)
        ids = torch.randint(0, n_rows, (M,), generator=g)
        ids[torch.randperm(M, generator=g)[:(3 * M) // 4]] = 3
        return ids, n_rows
    n_rows = 50                             # the first and the last row of the table occur
    ids = torch.randint(1, n_rows - 1, (M,), generator=g)
    if M > 0:
        ids[M // 2] = 0
    if M > 1:
        ids[0] = n_rows - 1
    return ids, n_rows


def index_add64(n_rows, ids, x):
    """zeros(n_rows, d).index_add_(0, ids, x) in float64, on the device.  Narrow rows are added on the host: the float64
    atomics of one wavefront then fall on a handful of addresses and serialise (seconds for 70,000 equal ids at d <= 64)."""
    where = 'cpu' if x.shape[1] < 200 else 'cuda'
    return torch.zeros(n_rows, x.shape[1], dtype=torch.float64, device=where).index_add_(0, ids.to(where), x.double().to(where)).cuda()


@pytest.mark.parametrize('d', [1, 7, 64, 200, 257, 513, 1030])
def test_coalesce_vs_float64_unique_layout_and_the_ordered_sum_bit_for_bit(R, d):
    from torchkge_amd import _hip_det
    gh = torch.Generator().manual_seed(300 + d)
    gd = torch.Generator(device='cuda').manual_seed(300 + d)
    ld, out_ld = d + 3, d + 5
    for M in (0, 1, 31, 32, 33, 513, 70000):
        for pattern in PATTERNS:
            tag = (d, M, pattern)
            ids_h, n_rows = make_ids(pattern, M, gh)
            ids = ids_h.cuda()
            rows = torch.full((max(M, 1), ld), float('nan'), device='cuda')       # NaN pads: reading one poisons a sum
            # magnitudes over 20 binades: the order of the additions shows in the low bits of a sum
            x = torch.randn(M, d, generator=gd, device='cuda') * \
                torch.exp2(torch.rand(M, d, generator=gd, device='cuda') * 20 - 10)
            rows[:M, :d] = x
            outs = []
            for _ in range(2):
                uniq = torch.full((max(M, 1),), -7, dtype=torch.int64, device='cuda')
                out = torch.full((max(M, 1), out_ld), float('nan'), device='cuda')
                count = torch.full((), -7, dtype=torch.int64, device='cuda')
                before = out.clone()
                R.rows_coalesce(rows, ld, d, ids, n_rows, uniq=uniq, out=out, out_ld=out_ld, count=count)
                outs.append((uniq, out, count))
                assert torch.equal(bits(out[:, d:]), bits(before[:, d:])), tag       # the pads keep every bit
            uniq, out, count = outs[0]
            want = torch.unique(ids)
            n_u = int(count)
            assert n_u == want.shape[0], tag
            assert torch.equal(uniq[:n_u], want), tag
            if M == 0:
                assert torch.equal(bits(out), bits(before)) and int(uniq[0]) == -7
                continue
            got = out[:n_u, :d]
            assert bool(torch.isfinite(got).all()), tag           # no pad column of `rows` reached a sum
            # two calls: the same bits
            assert int(outs[1][2]) == n_u and torch.equal(outs[1][0][:n_u], uniq[:n_u]), tag
            assert torch.equal(bits(outs[1][1][:n_u, :d]), bits(got)), tag
            # float64 index_add_ of the same rows; the forward bound of ANY fp32 summation order of a run of n rows
            sum64, abs64 = index_add64(n_rows, ids, x), index_add64(n_rows, ids, x.abs())
            n_run = torch.bincount(ids, minlength=n_rows).double().view(-1, 1)
            assert float(n_run.max()) * U < 0.01
            err = (got.double() - sum64[want]).abs()
            bound = 1.01 * n_run[want] * U * abs64[want]
            assert bool((err <= bound).all()), (tag, float((err - bound).max()))
            one = n_run[want].view(-1) == 1                         # a run of one row is that row
            where = torch.zeros(n_rows, dtype=torch.int64, device='cuda')
            where[ids] = torch.arange(M, device='cuda')
            assert torch.equal(got[one], x[where[want[one]]]), tag
            # scattered by uniq into a zero table: the bits of kge_segment_sum_ordered into a zeroed dense table
            dense = torch.zeros(n_rows, d, device='cuda')
            _hip_det.reduce_rows(rows, ld, d, ids, None, dense, det=True)
            scat = torch.zeros(n_rows, d, device='cuda')
            scat[uniq[:n_u]] = got
            assert torch.equal(bits(scat), bits(dense)), tag


def test_coalesce_refuses_bad_arguments_and_touches_nothing(R):
    lib = R.load_library()
    M, d, n_rows = 100, 8, 20
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, n_rows, (M,), generator=g).cuda()
    rows = torch.randn(M, d + 3, generator=g).cuda()
    uniq = torch.full((M,), -7, dtype=torch.int64, device='cuda')
    out = torch.full((M, d + 5), 1.5, device='cuda')
    count = torch.full((), -7, dtype=torch.int64, device='cuda')
    nb = R.ws_bytes(M, d)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')

    def call(d_=d, ld=d + 3, out_ld=d + 5, n=n_rows, w=ws, nbytes=nb, m=M, cnt=count):
        return raw(lib, 'kge_rows_coalesce', rows, ld, d_, ids, m, n, uniq, out, out_ld, cnt, w, nbytes)
    assert call(d_=0) != 0 and call(ld=d - 1) != 0 and call(out_ld=d - 1) != 0
    assert call(n=0) != 0 and call(n=(1 << 32) + 1) != 0 and call(m=-1) != 0 and call(m=1 << 31) != 0
    assert call(nbytes=nb - 1) != 0 and call(w=None) != 0 and call(cnt=None) != 0
    assert raw(lib, 'kge_rows_coalesce', rows, d + 3, d, ids, M, n_rows, uniq, out, d + 5, count, ws[1:], nb) != 0   # misaligned
    torch.cuda.synchronize()
    assert int(count) == -7 and bool((uniq == -7).all()) and bool((out == 1.5).all())
    assert call() == 0
    assert int(count) == int(torch.unique(ids).shape[0])
    # the updates: bad arguments launch nothing
    p = torch.ones(n_rows, d, device='cuda')
    gz = torch.ones(M, d, device='cuda')
    assert raw(lib, 'kge_row_sgd', p, d, 0, uniq, count, M, gz, d, 0.5) != 0
    assert raw(lib, 'kge_row_sgd', p, d - 1, d, uniq, count, M, gz, d, 0.5) != 0
    assert raw(lib, 'kge_row_sgd', p, d, d, uniq, None, M, gz, d, 0.5) != 0
    assert raw(lib, 'kge_row_adagrad', p, None, d, d, uniq, count, M, gz, d, 0.5, 1e-10) != 0
    assert raw(lib, 'kge_row_adam', p, p, None, d, d, uniq, count, M, gz, d, 0.5, 0.1, 0.001, 1e-8, 0.1, 0.001) != 0
    assert raw(lib, 'kge_row_adam', p, p, p, d, d, uniq, count, M, gz, d, 0.5, 0.1, 0.001, 1e-8, 0.0, 0.001) != 0   # step 0
    assert raw(lib, 'kge_row_sgd', None, d, d, None, None, 0, None, d, 0.5) == 0        # M = 0: a no-op
    torch.cuda.synchronize()
    assert bool((p == 1).all())


# ---------------------------------------------------------------------------
# 2. the row updates against torch's sparse optimizers
# ---------------------------------------------------------------------------
POISON = 12345.678
OPTS = {
    'sgd': (lambda o, p: o.RowSGD(p, lr=0.05), lambda p: torch.optim.SGD(p, lr=0.05), ()),
    'adagrad': (lambda o, p: o.RowAdagrad(p, lr=0.05, lr_decay=0.01, eps=1e-10, initial_accumulator_value=0.1),
                lambda p: torch.optim.Adagrad(p, lr=0.05, lr_decay=0.01, eps=1e-10, initial_accumulator_value=0.1), ('sum',)),
    'adam': (lambda o, p: o.RowAdam(p, lr=0.05, betas=(0.9, 0.999), eps=1e-8),
             lambda p: torch.optim.SparseAdam(p, lr=0.05, betas=(0.9, 0.999), eps=1e-8), ('exp_avg', 'exp_avg_sq')),
}


def stock_run(make, p0, grad, steps, dtype):
    """``steps`` steps of torch's optimizer on the CPU in ``dtype`` with the fixed sparse gradient; (param, states)."""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = make([p])
    for _ in range(steps):
        p.grad = grad.to(dtype)
        opt.step()
    return p.detach(), opt.state[p]


def assert_close_to_float64(name, ours, t32, t64):
    """|ours - float64| <= 2 |torch float32 - float64| + one float32 ulp of the table's largest magnitude; returns the
    two distances."""
    d_torch = float((t32.double() - t64).abs().max())
    d_ours = float((ours.double().cpu() - t64).abs().max())
    tol = 2 * d_torch + ulp_of(t64.abs().max())
    print('%s: |ours - f64| = %.3g, |torch f32 - f64| = %.3g, bound %.3g' % (name, d_ours, d_torch, tol))
    assert d_ours <= tol, (name, d_ours, tol)
    return d_ours, d_torch


def fixed_gradient(n_rows, d, M, seed):
    """(p0 with poison in the rows without a gradient; the float64-coalesced gradient of ids with repeats -- the first
    and the last row among them, n_rows odd -- rounded to float32, as a coalesced sparse tensor; the rows it touches)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, n_rows // 2, (M,), generator=g) * 2      # even rows only: every odd row has no gradient
    ids[0], ids[1] = 0, n_rows - 1
    vals = torch.randn(M, d, generator=g)
    g64 = torch.sparse_coo_tensor(ids.view(1, -1), vals.double(), (n_rows, d)).coalesce()
    grad = torch.sparse_coo_tensor(g64.indices(), g64.values().float(), (n_rows, d)).coalesce()
    p0 = torch.randn(n_rows, d, generator=g)
    touched = torch.zeros(n_rows, dtype=torch.bool)
    touched[g64.indices()[0]] = True
    p0[~touched] = POISON
    return p0, grad, touched


@pytest.mark.parametrize('d', [1, 7, 200, 1030])
@pytest.mark.parametrize('name', sorted(OPTS))
def test_row_updates_vs_torchs_sparse_optimizers_in_float64(R, name, d):
    from torchkge_amd import optim
    ours_make, stock_make, state_names = OPTS[name]
    n_rows, M = 301, 400
    p0, grad, touched = fixed_gradient(n_rows, d, M, 40 + d)
    for steps in (1, 3):
        p64, s64 = stock_run(stock_make, p0, grad, steps, torch.float64)
        p32, s32 = stock_run(stock_make, p0, grad, steps, torch.float32)
        p = torch.nn.Parameter(p0.clone().cuda())
        opt = ours_make(optim, [p])
        for _ in range(steps):
            p.grad = grad.cuda()
            opt.step()
        tag = '%s d = %d steps = %d' % (name, d, steps)
        # (closeness over the rows that have a gradient: the poison's magnitude must not set the ulp of the bound)
        assert_close_to_float64(tag + ' param', p.detach().cpu()[touched], p32[touched], p64[touched])
        for s in state_names:
            assert opt.state[p][s].shape == p.shape
            assert_close_to_float64(tag + ' ' + s, opt.state[p][s].cpu()[touched], s32[s][touched], s64[s][touched])
        assert int(opt.state[p]['step']) == steps if state_names else True
        # rows without a gradient keep their exact bit pattern, in the parameter and in every state table
        assert torch.equal(bits(p.detach().cpu()[~touched]), bits(p0[~touched]))
        assert not torch.equal(p.detach().cpu()[touched], p0[touched])
        for s in state_names:
            fresh = 0.1 if s == 'sum' else 0.0
            assert bool((opt.state[p][s].cpu()[~touched] == fresh).all()), (tag, s)


def test_updates_read_count_on_the_device_and_ignore_stale_entries(R):
    """Two rounds that differ only in *count: U = 1, and U above the grid cap; uniq holds valid ids behind count."""
    cap = R.max_waves()
    M, d, lr = cap + 100, 7, 0.25
    n_rows = M + 50
    g = torch.Generator().manual_seed(9)
    uniq = torch.randperm(n_rows, generator=g)[:M].cuda()
    grows = torch.randn(M, d, generator=g).cuda()
    p0 = torch.randn(n_rows, d, generator=g).cuda()
    for n_u in (1, cap + 37):
        count = torch.tensor(n_u, dtype=torch.int64, device='cuda')
        live = torch.zeros(n_rows, dtype=torch.bool, device='cuda')
        live[uniq[:n_u]] = True
        p = p0.clone()
        R.row_sgd(p, uniq, count, grows, lr)
        want = p0.clone()
        want[uniq[:n_u]] = p0[uniq[:n_u]] - grows[:n_u] * lr        # (lr = 1 / 4: the product is exact either way)
        assert torch.equal(bits(p), bits(want)), n_u
        p, s = p0.clone(), torch.full_like(p0, 0.5)
        R.row_adagrad(p, s, uniq, count, grows, lr, 1e-10)
        assert torch.equal(bits(p[~live]), bits(p0[~live])) and bool((s[~live] == 0.5).all()), n_u
        assert torch.equal(s[uniq[:n_u]], 0.5 + grows[:n_u] * grows[:n_u]), n_u
        assert bool((p[live] != p0[live]).any(dim=1).all()), n_u
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        R.row_adam(p, m, v, uniq, count, grows, lr, 0.9, 0.999, 1e-8, 1)
        assert torch.equal(bits(p[~live]), bits(p0[~live])) and not bool(m[~live].any()) and not bool(v[~live].any()), n_u
        assert bool((m[live] != 0).any(dim=1).all()) and bool((p[live] != p0[live]).any(dim=1).all()), n_u


def test_a_gradient_accumulated_from_two_backwards_is_one_step_on_the_sum(R):
    import torchkge_amd as tk
    from torchkge_amd import optim
    n_ent, n_rel, d, B = 500, 9, 40, 512
    torch.manual_seed(4)
    m = tk.TransEModel(d, n_ent, n_rel, 'L2').cuda()
    g = torch.Generator().manual_seed(5)
    with tk.row_gradients():
        for _ in range(2):
            h, t = torch.randint(0, n_ent, (B,), generator=g).cuda(), torch.randint(0, n_ent, (B,), generator=g).cuda()
            r = torch.randint(0, n_rel, (B,), generator=g).cuda()
            (m.scoring_function(h, t, r) * torch.randn(B, generator=g).cuda()).sum().backward()
    E, Rl = m.ent_emb.weight, m.rel_emb.weight
    # autograd's accumulation of two sparse gradients is their concatenation; torch's sparse add coalesces a sum that
    # has outgrown its table (the 9-row rel_emb here comes back with 9 entries): step() takes either
    assert E.grad.is_sparse and E.grad._nnz() == 4 * B and not E.grad.is_coalesced()
    assert Rl.grad.is_sparse and Rl.grad._nnz() <= 2 * B
    make = OPTS['adagrad'][1]
    opt = OPTS['adagrad'][0](optim, [E, Rl])
    refs = []
    for p in (E, Rl):
        g_host = p.grad.cpu()
        g64 = torch.sparse_coo_tensor(g_host._indices(), g_host._values().double(), g_host.shape).coalesce()
        refs.append((stock_run(make, p.detach().cpu(), g64, 1, torch.float64),
                     stock_run(make, p.detach().cpu(), g_host.coalesce(), 1, torch.float32)))
    opt.step()
    for name, p, ((p64, s64), (p32, s32)) in zip(('ent_emb', 'rel_emb'), (E, Rl), refs):
        assert_close_to_float64('accumulated ' + name, p.detach(), p32, p64)
        assert_close_to_float64('accumulated %s sum' % name, opt.state[p]['sum'], s32['sum'], s64['sum'])


# ---------------------------------------------------------------------------
# 3. every model: the switch on, off, and under deterministic()
# ---------------------------------------------------------------------------
def backward(case, h, t, r):
    m = case['build']()
    (m.scoring_function(h, t, r) * case['go'].cuda()).sum().backward()
    assert all(p.grad is not None for p in m.parameters())
    return m


@pytest.mark.parametrize('B', [64, 4096])
@pytest.mark.parametrize('name', sorted(MODEL_CASES))
def test_every_models_backward_gives_row_gradients(R, name, B):
    import torchkge_amd as tk
    from torchkge_amd import _hip, _hip_det, optim
    assert (B < _hip.BWD_SORTED_MIN_BATCH) == (B == 64)
    case = MODEL_CASES[name](B)
    h, t, r = (x.cuda() for x in case['idx'])
    # off: dense gradients, the reductions counted as ever
    before = dict(_hip_det.CALLS)
    m_off = backward(case, h, t, r)
    assert not any(p.grad.is_sparse for p in m_off.parameters())
    assert _hip_det.CALLS['ordered'] == before['ordered']
    if B == 4096:
        assert _hip_det.CALLS['atomic'] > before['atomic']
    with tk.deterministic():
        m_det = backward(case, h, t, r)
    assert _hip_det.CALLS['ordered'] > before['ordered']
    # on: read in the forward -- the backward runs outside the context
    before = dict(_hip_det.CALLS)
    m_row = case['build']()
    with tk.row_gradients():
        loss = (m_row.scoring_function(h, t, r) * case['go'].cuda()).sum()
    assert not tk.is_row_gradients()
    loss.backward()
    assert _hip_det.CALLS == before
    row_params, dense_params = optim.split_parameters(m_row)
    row_ids = {id(p) for p in row_params}
    assert len(row_params) >= 1 and len(row_params) + len(dense_params) == len(list(m_row.parameters()))
    for k, (p_row, p_det, p_off, ref) in enumerate(zip(case['tables'](m_row), case['tables'](m_det), case['tables'](m_off),
                                                       case['ref'])):
        assert p_row.grad.is_sparse == (id(p_row) in row_ids), k
        dense = p_row.grad.to_dense() if p_row.grad.is_sparse else p_row.grad
        assert dense.shape == ref.shape, k
        err, bound = float((dense.cpu().double() - ref.double()).abs().max()), case['bound'](ref)
        print('%s B = %d table %d: max |grad - reference| = %.3g (bound %.3g)' % (name, B, k, err, bound))
        assert err < bound, k
        if p_row.grad.is_sparse:
            n_ids = p_row.grad._nnz()
            assert n_ids in (B, 2 * B) and tuple(p_row.grad.shape) == tuple(p_row.shape), k
            uniq, rows, count = optim.coalesce_rows(p_row.grad)
            scat = torch.zeros_like(p_det.grad)
            scat[uniq[:int(count)]] = rows[:int(count)]
            assert torch.equal(bits(scat), bits(p_det.grad)), k
        else:
            assert torch.equal(bits(dense), bits(p_off.grad)) and torch.equal(bits(dense), bits(p_det.grad)), k
    for p_row, p_off in zip(m_row.parameters(), m_off.parameters()):     # every dense gradient, whatever case['tables'] lists
        if not p_row.grad.is_sparse:
            assert torch.equal(bits(p_row.grad), bits(p_off.grad))


# ---------------------------------------------------------------------------
# 4. training
# ---------------------------------------------------------------------------
N_ENT, N_REL, DIM, BATCH, STEPS, LR, MARGIN = 500, 9, 40, 512, 20, 0.05, 0.5


@functools.lru_cache(maxsize=None)
def batches():
    """The 20 batches (h, t, r, negative h, negative t) of every training below, drawn once on the host."""
    heads, tails, rels = orc.synthetic_triples_zipf(N_ENT, N_REL, 3000, seed=21)
    g = torch.Generator().manual_seed(22)
    out = []
    for step in range(STEPS):
        lo = (step * BATCH) % (heads.shape[0] - BATCH)
        h, t, r = heads[lo:lo + BATCH], tails[lo:lo + BATCH], rels[lo:lo + BATCH]
        swap = torch.rand(BATCH, generator=g) < 0.5
        rnd = torch.randint(0, N_ENT, (BATCH,), generator=g)
        out.append((h, t, r, torch.where(swap, rnd, h), torch.where(swap, t, rnd)))
    return out


def initial_tables():
    import torchkge_amd as tk
    torch.manual_seed(0)
    m = tk.TransEModel(DIM, N_ENT, N_REL, 'L2')
    return m.ent_emb.weight.detach().clone(), m.rel_emb.weight.detach().clone()


def engine_train(rows):
    """20 steps on the engine: RowAdagrad on row gradients, or torch's Adagrad on the dense deterministic path."""
    import torchkge_amd as tk
    from torchkge_amd import optim
    E0, R0 = initial_tables()
    m = tk.TransEModel(DIM, N_ENT, N_REL, 'L2')
    m.ent_emb.weight.data, m.rel_emb.weight.data = E0.clone(), R0.clone()
    m = m.cuda()
    loss_fn = tk.MarginLoss(MARGIN)
    opt = optim.RowAdagrad(m.parameters(), lr=LR) if rows else torch.optim.Adagrad(m.parameters(), lr=LR)
    with tk.row_gradients(rows), tk.deterministic(not rows):
        for step, batch in enumerate(batches()):
            h, t, r, nh, nt = (x.cuda() for x in batch)
            loss = loss_fn(*m(h, t, r, nh, nt))
            opt.zero_grad()
            loss.backward()
            if rows and step == 3:      # the Python side of step() reads nothing back: a read would raise here
                assert m.ent_emb.weight.grad.is_sparse
                torch.cuda.set_sync_debug_mode('error')
                try:
                    opt.step()
                finally:
                    torch.cuda.set_sync_debug_mode('default')
            else:
                opt.step()
    assert math.isfinite(float(loss.detach()))
    return m.ent_emb.weight.detach().cpu(), m.rel_emb.weight.detach().cpu()


def torch_train(dtype):
    """The same loop in plain torch on the host (the oracle's TransE score under autograd, torch's dense Adagrad)."""
    E0, R0 = initial_tables()
    E, Rl = torch.nn.Parameter(E0.to(dtype)), torch.nn.Parameter(R0.to(dtype))
    opt = torch.optim.Adagrad([E, Rl], lr=LR)
    for h, t, r, nh, nt in batches():
        s = orc.score_triples('transe', [E, Rl], torch.cat([h, nh]), torch.cat([t, nt]), torch.cat([r, r]), p=2)
        loss = (MARGIN - (s[:BATCH] - s[BATCH:])).clamp_min(0).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return E.detach(), Rl.detach()


def test_training_with_row_adagrad_same_bits_twice_and_close_to_the_dense_path(R):
    first, second = engine_train(True), engine_train(True)
    for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b))            # no deterministic() needed: the coalescing is ordered
    dense = engine_train(False)
    t32, t64 = torch_train(torch.float32), torch_train(torch.float64)
    E0, R0 = initial_tables()
    for name, a, b, x32, x64, x0 in zip(('ent_emb', 'rel_emb'), first, dense, t32, t64, (E0, R0)):
        assert float((a - x0).abs().max()) > 1e-3       # it trained
        measured = float((x32.double() - x64).abs().max())
        bound = 4 * (2 * measured + ulp_of(x64.abs().max()))
        diff = float((a.double() - b.double()).abs().max())
        print('%s after %d steps: |rows - dense deterministic| = %.3g; float32 vs float64 of the same loop = %.3g; bound %.3g; '
              '|rows - float64 loop| = %.3g' % (name, STEPS, diff, measured, bound, float((a.double() - x64).abs().max())))
        assert diff <= bound, name
