"""GPU tests of the 1-vs-all criterion kge_lp_xent_fwd / kge_lp_xent_bwd (include/kge_hip_xent.h; run with -m gpu on an
MI355X), at kernel level through tests.helpers.raw / carve / guarded_out.

Yardstick: the float64 forms of tests/xent_ref.py (tests/test_xent_host.py anchors them to torch's cross_entropy) applied
to the engine's OWN fp32 scores -- kge_lp_scores, bit-defined code that predates these kernels.

Comparator: torch's fp32 evaluation on the same device -- logsumexp / cross_entropy of those scores forward, autograd of
the materialised formula (A @ T.t(), cross_entropy, weights g) backward.  Tolerance, the shape of test_gpu_pair_loss.py:
4 * (2 * |torch fp32 - float64| + one fp32 ulp of the value), per output vector / matrix in max-norm with the ulp of its
largest float64 magnitude.  (Max-norm, as that file's gradients: a single row on which torch happens to round exactly
would otherwise ask for 4 ulp of a row loss that is a DIFFERENCE of two larger numbers, lse and the target score, each
good to its own ulp only.)

Shapes come from the constants the header publishes (BM = row panel, BN = candidate tile, the first N with two chunks);
the cases are a sparse cross in which every listed B, N and (K0, K1) occurs."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import raw, carve, guarded_out, assert_guard_intact
from tests import xent_ref

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
RECORD = []         # lines of the parity record (the parity_record fixture writes them out)


@pytest.fixture(scope='module')
def X():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_xent
    _hip_xent.load_library()
    return _hip_xent


@pytest.fixture(scope='module', autouse=True)
def parity_record():
    """After the module: the distances its tests measured go to the file KGE_XENT_PARITY_OUT names, when it names one
    (profiles/r10/xent_parity.txt is one such run)."""
    yield
    path = os.environ.get('KGE_XENT_PARITY_OUT')
    if path and RECORD:
        with open(path, 'w') as f:
            f.write('max-norm distances to the float64 forms of the engine\'s own fp32 scores (tests/test_gpu_xent.py)\n')
            f.write('\n'.join(RECORD) + '\n')


def _shapes():
    from torchkge_amd import _hip_xent as x
    BM, BN = x.BM, x.BN
    two = x.MIN_TILES_PER_CHUNK * BN + 1        # the first N with two chunks
    Bs = (1, BM - 1, BM + 1, 2 * BM + 5)
    Ns = (1, 2, BN - 1, BN + 1, 2 * BN + 3, two, two + BN + 1)
    Ks = ((1, 0), (5, 0), (8, 0), (33, 0), (200, 0), (3, 3), (200, 200), (512, 512))
    cases = [(Bs[i % 4], Ns[i % 7], Ks[i]) for i in range(8)]
    cases += [(Bs[(i + 1) % 4], Ns[(i + 3) % 7], Ks[i]) for i in range(8)]
    cases += [(Bs[3], Ns[6], Ks[7]), (Bs[3], Ns[5], Ks[6]), (Bs[2], Ns[6], Ks[4]), (Bs[0], Ns[6], Ks[1])]
    assert {c[0] for c in cases} == set(Bs) and {c[1] for c in cases} == set(Ns) and {c[2] for c in cases} == set(Ks)
    return cases


CASES = _shapes()


def bits(x):
    return x.contiguous().view(torch.int32)


def ulp_of(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def make(B, N, K0, K1, seed, scale=3.0):
    """(A, T, target, g) on the device: scores of standard deviation ~ `scale`, non-uniform row weights."""
    gen = torch.Generator().manual_seed(seed)
    K = K0 + K1
    A = torch.randn(B, K, generator=gen) * (scale / K ** 0.5)
    T = torch.randn(N, K, generator=gen)
    t = torch.randint(0, N, (B,), generator=gen)
    w = torch.rand(B, generator=gen) + 0.5
    return A.cuda(), T.cuda(), t.cuda(), w.cuda()


def segs(M, K0, K1):
    return [M[:, :K0].contiguous()] + ([M[:, K0:].contiguous()] if K1 else [])


def problem(As, Ts):
    from torchkge_amd import _hip
    return _hip.LpProblem(_hip.LP_DOT, As[0], Ts[0], A1=As[1] if len(As) > 1 else None, T1=Ts[1] if len(Ts) > 1 else None)


def workspace(X, prob):
    d = prob.desc
    return torch.empty(max(X.ws_bytes(int(d.B), int(d.N), int(d.K0), int(d.K1)), 16), dtype=torch.uint8, device='cuda')


def fwd(X, prob, t, eps, lse=None, loss=None, ws=None):
    lse = torch.empty(prob.B, device='cuda') if lse is None else lse
    loss = torch.empty(prob.B, device='cuda') if loss is None else loss
    ws = workspace(X, prob) if ws is None else ws
    rc = raw(X.load_library(), 'kge_lp_xent_fwd', prob.desc, t, float(eps), lse, loss, ws, ws.numel())
    return rc, lse, loss


def bwd(X, prob, t, eps, lse, w, dA='new', dT='new', ws=None):
    """dA / dT: 'new' allocates dense outputs, None leaves the group out, a list passes the given views."""
    d = prob.desc
    widths = [int(d.K0)] + ([int(d.K1)] if d.K1 else [])
    if dA == 'new':
        dA = [torch.empty(prob.B, k, device='cuda') for k in widths]
    if dT == 'new':
        dT = [torch.empty(prob.N, k, device='cuda') for k in widths]
    ws = workspace(X, prob) if ws is None else ws
    args = []
    for grp in (dA, dT):
        for j in range(2):
            x = grp[j] if grp is not None and j < len(grp) else None
            args += [x, 0 if x is None else x.stride(0)]
    rc = raw(X.load_library(), 'kge_lp_xent_bwd', prob.desc, t, float(eps), lse, w, *(args + [ws, ws.numel()]))
    return rc, dA, dT


def within(name, tag, ours, ref64, cmp32):
    """max-norm distances of `ours` and of torch's fp32 to the float64 form, under the module's tolerance."""
    assert bool(torch.isfinite(ours).all()), (name, tag)
    ref64 = ref64.double().cpu()
    d_ours = float((ours.double().cpu() - ref64).abs().max())
    d_cmp = float((cmp32.double().cpu() - ref64).abs().max())
    tol = 4 * (2 * d_cmp + ulp_of(ref64.abs().max()))
    line = '%-8s %-34s |fused - f64| %.3g  |torch fp32 - f64| %.3g  bound %.3g  (max |f64| %.4g)' % (
        name, tag, d_ours, d_cmp, tol, float(ref64.abs().max()))
    print('xent ' + line)
    RECORD.append(line)
    assert d_ours <= tol, (name, tag, d_ours, tol)


def check(X, A, T, t, w, K0, K1, eps, tag):
    """Forward and backward of one problem against the yardstick; returns (lse, row_loss, dA, dT) of the kernels."""
    As, Ts = segs(A, K0, K1), segs(T, K0, K1)
    prob = problem(As, Ts)
    S32 = prob.scores()
    rc, lse, loss = fwd(X, prob, t, eps)
    assert rc == 0
    lse64, loss64 = xent_ref.row_loss64(S32, t, eps)
    within('lse', tag, lse, lse64, torch.logsumexp(S32, dim=1))
    within('row_loss', tag, loss, loss64, F.cross_entropy(S32, t, label_smoothing=eps, reduction='none'))
    if eps == 0:        # ONE fp32 subtraction from the pair kernel's score of the target
        assert torch.equal(bits(loss), bits(lse - prob.pair_scores(t))), tag
    rc, dA, dT = bwd(X, prob, t, eps, lse, w)
    assert rc == 0
    dA, dT = torch.cat(dA, dim=1), torch.cat(dT, dim=1)
    dA64, dT64 = xent_ref.grads64(S32, t, eps, w, A, T)
    a32, t32 = A.clone().requires_grad_(), T.clone().requires_grad_()
    (F.cross_entropy(a32 @ t32.t(), t, label_smoothing=eps, reduction='none') * w).sum().backward()
    within('dA', tag, dA, dA64, a32.grad)
    within('dT', tag, dT, dT64, t32.grad)
    return lse, loss, dA, dT


# ---------------------------------------------------------------------------
# forward and backward against the float64 forms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,K', CASES, ids=['B%d-N%d-K%d+%d' % (b, n, k[0], k[1]) for b, n, k in CASES])
def test_forward_and_backward_match_the_float64_forms(X, B, N, K):
    A, T, t, w = make(B, N, K[0], K[1], seed=B * 1000 + N)
    for eps in (0.0, 0.1):
        check(X, A, T, t, w, K[0], K[1], eps, 'B=%d N=%d K=%d+%d eps=%g' % (B, N, K[0], K[1], eps))


def test_scores_of_magnitude_300_stay_finite_and_within_the_bound(X):
    B, N, K0, K1 = X.BM + 1, X.MIN_TILES_PER_CHUNK * X.BN + 1 + X.BN + 1, 33, 0
    A, T, t, w = make(B, N, K0, K1, seed=5)
    S = A @ T.t()
    A = A * (300.0 / S.abs().max(dim=1, keepdim=True).values)       # every row reaches +-300
    S32 = problem(segs(A, K0, K1), segs(T, K0, K1)).scores()
    assert float(S32.abs().max()) > 299 and float(S32.abs().max(dim=1).values.min()) > 299
    for eps in (0.0, 0.1):
        check(X, A, T, t, w, K0, K1, eps, 'scores +-300 eps=%g' % eps)


def test_a_target_that_wins_by_100_never_gives_a_negative_loss(X):
    B, N, K = X.BM + 1, 2 * X.BN + 3, 8
    gen = torch.Generator().manual_seed(11)
    T = F.normalize(torch.randn(N, K, generator=gen), dim=1)
    t = torch.randint(0, N, (B,), generator=gen)
    t[0], t[1], t[2] = 0, N - 1, 2 * X.BN       # first candidate, last one, first of the last partial tile
    cos = T[t] @ T.t()
    cos.scatter_(1, t.view(-1, 1), -2.0)
    c = 105.0 / float((1.0 - cos.max(dim=1).values).min())
    A, T, t = (T[t] * c).cuda(), T.cuda(), t.cuda()
    prob = problem([A], [T])
    S32 = prob.scores()
    st = S32.gather(1, t.view(-1, 1))
    gap = (st - S32.scatter(1, t.view(-1, 1), float('-inf')).max(dim=1, keepdim=True).values).min()
    assert float(gap) >= 100
    rc, lse, loss = fwd(X, prob, t, 0.0)
    assert rc == 0 and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(loss).all())
    assert bool((loss >= 0).all())
    assert torch.equal(bits(loss), bits(lse - prob.pair_scores(t)))


# ---------------------------------------------------------------------------
# masking and targets
# ---------------------------------------------------------------------------
def test_targets_at_the_edges_and_in_the_last_partial_tile(X):
    B, N, K0, K1 = X.BM + 1, 2 * X.BN + 3, 5, 0
    A, T, t, w = make(B, N, K0, K1, seed=21)
    edge = torch.tensor([0, N - 1, N - 2, 2 * X.BN, X.BN, X.BN - 1, 1], device='cuda')
    t = edge[torch.arange(B, device='cuda') % edge.shape[0]]
    for eps in (0.0, 0.1):
        check(X, A, T, t, w, K0, K1, eps, 'edge targets eps=%g' % eps)


def test_one_target_for_all_rows_and_repeated_query_rows(X):
    B, N, K0, K1 = 2 * X.BM + 5, X.MIN_TILES_PER_CHUNK * X.BN + 1, 3, 3
    A, T, t, w = make(B, N, K0, K1, seed=22)
    A = A[torch.arange(B, device='cuda') % 3].contiguous()        # three distinct query rows
    t = torch.full((B,), N - 1, dtype=torch.long, device='cuda')  # the one-hot term of ONE dT row is hit B times
    for eps in (0.0, 0.1):
        lse, loss, dA, dT = check(X, A, T, t, w, K0, K1, eps, 'one target, repeated rows eps=%g' % eps)
        for i in range(3, B):       # a row's lse / loss do not depend on where it stands
            assert int(bits(lse)[i]) == int(bits(lse)[i % 3]) and int(bits(loss)[i]) == int(bits(loss)[i % 3])


# ---------------------------------------------------------------------------
# layout, reproducibility, NULL groups
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,K0,K1', [(65, 131, 8, 0), (133, 257, 200, 200)])
def test_padded_offset_operands_give_the_bits_of_the_dense_call(X, B, N, K0, K1):
    eps = 0.1
    A, T, t, w = make(B, N, K0, K1, seed=31)
    As, Ts = segs(A, K0, K1), segs(T, K0, K1)
    dense = problem(As, Ts)
    rc, lse, loss = fwd(X, dense, t, eps)
    assert rc == 0
    rc, dA, dT = bwd(X, dense, t, eps, lse, w)
    assert rc == 0
    # operands with a pad and a 4-byte base offset out of NaN-poisoned buffers, outputs in guarded buffers
    Ac, Tc = [carve(x, pad=3, off=1) for x in As], [carve(x, pad=5, off=1) for x in Ts]
    tc, wc = carve(t, off=1, poison=-1), carve(w, off=1)
    assert all(x.data_ptr() % 16 == 4 for x in Ac + Tc + [wc])
    strided = problem(Ac, Tc)
    lse_g, loss_g = guarded_out(B, off=1), guarded_out(B, off=3)
    rc, _, _ = fwd(X, strided, tc, eps, lse=lse_g, loss=loss_g)
    assert rc == 0
    assert torch.equal(bits(lse_g), bits(lse)) and torch.equal(bits(loss_g), bits(loss))
    dA_g = [guarded_out(B, x.shape[1], pad=2, off=1) for x in dA]
    dT_g = [guarded_out(N, x.shape[1], pad=7, off=3) for x in dT]
    rc, _, _ = bwd(X, strided, tc, eps, lse_g, wc, dA=dA_g, dT=dT_g)
    assert rc == 0
    for g, ref in zip(dA_g + dT_g, dA + dT):
        assert torch.equal(bits(g), bits(ref))
    for v in [lse_g, loss_g] + dA_g + dT_g + Ac + Tc + [tc, wc]:
        assert_guard_intact(v)


def test_two_calls_give_the_same_bits_and_rows_do_not_depend_on_the_batch(X):
    B, N, K0, K1 = 2 * X.BM + 5, X.MIN_TILES_PER_CHUNK * X.BN + 1 + X.BN + 1, 200, 0
    eps = 0.1
    A, T, t, w = make(B, N, K0, K1, seed=41)
    prob = problem([A], [T])
    outs = []
    for _ in range(2):
        rc, lse, loss = fwd(X, prob, t, eps)
        assert rc == 0
        rc, dA, dT = bwd(X, prob, t, eps, lse, w)
        assert rc == 0
        outs.append([lse, loss] + dA + dT)
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b))
    # the first 37 rows alone
    small = problem([A[:37].contiguous()], [T])
    rc, lse37, loss37 = fwd(X, small, t[:37].contiguous(), eps)
    assert rc == 0
    assert torch.equal(bits(lse37), bits(outs[0][0][:37])) and torch.equal(bits(loss37), bits(outs[0][1][:37]))


def test_a_null_group_is_not_written_and_does_not_change_the_other(X):
    B, N, K0, K1 = X.BM + 1, 2 * X.BN + 3, 3, 3
    eps = 0.1
    A, T, t, w = make(B, N, K0, K1, seed=51)
    prob = problem(segs(A, K0, K1), segs(T, K0, K1))
    rc, lse, _ = fwd(X, prob, t, eps)
    assert rc == 0
    rc, dA, dT = bwd(X, prob, t, eps, lse, w)
    assert rc == 0
    # no table gradient: the guarded dT buffers are never handed over and stay as they are
    dT_g = [guarded_out(N, 3), guarded_out(N, 3)]
    rc, dA_only, none = bwd(X, prob, t, eps, lse, w, dT=None)
    assert rc == 0 and none is None
    for a, b in zip(dA_only, dA):
        assert torch.equal(bits(a), bits(b))
    # no query gradient
    rc, none, dT_only = bwd(X, prob, t, eps, lse, w, dA=None)
    assert rc == 0 and none is None
    for a, b in zip(dT_only, dT):
        assert torch.equal(bits(a), bits(b))
    # a group whose first pointer is NULL but whose second is given is malformed: nothing is written
    dA_g = [guarded_out(B, 3), guarded_out(B, 3)]
    args = [prob.desc, t, eps, lse, w, None, 0, dA_g[1], dA_g[1].stride(0), dT_g[0], dT_g[0].stride(0), dT_g[1],
            dT_g[1].stride(0)]
    ws = workspace(X, prob)
    assert raw(X.load_library(), 'kge_lp_xent_bwd', *(args + [ws, ws.numel()])) == EINVAL
    torch.cuda.synchronize()
    for v in dA_g + dT_g:
        assert_guard_intact(v, rows=0)


# ---------------------------------------------------------------------------
# refusals: nothing is launched, nothing is written
# ---------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched(X):
    from torchkge_amd import _hip
    B, N, K0, K1 = 5, 70, 8, 0
    A, T, t, w = make(B, N, K0, K1, seed=61)
    prob = problem([A], [T])
    lse_ok = fwd(X, prob, t, 0.0)[1]
    lib = X.load_library()
    ws = workspace(X, prob)
    outs = {'lse': guarded_out(B), 'loss': guarded_out(B), 'dA': guarded_out(B, K0), 'dT': guarded_out(N, K0)}

    def both(desc, expect, lse='out', ws_n=None, tag=''):
        n = ws.numel() if ws_n is None else ws_n
        f_lse = outs['lse'] if lse == 'out' else lse
        assert raw(lib, 'kge_lp_xent_fwd', desc, t, 0.0, f_lse, outs['loss'], ws, n) == expect, ('fwd', tag)
        b_lse = lse_ok if lse == 'out' else lse
        assert raw(lib, 'kge_lp_xent_bwd', desc, t, 0.0, b_lse, w, outs['dA'], K0, None, 0, outs['dT'], K0, None, 0, ws,
                   n) == expect, ('bwd', tag)

    def variant(**kw):
        d = _hip.LpDesc.from_buffer_copy(prob.desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    qn, en = torch.zeros(B, device='cuda'), torch.zeros(N, device='cuda')
    for mode in (_hip.LP_L2_EXPAND, _hip.LP_L2_DIRECT, _hip.LP_L1_DIRECT):
        both(variant(mode=mode, qn=qn.data_ptr(), en=en.data_ptr()), EUNSUPPORTED, tag='mode %d' % mode)
    both(variant(c_base=1), EUNSUPPORTED, tag='c_base')
    wide_a, wide_t = torch.zeros(B, 513, device='cuda'), torch.zeros(N, 513, device='cuda')
    wide = problem([wide_a, wide_a[:, :512].contiguous()], [wide_t, wide_t[:, :512].contiguous()])
    assert int(wide.desc.K0) + int(wide.desc.K1) == 1025
    both(wide.desc, EUNSUPPORTED, tag='K0 + K1 = 1025')
    both(prob.desc, EINVAL, lse=None, tag='NULL lse')
    both(prob.desc, EINVAL, ws_n=X.ws_bytes(B, N, K0, K1) - 1, tag='short workspace')
    both(variant(B=-1), EINVAL, tag='B < 0')
    assert raw(lib, 'kge_lp_xent_fwd', prob.desc, t, 0.0, outs['lse'], outs['loss'], None, ws.numel()) == EINVAL
    assert raw(lib, 'kge_lp_xent_fwd', prob.desc, t, 1.5, outs['lse'], outs['loss'], ws, ws.numel()) == EINVAL
    assert raw(lib, 'kge_lp_xent_fwd', prob.desc, None, 0.0, outs['lse'], outs['loss'], ws, ws.numel()) == EINVAL
    assert raw(lib, 'kge_lp_xent_bwd', prob.desc, t, 0.0, lse_ok, None, outs['dA'], K0, None, 0, outs['dT'], K0, None, 0, ws,
               ws.numel()) == EINVAL       # NULL g
    torch.cuda.synchronize()
    for v in outs.values():
        assert_guard_intact(v, rows=0)
    # B = 0: success, nothing launched
    assert raw(lib, 'kge_lp_xent_fwd', variant(B=0), t, 0.0, outs['lse'], outs['loss'], ws, ws.numel()) == 0
    torch.cuda.synchronize()
    assert_guard_intact(outs['lse'], rows=0)
