"""GPU tests of the grouped training criteria kge_group_loss (include/kge_hip_group.h; run with -m gpu on an MI355X).

Yardstick: the header's forms in float64 on the CPU (tests/group_loss_ref.py ``forms64``; tests/test_group_loss_host.py
anchors them to torch's stock operators).  Comparator: the same criterion written out in torch, fp32, on the same device
and inputs (``stock``).  Tolerance, the shape of tests/test_gpu_pair_loss.py: for the loss
4 * (2 * |torch fp32 - float64| + one fp32 ulp of the loss); for the gradients and row_loss the same in max-norm with the
ulp of 1.0.  Where the comparator is not finite (the saturation test) its distance is replaced by one fp32 ulp per term
for the loss and per row term, one ulp of 1.0 for a gradient.

The shapes come from the header's geometry: R rows per panel, S k-slices per block, C negatives per chunk at least, M
chunks at most."""
import numpy as np
import pytest
import torch

from tests.helpers import raw, carve, guarded_out, assert_guard_intact
from tests.group_loss_ref import KINDS, forms64, stock

pytestmark = pytest.mark.gpu

MARGIN = 0.5
EINVAL = -1
ULP1 = 2.0 ** -23
ALPHAS = (0.0, 0.5, 1.0)


@pytest.fixture(scope='module')
def G():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_group
    _hip_group.load_library()
    return _hip_group


def geometry(G):
    R, S, C, M = G.ROWS, G.SLICES, G.MIN_K_PER_CHUNK, G.MAX_CHUNKS
    Bs = (1, R - 1, R, R + 1, 2 * R + 1)
    Ks = (1, 2, S - 1, S, S + 1, C - 1, C, C + 1, 2 * C + 1, M * C, M * C + 1, 2 * M * C + 3)
    return Bs, Ks


def code(G, kind):
    return {'nssa': G.GROUP_NSSA, 'softmax': G.GROUP_SOFTMAX}[kind]


def bits(x):
    return x.contiguous().view(torch.int32)


def ulp_of(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def scores(B, K, seed, scale=1.0, weighted=False):
    g = torch.Generator().manual_seed(seed)
    pos, neg = torch.randn(B, generator=g) * scale, torch.randn(K, B, generator=g) * scale
    w = (torch.rand(B, generator=g) + 0.25) if weighted else None
    return pos.cuda(), neg.cuda(), None if w is None else w.cuda()


def fused(G, kind, alpha, pos, neg, w=None, acc=None, margin=MARGIN):
    """(loss, row_loss, dpos, dneg (K, B)) of the wrapper."""
    K, B = neg.shape
    loss, row, grads = G.group_loss(code(G, kind), margin, alpha, pos, neg, K, w, acc)
    return loss, row, grads[:B], grads[B:].view(K, B)


def distances(got, ref64):
    """|got - float64| for (row_loss, loss, dpos, dneg): loss absolute, the others in max-norm."""
    row, loss, dp, dn = got
    row64, l64, dp64, dn64 = ref64
    return (float((row.double().cpu() - row64).abs().max()), abs(float(loss.double().cpu()) - float(l64)),
            max(float((dp.double().cpu() - dp64).abs().max()), float((dn.double().cpu() - dn64).abs().max())))


def check_against_yardstick(G, kind, alpha, pos, neg, w, tag, record=None):
    loss, row, dp, dn = fused(G, kind, alpha, pos, neg, w)
    ref64 = forms64(kind, MARGIN, alpha, pos, neg, w)
    ours = distances((row, loss, dp, dn), ref64)
    cmp_ = distances(stock(kind, MARGIN, alpha, pos, neg, w), ref64)
    tol = (4 * (2 * cmp_[0] + ULP1), 4 * (2 * cmp_[1] + ulp_of(ref64[1])), 4 * (2 * cmp_[2] + ULP1))
    print('group_loss %-7s a=%.1f %-16s loss %.9g: |fused - f64| %.3g (torch fp32 %.3g, bound %.3g); row_loss %.3g (%.3g, '
          '%.3g); gradients %.3g (%.3g, %.3g)' % (kind, alpha, tag, float(ref64[1]), ours[1], cmp_[1], tol[1], ours[0], cmp_[0],
                                                   tol[0], ours[2], cmp_[2], tol[2]))
    if record is not None:
        record.append(ours + cmp_)
    for o, t, what in zip(ours, tol, ('row_loss', 'loss', 'gradients')):
        assert o <= t, (kind, alpha, tag, what, o, t)
    return loss, row, dp, dn


# ---------------------------------------------------------------------------
# every shape of the geometry against the yardstick, the same bits twice, the value alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('kind', KINDS)
def test_shapes_against_the_yardstick_and_the_same_bits_twice(G, kind, weighted):
    Bs, Ks = geometry(G)
    rec = []
    for B in Bs:
        for K in Ks:
            pos, neg, w = scores(B, K, 1000 * B + K, weighted=weighted)
            for alpha in (ALPHAS if kind == 'nssa' else (1.0,)):
                out = check_against_yardstick(G, kind, alpha, pos, neg, w, 'B=%d K=%d' % (B, K), rec)
                again = fused(G, kind, alpha, pos, neg, w)
                assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out, again)), (B, K, alpha)
            # the value alone: the same bits, no gradient vector
            lv, rv, gv = G.group_loss(code(G, kind), MARGIN, alpha, pos, neg, K, w, need_grad=False)
            assert gv is None and torch.equal(bits(lv), bits(out[0])) and torch.equal(bits(rv), bits(out[1])), (B, K)
    print('group_loss %-7s worst over the shapes: row_loss %.3g, loss %.3g, gradients %.3g (torch fp32 %.3g, %.3g, %.3g)'
          % ((kind,) + tuple(max(r[i] for r in rec) for i in range(6))))


# ---------------------------------------------------------------------------
# alignment and leading dimensions: quads and scalars give the same bits; pads are neither read nor written
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_every_offset_and_leading_dimension_gives_the_bits_of_the_aligned_copy(G, kind):
    lib = G.load_library()
    R, C = G.ROWS, G.MIN_K_PER_CHUNK
    k = code(G, kind)
    for B, K in ((R + 4, C + 3), (2 * R + 1, 5)):
        pos, neg, w = scores(B, K, 31 + B, weighted=True)
        want = fused(G, kind, 0.5, pos, neg, w)
        ws = torch.empty(G.ws_bytes(B, K), dtype=torch.uint8, device='cuda')
        assert ws.data_ptr() % 16 == 0
        for off in range(4):
            for pad_n, pad_d in ((0, 0), (1, 3), (3, 1), (0, 3), (3, 0), (1, 1)):
                # NaN in the pad columns of neg (carve's poison) must reach nothing
                p, x, rw = carve(pos, off=off), carve(neg, pad=pad_n, off=(off + 1) % 4), carve(w, off=(off + 2) % 4)
                dp, dx = guarded_out(B, off=(off + 3) % 4), guarded_out(K, B, pad=pad_d, off=off)
                row, loss, acc = guarded_out(B, off=(off + 1) % 4), guarded_out(1), guarded_out(1)
                assert x.stride(0) == B + pad_n and dx.stride(0) == B + pad_d and p.data_ptr() % 16 == 4 * off
                assert raw(lib, 'kge_group_loss', k, MARGIN, 0.5, p, x, B + pad_n, rw, B, K, loss, None, row, dp, dx,
                           B + pad_d, ws, ws.numel()) == 0
                torch.cuda.synchronize()
                for v in (p, x, rw, dp, dx, row, loss):
                    assert_guard_intact(v)
                assert_guard_intact(acc, rows=0)
                got = (loss.clone().view(()), row.clone(), dp.clone(), dx.clone())
                for a, b, what in zip(want, got, ('loss', 'row_loss', 'dpos', 'dneg')):
                    assert torch.equal(bits(a), bits(b)), (B, K, off, pad_n, pad_d, what)


# ---------------------------------------------------------------------------
# row independence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_a_range_of_rows_alone_reproduces_its_bits_from_the_full_batch(G, kind):
    R, C, M = G.ROWS, G.MIN_K_PER_CHUNK, G.MAX_CHUNKS
    B = 2 * R + 9
    for K in (3, 2 * C + 1, M * C + 1):
        pos, neg, w = scores(B, K, 77 + K, weighted=True)
        _, row, dp, dn = fused(G, kind, 1.0, pos, neg, w)
        for a, b in ((0, 1), (5, 70), (R - 3, R + 2), (R - 1, 2 * R + 1), (R, 2 * R), (B - 1, B), (1, B)):
            _, row2, dp2, dn2 = fused(G, kind, 1.0, pos[a:b].clone(), neg[:, a:b].contiguous(), w[a:b].clone())
            assert torch.equal(bits(row[a:b]), bits(row2)) and torch.equal(bits(dp[a:b]), bits(dp2)), (K, a, b)
            assert torch.equal(bits(dn[:, a:b]), bits(dn2)), (K, a, b)
            # ... and where it lies: the columns [a, b) of the full matrix, leading dimension B
            l3, row3, g3 = G.group_loss(code(G, kind), MARGIN, 1.0, pos[a:b], neg[:, a:b], K, w[a:b])
            assert torch.equal(bits(row3), bits(row2)) and torch.equal(bits(g3[b - a:].view(K, b - a)), bits(dn2)), (K, a, b)


# ---------------------------------------------------------------------------
# saturation
# ---------------------------------------------------------------------------
def test_saturated_scores_stay_finite_and_underflowing_weights_are_zero(G, record_property):
    vals = torch.tensor([s * v for v in (17.0, 88.0, 89.0, 120.0, 1e4) for s in (1.0, -1.0)])
    B = vals.shape[0] ** 2
    pos = vals.repeat_interleave(vals.shape[0])
    neg = torch.stack([vals.repeat(vals.shape[0]), vals.flip(0).repeat(vals.shape[0]), pos.clone(), -pos,
                       torch.full((B,), 3.0), torch.full((B,), -250.0)])
    pos, neg = pos.cuda(), neg.cuda()
    K = neg.shape[0]
    for kind, margin, alpha in (('nssa', 0.5, 1.0), ('nssa', 1e3, 1.0), ('nssa', 1e3, 0.0), ('nssa', 6.0, 0.5), ('softmax', 0.0, 1.0)):
        loss, row, dp, dn = fused(G, kind, alpha, pos, neg, margin=margin)
        for x in (loss, row, dp, dn):
            assert bool(torch.isfinite(x).all()), (kind, margin, alpha)
        ref64 = forms64(kind, margin, alpha, pos, neg)
        ours = distances((row, loss, dp, dn), ref64)
        cmp_ = list(distances(stock(kind, margin, alpha, pos, neg), ref64))
        # where the comparator is not finite, one fp32 ulp per term / of 1.0 stands for its distance (module docstring)
        per_term = [float(np.spacing(np.float32(abs(v)))) for v in ref64[0].tolist()]
        substituted = [not np.isfinite(c) for c in cmp_]
        if substituted[0]:
            cmp_[0] = max(per_term)
        if substituted[1]:
            cmp_[1] = sum(per_term)
        if substituted[2]:
            cmp_[2] = ULP1
        tol = (4 * (2 * cmp_[0] + ULP1), 4 * (2 * cmp_[1] + ulp_of(ref64[1])), 4 * (2 * cmp_[2] + ULP1))
        print('group_loss %-7s margin %g a=%g saturation loss %.9g: |fused - f64| %.3g (bound %.3g); row_loss %.3g (%.3g); '
              'gradients %.3g (%.3g); comparator substituted: %s' % (kind, margin, alpha, float(ref64[1]), ours[1], tol[1],
                                                                      ours[0], tol[0], ours[2], tol[2], substituted))
        record_property('group_%s_margin%g_a%g_distances' % (kind, margin, alpha), ours)
        for o, t in zip(ours, tol):
            assert o <= t, (kind, margin, alpha, ours, tol)
    # a spread of temperature * x beyond 200: the weights that underflow are exactly 0, the dominant one is 1 to an ulp
    K, B = 70, 9
    neg = torch.linspace(-150.0, -60.0, K).view(K, 1).repeat(1, B)
    neg[37] = 120.0                                    # one dominant negative, 180 and more above every other
    neg[3, 4] = -1e4
    pos = torch.zeros(B)
    pos, neg = pos.cuda(), neg.cuda()
    margin = 2.0
    _, row, dp, dn = fused(G, 'nssa', 1.0, pos, neg, margin=margin)
    others = torch.ones(K, dtype=torch.bool)
    others[37] = False
    assert bool((dn[others] == 0).all()) and bool(torch.isfinite(dn).all())
    # sigma(margin + 120) is 1 in fp32: the gradient of the dominant negative IS its weight
    assert float((dn[37] - 1.0).abs().max()) <= ULP1
    want = forms64('nssa', margin, 1.0, pos, neg)[0]
    assert float((row.double().cpu() - want).abs().max()) <= 4 * ulp_of(122.0)
    # half that spread with temperature 0.5 underflows nothing that fp32 can hold: compare the weights themselves
    _, _, _, dn_half = fused(G, 'nssa', 0.5, pos, neg, margin=margin)
    ref = forms64('nssa', margin, 0.5, pos, neg)[3]
    assert float((dn_half.double().cpu() - ref).abs().max()) <= 4 * ULP1
    assert bool((dn_half[3, 4] == 0).all())
    # the softmax of a fact far below / far above its negatives
    lo = fused(G, 'softmax', 1.0, torch.tensor([-1e4, 1e4]).cuda(), torch.tensor([[1e4, -1e4], [0.0, 0.0]]).cuda())
    assert lo[1].tolist() == [2e4, 0.0] and lo[2].tolist() == [-1.0, 0.0] and lo[3].tolist() == [[1.0, 0.0], [0.0, 0.0]]


# ---------------------------------------------------------------------------
# acc_io, the value-only mode, B = 0, refusals
# ---------------------------------------------------------------------------
def test_acc_io_is_the_fp32_sum_of_the_losses_in_call_order(G):
    acc = torch.full((), 0.75, device='cuda')
    want = np.float32(0.75)
    for i, (kind, B, K) in enumerate((('nssa', 300, 7), ('softmax', 1500, 3), ('nssa', 1, 1))):
        pos, neg, _ = scores(B, K, 40 + i)
        loss = fused(G, kind, 1.0, pos, neg, None, acc)[0]
        plain = fused(G, kind, 1.0, pos, neg)[0]
        assert torch.equal(bits(loss), bits(plain))             # the running sum does not change the value
        want = np.float32(want + np.float32(float(loss)))
    assert float(acc) == float(want)
    # value-only mode adds as well
    pos, neg, _ = scores(77, 5, 1)
    lv = G.group_loss(G.GROUP_SOFTMAX, 0.0, 1.0, pos, neg, 5, None, acc, need_grad=False)[0]
    assert float(acc) == float(np.float32(want + np.float32(float(lv))))


def test_value_only_b_zero_and_refusals_leave_poisoned_outputs_alone(G):
    lib = G.load_library()
    B, K = G.ROWS + 3, G.MIN_K_PER_CHUNK + 1
    pos, neg, w = scores(B, K, 2, weighted=True)
    need = G.ws_bytes(B, K)
    ws = torch.empty(need + 64, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 16 == 0 and need % 16 == 0 and G.chunks(K) == 2

    def outputs():      # loss, acc, row_loss, dpos, dneg
        return guarded_out(1), guarded_out(1), guarded_out(B), guarded_out(B), guarded_out(K, B)

    def untouched(*views):
        torch.cuda.synchronize()
        for v in views:
            assert_guard_intact(v, rows=0)

    k = G.GROUP_NSSA
    # the value only: loss and row_loss written, no gradient
    loss, acc, row, dp, dx = outputs()
    assert raw(lib, 'kge_group_loss', k, MARGIN, 1.0, pos, neg, B, w, B, K, loss, None, row, None, None, 0, ws, need) == 0
    untouched(acc, dp, dx)
    assert_guard_intact(loss)
    assert_guard_intact(row)
    want = fused(G, 'nssa', 1.0, pos, neg, w)
    assert torch.equal(bits(loss), bits(want[0].view(1))) and torch.equal(bits(row), bits(want[1]))
    # ... and without row_loss
    loss, acc, row, dp, dx = outputs()
    assert raw(lib, 'kge_group_loss', k, MARGIN, 1.0, pos, neg, B, w, B, K, loss, None, None, None, None, 0, ws, need) == 0
    untouched(acc, row, dp, dx)
    assert torch.equal(bits(loss), bits(want[0].view(1)))
    # B = 0: *loss = 0, *acc_io left alone, no workspace needed
    loss, acc, row, dp, dx = outputs()
    assert raw(lib, 'kge_group_loss', k, MARGIN, 1.0, None, None, 0, None, 0, K, loss, acc, row, dp, dx, 0, None, 0) == 0
    untouched(acc, row, dp, dx)
    assert_guard_intact(loss)
    assert int(bits(loss)) == 0
    l0, r0, g0 = G.group_loss(k, MARGIN, 1.0, pos[:0], neg[:, :0], K)
    assert float(l0) == 0.0 and r0.shape == (0,) and g0.shape == (0,)
    # refusals
    loss, acc, row, dp, dx = outputs()
    nan, inf = float('nan'), float('inf')
    ok = dict(kind=k, margin=MARGIN, alpha=1.0, pos=pos, neg=neg, ld=B, w=w, B=B, K=K, loss=loss, acc=acc, row=row, dp=dp,
              dx=dx, ldd=B, ws=ws, nb=need)
    order = ('kind', 'margin', 'alpha', 'pos', 'neg', 'ld', 'w', 'B', 'K', 'loss', 'acc', 'row', 'dp', 'dx', 'ldd', 'ws', 'nb')
    for change in (dict(kind=-1), dict(kind=2), dict(B=-1), dict(K=0), dict(K=-3), dict(B=1 << 16, K=1 << 15, ld=1 << 16, ldd=1 << 16),
                   dict(alpha=-0.5), dict(alpha=inf), dict(alpha=nan), dict(ld=B - 1), dict(ldd=B - 1), dict(loss=None),
                   dict(pos=None), dict(neg=None), dict(dp=None), dict(dx=None), dict(ws=None), dict(ws=ws[8:]),
                   dict(nb=need - 1), dict(nb=0)):
        args = dict(ok, **change)
        assert raw(lib, 'kge_group_loss', *(args[n] for n in order)) == EINVAL, sorted(change)
    untouched(loss, acc, row, dp, dx)
    # the softmax kind ignores margin and temperature: a negative one is not refused there
    assert raw(lib, 'kge_group_loss', *(dict(ok, kind=G.GROUP_SOFTMAX, alpha=-1.0, margin=nan)[n] for n in order)) == 0
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(loss).all())
    with pytest.raises(ValueError, match='per fact'):
        G.group_loss(k, MARGIN, 1.0, pos, neg.reshape(-1)[:-1], K)
    with pytest.raises(RuntimeError, match='float32'):
        G.group_loss(k, MARGIN, 1.0, pos.double(), neg.reshape(-1).double(), K)


# ---------------------------------------------------------------------------
# autograd and the criteria
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_the_function_scales_by_the_incoming_scalar_and_both_forms_of_pos_agree(G, kind):
    from torchkge_amd.utils import group_losses
    B, K = 301, 6
    crit = group_losses.SelfAdversarialLoss(MARGIN, 0.5, n_neg=K) if kind == 'nssa' else group_losses.SampledSoftmaxLoss(n_neg=K)
    pos, neg, w = scores(B, K, 21, weighted=True)
    flat = neg.reshape(-1)
    want_loss, _, dp, dn = fused(G, kind, 0.5, pos, neg)
    p, q = pos.clone().requires_grad_(), flat.clone().requires_grad_()
    loss = crit(p, q)
    assert loss.shape == () and loss.requires_grad and torch.equal(bits(loss.detach()), bits(want_loss))
    (loss * 0.25).backward()
    assert torch.equal(p.grad, 0.25 * dp) and torch.equal(q.grad, 0.25 * dn.reshape(-1))      # a power of two: exact
    # the repeated form, as Model.forward hands it over: the same bits, the gradient once through repeat's backward
    p = pos.clone().requires_grad_()
    rep = p.repeat(K)
    loss2 = crit(rep, flat)
    assert torch.equal(bits(loss2.detach()), bits(want_loss))
    loss2.backward()
    assert torch.equal(p.grad, dp)
    # the two halves of one differentiable score vector
    s = torch.cat([pos.repeat(K), flat]).requires_grad_()
    crit(s[:B * K], s[B * K:]).backward()
    assert torch.equal(s.grad, torch.cat([dp, torch.zeros(B * (K - 1), device='cuda'), dn.reshape(-1)]))
    # one side only, and none
    p = pos.clone().requires_grad_()
    crit(p, flat).backward()
    assert torch.equal(p.grad, dp) and not crit(pos, flat).requires_grad
    # weights, the mean, the running sum
    lw = crit(pos, flat, weights=w)
    assert torch.equal(bits(lw), bits(fused(G, kind, 0.5, pos, neg, w)[0]))
    crit.reduction = 'mean'
    acc = torch.zeros((), device='cuda')
    lm = crit(pos, flat, acc)
    # (a division by a host scalar may run as a multiplication by its reciprocal: one more rounding)
    assert abs(float(lm) - float(want_loss) / B) <= ulp_of(float(want_loss) / B) and float(acc) == float(lm)
    crit.reduction = 'sum'
    crit(pos, flat, acc)
    assert float(acc) == float(np.float32(np.float32(float(lm)) + np.float32(float(want_loss))))
