"""GPU tests of the fused training criterion kge_pair_loss (include/kge_hip_train.h; run with -m gpu on an MI355X).

Yardstick: the closed forms of the header's table evaluated in float64 on the CPU (``forms64``).  The first test shows
on scores in [-10, 10] that these ARE the reference's stock criteria -- MarginRankingLoss, SoftMarginLoss and
BCELoss o sigmoid with reduction='sum' -- in float64, loss and autograd gradients alike: the forms under test are
anchored to the reference, not to the kernel.

Comparator: torch's own fp32 evaluation of utils/losses.py on the same device and inputs.  Tolerance, the shape of
DESIGN.md section 3.15's bound: for the loss 4 * (2 * |torch fp32 - float64| + one fp32 ulp of the loss); for the
gradients the same in max-norm with the ulp of 1.0.  Where the comparator is not finite (the saturation test: that is
why the fused forms exist) its distance is replaced by an a-priori one: one fp32 ulp per term for the loss (expf and
log1pf are good to an ulp and the sum itself is carried in fp64), one ulp of 1.0 for a gradient."""
import numpy as np
import pytest
import torch

from tests.helpers import raw, carve, guarded_out, assert_guard_intact

pytestmark = pytest.mark.gpu

KINDS = ('margin', 'logistic', 'bce')
MARGIN = 0.5
EINVAL = -1
ULP1 = 2.0 ** -23
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 32768 + 105)


@pytest.fixture(scope='module')
def T():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_train
    _hip_train.load_library()
    return _hip_train


def code(T, kind):
    return {'margin': T.LOSS_MARGIN, 'logistic': T.LOSS_LOGISTIC, 'bce': T.LOSS_BCE}[kind]


def bits(x):
    return x.contiguous().view(torch.int32)


def ulp_of(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def softplus64(x):
    return x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))


def sigma64(x):
    e = torch.exp(-x.abs())
    return torch.where(x >= 0, 1 / (1 + e), e / (1 + e))


def forms64(kind, margin, pos, neg, terms=False):
    """(loss, dpos, dneg) of the header's table in float64 on the CPU, from fp32 scores taken as they are."""
    p, n = pos.detach().double().cpu(), neg.detach().double().cpu()
    if kind == 'margin':
        a = np.float64(margin) - p + n
        t = a.clamp_min(0)
        on = (a >= 0).double()
        dp, dn = -on, on
    else:
        sp, sn = softplus64(-p), softplus64(n)
        dp, dn = -sigma64(-p), sigma64(n)
        if kind == 'bce':
            dp, dn = torch.where(sp > 100, torch.zeros_like(dp), dp), torch.where(sn > 100, torch.zeros_like(dn), dn)
            sp, sn = sp.clamp_max(100), sn.clamp_max(100)
        t = sp + sn
    return (t if terms else t.sum()), dp, dn


def stock32(kind, margin, pos, neg):
    """(loss, dpos, dneg) of utils/losses.py in fp32 on the scores' device, gradients by autograd."""
    from torchkge_amd.utils import losses
    crit = {'margin': losses.MarginLoss(margin), 'logistic': losses.LogisticLoss(), 'bce': losses.BinaryCrossEntropyLoss()}[kind]
    p, n = pos.detach().clone().requires_grad_(), neg.detach().clone().requires_grad_()
    loss = crit(p, n)
    loss.backward()
    return loss.detach(), p.grad, n.grad


def fused(T, kind, margin, pos, neg, acc=None):
    loss, grads = T.pair_loss(code(T, kind), margin, pos, neg, acc)
    n = pos.shape[0]
    return loss, grads[:n], grads[n:]


def scores(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    scale = 1.0 if kind == 'margin' else 3.0
    return (torch.randn(n, generator=g) * scale).cuda(), (torch.randn(n, generator=g) * scale).cuda()


def check_against_yardstick(T, kind, pos, neg, tag, record=None):
    """The kernel against forms64 under the module's tolerance; returns (loss, dpos, dneg) of the kernel."""
    loss, dp, dn = fused(T, kind, MARGIN, pos, neg)
    l64, dp64, dn64 = forms64(kind, MARGIN, pos, neg)
    l32, dp32, dn32 = stock32(kind, MARGIN, pos, neg)
    cmp_loss = abs(float(l32.double().cpu()) - float(l64))
    cmp_grad = max(float((dp32.double().cpu() - dp64).abs().max()), float((dn32.double().cpu() - dn64).abs().max()))
    our_loss = abs(float(loss.double().cpu()) - float(l64))
    our_grad = max(float((dp.double().cpu() - dp64).abs().max()), float((dn.double().cpu() - dn64).abs().max()))
    tol_loss = 4 * (2 * cmp_loss + ulp_of(l64))
    tol_grad = 4 * (2 * cmp_grad + ULP1)
    print('pair_loss %-8s %-14s loss %.9g: |fused - f64| %.3g (torch fp32 %.3g, bound %.3g); gradients %.3g (torch fp32 %.3g, '
          'bound %.3g)' % (kind, tag, float(l64), our_loss, cmp_loss, tol_loss, our_grad, cmp_grad, tol_grad))
    if record is not None:
        record.append((our_loss / max(abs(float(l64)), 1e-30), cmp_loss / max(abs(float(l64)), 1e-30), our_grad, cmp_grad))
    assert our_loss <= tol_loss, (kind, tag, our_loss, tol_loss)
    assert our_grad <= tol_grad, (kind, tag, our_grad, tol_grad)
    return loss, dp, dn


# ---------------------------------------------------------------------------
# the yardstick is the reference's stock criteria
# ---------------------------------------------------------------------------
def test_the_float64_forms_are_the_stock_criteria():
    g = torch.Generator().manual_seed(5)
    n = 4099
    pos = (torch.rand(n, generator=g, dtype=torch.float64) * 20 - 10).float()
    neg = (torch.rand(n, generator=g, dtype=torch.float64) * 20 - 10).float()
    pos[:2], neg[:2] = torch.tensor([10.0, -10.0]), torch.tensor([-10.0, 10.0])
    for kind in KINDS:
        p, q = pos.double().requires_grad_(), neg.double().requires_grad_()
        if kind == 'margin':
            loss = torch.nn.MarginRankingLoss(margin=MARGIN, reduction='sum')(p, q, torch.ones(n, dtype=torch.float64))
        elif kind == 'logistic':
            y = torch.cat([torch.ones(n), -torch.ones(n)]).double()
            loss = torch.nn.SoftMarginLoss(reduction='sum')(torch.cat([p, q]), y)
        else:
            y = torch.cat([torch.ones(n), torch.zeros(n)]).double()
            loss = torch.nn.BCELoss(reduction='sum')(torch.sigmoid(torch.cat([p, q])), y)
        loss.backward()
        l64, dp64, dn64 = forms64(kind, MARGIN, pos, neg)
        assert abs(float(loss.detach()) - float(l64)) <= 1e-12 * abs(float(l64)), kind
        # (sigmoid's autograd in float64 near |x| = 10: relative 1e-12 of gradients down to 4.5e-5)
        assert float((p.grad - dp64).abs().max()) <= 1e-12 and float((q.grad - dn64).abs().max()) <= 1e-12, kind


# ---------------------------------------------------------------------------
# every length, twice, against the yardstick
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_lengths_against_the_yardstick_and_the_same_bits_twice(T, kind):
    beyond_cap = T.max_blocks() * T.CHUNK + T.CHUNK + 5     # every block takes two turns, the last one a short one
    rec = []
    for n in LENGTHS + (beyond_cap,):
        pos, neg = scores(kind, n, 100 + n % 9973)
        loss, dp, dn = check_against_yardstick(T, kind, pos, neg, 'n=%d' % n, rec)
        loss2, dp2, dn2 = fused(T, kind, MARGIN, pos, neg)
        assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(dp), bits(dp2)) and torch.equal(bits(dn), bits(dn2)), n
        # the value alone: the same bits, no gradient vector
        lv, gv = T.pair_loss(code(T, kind), MARGIN, pos, neg, need_grad=False)
        assert gv is None and torch.equal(bits(lv), bits(loss)), n
    print('pair_loss %-8s worst over the lengths: loss relative %.3g (torch fp32 %.3g), gradients %.3g (torch fp32 %.3g)'
          % ((kind,) + tuple(max(r[i] for r in rec) for i in range(4))))


# ---------------------------------------------------------------------------
# alignment: 16-byte quads and scalars give the same bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_every_alignment_gives_the_bits_of_the_aligned_copy(T, kind):
    lib = T.load_library()
    b = 257
    # the Trainer's layout: the two halves of one score vector, neg 4 * 257 bytes after pos
    both = torch.cat(scores(kind, b, 7))
    assert both.data_ptr() % 16 == 0 and both[b:].data_ptr() % 16 == 4
    want = fused(T, kind, MARGIN, both[:b].clone(), both[b:].clone())
    assert all(x.data_ptr() % 16 == 0 for x in (want[1],)) and want[2].data_ptr() % 16 == 4     # (the wrapper's own halves)
    got = fused(T, kind, MARGIN, both[:b], both[b:])
    for w, g in zip(want, got):
        assert torch.equal(bits(w), bits(g))
    check_against_yardstick(T, kind, both[:b], both[b:], 'halves b=257')
    # every pointer by itself: separate allocations at chosen offsets past a 16-byte boundary, poisoned around
    for n in (257, 1029, 2 * T.CHUNK + 3):
        pos, neg = scores(kind, n, 11 + n)
        ws = torch.empty(T.ws_bytes(n), dtype=torch.uint8, device='cuda')
        ref = None
        for offs in ((0, 0, 0, 0), (0, 1, 0, 1), (1, 0, 2, 0), (1, 2, 3, 0), (3, 3, 2, 1), (2, 2, 2, 2)):
            p, q = carve(pos, off=offs[0]), carve(neg, off=offs[1])
            dp, dq = guarded_out(n, off=offs[2]), guarded_out(n, off=offs[3])
            loss = guarded_out(1)
            assert [x.data_ptr() % 16 for x in (p, q, dp, dq)] == [4 * o for o in offs]
            assert raw(lib, 'kge_pair_loss', code(T, kind), MARGIN, p, q, n, loss, None, dp, dq, ws, ws.numel()) == 0
            for x in (p, q, dp, dq, loss):
                assert_guard_intact(x)
            out = (loss.clone(), dp.clone(), dq.clone())
            if ref is None:
                ref = out
                w = fused(T, kind, MARGIN, pos, neg)
                assert all(torch.equal(bits(a), bits(c.view_as(a))) for a, c in zip(w, ref))
            assert all(torch.equal(bits(a), bits(c)) for a, c in zip(ref, out)), (n, offs)


# ---------------------------------------------------------------------------
# margin ties: a hinge of exactly zero passes the gradient
# ---------------------------------------------------------------------------
def test_margin_ties_are_exact(T):
    g = torch.Generator().manual_seed(3)
    n = 3000
    pos = torch.randint(-5, 6, (n,), generator=g).float().cuda()
    neg = torch.randint(-5, 6, (n,), generator=g).float().cuda()
    margin = 2.0
    tie = (pos - neg) == margin
    assert 100 < int(tie.sum()) < n // 4 and int(((margin - pos + neg) > 0).sum()) > 100 and int(((margin - pos + neg) < 0).sum()) > 100
    loss, dp, dn = fused(T, 'margin', margin, pos, neg)
    l64, dp64, dn64 = forms64('margin', margin, pos, neg)
    assert float(loss) == float(l64)                                # integers: every sum is exact
    assert torch.equal(dp.cpu().double(), dp64) and torch.equal(dn.cpu().double(), dn64)
    assert bool((dp[tie] == -1).all()) and bool((dn[tie] == 1).all())
    # the existing MarginLoss passes the gradient at a tie as well
    _, dp32, dn32 = stock32('margin', margin, pos, neg)
    assert torch.equal(dp32, dp) and torch.equal(dn32, dn)


# ---------------------------------------------------------------------------
# saturation
# ---------------------------------------------------------------------------
def test_saturated_scores_stay_finite_and_capped(T, record_property):
    vals = torch.tensor([s * v for v in (17, 30, 88, 89, 99.9, 100.1, 120, 1e4) for s in (1.0, -1.0)])
    pos, neg = vals.repeat_interleave(16).cuda(), vals.repeat(16).cuda()       # every (pos, neg) combination
    n = pos.shape[0]
    for kind in KINDS:
        loss, dp, dn = fused(T, kind, MARGIN, pos, neg)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dp).all()) and bool(torch.isfinite(dn).all()), kind
        t64, dp64, dn64 = forms64(kind, MARGIN, pos, neg, terms=True)
        l64 = float(t64.sum())
        l32, dp32, dn32 = stock32(kind, MARGIN, pos, neg)
        # where the comparator is not finite, one fp32 ulp per term / of 1.0 stands for its distance (module docstring)
        cmp_loss = abs(float(l32.double().cpu()) - l64)
        cmp_grad = max(float((dp32.double().cpu() - dp64).abs().max()), float((dn32.double().cpu() - dn64).abs().max()))
        if not np.isfinite(cmp_loss):
            cmp_loss = float(sum(np.spacing(np.float32(abs(x))) for x in t64.tolist()))
        if not np.isfinite(cmp_grad):
            cmp_grad = ULP1
        tol_loss, tol_grad = 4 * (2 * cmp_loss + ulp_of(l64)), 4 * (2 * cmp_grad + ULP1)
        our_loss = abs(float(loss.double().cpu()) - l64)
        our_grad = max(float((dp.double().cpu() - dp64).abs().max()), float((dn.double().cpu() - dn64).abs().max()))
        print('pair_loss %-8s saturation     loss %.9g: |fused - f64| %.3g (bound %.3g); gradients %.3g (bound %.3g)'
              % (kind, l64, our_loss, tol_loss, our_grad, tol_grad))
        if kind != 'margin':        # (the hinge has no saturation: its values are covered by the length test)
            assert our_loss <= tol_loss and our_grad <= tol_grad, kind
        # what the written-out criteria give on the same inputs (recorded, not asserted: they are not under test)
        bad = int((~torch.isfinite(dp32)).sum() + (~torch.isfinite(dn32)).sum())
        print('          utils/losses.py on the same inputs: loss %s, %d of %d gradient entries not finite'
              % (float(l32), bad, 2 * n))
        record_property('stock_%s_nonfinite_gradients' % kind, bad)
    # BCE: a term is cut off at 100, and beyond the cut-off the gradient is exactly 0
    _, dp, dn = fused(T, 'bce', 0.0, pos, neg)
    capped_p, capped_n = pos < -100, neg > 100
    assert int(capped_p.sum()) == 3 * 16 == int(capped_n.sum())
    assert bool((dp[capped_p] == 0).all()) and bool((dn[capped_n] == 0).all())
    assert bool((dp[(pos > -100) & (pos < 0)] < 0).all()) and bool((dn[(neg < 100) & (neg > 0)] > 0).all())
    one = lambda p, q: float(fused(T, 'bce', 0.0, torch.tensor([p]).cuda(), torch.tensor([q]).cuda())[0])     # noqa: E731
    assert one(-120.0, -1e4) == 100.0 and one(1e4, 100.1) == 100.0 and one(-1e4, 1e4) == 200.0
    assert abs(one(-99.9, -1e4) - 99.9) <= ulp_of(99.9)
    # logistic has no cut-off
    assert float(fused(T, 'logistic', 0.0, torch.tensor([-1e4]).cuda(), torch.tensor([120.0]).cuda())[0]) == 10120.0


# ---------------------------------------------------------------------------
# acc_io, the value-only mode, n = 0, refusals
# ---------------------------------------------------------------------------
def test_acc_io_is_the_fp32_sum_of_the_losses_in_call_order(T):
    acc = torch.full((), 0.75, device='cuda')
    want = np.float32(0.75)
    for i, (kind, n) in enumerate((('logistic', 1000), ('margin', 5000), ('bce', 1))):
        pos, neg = scores(kind, n, 40 + i)
        loss, _, _ = fused(T, kind, MARGIN, pos, neg, acc)
        plain, _, _ = fused(T, kind, MARGIN, pos, neg)
        assert torch.equal(bits(loss), bits(plain))             # the running sum does not change the value
        want = np.float32(want + np.float32(float(loss)))
    assert float(acc) == float(want)
    # value-only mode adds as well
    pos, neg = scores('margin', 77, 1)
    lv, _ = T.pair_loss(T.LOSS_MARGIN, MARGIN, pos, neg, acc, need_grad=False)
    assert float(acc) == float(np.float32(want + np.float32(float(lv))))


def test_value_only_n_zero_and_refusals_leave_poisoned_outputs_alone(T):
    lib = T.load_library()
    n = 2 * T.CHUNK + 1                                         # three blocks: 24 bytes of workspace
    pos, neg = scores('logistic', n, 2)
    ws = torch.empty(64, dtype=torch.uint8, device='cuda')
    assert T.ws_bytes(n) == 24 and ws.data_ptr() % 8 == 0

    def outputs():
        return guarded_out(1), guarded_out(1), guarded_out(n), guarded_out(n)      # loss, acc, dpos, dneg

    def untouched(*views):
        torch.cuda.synchronize()
        for v in views:
            assert_guard_intact(v, rows=0)

    k = T.LOSS_LOGISTIC
    # the value only: loss written, nothing else
    loss, acc, dp, dq = outputs()
    assert raw(lib, 'kge_pair_loss', k, 0.0, pos, neg, n, loss, None, None, None, ws, 24) == 0
    untouched(acc, dp, dq)
    assert_guard_intact(loss)
    assert torch.equal(bits(loss), bits(fused(T, 'logistic', 0.0, pos, neg)[0].view(1)))
    # n = 0: *loss = 0, *acc_io left alone, no workspace needed
    loss, acc, dp, dq = outputs()
    assert raw(lib, 'kge_pair_loss', k, 0.0, None, None, 0, loss, acc, dp, dq, None, 0) == 0
    untouched(acc, dp, dq)
    assert_guard_intact(loss)
    assert float(loss) == 0.0 and int(bits(loss)) == 0
    l0, g0 = T.pair_loss(k, 0.0, pos[:0], neg[:0])
    assert float(l0) == 0.0 and g0.shape == (0,)
    # refusals
    loss, acc, dp, dq = outputs()
    misaligned = ws[4:]
    for args in ((-1, 0.0, pos, neg, n, loss, acc, dp, dq, ws, 64),             # a kind outside the three
                 (3, 0.0, pos, neg, n, loss, acc, dp, dq, ws, 64),
                 (k, 0.0, pos, neg, n, loss, acc, dp, dq, None, 64),            # no workspace
                 (k, 0.0, pos, neg, n, loss, acc, dp, dq, ws, 23),              # a short one
                 (k, 0.0, pos, neg, n, loss, acc, dp, dq, ws, 0),
                 (k, 0.0, pos, neg, n, loss, acc, dp, dq, misaligned, 60),      # off the 8-byte grid
                 (k, 0.0, pos, neg, n, loss, acc, dp, None, ws, 64),            # one gradient vector without the other
                 (k, 0.0, pos, neg, n, loss, acc, None, dq, ws, 64),
                 (k, 0.0, None, neg, n, loss, acc, dp, dq, ws, 64),
                 (k, 0.0, pos, None, n, loss, acc, dp, dq, ws, 64),
                 (k, 0.0, pos, neg, n, None, acc, dp, dq, ws, 64),
                 (k, 0.0, pos, neg, -1, loss, acc, dp, dq, ws, 64),
                 (k, 0.0, pos, neg, 1 << 31, loss, acc, dp, dq, ws, 64)):
        assert raw(lib, 'kge_pair_loss', *args) == EINVAL, args[:1] + args[4:5] + args[10:]
    untouched(loss, acc, dp, dq)
    with pytest.raises(RuntimeError, match='as many negative as positive'):
        T.pair_loss(k, 0.0, pos, neg[:-1])
    with pytest.raises(RuntimeError, match='float32 vectors'):
        T.pair_loss(k, 0.0, pos.double(), neg.double())


# ---------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_the_function_scales_the_saved_vectors_by_the_incoming_scalar(T, kind):
    from torchkge_amd.utils import fused_losses
    crit = {'margin': fused_losses.FusedMarginLoss(MARGIN), 'logistic': fused_losses.FusedLogisticLoss(),
            'bce': fused_losses.FusedBinaryCrossEntropyLoss()}[kind]
    n = 1500
    pos, neg = scores(kind, n, 21)
    want_loss, dp, dn = fused(T, kind, MARGIN, pos, neg)
    p, q = pos.clone().requires_grad_(), neg.clone().requires_grad_()
    loss = crit(p, q)
    assert loss.shape == () and loss.requires_grad and torch.equal(bits(loss.detach()), bits(want_loss))
    (loss * 0.25).backward()
    assert torch.equal(p.grad, 0.25 * dp) and torch.equal(q.grad, 0.25 * dn)        # a power of two: exact
    # the two halves of one differentiable score vector, as Model.forward hands them over
    s = torch.cat([pos, neg]).requires_grad_()
    crit(s[:n], s[n:]).backward()
    assert torch.equal(s.grad, torch.cat([dp, dn]))
    # one side only, and none
    p = pos.clone().requires_grad_()
    crit(p, neg).backward()
    assert torch.equal(p.grad, dp)
    assert not crit(pos, neg).requires_grad
    # the running sum through the module's call
    acc = torch.zeros((), device='cuda')
    crit(pos, neg, acc)
    crit(pos, neg, acc)
    assert float(acc) == float(np.float32(np.float32(float(want_loss)) * 2))
