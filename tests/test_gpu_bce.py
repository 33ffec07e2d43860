"""GPU tests of the K-vs-all criterion kge_lp_bce_fwd / kge_lp_bce_bwd (include/kge_hip_bce.h; run with -m gpu on an
MI355X), at kernel level through tests.helpers.raw / carve / guarded_out.

Yardstick: the float64 forms of tests/bce_ref.py (tests/test_bce_host.py anchors them to torch's
binary_cross_entropy_with_logits) applied to the engine's OWN fp32 scores -- kge_lp_scores, bit-defined code that
predates these kernels -- and to the dense label matrix scattered from the CSR.

Comparator: torch's fp32 evaluation on the same device -- binary_cross_entropy_with_logits of those scores forward,
autograd of the materialised formula (A @ T.t(), the criterion, weights g) backward.  Tolerance, that of
tests/test_gpu_xent.py: 4 * (2 * |torch fp32 - float64| + one fp32 ulp of the value), per output vector / matrix in
max-norm with the ulp of its largest float64 magnitude.

Shapes come from the constants the header publishes (BM = row panel, BN = candidate tile, the first N with two chunks);
the cases are a sparse cross in which every listed B, N and (K0, K1) occurs."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import raw, carve, guarded_out, assert_guard_intact
from tests import bce_ref

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
RECORD = []         # lines of the parity record (the parity_record fixture writes them out)
WORST = {}          # output name -> the largest |fused - f64| / bound seen


@pytest.fixture(scope='module')
def X():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_bce
    _hip_bce.load_library()
    return _hip_bce


@pytest.fixture(scope='module', autouse=True)
def parity_record():
    """After the module: the distances its tests measured go to the file KGE_BCE_PARITY_OUT names, when it names one
    (profiles/r11/bce_parity.txt is one such run)."""
    yield
    path = os.environ.get('KGE_BCE_PARITY_OUT')
    if path and RECORD:
        with open(path, 'w') as f:
            f.write('max-norm distances to the float64 forms of the engine\'s own fp32 scores (tests/test_gpu_bce.py)\n')
            f.write('\n'.join(RECORD) + '\n')
            for name, (ratio, tag) in sorted(WORST.items()):
                f.write('worst |fused - f64| / bound of %-8s %.3g  (%s)\n' % (name, ratio, tag))


def _shapes():
    from torchkge_amd import _hip_bce as x
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


def csr(sets, rows=None, front=0):
    """(seg_lo, seg_hi, labels) on the device from a list of ascending id lists; ``rows``: the segment of every row
    (default: row i takes set i); ``front``: unused entries in front of the first segment."""
    lens = torch.tensor([len(s) for s in sets], dtype=torch.long)
    hi = torch.cumsum(lens, 0) + front
    lo = hi - lens
    flat = [-7] * front + [c for s in sets for c in s]
    labels = torch.tensor(flat if flat else [0], dtype=torch.int32)
    rows = torch.arange(len(sets)) if rows is None else torch.as_tensor(rows)
    return lo[rows].contiguous().cuda(), hi[rows].contiguous().cuda(), labels.cuda()


def random_sets(B, N, gen):
    """Label sets of mixed length: empty, single, a few, and up to half of the candidates."""
    sets = []
    for i in range(B):
        n = (0, 1, 2, 5, N // 2, 1, 3, min(N, 70))[int(torch.randint(0, 8, (1,), generator=gen))]
        sets.append(sorted(torch.randperm(N, generator=gen)[:min(n, N)].tolist()))
    return sets


def make(B, N, K0, K1, seed, scale=3.0):
    """(A, T, labels, g) on the device: scores of standard deviation ~ `scale`, random label sets, non-uniform weights."""
    gen = torch.Generator().manual_seed(seed)
    K = K0 + K1
    A = torch.randn(B, K, generator=gen) * (scale / K ** 0.5)
    T = torch.randn(N, K, generator=gen)
    w = torch.rand(B, generator=gen) + 0.5
    return A.cuda(), T.cuda(), csr(random_sets(B, N, gen)), w.cuda()


def segs(M, K0, K1):
    return [M[:, :K0].contiguous()] + ([M[:, K0:].contiguous()] if K1 else [])


def problem(As, Ts):
    from torchkge_amd import _hip
    return _hip.LpProblem(_hip.LP_DOT, As[0], Ts[0], A1=As[1] if len(As) > 1 else None, T1=Ts[1] if len(Ts) > 1 else None)


def workspace(X, prob):
    d = prob.desc
    return torch.empty(max(X.ws_bytes(int(d.B), int(d.N), int(d.K0), int(d.K1)), 16), dtype=torch.uint8, device='cuda')


def fwd(X, prob, lab, eps, loss=None, ws=None):
    loss = torch.empty(prob.B, device='cuda') if loss is None else loss
    ws = workspace(X, prob) if ws is None else ws
    rc = raw(X.load_library(), 'kge_lp_bce_fwd', prob.desc, lab[0], lab[1], lab[2], float(eps), loss, ws, ws.numel())
    return rc, loss


def bwd(X, prob, lab, eps, w, dA='new', dT='new', ws=None):
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
    rc = raw(X.load_library(), 'kge_lp_bce_bwd', prob.desc, lab[0], lab[1], lab[2], float(eps), w, *(args + [ws, ws.numel()]))
    return rc, dA, dT


def within(name, tag, ours, ref64, cmp32):
    """max-norm distances of `ours` and of torch's fp32 to the float64 form, under the module's tolerance."""
    assert bool(torch.isfinite(ours).all()), (name, tag)
    ref64 = ref64.double().cpu()
    d_ours = float((ours.double().cpu() - ref64).abs().max())
    d_cmp = float((cmp32.double().cpu() - ref64).abs().max())
    tol = 4 * (2 * d_cmp + ulp_of(ref64.abs().max()))
    line = '%-8s %-40s |fused - f64| %.3g  |torch fp32 - f64| %.3g  bound %.3g  ratio %.3g  (max |f64| %.4g)' % (
        name, tag, d_ours, d_cmp, tol, d_ours / tol, float(ref64.abs().max()))
    print('bce ' + line)
    RECORD.append(line)
    if d_ours / tol > WORST.get(name, (-1.0, ''))[0]:
        WORST[name] = (d_ours / tol, tag)
    assert d_ours <= tol, (name, tag, d_ours, tol)


def check(X, A, T, lab, w, K0, K1, eps, tag):
    """Forward and backward of one problem against the yardstick; returns (row_loss, dA, dT) of the kernels."""
    As, Ts = segs(A, K0, K1), segs(T, K0, K1)
    prob = problem(As, Ts)
    N = T.shape[0]
    S32 = prob.scores()
    Y = bce_ref.dense_labels(lab[0], lab[1], lab[2], N)
    Y32 = bce_ref.smooth(Y, eps).float().cuda()
    rc, loss = fwd(X, prob, lab, eps)
    assert rc == 0
    within('row_loss', tag, loss, bce_ref.row_loss64(S32, Y, eps),
           F.binary_cross_entropy_with_logits(S32, Y32, reduction='none').sum(dim=1))
    rc, dA, dT = bwd(X, prob, lab, eps, w)
    assert rc == 0
    dA, dT = torch.cat(dA, dim=1), torch.cat(dT, dim=1)
    dA64, dT64 = bce_ref.grads64(S32, Y, eps, w, A, T)
    a32, t32 = A.clone().requires_grad_(), T.clone().requires_grad_()
    (F.binary_cross_entropy_with_logits(a32 @ t32.t(), Y32, reduction='none').sum(dim=1) * w).sum().backward()
    within('dA', tag, dA, dA64, a32.grad)
    within('dT', tag, dT, dT64, t32.grad)
    return loss, dA, dT


# ---------------------------------------------------------------------------
# forward and backward against the float64 forms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,K', CASES, ids=['B%d-N%d-K%d+%d' % (b, n, k[0], k[1]) for b, n, k in CASES])
def test_forward_and_backward_match_the_float64_forms(X, B, N, K):
    A, T, lab, w = make(B, N, K[0], K[1], seed=B * 1000 + N)
    for eps in (0.0, 0.1):
        check(X, A, T, lab, w, K[0], K[1], eps, 'B=%d N=%d K=%d+%d eps=%g' % (B, N, K[0], K[1], eps))


def test_scores_of_magnitude_300_stay_finite_and_within_the_bound(X):
    B, N, K0, K1 = X.BM + 1, X.MIN_TILES_PER_CHUNK * X.BN + 1 + X.BN + 1, 33, 0
    A, T, lab, w = make(B, N, K0, K1, seed=5)
    S = A @ T.t()
    A = A * (300.0 / S.abs().max(dim=1, keepdim=True).values)       # every row reaches +-300
    S32 = problem(segs(A, K0, K1), segs(T, K0, K1)).scores()
    assert float(S32.abs().max()) > 299 and float(S32.abs().max(dim=1).values.min()) > 299
    for eps in (0.0, 0.1):
        check(X, A, T, lab, w, K0, K1, eps, 'scores +-300 eps=%g' % eps)


def test_labels_that_win_by_100_never_give_a_negative_loss(X):
    """s(i, c) = +100 on row i's labels, -100 elsewhere (exactly: one coordinate per row, candidates of +-1)."""
    B, N = X.BM + 1, 2 * X.BN + 3
    gen = torch.Generator().manual_seed(11)
    sets = random_sets(B, N, gen)
    sets[0], sets[1], sets[2] = [], list(range(N)), [0, N - 1, 2 * X.BN]
    T = -torch.ones(N, B)
    for i, s in enumerate(sets):
        T[s, i] = 1.0
    A = 100.0 * torch.eye(B)
    lab = csr(sets)
    prob = problem([A.cuda()], [T.cuda()])
    S32 = prob.scores()
    Y = bce_ref.dense_labels(lab[0], lab[1], lab[2], N).cuda()
    assert torch.equal(S32.double(), 200.0 * Y - 100.0)
    rc, loss = fwd(X, prob, lab, 0.0)
    assert rc == 0 and bool(torch.isfinite(loss).all())
    assert bool((loss >= 0).all())
    assert float(loss.max()) <= N * 4e-44 + 1e-30       # sum_c log1p(exp(-100)): nothing of the +-100 is left
    rc, dA, dT = bwd(X, prob, lab, 0.0, torch.ones(B, device='cuda'))
    assert rc == 0 and float(dA[0].abs().max()) < 1e-38 and float(dT[0].abs().max()) < 1e-38


# ---------------------------------------------------------------------------
# label placement
# ---------------------------------------------------------------------------
def test_label_placement_edges_hubs_and_shared_segments(X):
    BM, BN = X.BM, X.BN
    N = X.MIN_TILES_PER_CHUNK * BN + 1 + BN + 1
    tiles, chunks = -(-N // BN), X.chunks(N)
    assert chunks == 2 and N % BN != 0
    split = (tiles * 1 // chunks) * BN          # the first column of the second chunk
    last_tile = (tiles - 1) * BN
    gen = torch.Generator().manual_seed(17)
    hub = sorted(torch.randperm(N, generator=gen)[:2 * BN + 37].tolist())
    assert len(hub) > 2 * BN
    sets = [[], list(range(N)), [0], [BN - 1], [BN], [split - 1], [split], [N - 1], list(range(last_tile, N)), hub,
            [3, BN + 1, split + 5],         # ... shared by two rows
            [5, split - 1, split, N - 2], [5, split - 1, split, N - 2]]     # one set stored at two offsets
    rows = list(range(len(sets) - 2)) + [10, 10, 11, 12]
    B = BM + 1
    rows += [int(x) for x in torch.randint(0, len(sets), (B - len(rows),), generator=gen)]
    K0, K1 = 5, 0
    A, T, _, w = make(B, N, K0, K1, seed=21)
    i1, i2 = rows.index(11), rows.index(12)
    A[i2] = A[i1]
    w[i2] = w[i1]
    lab = csr(sets, rows, front=3)
    assert int(lab[0][i1]) != int(lab[0][i2])
    for eps in (0.0, 0.1):
        loss, dA, dT = check(X, A, T, lab, w, K0, K1, eps, 'label placement eps=%g' % eps)
        # the same query row with the same label set at another offset of `labels`: the same bits
        assert int(bits(loss)[i1]) == int(bits(loss)[i2]) and torch.equal(bits(dA[i1]), bits(dA[i2]))
    # an empty segment given as lo > hi, pointing into the middle of another row's labels, is empty too
    lo, hi, labels = lab
    lo2, hi2 = lo.clone(), hi.clone()
    lo2[0], hi2[0] = int(lo[9]) + 4, int(lo[9]) + 1
    rc, loss2 = fwd(X, problem([A], [T]), (lo2, hi2, labels), 0.0)
    rc1, loss1 = fwd(X, problem([A], [T]), lab, 0.0)
    assert rc == 0 and rc1 == 0 and torch.equal(bits(loss1), bits(loss2))


# ---------------------------------------------------------------------------
# layout, reproducibility, NULL groups
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,K0,K1', [(65, 131, 8, 0), (133, 257, 200, 200)])
def test_padded_offset_operands_give_the_bits_of_the_dense_call(X, B, N, K0, K1):
    eps = 0.1
    A, T, lab, w = make(B, N, K0, K1, seed=31)
    As, Ts = segs(A, K0, K1), segs(T, K0, K1)
    dense = problem(As, Ts)
    rc, loss = fwd(X, dense, lab, eps)
    assert rc == 0
    rc, dA, dT = bwd(X, dense, lab, eps, w)
    assert rc == 0
    # operands with a pad and a 4-byte base offset out of NaN-poisoned buffers, outputs in guarded buffers
    Ac, Tc = [carve(x, pad=3, off=1) for x in As], [carve(x, pad=5, off=1) for x in Ts]
    labc = (carve(lab[0], off=1, poison=-1), carve(lab[1], off=1, poison=-1), carve(lab[2], off=3, poison=-1))
    wc = carve(w, off=1)
    assert all(x.data_ptr() % 16 == 4 for x in Ac + Tc + [wc])
    strided = problem(Ac, Tc)
    loss_g = guarded_out(B, off=3)
    rc, _ = fwd(X, strided, labc, eps, loss=loss_g)
    assert rc == 0
    assert torch.equal(bits(loss_g), bits(loss))
    dA_g = [guarded_out(B, x.shape[1], pad=2, off=1) for x in dA]
    dT_g = [guarded_out(N, x.shape[1], pad=7, off=3) for x in dT]
    rc, _, _ = bwd(X, strided, labc, eps, wc, dA=dA_g, dT=dT_g)
    assert rc == 0
    for g, ref in zip(dA_g + dT_g, dA + dT):
        assert torch.equal(bits(g), bits(ref))
    for v in [loss_g] + dA_g + dT_g + Ac + Tc + list(labc) + [wc]:
        assert_guard_intact(v)


def test_two_calls_give_the_same_bits_and_rows_do_not_depend_on_the_batch(X):
    B, N, K0, K1 = 2 * X.BM + 5, X.MIN_TILES_PER_CHUNK * X.BN + 1 + X.BN + 1, 200, 0
    eps = 0.1
    A, T, lab, w = make(B, N, K0, K1, seed=41)
    prob = problem([A], [T])
    outs = []
    for _ in range(2):
        rc, loss = fwd(X, prob, lab, eps)
        assert rc == 0
        rc, dA, dT = bwd(X, prob, lab, eps, w)
        assert rc == 0
        outs.append([loss] + dA + dT)
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b))
    # rows 70 .. 106 alone, as rows 0 .. 36 of another batch: the same loss and the same dA rows
    sl = slice(70, 107)
    small = problem([A[sl].contiguous()], [T])
    lab37 = (lab[0][sl].contiguous(), lab[1][sl].contiguous(), lab[2])
    rc, loss37 = fwd(X, small, lab37, eps)
    assert rc == 0 and torch.equal(bits(loss37), bits(outs[0][0][sl]))
    rc, dA37, _ = bwd(X, small, lab37, eps, w[sl].contiguous(), dT=None)
    assert rc == 0 and torch.equal(bits(dA37[0]), bits(outs[0][1][sl]))


def test_a_null_group_is_not_written_and_does_not_change_the_other(X):
    B, N, K0, K1 = X.BM + 1, 2 * X.BN + 3, 3, 3
    eps = 0.1
    A, T, lab, w = make(B, N, K0, K1, seed=51)
    prob = problem(segs(A, K0, K1), segs(T, K0, K1))
    rc, dA, dT = bwd(X, prob, lab, eps, w)
    assert rc == 0
    # no table gradient: the guarded dT buffers are never handed over and stay as they are
    dT_g = [guarded_out(N, 3), guarded_out(N, 3)]
    rc, dA_only, none = bwd(X, prob, lab, eps, w, dT=None)
    assert rc == 0 and none is None
    for a, b in zip(dA_only, dA):
        assert torch.equal(bits(a), bits(b))
    # no query gradient
    rc, none, dT_only = bwd(X, prob, lab, eps, w, dA=None)
    assert rc == 0 and none is None
    for a, b in zip(dT_only, dT):
        assert torch.equal(bits(a), bits(b))
    # a group whose first pointer is NULL but whose second is given is malformed: nothing is written
    dA_g = [guarded_out(B, 3), guarded_out(B, 3)]
    args = [prob.desc, lab[0], lab[1], lab[2], eps, w, None, 0, dA_g[1], dA_g[1].stride(0), dT_g[0], dT_g[0].stride(0),
            dT_g[1], dT_g[1].stride(0)]
    ws = workspace(X, prob)
    assert raw(X.load_library(), 'kge_lp_bce_bwd', *(args + [ws, ws.numel()])) == EINVAL
    torch.cuda.synchronize()
    for v in dA_g + dT_g:
        assert_guard_intact(v, rows=0)


# ---------------------------------------------------------------------------
# refusals: nothing is launched, nothing is written
# ---------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched(X):
    from torchkge_amd import _hip
    B, N, K0, K1 = 5, 70, 8, 0
    A, T, lab, w = make(B, N, K0, K1, seed=61)
    lo, hi, labels = lab
    prob = problem([A], [T])
    lib = X.load_library()
    ws = workspace(X, prob)
    outs = {'loss': guarded_out(B), 'dA': guarded_out(B, K0), 'dT': guarded_out(N, K0)}

    def both(desc, expect, ws_n=None, tag='', lab=(lo, hi, labels), eps=0.0):
        n = ws.numel() if ws_n is None else ws_n
        assert raw(lib, 'kge_lp_bce_fwd', desc, lab[0], lab[1], lab[2], eps, outs['loss'], ws, n) == expect, ('fwd', tag)
        assert raw(lib, 'kge_lp_bce_bwd', desc, lab[0], lab[1], lab[2], eps, w, outs['dA'], K0, None, 0, outs['dT'], K0, None, 0,
                   ws, n) == expect, ('bwd', tag)

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
    both(prob.desc, EINVAL, ws_n=X.ws_bytes(B, N, K0, K1) - 1, tag='short workspace')
    both(variant(B=-1), EINVAL, tag='B < 0')
    both(prob.desc, EINVAL, lab=(None, hi, labels), tag='NULL seg_lo')
    both(prob.desc, EINVAL, lab=(lo, None, labels), tag='NULL seg_hi')
    both(prob.desc, EINVAL, lab=(lo, hi, None), tag='NULL labels')
    both(prob.desc, EINVAL, eps=1.5, tag='label_smoothing 1.5')
    both(prob.desc, EINVAL, eps=-0.5, tag='label_smoothing -0.5')
    assert raw(lib, 'kge_lp_bce_fwd', prob.desc, lo, hi, labels, 0.0, outs['loss'], None, ws.numel()) == EINVAL
    assert raw(lib, 'kge_lp_bce_fwd', prob.desc, lo, hi, labels, 0.0, None, ws, ws.numel()) == EINVAL      # NULL row_loss
    assert raw(lib, 'kge_lp_bce_bwd', prob.desc, lo, hi, labels, 0.0, None, outs['dA'], K0, None, 0, outs['dT'], K0, None, 0,
               ws, ws.numel()) == EINVAL       # NULL g
    assert raw(lib, 'kge_lp_bce_bwd', prob.desc, lo, hi, labels, 0.0, w, outs['dA'], K0 - 1, None, 0, outs['dT'], K0, None, 0,
               ws, ws.numel()) == EINVAL       # a leading dimension below K
    torch.cuda.synchronize()
    for v in outs.values():
        assert_guard_intact(v, rows=0)
    # B = 0: success, nothing launched
    assert raw(lib, 'kge_lp_bce_fwd', variant(B=0), lo, hi, labels, 0.0, outs['loss'], ws, ws.numel()) == 0
    assert raw(lib, 'kge_lp_bce_bwd', variant(B=0), lo, hi, labels, 0.0, w, outs['dA'], K0, None, 0, outs['dT'], K0, None, 0,
               ws, ws.numel()) == 0
    torch.cuda.synchronize()
    for v in outs.values():
        assert_guard_intact(v, rows=0)
